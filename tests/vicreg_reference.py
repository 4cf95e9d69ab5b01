"""Float64 restatement of the VICReg loss (objective.add_vicreg_loss / csrc/vicreg.hip): Bardes, Ponce, LeCun 2022, VICReg:
Variance-Invariance-Covariance Regularization for Self-Supervised Learning, written with explicit formulas -- once in the DIRECT form (the
D x D covariance matrix of each view), once in the GRAM form the kernels run, which never builds that matrix, and once as a float32
EMULATION of the Gram form whose own error against float64 supplies every GPU tolerance.

R replicas; replica r holds h_r [2n, D] = [view-1 rows; view-2 rows].  h_all [2N, D], N = R n: every replica's view-1 rows, then every
replica's view-2 rows (the NT-Xent layout).  Per view v and column i over the N rows of the GLOBAL batch:
    xc = h - mean_a h,   var_i = sum_a xc_ai^2 / (N - 1) (unbiased),   std_i = sqrt(var_i + eps)

direct form:
    Cov  = xc^T xc / (N - 1)                             [D, D]
    inv  = (1 / (N D)) sum_{a,i} (h1_ai - h2_ai)^2
    var  = (1/2) sum_v (1 / D) sum_i max(0, gamma - std_vi)
    cov  = sum_v (1 / D) sum_{i != j} Cov_v,ij^2
    L    = sim_coeff * inv + std_coeff * var + cov_coeff * cov
Gram form:
    G = xc xc^T [N, N];  sum_ij Cov_ij^2 = tr(Cov^T Cov) = (1 / (N-1)^2) sum_ab G_ab^2,  Cov_ii = var_i
    cov_v = (1 / D) ((1 / (N-1)^2) sum_ab G_ab^2 - sum_i var_i^2)        ("minuend" - "subtrahend")
    replica r owns the rows a in [r n, (r + 1) n) against all N columns and reports inv over its own rows (1 / (n D)), the global var,
    and cov with R / (N-1)^2 * sum_{a in r, b} G_ab^2 in place of the full sum;  mean_r loss_r = L
    dL/dh_a = cov_coeff * (4 / ((N-1)^2 D) * sum_b G_ab xc_b - 4 / ((N-1) D) * var o xc_a)
            - std_coeff * (1 / (2 D)) * [std < gamma] o xc_a / ((N-1) std) + sim_coeff * (2 / (N D)) * (x_a - o_a)
    (x, o: the raw rows of this view and of the other one).  The centring has no backward: the gradient with respect to xc is a combination
    of rows of xc, its column sums vanish, and the projection onto centred columns changes nothing.

tests/test_vicreg_reference.py pins the forms against torch float64 autograd of the direct form and a hand-derived case."""
import numpy as np

DEFAULTS = dict(sim_coeff=25.0, std_coeff=25.0, cov_coeff=1.0, eps=1e-4, gamma=1.0)
# the loss-and-gradient cases of tests/test_gpu_vicreg.py: (n, N, D, rank) and the two coefficient sets (sim, std, cov)
MAIN_SHAPES = [(2, 2, 64, 0), (1, 2, 64, 1), (5, 5, 64, 0), (70, 70, 128, 0), (64, 128, 64, 1), (33, 99, 320, 2), (70, 70, 448, 0),
               (16, 16, 2048, 0)]
COEFF_SETS = [(25.0, 25.0, 1.0), (1.0, 0.0, 3.0)]
CENTER_SHAPES = [(2, 64), (5, 64), (70, 128), (256, 320)]
BUDGET_SEEDS = (0, 1, 2, 3, 4)
WHITENED_SEEDS = (4, 5, 6)
# Per GPU case (n, N, D, rank): the worst error of the float32 emulation against float64 over COEFF_SETS x BUDGET_SEEDS, each quantity on
# its own scale (error_scales), as tests/test_vicreg_reference.py re-measures it (tests/golden/VICREG_HAND_DERIVED.md, "Error budget").
# The tolerances of tests/test_gpu_vicreg.py are 4x these.
EMULATION_ERROR = {
    (2, 2, 64, 0): dict(loss=3.19e-7, inv=3.30e-8, var=1.48e-8, cov=3.26e-7, grad=3.03e-7),
    (1, 2, 64, 1): dict(loss=4.28e-7, inv=3.85e-8, var=1.47e-8, cov=4.54e-7, grad=2.81e-7),
    (5, 5, 64, 0): dict(loss=8.63e-8, inv=2.71e-8, var=7.37e-9, cov=1.54e-7, grad=4.07e-7),
    (70, 70, 128, 0): dict(loss=3.16e-8, inv=4.19e-8, var=6.71e-9, cov=3.20e-8, grad=6.99e-7),
    (64, 128, 64, 1): dict(loss=2.64e-8, inv=3.59e-8, var=6.18e-9, cov=9.20e-9, grad=1.05e-6),
    (33, 99, 320, 2): dict(loss=5.84e-8, inv=4.06e-8, var=7.26e-9, cov=4.15e-8, grad=5.32e-7),
    (70, 70, 448, 0): dict(loss=2.95e-8, inv=4.10e-8, var=6.24e-9, cov=3.84e-8, grad=5.55e-7),
    (16, 16, 2048, 0): dict(loss=8.37e-8, inv=3.62e-8, var=6.52e-9, cov=3.98e-8, grad=2.90e-7),
}
# per centre case (N, D): xc relative to the largest |xc|, var and std relative to their largest value, over BUDGET_SEEDS
CENTER_ERROR = {
    (2, 64): dict(xc=0.0, stat_var=0.0, stat_std=5.25e-11),
    (5, 64): dict(xc=3.98e-8, stat_var=5.91e-8, stat_std=3.31e-8),
    (70, 128): dict(xc=3.29e-8, stat_var=2.77e-8, stat_std=1.61e-8),
    (256, 320): dict(xc=5.41e-8, stat_var=1.88e-8, stat_std=1.03e-8),
}
# the same for the whitened near-decorrelated case (N = 256, D = 64) over WHITENED_SEEDS, cov relative to its minuend
WHITENED_ERROR = dict(loss=3.6e-8, inv=3.7e-8, var=3.7e-9, cov=6.0e-9, grad=1.4e-7)
TOL = {c: {k: 4.0 * v for k, v in e.items()} for c, e in EMULATION_ERROR.items()}
CENTER_TOL = {c: {k: 4.0 * v for k, v in e.items()} for c, e in CENTER_ERROR.items()}
WHITENED_TOL = {k: 4.0 * v for k, v in WHITENED_ERROR.items()}


def h_all_of(hs, n):
    return np.concatenate([h[:n] for h in hs] + [h[n:] for h in hs], axis=0)


def replica_rows(r, n, N):
    """Global rows of replica r's [view-1; view-2] block."""
    return np.concatenate([np.arange(r * n, (r + 1) * n), N + np.arange(r * n, (r + 1) * n)])


def case_views(n, R, D, seed):
    """The float32 blocks of a loss-and-gradient case: R replicas of [2n, D].  Column i is scaled by 0.5 ... 1.5 so that some columns
    sit on each side of the hinge at gamma = 1, carries a mean of up to +/- 2, and view 2 is view 1 plus noise."""
    g = np.random.default_rng(1000 * seed + 7 * n + D + R)
    scale = 0.5 + (np.arange(D) % 5) / 4.0
    shift = 2.0 * np.cos(np.arange(D))
    out = []
    for _ in range(R):
        h1 = g.standard_normal((n, D)) * scale + shift
        h2 = h1 + 0.4 * g.standard_normal((n, D)) * scale
        out.append(np.concatenate([h1, h2]).astype(np.float32))
    return out


def whitened_views(N=256, D=64, var=0.81, mean=5.0, seed=4):
    """One replica whose two views have QR-whitened columns: Cov = var * I up to rounding, so cov is the difference of two sums of
    size var^2 each that cancel to (almost) nothing."""
    g = np.random.default_rng(seed)
    views = []
    for _ in range(2):
        x = g.standard_normal((N, D))
        q, _ = np.linalg.qr(x - x.mean(0))
        views.append(q * np.sqrt(var * (N - 1)) + mean)
    return [np.concatenate(views).astype(np.float32)]


def center(h):
    """One view [N, D] -> (xc, var [D]) over its rows, unbiased variance."""
    h = np.asarray(h, dtype=np.float64)
    xc = h - h.mean(axis=0)
    return xc, (xc ** 2).sum(axis=0) / (h.shape[0] - 1)


def _views(hiddens):
    hs = [np.asarray(h, dtype=np.float64) for h in hiddens]
    R, n = len(hs), hs[0].shape[0] // 2
    N = R * n
    assert N >= 2, 'the unbiased variance needs N >= 2'
    h_all = h_all_of(hs, n)
    return R, n, N, h_all[:N], h_all[N:]


def vicreg_direct(hiddens, sim_coeff=25.0, std_coeff=25.0, cov_coeff=1.0, eps=1e-4, gamma=1.0):
    """The D x D form on the global batch.  Returns dict(loss, inv, var, cov, frob = sum_v (1 / D) sum_ij Cov_v,ij^2 (the minuend of the
    Gram form), std [2, D]) in float64."""
    R, n, N, h1, h2 = _views(hiddens)
    D = h1.shape[1]
    inv = float(((h1 - h2) ** 2).sum() / (N * D))
    var_term = cov = frob = 0.0
    stds = []
    for h in (h1, h2):
        xc, var = center(h)
        std = np.sqrt(var + eps)
        stds.append(std)
        var_term += 0.5 * float(np.maximum(0.0, gamma - std).sum() / D)
        C = xc.T @ xc / (N - 1)
        frob += float((C ** 2).sum() / D)
        cov += float(((C ** 2).sum() - (np.diag(C) ** 2).sum()) / D)
    return dict(loss=sim_coeff * inv + std_coeff * var_term + cov_coeff * cov, inv=inv, var=var_term, cov=cov, frob=frob,
                std=np.stack(stds))


def vicreg_direct_torch(h_all, sim_coeff=25.0, std_coeff=25.0, cov_coeff=1.0, eps=1e-4, gamma=1.0):
    """The direct form on a float64 torch tensor h_all [2N, D] (differentiable: the autograd reference)."""
    import torch
    N, D = h_all.shape[0] // 2, h_all.shape[1]
    h1, h2 = h_all[:N], h_all[N:]
    loss = sim_coeff * ((h1 - h2) ** 2).sum() / (N * D)
    for h in (h1, h2):
        xc = h - h.mean(0)
        C = xc.T @ xc / (N - 1)
        std = torch.sqrt(torch.diagonal(C) + eps)
        loss = loss + std_coeff * 0.5 * torch.relu(gamma - std).sum() / D
        loss = loss + cov_coeff * ((C ** 2).sum() - (torch.diagonal(C) ** 2).sum()) / D
    return loss


def xc_gradient(xc, var, std, N, D, std_coeff, cov_coeff, gamma):
    """Gradient of std_coeff * var-term + cov_coeff * cov-term of ONE view with respect to its centred rows xc [N, D] (all rows)."""
    G = xc @ xc.T
    g = cov_coeff * (4.0 / ((N - 1) ** 2 * D) * G @ xc - 4.0 / ((N - 1) * D) * var * xc)
    with np.errstate(divide='ignore', invalid='ignore'):
        w = np.where((std < gamma) & (std > 0), 1.0 / ((N - 1) * std), 0.0)
    return g - std_coeff / (2.0 * D) * w * xc


def vicreg_gram(hiddens, sim_coeff=25.0, std_coeff=25.0, cov_coeff=1.0, eps=1e-4, gamma=1.0):
    """The Gram form, per replica.  Returns dict(loss, inv, var, cov, minuend: lists over replicas of the per-replica values (minuend =
    sum_v R / ((N-1)^2 D) sum_{a in r, b} G_v,ab^2, the larger side of cov's subtraction); grads: list over replicas of dL/dh_r
    [2n, D]; xc_all [2N, D]; stats [2, 2, D] = {var, std} per view; gram: list over replicas of [2, n, N]) in float64."""
    R, n, N, h1, h2 = _views(hiddens)
    D = h1.shape[1]
    xcs, vars_, stds, Gs, gx = [], [], [], [], []
    for h in (h1, h2):
        xc, var = center(h)
        std = np.sqrt(var + eps)
        xcs.append(xc); vars_.append(var); stds.append(std); Gs.append(xc @ xc.T)
        gx.append(xc_gradient(xc, var, std, N, D, std_coeff, cov_coeff, gamma))
    var_term = sum(0.5 * float(np.maximum(0.0, gamma - s).sum() / D) for s in stds)
    sub = sum(float((v ** 2).sum() / D) for v in vars_)
    d1 = gx[0] + sim_coeff * 2.0 / (N * D) * (h1 - h2)
    d2 = gx[1] + sim_coeff * 2.0 / (N * D) * (h2 - h1)
    dh = np.concatenate([d1, d2], axis=0)
    loss, invs, covs, minuends, gram = [], [], [], [], []
    for r in range(R):
        a = slice(r * n, (r + 1) * n)
        inv_r = float(((h1[a] - h2[a]) ** 2).sum() / (n * D))
        minuend = sum(float(R / (N - 1) ** 2 * (G[a] ** 2).sum() / D) for G in Gs)
        invs.append(inv_r); minuends.append(minuend); covs.append(minuend - sub)
        loss.append(sim_coeff * inv_r + std_coeff * var_term + cov_coeff * (minuend - sub))
        gram.append(np.stack([G[a] for G in Gs]))
    rows = [replica_rows(r, n, N) for r in range(R)]
    return dict(loss=loss, inv=invs, var=[var_term] * R, cov=covs, minuend=minuends, grads=[dh[i] for i in rows],
                xc_all=np.concatenate(xcs, axis=0), stats=np.stack([np.stack([v, s]) for v, s in zip(vars_, stds)]), gram=gram)


# ---------------------------------------------------------------------------------------------------------------- float32 emulation
def k_splits(n, N, D):
    """The split rule of csrc/vicreg.hip (simclr_vicreg_k_splits): one view per workgroup, tile edge 128 where both views' tiles give
    >= 256 workgroups, else 64; a grid below 256 workgroups splits D towards 1024 workgroups, with at least 4 stages of 32 per part and
    at most 16 parts; the stages are dealt in equal chunks, the last part may be shorter.  -> (S, k per part)."""
    cd = lambda a, b: -(-a // b)
    E = 128 if 2 * cd(N, 128) * cd(n, 128) >= 256 else 64
    wgs, stages = 2 * cd(n, E) * cd(N, E), D // 32
    S = 1
    if wgs < 256:
        S = max(1, min(cd(1024, wgs), stages // 4, 16))
    chunk = cd(stages, S)
    return cd(stages, chunk), chunk * 32


def _seq_matmul_f32(A, B):
    """A [m, K] B^T [K, c] with ONE float32 accumulator per entry, k in order, every product and every sum rounded to float32: the
    worst case of the MFMA k loop (which keeps at least this much)."""
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    acc = np.zeros((A.shape[0], B.shape[0]), np.float32)
    for k in range(A.shape[1]):
        acc = acc + A[:, k:k + 1] * B[None, :, k]
    return acc


def center_emulated(h, eps):
    """csrc/vicreg.hip's centre launch on one float32 view: the mean in double, xc rounded to float32, var from the ROUNDED xc in
    double.  -> (xc float32, var float64, std float64)."""
    h = np.asarray(h, np.float32)
    eps = float(np.float32(eps))          # eps crosses the C ABI as a float
    mu = h.astype(np.float64).mean(axis=0)
    xc = (h.astype(np.float64) - mu).astype(np.float32)
    var = (xc.astype(np.float64) ** 2).sum(axis=0) / (h.shape[0] - 1)
    return xc, var, np.sqrt(var + eps)


def vicreg_emulated(hiddens, rank, sim_coeff=25.0, std_coeff=25.0, cov_coeff=1.0, eps=1e-4, gamma=1.0, grad_scale=None, gram=None):
    """The float32 arithmetic of the kernels for replica `rank`: fp32 centring, fp32 Gram blocks with fp32 accumulation over each k part
    and the fixed-order merge ((p0 + p1) + p2) + ..., the sums and the subtraction in double, the four outputs rounded to float32; the
    gradient with float32 coefficients, a float32 k loop over the Gram block and a float32 epilogue.  grad_scale defaults to 1 / R, so
    grad = dL/dh of the local rows.  `gram`: blocks [2, n, N] of an earlier call on the same data (they do not depend on the
    coefficients).  -> dict(loss, inv, var, cov (float32 values), grad [2n, D], xc_all, stats, gram, splits)."""
    f32 = np.float32
    hs = [np.asarray(h, f32) for h in hiddens]
    R, n = len(hs), hs[0].shape[0] // 2
    N, D = R * n, hs[0].shape[1]
    h_all = h_all_of(hs, n)
    a = slice(rank * n, (rank + 1) * n)
    S, kc = k_splits(n, N, D)
    views = [center_emulated(h_all[v * N:(v + 1) * N], eps) for v in range(2)]
    if gram is None:
        gram = []
        for xc, _, _ in views:
            G = None
            for p in range(S):
                part = _seq_matmul_f32(xc[a, p * kc:(p + 1) * kc], xc[:, p * kc:(p + 1) * kc])
                G = part if G is None else G + part
            gram.append(G)
        gram = np.stack(gram)
    x1, x2 = h_all[:N][a].astype(np.float64), h_all[N:][a].astype(np.float64)
    inv = ((x1 - x2) ** 2).sum() / (n * D)
    var_term = sum(0.5 * np.maximum(0.0, gamma - sd).sum() / D for _, _, sd in views)
    fr = sum((gram[v].astype(np.float64) ** 2).sum() for v in range(2))
    v2 = sum((var ** 2).sum() for _, var, _ in views)
    cov = (fr * (R / (N - 1.0) ** 2) - v2) / D
    loss = sim_coeff * inv + std_coeff * var_term + cov_coeff * cov
    s = (1.0 / R if grad_scale is None else grad_scale) * R
    c_gram, c_var = f32(s * cov_coeff * 4.0 / ((N - 1.0) ** 2 * D)), f32(-s * cov_coeff * 4.0 / ((N - 1.0) * D))
    c_std, c_inv = f32(-s * std_coeff / (2.0 * D * (N - 1.0))), f32(s * sim_coeff * 2.0 / (N * D))
    grads = []
    for v in range(2):
        xc, var, sd = views[v]
        acc = _seq_matmul_f32(gram[v], xc.T)
        var32, sd32 = var.astype(f32), sd.astype(f32)
        with np.errstate(divide='ignore', invalid='ignore'):
            cj = c_var * var32 + np.where((sd32 < f32(gamma)) & (sd32 > 0), c_std / sd32, f32(0)).astype(f32)
        x, o = h_all[v * N:(v + 1) * N][a], h_all[(1 - v) * N:(2 - v) * N][a]
        grads.append(c_gram * acc + cj * xc[a] + c_inv * (x - o))
    assert all(g.dtype == f32 for g in grads)
    return dict(loss=f32(loss), inv=f32(inv), var=f32(var_term), cov=f32(cov), grad=np.concatenate(grads), gram=gram, splits=S,
                xc_all=np.concatenate([v[0] for v in views]), stats=np.stack([np.stack([v[1], v[2]]) for v in views]))


def error_scales(ref, rank, sim_coeff, std_coeff, cov_coeff, gamma=1.0):
    """The scale every error of a case is divided by: loss -> the sum of the magnitudes of its pieces (cov enters with its MINUEND);
    inv -> itself; var -> gamma (a mean of hinges of at most gamma each); cov -> its minuend; grad -> the case's largest gradient entry."""
    m = ref['minuend'][rank]
    return dict(loss=sim_coeff * ref['inv'][rank] + std_coeff * ref['var'][rank] + cov_coeff * m, inv=ref['inv'][rank], var=gamma, cov=m,
                grad=float(np.abs(ref['grads'][rank]).max()))


def relative_errors(got, ref, rank, coeffs, gamma=1.0):
    """|got - ref| / scale of loss, inv, var, cov and grad (the largest entry) for replica `rank`; got: dict of values / arrays."""
    sc = error_scales(ref, rank, *coeffs, gamma=gamma)
    out = {k: abs(float(got[k]) - ref[k][rank]) / sc[k] for k in ('loss', 'inv', 'var', 'cov')}
    out['grad'] = float(np.abs(np.asarray(got['grad'], np.float64) - ref['grads'][rank]).max()) / sc['grad']
    return out


def center_errors(xc, stats, h, eps=1e-4):
    """Errors of a centre launch's outputs (xc_all [2N, D], stats [2, 2, D] = {var, std}) on the float32 block h [2N, D] against
    float64: xc relative to the largest |xc|, var and std relative to their largest value."""
    N = h.shape[0] // 2
    xc, stats = np.asarray(xc, np.float64), np.asarray(stats, np.float64)
    out = dict(xc=0.0, stat_var=0.0, stat_std=0.0)
    for v in range(2):
        rx, rvar = center(h[v * N:(v + 1) * N])
        rsd = np.sqrt(rvar + eps)
        out['xc'] = max(out['xc'], float(np.abs(xc[v * N:(v + 1) * N] - rx).max() / np.abs(rx).max()))
        out['stat_var'] = max(out['stat_var'], float(np.abs(stats[v][0] - rvar).max() / rvar.max()))
        out['stat_std'] = max(out['stat_std'], float(np.abs(stats[v][1] - rsd).max() / rsd.max()))
    return out


def center_case(N, D, seed):
    """Rows randn + 10: raw moments (E[x^2] - E[x]^2) in float32 lose the variance here, the two-pass form does not."""
    g = np.random.default_rng(100 * seed + N + D)
    return (g.standard_normal((2 * N, D)) + 10.0).astype(np.float32)


def center_emulation_errors(N, D, seed, eps=1e-4):
    h = center_case(N, D, seed)
    views = [center_emulated(h[v * N:(v + 1) * N], eps) for v in range(2)]
    return center_errors(np.concatenate([v[0] for v in views]), np.stack([np.stack([v[1], v[2]]) for v in views]), h, eps)


def measured_budget():
    """Re-measures EMULATION_ERROR: per GPU case, the worst emulation error of every quantity over COEFF_SETS x BUDGET_SEEDS."""
    out = {}
    for n, N, D, rank in MAIN_SHAPES:
        worst = dict(loss=0.0, inv=0.0, var=0.0, cov=0.0, grad=0.0)
        for seed in BUDGET_SEEDS:
            hs = case_views(n, N // n, D, seed)
            gram = None
            for coeffs in COEFF_SETS:
                ref = vicreg_gram(hs, *coeffs)
                emu = vicreg_emulated(hs, rank, *coeffs, gram=gram)
                gram = emu['gram']
                for k, e in relative_errors(emu, ref, rank, coeffs).items():
                    worst[k] = max(worst[k], e)
        out[(n, N, D, rank)] = worst
    return out


def measured_center_budget():
    """Re-measures CENTER_ERROR: per centre case, the worst emulation error of xc, var and std over BUDGET_SEEDS."""
    out = {}
    for N, D in CENTER_SHAPES:
        worst = dict(xc=0.0, stat_var=0.0, stat_std=0.0)
        for seed in BUDGET_SEEDS:
            for k, e in center_emulation_errors(N, D, seed).items():
                worst[k] = max(worst[k], e)
        out[(N, D)] = worst
    return out


def measured_whitened_budget():
    """Re-measures WHITENED_ERROR: the worst emulation error over WHITENED_SEEDS (tests/test_gpu_vicreg.py runs the first)."""
    coeffs = COEFF_SETS[0]
    worst = {k: 0.0 for k in WHITENED_ERROR}
    for seed in WHITENED_SEEDS:
        hs = whitened_views(seed=seed)
        ref = vicreg_gram(hs, *coeffs)
        for k, e in relative_errors(vicreg_emulated(hs, 0, *coeffs), ref, 0, coeffs).items():
            worst[k] = max(worst[k], e)
    return worst
