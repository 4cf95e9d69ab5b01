"""Float64 restatement of the hard-negative / debiased NT-Xent (objective.add_hard_negative_contrastive_loss / csrc/hcl.hip), its
analytic gradient, and a float32 emulation of the kernels' arithmetic.  The formulas are this project's definition of the two
corrections (Robinson et al. 2021: beta; Chuang et al. 2020: tau_plus), written from memory of the papers: not a parity claim.

R replicas; replica r holds h_r [2n, D] = [view-a rows; view-b rows].  z_r = l2-normalised h_r (hidden_norm) or h_r itself.
z_all [2N, D], N = R n: every replica's view-a rows, then every replica's view-b rows (the NT-Xent layout).  Global row i has the own
column i and the positive column pos(i) = (i + N) mod 2N; Neg(i) = the other M = 2N - 2 columns.  With a = 1 / T, s_ik = z_i . z_k:

    p_i     = exp(a s_i,pos)
    A_i     = sum_{k in Neg(i)} exp((1 + beta) a s_ik),    B_i = sum_{k in Neg(i)} exp(beta a s_ik)
    G_raw_i = (M A_i / B_i - tau_plus M p_i) / (1 - tau_plus)
    G_i     = max(G_raw_i, M exp(-a))                                    (the floor)
    l_i     = log(p_i + G_i) - a s_i,pos
    loss_r  = (1 / n) sum_{i in r's 2n rows} l_i                         (the sum of the two per-view means, as NT-Xent here)
    objective of the step = (1 / R) sum_r loss_r

Gradient (the weights exp(beta a s) are differentiated through), P1 / P0 the softmaxes over Neg(i) at scales (1 + beta) a / beta a:
    above the floor:  W_ik = a w_i ((1 + beta) P1_ik - beta P0_ik),  w_i = (M A_i / B_i) / ((1 - tau_plus)(p_i + G_i))
                      W_i,pos = a (p_i (1 - tau_plus M / (1 - tau_plus)) / (p_i + G_i) - 1)
    on the floor:     W_ik = 0,  W_i,pos = a (p_i / (p_i + G_i) - 1)
    W_ii = 0;   d objective / d z_all = (W + W^T) z_all / (R n);   l2 normalisation: d/dh = (dz - z (z . dz)) / |h|

The gradient jumps where G_raw crosses the floor: a comparison is meaningful for rows with |G_raw / floor - 1| >= KINK_MARGIN only,
and the GPU cases are chosen (CASE_SEED) so that this holds for EVERY row.

tests/test_hcl_reference.py pins this file against torch float64 autograd, the NT-Xent oracle and tests/golden/HCL_HAND_DERIVED.md."""
import itertools

import numpy as np

KINK_MARGIN = 1e-2
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453

# the kernel cases of tests/test_gpu_hcl.py: (n, R, D, rank) x temperatures x betas x tau_plus x the two input families
SHAPES = [(2, 1, 64, 0), (8, 1, 64, 0), (24, 1, 128, 0), (64, 2, 128, 1), (96, 2, 256, 0), (100, 1, 128, 0), (65, 1, 64, 0)]
TEMPERATURES, BETAS, TAU_PLUS = (0.1, 0.5), (0.0, 0.5, 1.0), (0.0, 0.1)
FAMILIES = ('independent', 'correlated')
PARAMS = list(itertools.product(TEMPERATURES, BETAS, TAU_PLUS))
# seed of every (shape, family): the first for which no row of any replica lies within KINK_MARGIN of the floor under any of PARAMS
# (tests/test_hcl_reference.py re-checks; a case that comes too close gets another seed, never a smaller margin)
CASE_SEED = {(s, f): 0 for s in SHAPES for f in FAMILIES}
CASE_SEED[((8, 1, 64, 0), 'correlated')] = 1          # seed 0 leaves a row 3.4e-3 from the floor at T = 0.5, beta = 0.5, tau_plus = 0.1
# per (shape, family): the worst error of the float32 emulation against float64 over PARAMS on the case's own inputs -- the loss
# relative to itself, the gradient relative to its largest entry -- as tests/test_hcl_reference.py re-measures it
# (tests/golden/HCL_HAND_DERIVED.md, "Error budget").  The tolerances of tests/test_gpu_hcl.py are 4x these.
EMULATION_ERROR = {
    ((2, 1, 64, 0), 'independent'): dict(loss=1.02e-07, grad=2.84e-07),
    ((2, 1, 64, 0), 'correlated'): dict(loss=8.52e-07, grad=8.60e-07),
    ((8, 1, 64, 0), 'independent'): dict(loss=9.30e-08, grad=2.35e-07),
    ((8, 1, 64, 0), 'correlated'): dict(loss=2.10e-07, grad=1.32e-06),
    ((24, 1, 128, 0), 'independent'): dict(loss=5.17e-08, grad=4.47e-07),
    ((24, 1, 128, 0), 'correlated'): dict(loss=3.30e-07, grad=3.59e-06),
    ((64, 2, 128, 1), 'independent'): dict(loss=3.96e-08, grad=5.81e-07),
    ((64, 2, 128, 1), 'correlated'): dict(loss=1.92e-07, grad=2.88e-06),
    ((96, 2, 256, 0), 'independent'): dict(loss=3.66e-08, grad=7.60e-07),
    ((96, 2, 256, 0), 'correlated'): dict(loss=8.49e-08, grad=3.58e-06),
    ((100, 1, 128, 0), 'independent'): dict(loss=4.54e-08, grad=1.39e-06),
    ((100, 1, 128, 0), 'correlated'): dict(loss=2.46e-07, grad=3.48e-06),
    ((65, 1, 64, 0), 'independent'): dict(loss=3.62e-08, grad=7.84e-07),
    ((65, 1, 64, 0), 'correlated'): dict(loss=2.67e-07, grad=1.77e-06),
}
TOL = {c: {k: 4.0 * v for k, v in e.items()} for c, e in EMULATION_ERROR.items()}


def f32(x):
    """A scalar as it crosses the C ABI: rounded to float32, held as a Python float."""
    return float(np.float32(x))


def l2_normalize(h):
    nrm = np.sqrt(np.maximum((h * h).sum(axis=1, keepdims=True), 1e-12))
    return h / nrm, nrm


def z_all_of(zs, n):
    return np.concatenate([z[:n] for z in zs] + [z[n:] for z in zs], axis=0)


def replica_rows(r, n, N):
    """Global rows of replica r's [view-a; view-b] block."""
    return np.concatenate([np.arange(r * n, (r + 1) * n), N + np.arange(r * n, (r + 1) * n)])


def case_views(n, R, D, family, seed):
    """The float32, l2-normalised blocks [2n, D] of R replicas.  'independent': the two views are unrelated random rows;
    'correlated': h_b = h_a + 0.05 noise (the positive's logit close to 1 / T: the debiasing term pushes rows onto the floor)."""
    g = np.random.default_rng(1000 * seed + 10 * n + R)
    out = []
    for _ in range(R):
        ha = g.standard_normal((n, D))
        hb = g.standard_normal((n, D)) if family == 'independent' else ha + 0.05 * g.standard_normal((n, D))
        out.append(l2_normalize(np.concatenate([ha, hb]))[0].astype(np.float32))
    return out


def _masks(N):
    M2 = 2 * N
    idx = np.arange(M2)
    own = np.eye(M2, dtype=bool)
    pos = np.zeros((M2, M2), dtype=bool)
    pos[idx, (idx + N) % M2] = True
    return own, pos, ~(own | pos)


def hcl_direct_torch(z_all, n, temperature, beta, tau_plus):
    """The direct form on a torch float64 z_all [2N, D] (N = R n): -> the list over replicas of loss_r (for autograd)."""
    import torch
    N = z_all.shape[0] // 2
    R, M, a = N // n, 2.0 * N - 2.0, 1.0 / temperature
    _, pos, neg = (torch.from_numpy(m) for m in _masks(N))
    S = z_all @ z_all.T
    spos = S[pos]                                           # row-major: one per row
    p = torch.exp(a * spos)
    A = torch.where(neg, torch.exp((1.0 + beta) * a * S), torch.zeros_like(S)).sum(1)
    B = torch.where(neg, torch.exp(beta * a * S), torch.zeros_like(S)).sum(1)
    graw = (M * A / B - tau_plus * M * p) / (1.0 - tau_plus)
    G = torch.maximum(graw, torch.full_like(graw, M * float(np.exp(-a))))
    row = torch.log(p + G) - a * spos
    return [row[torch.from_numpy(replica_rows(r, n, N))].sum() / n for r in range(R)]


def hcl_reference(hiddens, temperature, beta, tau_plus, hidden_norm=True):
    """hiddens: list over replicas of [2n, D] array-likes.  Returns dict(loss, floor_share: lists over replicas; grads: list over
    replicas of d objective / d h_r; row, on_floor, ratio = G_raw / floor: [2N] in global row order; W [2N, 2N]) in float64."""
    hs = [np.asarray(h, dtype=np.float64) for h in hiddens]
    R, n = len(hs), hs[0].shape[0] // 2
    N = R * n
    M, a = 2.0 * N - 2.0, 1.0 / float(temperature)
    assert N >= 2 and beta >= 0 and 0 <= tau_plus < 1
    if hidden_norm:
        zs, nrms = zip(*[l2_normalize(h) for h in hs])
    else:
        zs, nrms = hs, [None] * R
    z_all = z_all_of(zs, n)
    own, pos, neg = _masks(N)
    S = z_all @ z_all.T
    spos = S[pos]
    # relative to exp(c), c = the row's largest exponent: nothing overflows at any temperature
    e1 = np.where(neg, (1.0 + beta) * a * S, -np.inf)
    e0 = np.where(neg, beta * a * S, -np.inf)
    m1, m0 = e1.max(1, keepdims=True), e0.max(1, keepdims=True)
    x1, x0 = np.exp(e1 - m1), np.exp(e0 - m0)
    logA, logB = m1[:, 0] + np.log(x1.sum(1)), m0[:, 0] + np.log(x0.sum(1))
    P1, P0 = x1 / x1.sum(1, keepdims=True), x0 / x0.sum(1, keepdims=True)
    logr, logp = np.log(M) + logA - logB, a * spos
    c = np.maximum(logr, logp)
    er, ep = np.exp(logr - c), np.exp(logp - c)
    graw = (er - tau_plus * M * ep) / (1.0 - tau_plus)
    flo = M * np.exp(-a - c)
    on_floor = ~(graw > flo)
    G = np.where(on_floor, flo, graw)
    den = ep + G
    row = c + np.log(den) - logp
    w = np.where(on_floor, 0.0, er / ((1.0 - tau_plus) * den))
    wpos = np.where(on_floor, a * (ep / den - 1.0), a * (ep * (1.0 - tau_plus * M / (1.0 - tau_plus)) / den - 1.0))
    W = a * w[:, None] * ((1.0 + beta) * P1 - beta * P0)
    W[pos] = wpos
    W[own] = 0.0
    g_all = (W + W.T) @ z_all / (R * n)
    loss, share, grads = [], [], []
    for r in range(R):
        rows = replica_rows(r, n, N)
        loss.append(float(row[rows].sum() / n))
        share.append(float(on_floor[rows].sum() / (2.0 * n)))
        dz = g_all[rows]
        if hidden_norm:
            dz = (dz - zs[r] * (zs[r] * dz).sum(axis=1, keepdims=True)) / nrms[r]
        grads.append(dz)
    return dict(loss=loss, floor_share=share, grads=grads, row=row, on_floor=on_floor, ratio=graw / flo, W=W)


def kink_distance(ref):
    """The smallest |G_raw / floor - 1| over all rows of a reference result."""
    return float(np.abs(ref['ratio'] - 1.0).min())


# ---------------------------------------------------------------------------------------------------------------- float32 emulation
def _seq_matmul_f32(A, B):
    """A [m, K] B^T [K, c] with ONE float32 accumulator per entry, k in order, every product and every sum rounded to float32: the
    worst case of the MFMA k loop (which keeps at least this much)."""
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    acc = np.zeros((A.shape[0], B.shape[0]), np.float32)
    for k in range(A.shape[1]):
        acc = acc + A[:, k:k + 1] * B[None, :, k]
    return acc


def _online_lse2(t, live):
    """sweep::ml_push over the live columns of every row in column order, all in float32 -> (m, l)."""
    one = np.float32
    m = np.full(t.shape[0], -np.inf, one)
    l = np.zeros(t.shape[0], one)
    with np.errstate(invalid='ignore'):
        for k in range(t.shape[1]):
            x = t[:, k]
            mn = np.maximum(m, x)
            ln = (l * np.where(np.isfinite(m), np.exp2(m - mn), one(0))).astype(one) + np.exp2(x - mn).astype(one)
            m, l = np.where(live[:, k], mn, m).astype(one), np.where(live[:, k], ln, l).astype(one)
    return m, l


def hcl_emulated(zs, rank, temperature, beta, tau_plus, dots=None):
    """The float32 arithmetic of csrc/hcl.hip on float32 blocks zs (used as they are: the kernels take normalised rows) for replica
    `rank`: float32 dot products, the two base-2 logits each rounded once, online (max, sum) in float32, the row finalize in double,
    float32 coefficients and log-sum-exps for the backward, float32 gradient products; grad_scale = 1 / R.  `dots`: the per-replica
    dot products of an earlier call on the same data.  -> dict(loss (float32 value), floor_share, on_floor [2n] of `rank`,
    grad [2n, D] = d objective / d z_rank, dots)."""
    one = np.float32
    zs = [np.asarray(z, one) for z in zs]
    R, n = len(zs), zs[0].shape[0] // 2
    N = R * n
    T, beta, tau = f32(temperature), f32(beta), f32(tau_plus)
    M, a = 2.0 * N - 2.0, 1.0 / T
    hard = beta != 0.0
    scale1, scale0 = one((1.0 + beta) * LOG2E / T), one(beta * LOG2E / T)
    beta1, beta_f = one(1.0) + one(beta), one(beta)
    z_all = z_all_of(zs, n)
    own_all, pos_all, neg_all = _masks(N)
    if dots is None:
        dots = [_seq_matmul_f32(z, z_all) for z in zs]
    coeff = one((1.0 / R) / n)
    total = np.zeros_like(zs[rank])
    res = {}
    for q in range(R):
        rows = replica_rows(q, n, N)
        S, own, pos, neg = dots[q], own_all[rows], pos_all[rows], neg_all[rows]
        t1, t0 = (S * scale1).astype(one), (S * scale0).astype(one)
        m1, l1 = _online_lse2(t1, neg)
        lse1 = m1.astype(np.float64) + np.log2(l1.astype(np.float64))
        if hard:
            m0, l0 = _online_lse2(t0, neg)
            lse0 = m0.astype(np.float64) + np.log2(l0.astype(np.float64))
        else:
            lse0 = np.full(2 * n, np.log2(M))
        logr, logp = np.log(M) + (lse1 - lse0) * LN2, a * S[pos].astype(np.float64)
        c = np.maximum(logr, logp)
        er, ep = np.exp(logr - c), np.exp(logp - c)
        graw = (er - tau * M * ep) / (1.0 - tau)
        flo = M * np.exp(-a - c)
        fl = ~(graw > flo)
        G = np.where(fl, flo, graw)
        den = ep + G
        row = c + np.log(den) - logp
        cneg = np.where(fl, 0.0, a * er / ((1.0 - tau) * den)).astype(one)
        cpos = np.where(fl, a * (ep / den - 1.0), a * (ep * (1.0 - tau * M / (1.0 - tau)) / den - 1.0)).astype(one)
        w = (cneg * beta1).astype(one)[:, None] * np.exp2(t1 - lse1.astype(one)[:, None]).astype(one)
        if hard:
            w = w.astype(one) - (cneg * beta_f).astype(one)[:, None] * np.exp2(t0 - lse0.astype(one)[:, None]).astype(one)
        ds = np.where(pos, cpos[:, None], w).astype(one)
        ds[own] = 0
        dz_all = _seq_matmul_f32(ds.T, zs[q].T) * coeff
        total += dz_all[replica_rows(rank, n, N)]
        if q == rank:
            total += _seq_matmul_f32(ds, z_all.T) * coeff
            res = dict(loss=one(row.sum() / n), floor_share=float(fl.sum() / (2.0 * n)), on_floor=fl)
    assert total.dtype == one
    res.update(grad=total, dots=dots)
    return res


def relative_errors(got_loss, got_grad, ref, rank):
    """|got - ref| of the loss relative to the loss and of the gradient relative to its largest entry, for replica `rank`."""
    g = ref['grads'][rank]
    return dict(loss=abs(float(got_loss) - ref['loss'][rank]) / abs(ref['loss'][rank]),
                grad=float(np.abs(np.asarray(got_grad, np.float64) - g).max() / np.abs(g).max()))


def case_reference(shape, family, params):
    """The float64 reference of one kernel case on its float32 inputs (hidden_norm=False: the kernels take the rows as they are) with
    the scalars as they cross the C ABI.  -> (zs, ref)"""
    n, R, D, rank = shape
    T, beta, tau_plus = params
    zs = case_views(n, R, D, family, CASE_SEED[(shape, family)])
    return zs, hcl_reference(zs, f32(T), f32(beta), f32(tau_plus), hidden_norm=False)


def measured_budget(shapes=SHAPES):
    """Re-measures EMULATION_ERROR (and, per case, the smallest distance of any row to the kink over PARAMS)."""
    out, dist = {}, {}
    for shape in shapes:
        for family in FAMILIES:
            worst, near, dots = dict(loss=0.0, grad=0.0), np.inf, None
            for params in PARAMS:
                zs, ref = case_reference(shape, family, params)
                near = min(near, kink_distance(ref))
                emu = hcl_emulated(zs, shape[3], *params, dots=dots)
                dots = emu['dots']
                for k, e in relative_errors(emu['loss'], emu['grad'], ref, shape[3]).items():
                    worst[k] = max(worst[k], e)
            out[(shape, family)], dist[(shape, family)] = worst, near
    return out, dist
