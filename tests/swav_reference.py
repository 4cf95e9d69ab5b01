"""numpy restatement of the SwAV pieces (Caron et al. 2020, Unsupervised Learning of Visual Features by Contrasting Cluster
Assignments): the Sinkhorn-Knopp assignment as scaling potentials, the official iteration transcribed, the codes, the loss with the code
entropy and both analytic gradients in float64 (or, for the error budget, in float32), the autograd gradients with and without the
stop-gradient on the codes, and the freeze boundary.

Conventions of simclr_amd.objective.add_swav_loss: q [2b, D] is the online projection output, [view a; view b]; row r pairs with row
p(r) = (r + b) mod 2b; v [K, D] is the RAW prototype variable, w its row-normalised form; normalisation is tf.math.l2_normalize
(x / sqrt(max(sum x^2, 1e-12))).  z_all [2N, D] is the gathered normalised batch, view-major.
  L_gj = z_g . w_j / eps,  beta^(0) = 0,  it = 1 .. I:
    alpha^v_j = -ln K - logsumexp_{g in view v}(L_gj + beta_g);   for it < I: beta_g = -ln N - logsumexp_j(L_gj + alpha^{v(g)}_j)
  code of row g = softmax_j(L_gj + alpha^{v(g)}_j)
  s_rj = qhat_r . w_j / T,   t_rj = qhat_r . w_j / eps + alpha^{v(r)}_j,   Ps = softmax_j(s_r),   Pt = softmax_j(t_r)
  l_r = logsumexp_j(s_r) - sum_j Pt[p(r), j] s_rj,   loss = (1 / 2b) sum_r l_r,   entropy = (1 / 2b) sum_r H(Pt[r])
  alpha and Pt get no gradient (the codes are stop-gradient)."""
import numpy as np

EPS = 1e-12
GATE_LOSS, GATE_GRAD = 1e-5, 2e-4           # the project's gates for this arithmetic (tests/golden/DINO_HAND_DERIVED.md, "Error budget")
# worst float32-emulation error of alpha over SINK_CASES in nats, as tests/test_swav_reference.py re-measures it
# (tests/golden/SWAV_HAND_DERIVED.md, "Error budget"); the alpha tolerance of tests/test_gpu_swav.py is 4x this
ALPHA_EMULATION_ERROR = 3.5e-6
ALPHA_TOL = 4.0 * ALPHA_EMULATION_ERROR


def l2_normalize(x, dtype=np.float64):
    x = np.asarray(x, dtype)
    ss = (x * x).sum(-1, keepdims=True)
    return x / np.sqrt(np.maximum(ss, dtype(EPS))), ss


def l2_normalize_bwd(xh, ss, g):
    """Gradient through l2_normalize: (g - xh (xh . g)) / norm; a row with sum x^2 < 1e-12 has the constant norm 1e-6."""
    radial = np.where(ss >= EPS, (xh * g).sum(-1, keepdims=True), 0.0)
    return (g - xh * radial) / np.sqrt(np.maximum(ss, EPS))


def pair(x):
    """Row r reads row (r + b) mod 2b."""
    return np.roll(x, -(x.shape[0] // 2), axis=0)


def logsumexp(x, axis):
    m = x.max(axis=axis, keepdims=True)
    return (m + np.log(np.exp(x - m).sum(axis=axis, keepdims=True))).squeeze(axis)


def sinkhorn_potentials(z_all, w, epsilon=0.05, iters=3, dtype=np.float64):
    """-> (alpha [2, K], beta [2N]) in nats after `iters` iterations, beta^(0) = 0; beta is the one the LAST column step read.
    dtype=float32: every array operation rounds to float32 (the error budget of this arithmetic, not the kernel's operation order)."""
    f = dtype
    z_all, w = np.asarray(z_all, f), np.asarray(w, f)
    rows, K = z_all.shape[0], w.shape[0]
    assert rows >= 2 and rows % 2 == 0 and K >= 2 and iters >= 1
    N = rows // 2
    L = (z_all @ w.T) / f(epsilon)
    beta = np.zeros(rows, f)
    alpha = np.zeros((2, K), f)
    for it in range(1, iters + 1):
        x = L + beta[:, None]
        for v in range(2):
            alpha[v] = -f(np.log(K)) - logsumexp(x[v * N:(v + 1) * N], 0)
        if it < iters:
            beta = -f(np.log(N)) - logsumexp(L + np.repeat(alpha, N, axis=0), 1)
    return alpha.astype(f), beta.astype(f)


def sinkhorn_official(scores, epsilon=0.05, iters=3, initial_normalisation=True):
    """The official distributed_sinkhorn on ONE view's scores [N, K] (world size 1), transcribed operation by operation in float64:
    Q = exp(scores / eps).T; Q /= sum(Q); iters x {Q /= row sums; Q /= K; Q /= column sums; Q /= N}; Q *= N; return Q.T
    -> the codes [N, K] (rows sum to 1)."""
    Q = np.exp(np.asarray(scores, np.float64) / epsilon).T          # [K, N]
    K, N = Q.shape
    if initial_normalisation:
        Q = Q / Q.sum()
    for _ in range(iters):
        Q = Q / Q.sum(axis=1, keepdims=True)
        Q = Q / K
        Q = Q / Q.sum(axis=0, keepdims=True)
        Q = Q / N
    Q = Q * N
    return Q.T


def official_alpha(scores, epsilon=0.05, iters=3, initial_normalisation=True):
    """The column scaling the official iteration ends with, in nats: log of the product of every per-prototype factor it applied to
    prototype j's row of Q.  The initial Q /= sum(Q) is one factor for the whole matrix -- the start beta^(0) = -ln sum(Q) of the ROW
    scaling -- so with it alpha comes out shifted by the constant +ln sum(Q); without it, it is alpha itself (beta^(0) = 0)."""
    Q = np.exp(np.asarray(scores, np.float64) / epsilon).T
    K, N = Q.shape
    a = np.zeros(K)
    if initial_normalisation:
        Q = Q / Q.sum()
    for _ in range(iters):
        r = Q.sum(axis=1, keepdims=True)
        a -= np.log(r[:, 0]) + np.log(K)
        Q = Q / r / K
        Q = Q / Q.sum(axis=0, keepdims=True) / N
    return a


def codes(z, w, alpha, epsilon=0.05, dtype=np.float64):
    """softmax_j(z_g . w_j / eps + alpha^{v(g)}_j) for the view-major block z [2n, D]."""
    f = dtype
    z, w, alpha = np.asarray(z, f), np.asarray(w, f), np.asarray(alpha, f)
    n = z.shape[0] // 2
    t = (z @ w.T) / f(epsilon) + np.repeat(alpha, n, axis=0)
    return np.exp(t - logsumexp(t, 1)[:, None])


def softmax_stats(t):
    """Rows of logits -> (m, rest, a): the maximum, the NON-maximum mass sum_{others} exp(t - m) (one instance of the maximum left
    out), and sum exp(t - m) (t - m), every term <= 0."""
    m = t.max(-1)
    e = np.exp(t - m[:, None])
    first = np.zeros_like(e, dtype=bool)
    first[np.arange(t.shape[0]), t.argmax(-1)] = True
    rest = np.where(first, 0.0, e).sum(-1)
    a = (e * (t - m[:, None])).sum(-1)
    return m, rest, a


def swav_loss_normalized(qh, w, alpha, temperature=0.1, epsilon=0.05, grad_scale=1.0, dtype=np.float64):
    """The loss on rows that are normalised already and a GIVEN alpha (what simclr_swav_fwd / _bwd_q / _bwd_w take).
    -> dict(loss, entropy, rows [2b] (l_r), row_entropy [2b], u [2b, D] = Pt . w, grad_q [2b, D], grad_w [K, D], Ps, Pt, lse_s, lse_t,
    smax / tmax = the largest |logit| of either side)."""
    f = dtype
    qh, w, alpha = (np.asarray(x, f) for x in (qh, w, alpha))
    assert qh.ndim == 2 and qh.shape[0] % 2 == 0 and qh.shape[0] >= 2 and alpha.shape == (2, w.shape[0])
    rows = qh.shape[0]
    dots = qh @ w.T
    s = dots / f(temperature)
    t = dots / f(epsilon) + np.repeat(alpha, rows // 2, axis=0)
    ms, rs, _ = softmax_stats(s)
    mt, rt, at = softmax_stats(t)
    lse_s = ms + np.log1p(rs)
    lse_t = mt + np.log1p(rt)
    Ps = np.exp(s - lse_s[:, None])
    Pt = np.exp(t - lse_t[:, None])
    row_entropy = np.log1p(rt) - at / (f(1.0) + rt)              # log(sum) - sum e^(t-m)(t-m) / sum: two non-negative terms
    u = Pt @ w
    l = lse_s - (qh * pair(u)).sum(-1) / f(temperature)
    coeff = f(grad_scale) / (f(rows) * f(temperature))
    grad_q = (Ps @ w - pair(u)) * coeff
    grad_w = ((Ps - pair(Pt)).T @ qh) * coeff
    return dict(loss=l.sum() / f(rows), entropy=row_entropy.sum() / f(rows), rows=l, row_entropy=row_entropy, u=u, grad_q=grad_q,
                grad_w=grad_w, Ps=Ps, Pt=Pt, lse_s=lse_s, lse_t=lse_t, smax=np.abs(s).max(), tmax=np.abs(t).max())


def swav_loss(q, v, temperature=0.1, epsilon=0.05, iters=3, grad_scale=1.0, z_all=None):
    """The loss on raw projections q [2b, D] and the raw prototype variable v [K, D].  z_all: the gathered NORMALISED batch the Sinkhorn
    runs on (default: the normalised local rows: one replica).  -> as swav_loss_normalized plus grad_q / grad_v through the row
    normalisations, qh, w and alpha."""
    qh, ssq = l2_normalize(q)
    w, ssw = l2_normalize(v)
    alpha, _ = sinkhorn_potentials(qh if z_all is None else z_all, w, epsilon, iters)
    out = swav_loss_normalized(qh, w, alpha, temperature, epsilon, grad_scale)
    out['grad_qhat'], out['grad_w_hat'] = out['grad_q'], out['grad_w']
    out['grad_q'] = l2_normalize_bwd(qh, ssq, out['grad_qhat'])
    out['grad_v'] = l2_normalize_bwd(w, ssw, out['grad_w_hat'])
    out.update(qh=qh, w=w, alpha=alpha)
    return out


def gather_view_major(blocks):
    """comm.gather_hidden's layout: replica blocks [2b, D] (each [view a; view b]) -> [2N, D] = [every replica's view a; every view b]."""
    b = blocks[0].shape[0] // 2
    return np.concatenate([x[:b] for x in blocks] + [x[b:] for x in blocks])


def autograd_gradients(qh, w, temperature=0.1, epsilon=0.05, iters=3, detach=True):
    """float64 torch autograd of the DIRECT form on one replica (the Sinkhorn on the rows themselves): the potentials by the iteration,
    the codes as their softmax, loss = mean_r [logsumexp(s_r) - sum_j code[p(r), j] s_rj].  detach=True: the codes are constants (the
    official `with torch.no_grad()`); detach=False: the gradient that also flows through the Sinkhorn.  -> (loss, grad_q, grad_w)."""
    import torch
    q = torch.tensor(np.asarray(qh, np.float64), requires_grad=True)
    p = torch.tensor(np.asarray(w, np.float64), requires_grad=True)
    rows, K = q.shape[0], p.shape[0]
    N = rows // 2
    dots = q @ p.T
    L = dots / epsilon
    beta = torch.zeros(rows, dtype=torch.float64)
    for it in range(1, iters + 1):
        x = L + beta[:, None]
        alpha = torch.stack([-np.log(K) - torch.logsumexp(x[v * N:(v + 1) * N], 0) for v in range(2)])
        if it < iters:
            beta = -np.log(N) - torch.logsumexp(L + alpha.repeat_interleave(N, 0), 1)
    code = torch.softmax(L + alpha.repeat_interleave(N, 0), 1)
    if detach:
        code = code.detach()
    s = dots / temperature
    loss = (torch.logsumexp(s, 1) - (torch.roll(code, -N, 0) * s).sum(1)).mean()
    loss.backward()
    return float(loss.detach()), q.grad.numpy(), p.grad.numpy()


def prototypes_frozen(step, steps_per_epoch, freeze_epochs=1):
    return int(step) < int(freeze_epochs) * int(steps_per_epoch)


# ---- the kernel cases shared by tests/test_swav_reference.py (error budget) and tests/test_gpu_swav.py --------------------------------
# Sinkhorn: (N, K, D, eps, I, concentrated).  N: 1 (every code uniform), 3, 33 and 70 (the view boundary inside a 64-row tile), 64 (on a
# tile edge); K: the smallest table, a ragged single tile, one row past a tile, several tiles with a ragged last one, 65 tiles (several
# key splits of the row sweep); I = 1 (the column sweep alone), 2 (one row sweep), 3; every width; both eps.  (33, 2) and (70, 63) have
# 2 and 3 row splits of the column sweep.  Concentrated: every row near one of three prototypes, alpha spans more than 15 nats.
SINK_CASES = [(1, 2, 64, 0.05, 1, False), (1, 63, 128, 1.0, 3, False), (1, 4097, 256, 0.05, 2, False), (3, 65, 256, 1.0, 3, False),
              (3, 200, 64, 0.05, 3, False), (3, 4097, 128, 0.05, 3, False), (33, 2, 128, 0.05, 3, False), (33, 63, 256, 0.05, 2, False),
              (33, 200, 64, 1.0, 1, False), (33, 4097, 64, 0.05, 3, False), (64, 65, 64, 0.05, 3, False), (64, 200, 128, 0.05, 2, False),
              (70, 65, 64, 0.05, 3, False), (70, 200, 128, 0.05, 3, True), (70, 63, 256, 1.0, 3, False), (70, 63, 128, 0.05, 3, True),
              (70, 63, 64, 0.05, 1, False)]
# loss: (b, K, D, T, eps, concentrated), alpha from the float64 Sinkhorn (I = 3) on the rows themselves
LOSS_CASES = [(1, 2, 64, 0.1, 0.05, False), (1, 63, 128, 1.0, 1.0, False), (1, 4097, 256, 0.1, 0.05, False), (3, 65, 256, 1.0, 1.0, False),
              (3, 200, 64, 0.1, 0.05, False), (3, 4097, 128, 1.0, 1.0, False), (33, 2, 128, 0.1, 0.05, False), (33, 63, 256, 0.1, 0.05, False),
              (33, 200, 64, 1.0, 1.0, False), (33, 4097, 64, 0.1, 0.05, False), (70, 65, 64, 0.1, 0.05, False),
              (70, 200, 128, 0.1, 0.05, True), (70, 63, 256, 1.0, 1.0, False)]


def case_inputs(n, K, D, concentrated=False):
    """Unit float32 rows [2n, D], view b correlated with view a, and unit float32 prototypes [K, D].  concentrated: every row within
    0.05 noise of one of the first three prototypes."""
    g = np.random.default_rng(1000 * n + K + D + (7 if concentrated else 0))
    unit = lambda x: l2_normalize(x)[0].astype(np.float32)
    w = unit(g.standard_normal((K, D)))
    if concentrated:
        pick = g.integers(0, min(3, K), size=2 * n)
        z = unit(w[pick] + 0.05 * g.standard_normal((2 * n, D)) / np.sqrt(D))
    else:
        a = g.standard_normal((n, D))
        z = unit(np.concatenate([a, a + 0.5 * g.standard_normal((n, D))]))
    return z, w


def loss_case_inputs(b, K, D, T, eps, concentrated=False):
    """-> (qh, w, alpha float32 [2, K]): alpha is the float64 Sinkhorn's (I = 3) on the rows themselves, rounded to float32 ONCE -- the
    loss kernels and the restatement read the same float32 alpha, so a Sinkhorn error cannot hide a loss error."""
    qh, w = case_inputs(b, K, D, concentrated)
    alpha, _ = sinkhorn_potentials(qh, w, eps, 3)
    return qh, w, alpha.astype(np.float32)


def alpha_emulation_error(N, K, D, eps, iters, concentrated):
    z, w = case_inputs(N, K, D, concentrated)
    a64, _ = sinkhorn_potentials(z, w, eps, iters)
    a32, _ = sinkhorn_potentials(z, w, eps, iters, dtype=np.float32)
    return float(np.abs(a32.astype(np.float64) - a64).max())


def case_gates(b, K, D, T, eps, concentrated=False):
    """The gates of one loss case, relative to the reference tensor's maximum: the project's, or 4x the error of the float32 emulation of
    the restatement where that emulation alone uses more than a quarter of the project's.  -> dict(name -> (gate, emulation error))."""
    return gates_of_inputs(*loss_case_inputs(b, K, D, T, eps, concentrated), T, eps)


def gates_of_inputs(qh, w, alpha, T, eps):
    """case_gates for given inputs."""
    x = (qh, w, alpha)
    r64 = swav_loss_normalized(*x, T, eps)
    r32 = swav_loss_normalized(*x, T, eps, dtype=np.float32)
    out = {}
    for name, project in (('loss', GATE_LOSS), ('entropy', GATE_LOSS), ('grad_q', GATE_GRAD), ('grad_w', GATE_GRAD), ('u', GATE_GRAD)):
        ref = np.asarray(r64[name], np.float64)
        err = float(np.abs(np.asarray(r32[name], np.float64) - ref).max() / np.abs(ref).max())
        out[name] = (4.0 * err if err > project / 4.0 else project, err)
    return out
