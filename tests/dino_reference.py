"""numpy restatement of the DINO pieces (Caron et al. 2021, Emerging Properties in Self-Supervised Vision Transformers): the loss with
the teacher entropy and the analytic gradients in float64 (or, for the error budget, in float32), the centre update, the teacher
temperature schedule, the freeze boundary, and a float32 emulation of the two ways to form a row's entropy.

Conventions of simclr_amd.objective.add_dino_loss: q [2b, D] is the online projection output, k [2b, D] the target network's, row r
of q pairs with row p(r) = (r + b) mod 2b of k; vs / vt [K, D] are the RAW prototype variables of the two networks, ws / wt their
row-normalised forms; normalisation is tf.math.l2_normalize (x / sqrt(max(sum x^2, 1e-12))); c [K] is the centre.
  s_rj = qhat_r . ws_j / Ts,   t_rj = (khat_r . wt_j - c_j) / Tt,   Ps = softmax_j(s_r),   Pt = softmax_j(t_r)
  l_r = logsumexp_j(s_r) - sum_j Pt[p(r), j] s_rj,   loss = (1 / 2b) sum_r l_r   (the mean over the two cross-view terms)
  entropy = (1 / 2b) sum_r H(Pt[r]);   k, wt and c get no gradient."""
import math

import numpy as np

EPS = 1e-12
GATE_LOSS, GATE_GRAD = 1e-5, 2e-4           # the project's gates for this arithmetic (tests/test_gpu_moco.py, tests/test_gpu_supcon.py)


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


def dino_loss_normalized(qh, kh, ws, wt, c, student_temp=0.1, teacher_temp=0.04, grad_scale=1.0, dtype=np.float64):
    """The loss on rows that are normalised already (what simclr_dino_fwd / _bwd_q / _bwd_w take).
    -> dict(loss, entropy, rows [2b] (l_r), row_entropy [2b], u [2b, D] = Pt . ws, grad_q [2b, D], grad_ws [K, D], Ps, Pt), in `dtype`
    (float32: every array operation rounds to float32 -- the error budget of this arithmetic, not the kernel's operation order)."""
    f = dtype
    qh, kh, ws, wt, c = (np.asarray(x, f) for x in (qh, kh, ws, wt, c))
    assert qh.ndim == 2 and qh.shape == kh.shape and qh.shape[0] % 2 == 0 and qh.shape[0] >= 2
    assert ws.shape == wt.shape and ws.shape[0] >= 2 and c.shape == (ws.shape[0],)
    rows = qh.shape[0]
    s = (qh @ ws.T) / f(student_temp)
    t = ((kh @ wt.T) - c[None, :]) / f(teacher_temp)
    ms, rs, _ = softmax_stats(s)
    mt, rt, at = softmax_stats(t)
    lse_s = ms + np.log1p(rs)
    lse_t = mt + np.log1p(rt)
    Ps = np.exp(s - lse_s[:, None])
    Pt = np.exp(t - lse_t[:, None])
    row_entropy = np.log1p(rt) - at / (f(1.0) + rt)              # log(sum) - sum e^(t-m)(t-m) / sum: two non-negative terms
    u = Pt @ ws
    l = lse_s - (qh * pair(u)).sum(-1) / f(student_temp)
    coeff = f(grad_scale) / (f(rows) * f(student_temp))
    grad_q = (Ps @ ws - pair(u)) * coeff
    grad_ws = ((Ps - pair(Pt)).T @ qh) * coeff
    return dict(loss=l.sum() / f(rows), entropy=row_entropy.sum() / f(rows), rows=l, row_entropy=row_entropy, u=u, grad_q=grad_q,
                grad_ws=grad_ws, Ps=Ps, Pt=Pt, lse_s=lse_s, lse_t=lse_t)


def dino_loss(q, k, vs, vt, c, student_temp=0.1, teacher_temp=0.04, grad_scale=1.0):
    """The loss on raw projections and raw prototype variables -> as dino_loss_normalized plus grad_q / grad_vs through the row
    normalisations, qh / kh / ws / wt and kbar = the mean of the rows of kh."""
    qh, ssq = l2_normalize(q)
    kh, _ = l2_normalize(k)
    ws, ssw = l2_normalize(vs)
    wt, _ = l2_normalize(vt)
    out = dino_loss_normalized(qh, kh, ws, wt, c, student_temp, teacher_temp, grad_scale)
    out['grad_qhat'], out['grad_ws_hat'] = out['grad_q'], out['grad_ws']
    out['grad_q'] = l2_normalize_bwd(qh, ssq, out['grad_qhat'])
    out['grad_vs'] = l2_normalize_bwd(ws, ssw, out['grad_ws_hat'])
    out.update(qh=qh, kh=kh, ws=ws, wt=wt, kbar=kh.mean(0))
    return out


def center_blend_f32(center, batch_center, momentum):
    """The fp32 blend of simclr_dino_center: c + (1 - m) (x - c) with three separate roundings; 1 - m is formed in double from the
    float32 momentum and cast once."""
    f = np.float32
    omm = f(1.0 - float(f(momentum)))
    c = np.asarray(center, f)
    d = (np.asarray(batch_center, f) - c).astype(f)
    return (c + (omm * d).astype(f)).astype(f)


def center_update(center, wt, kh_all, momentum):
    """c <- m c + (1 - m) mean over ALL rows of (khat . wt_j), the column mean of the uncentred teacher logits in float64, rounded to
    float32 once and blended in float32."""
    logits = np.asarray(kh_all, np.float64) @ np.asarray(wt, np.float64).T
    return center_blend_f32(center, logits.mean(0).astype(np.float32), momentum)


def teacher_temp(step, steps_per_epoch, final=0.04, warmup=0.04, warmup_epochs=0):
    """Linear from `warmup` to `final` over warmup_epochs * steps_per_epoch steps, then constant; in double, cast to float32 once."""
    n = int(warmup_epochs) * int(steps_per_epoch)
    if n <= 0 or int(step) >= n:
        return float(np.float32(float(final)))
    return float(np.float32(float(warmup) + (float(final) - float(warmup)) * (float(int(step)) / float(n))))


def last_layer_frozen(step, steps_per_epoch, freeze_epochs=1):
    return int(step) < int(freeze_epochs) * int(steps_per_epoch)


def entropy_f32(t, stable=True):
    """float32 emulation of a row's entropy from float32 logits t [rows, K] (natural-log domain), every operation rounded to float32,
    the sums as one running float32 sum per row.
    stable: the non-maximum mass kept apart, H = log1p(rest) - sum e^(t-m)(t-m) / (1 + rest) -- the kernel's form (which finishes in
            double: this emulation is its float32 worst case);
    naive:  H = logsumexp(t) - sum softmax(t) t, the difference of two numbers of the size of max t."""
    f = np.float32
    t = np.asarray(t, f)
    m = t.max(-1).astype(f)
    am = t.argmax(-1)
    rest, a, total, et = (np.zeros(t.shape[0], f) for _ in range(4))
    for j in range(t.shape[1]):
        x = (t[:, j] - m).astype(f)
        e = np.exp(x).astype(f)
        rest = (rest + np.where(am == j, f(0), e)).astype(f)
        a = (a + (e * x).astype(f)).astype(f)
        total = (total + e).astype(f)
        et = (et + (e * t[:, j]).astype(f)).astype(f)
    if stable:
        return (np.log1p(rest).astype(f) - (a / (f(1) + rest).astype(f)).astype(f)).astype(f)
    lse = (m + np.log(total).astype(f)).astype(f)
    return (lse - (et / total).astype(f)).astype(f)


# ---- the kernel cases shared by tests/test_dino_reference.py (error budget) and tests/test_gpu_dino.py -------------------------------
# (b, K, D, Ts, Tt).  b: rows 2 .. 140 -- below, across and past one 64-row block, the partner row in another workgroup; K: the
# smallest table, a ragged single tile, one row past a tile, several tiles with a ragged last one, 65 tiles with one row in the last
# (more than one key split); both temperature pairs; every width.  b = 33, K = 2 is the smallest shape with two row splits.
CASES = [(1, 2, 64, 0.1, 0.04), (1, 63, 128, 1.0, 1.0), (1, 4097, 256, 0.1, 0.04), (3, 65, 256, 1.0, 1.0), (3, 200, 64, 0.1, 0.04),
         (3, 4097, 128, 1.0, 1.0), (33, 2, 128, 0.1, 0.04), (33, 63, 256, 0.1, 0.04), (33, 200, 64, 1.0, 1.0), (33, 4097, 64, 0.1, 0.04),
         (70, 65, 64, 0.1, 0.04), (70, 200, 128, 0.1, 0.04), (70, 63, 256, 1.0, 1.0)]


def case_inputs(b, K, D, Ts, Tt):
    """Unit float32 rows: keys correlated with their queries' other view, target prototypes near the online ones (a momentum copy),
    a non-zero centre of the size of the logits' spread."""
    g = np.random.default_rng(1000 * b + K + D)
    unit = lambda x: l2_normalize(x)[0].astype(np.float32)
    qh = unit(g.standard_normal((2 * b, D)))
    kh = unit(qh + 0.5 * g.standard_normal((2 * b, D)))
    ws = unit(g.standard_normal((K, D)))
    wt = unit(ws + 0.1 * g.standard_normal((K, D)))
    c = (0.05 * g.standard_normal(K)).astype(np.float32)
    return qh, kh, ws, wt, c


def case_gates(b, K, D, Ts, Tt):
    """The gates of one case, relative to the reference tensor's maximum: the project's, or 4x the error of the float32 emulation of
    the restatement (the rule of tests/augment_reference.py) where that emulation alone uses more than a quarter of the project's.
    -> dict(name -> (gate, emulation error))."""
    x = case_inputs(b, K, D, Ts, Tt)
    r64 = dino_loss_normalized(*x, Ts, Tt)
    r32 = dino_loss_normalized(*x, Ts, Tt, dtype=np.float32)
    out = {}
    for name, project in (('loss', GATE_LOSS), ('entropy', GATE_LOSS), ('grad_q', GATE_GRAD), ('grad_ws', GATE_GRAD), ('u', GATE_GRAD)):
        ref = np.asarray(r64[name], np.float64)
        err = float(np.abs(np.asarray(r32[name], np.float64) - ref).max() / np.abs(ref).max())
        out[name] = (4.0 * err if err > project / 4.0 else project, err)
    return out
