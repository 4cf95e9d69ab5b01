"""numpy restatement of SwAV's multi-crop loss (Caron et al. 2020, section 4; the official main_swav.py loop with
crops_for_assign = [0, 1]) in the form the kernels of csrc/swav_multicrop.hip compute, beside a transcription of the official loop,
float64 autograd with and without the stop-gradient, and the float32 emulation that supplies the GPU tolerances.

Conventions of simclr_amd.objective.add_swav_local_loss: qh [2b, D] = the normalised GLOBAL rows, [view a; view b]; xh [L b, D] = the
normalised LOCAL rows, view-major (row v b + i = local view v of image i); w [K, D] the row-normalised prototypes; alpha [2, K] the
potentials of the Sinkhorn on the global rows alone; V = 2 + L.
  Pt[g] = softmax_j(qh_g . w_j / eps + alpha[v(g)][j])  (the code, no gradient),   u_g = sum_j Pt[g, j] w_j
  s_rj = row . w_j / T
  loss = 1 / (2 (V-1) b) [ sum_{r < 2b} (lse(s_r) - qh_r . u_p(r) / T) + sum_{local r} (2 lse(s_r) - xh_r . (u_i + u_{b+i}) / T) ],  i = r mod b
  m_g = sum_v xh_{v b + (g mod b)}
  d/dxh_r = c (2 sum_j Ps[r, j] w_j - u_i - u_{b+i}),  d/dw_j (local share) = c (sum_r 2 Ps[r, j] xh_r - sum_g Pt[g, j] m_g),  c = 1 / (2 (V-1) b T)"""
import numpy as np

from tests import swav_reference as sr

LOG2E = 1.4426950408889634
# worst float32-emulation error of the restatement over MC_CASES, relative to the reference tensor's largest magnitude, as
# tests/test_swav_multicrop_reference.py re-measures it (tests/golden/SWAV_MULTICROP_HAND_DERIVED.md, "Error budget"); the tolerances
# of tests/test_gpu_swav_multicrop.py are 4x these
EMULATION_ERROR = dict(loss=2.5e-7, row_stats=1.7e-7, grad_x=1.9e-6, grad_w=2.75e-6)
TOL = {k: 4.0 * v for k, v in EMULATION_ERROR.items()}


def local_loss_normalized(xh, w, u, b, temperature=0.1, grad_scale=1.0, dtype=np.float64, shift=0):
    """The LOCAL share on normalised rows and GIVEN code expectations u [2b, D] (what simclr_swav_local_fwd / _bwd_x take).
    shift: pair local row r with image (i + shift) mod b (the mis-pairing probe).
    -> dict(loss = the local sum / (2 (V-1) b), rows [L b], lse [L b] in nats, Ps, grad_x [L b, D], student_w [K, D] = c sum_r 2 Ps x_r)."""
    f = dtype
    xh, w, u = (np.asarray(a, f) for a in (xh, w, u))
    rows = xh.shape[0]
    assert rows % b == 0 and u.shape[0] == 2 * b
    L = rows // b
    img = (np.arange(rows) % b + shift) % b
    s = (xh @ w.T) / f(temperature)
    ms, rs, _ = sr.softmax_stats(s)
    lse = ms + np.log1p(rs)
    Ps = np.exp(s - lse[:, None])
    uu = u[img] + u[b + img]
    l = f(2.0) * lse - (xh * uu).sum(-1) / f(temperature)
    denom = f(2.0) * f(L + 1) * f(b)
    c = f(grad_scale) / (denom * f(temperature))
    grad_x = (f(2.0) * (Ps @ w) - uu) * c
    student_w = (f(2.0) * (Ps.T @ xh)) * c
    return dict(loss=l.sum() / denom, rows=l, lse=lse, Ps=Ps, grad_x=grad_x, student_w=student_w, c=c, img=img, L=L)


def multicrop_loss_normalized(qh, xh, w, alpha, temperature=0.1, epsilon=0.05, grad_scale=1.0, dtype=np.float64, shift=0):
    """The whole loss in the u / m form on normalised rows and a GIVEN alpha.  xh with 0 rows: L = 0, today's loss.
    -> dict(loss, global_loss (already / (V-1)), local_loss, grad_q [2b, D], grad_x [L b, D], grad_w [K, D] (the total),
    grad_w_local [K, D], grad_w_global [K, D], u, m, lse_t (nats), row_stats (local lse, base 2), global_row_stats [2b, 2] (base 2))."""
    f = dtype
    qh, xh, w, alpha = (np.asarray(a, f) for a in (qh, xh, w, alpha))
    b = qh.shape[0] // 2
    g = sr.swav_loss_normalized(qh, w, alpha, temperature, epsilon, grad_scale, dtype)
    L = xh.shape[0] // b
    out = dict(u=g['u'], Pt=g['Pt'], lse_t=g['lse_t'],
               global_row_stats=np.stack([g['lse_s'], g['lse_t']], 1) * f(LOG2E))
    if L == 0:
        out.update(loss=g['loss'], global_loss=g['loss'], local_loss=f(0.0), grad_q=g['grad_q'], grad_x=xh, grad_w=g['grad_w'],
                   grad_w_global=g['grad_w'], grad_w_local=np.zeros_like(w))
        return out
    loc = local_loss_normalized(xh, w, g['u'], b, temperature, grad_scale, dtype, shift)
    m = np.zeros((b, xh.shape[1]), f)
    for v in range(L):                      # the views in the order 0, 1, ...
        m = m + xh[v * b:(v + 1) * b]
    if shift:
        m = np.roll(m, shift, axis=0)       # image i receives the rows paired to it
    code_w = (g['Pt'][:b].T @ m + g['Pt'][b:].T @ m) * loc['c']
    share = f(1.0) / f(L + 1)
    out.update(loss=g['loss'] * share + loc['loss'], global_loss=g['loss'] * share, local_loss=loc['loss'], grad_q=g['grad_q'] * share,
               grad_x=loc['grad_x'], grad_w_global=g['grad_w'] * share, grad_w_local=loc['student_w'] - code_w,
               m=m, row_stats=loc['lse'] * f(LOG2E), rows=loc['rows'], Ps=loc['Ps'])
    out['grad_w'] = out['grad_w_global'] + out['grad_w_local']
    return out


def official_loop(qh, xh, w, alpha, temperature=0.1, epsilon=0.05):
    """The official crop loop transcribed in float64 (main_swav.py, crops_for_assign = [0, 1], nmb_crops = [2, L]):
        loss = 0
        for crop_id in [0, 1]:
            q = the code of view crop_id                           (no gradient)
            subloss = 0
            for v in every view but crop_id:
                subloss -= mean_i(sum_j q[i, j] log_softmax(view_v . w / T)[i, j])
            loss += subloss / (V - 1)
        loss /= 2"""
    qh, xh, w = (np.asarray(a, np.float64) for a in (qh, xh, w))
    b = qh.shape[0] // 2
    L = xh.shape[0] // b
    views = [qh[:b], qh[b:]] + [xh[v * b:(v + 1) * b] for v in range(L)]
    code = sr.codes(qh, w, alpha, epsilon)
    loss = 0.0
    for crop_id in (0, 1):
        q = code[crop_id * b:(crop_id + 1) * b]
        subloss = 0.0
        for v in range(len(views)):
            if v == crop_id:
                continue
            s = (views[v] @ w.T) / temperature
            logp = s - sr.logsumexp(s, 1)[:, None]
            subloss -= (q * logp).sum(1).mean()
        loss += subloss / (len(views) - 1)
    return loss / 2.0


def autograd_gradients(qh, xh, w, temperature=0.1, epsilon=0.05, iters=3, detach=True):
    """float64 torch autograd of the official loop, the Sinkhorn on the global rows themselves (one replica).  detach=False lets the
    gradient flow through the codes as well.  -> (loss, grad_q, grad_x, grad_w)."""
    import torch
    q = torch.tensor(np.asarray(qh, np.float64), requires_grad=True)
    x = torch.tensor(np.asarray(xh, np.float64), requires_grad=True)
    p = torch.tensor(np.asarray(w, np.float64), requires_grad=True)
    rows, K = q.shape[0], p.shape[0]
    b = rows // 2
    L = x.shape[0] // b
    Lg = (q @ p.T) / epsilon
    beta = torch.zeros(rows, dtype=torch.float64)
    for it in range(1, iters + 1):
        y = Lg + beta[:, None]
        alpha = torch.stack([-np.log(K) - torch.logsumexp(y[v * b:(v + 1) * b], 0) for v in range(2)])
        if it < iters:
            beta = -np.log(b) - torch.logsumexp(Lg + alpha.repeat_interleave(b, 0), 1)
    code = torch.softmax(Lg + alpha.repeat_interleave(b, 0), 1)
    if detach:
        code = code.detach()
    views = [q[:b], q[b:]] + [x[v * b:(v + 1) * b] for v in range(L)]
    loss = 0.0
    for crop_id in (0, 1):
        c = code[crop_id * b:(crop_id + 1) * b]
        sub = 0.0
        for v in range(len(views)):
            if v != crop_id:
                sub = sub - (c * torch.log_softmax((views[v] @ p.T) / temperature, 1)).sum(1).mean()
        loss = loss + sub / (len(views) - 1)
    loss = loss / 2.0
    loss.backward()
    gx = x.grad.numpy() if x.grad is not None else np.zeros_like(np.asarray(xh, np.float64))
    return float(loss.detach()), q.grad.numpy(), gx, p.grad.numpy()


# ---- the kernel cases shared by tests/test_swav_multicrop_reference.py (error budget) and tests/test_gpu_swav_multicrop.py -----------
# (b, L): one row; 6 rows; 66 rows = a 64-row tile straddling the local-view boundary and 2 row splits at K = 2; 66 rows of six views;
# 70 rows = one ragged tile past a full one.  K: the smallest table, one row past a tile, 65 tiles with a ragged last one (65 key splits
# at one row tile).  Every width.
MC_SHAPES = [(1, 1), (3, 2), (33, 2), (11, 6), (70, 1)]
MC_KS = [2, 65, 4097]
MC_DIMS = [64, 128, 256]
MC_CASES = [(b, L, K, D) for (b, L) in MC_SHAPES for K in MC_KS for D in MC_DIMS]
MC_T, MC_EPS = 0.1, 0.05


def case_inputs(b, L, K, D):
    """-> (qh [2b, D], xh [L b, D], w [K, D], alpha [2, K]) float32: swav_reference's global rows and prototypes, local rows that are
    noisy copies of their image's view a (so a mis-pairing moves every figure), alpha of the float64 Sinkhorn (I = 3) on the global
    rows rounded to float32 ONCE."""
    qh, w, alpha = sr.loss_case_inputs(b, K, D, MC_T, MC_EPS)
    g = np.random.default_rng(77 + 1000 * b + 10 * L + K + D)
    base = np.tile(qh[:b].astype(np.float64), (L, 1))
    xh = sr.l2_normalize(base + 0.7 * g.standard_normal((L * b, D)) / np.sqrt(D))[0].astype(np.float32)
    return qh, xh, w, alpha


_REF = {}


def case_reference(b, L, K, D):
    """The float64 reference of a case, computed once and shared (treat as read-only).  u and global_row_stats are ALSO kept rounded to
    float32 (u32, grs32): what the kernels are handed in the place of simclr_swav_fwd's outputs."""
    key = (b, L, K, D)
    if key not in _REF:
        qh, xh, w, alpha = case_inputs(b, L, K, D)
        r = multicrop_loss_normalized(qh, xh, w, alpha, MC_T, MC_EPS)
        r.update(qh=qh, xh=xh, w=w, alpha=alpha, u32=r['u'].astype(np.float32), grs32=r['global_row_stats'].astype(np.float32))
        _REF[key] = r
    return _REF[key]


def relerr(got, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300))


def emulation_errors(b, L, K, D):
    """Relative error of the float32 emulation (every array operation rounds to float32) of the LOCAL share against float64."""
    r = case_reference(b, L, K, D)
    e = multicrop_loss_normalized(r['qh'], r['xh'], r['w'], r['alpha'], MC_T, MC_EPS, dtype=np.float32)
    return dict(loss=relerr(e['local_loss'], r['local_loss']), row_stats=relerr(e['row_stats'], r['row_stats']),
                grad_x=relerr(e['grad_x'], r['grad_x']), grad_w=relerr(e['grad_w_local'], r['grad_w_local']))
