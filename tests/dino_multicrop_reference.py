"""numpy restatement of DINO's multi-crop loss (Caron et al. 2021; the official DINOLoss.forward with ncrops = 2 + L) in the form the
kernels compute, beside a transcription of the official crop loop, float64 autograd with and without the stop-gradient, and the
float32 emulation that supplies the GPU tolerances.

Conventions of simclr_amd.objective.add_dino_local_loss: qh / kh [2b, D] = the normalised GLOBAL online rows / momentum keys, [view a;
view b]; xh [L b, D] = the normalised LOCAL rows, view-major (row v b + i = local view v of image i); ws / wt [K, D] the row-normalised
online / target prototypes; c [K] the centre; V = 2 + L; i = r mod b; cst = 1 / (2 (V - 1) b).
  s_rj   = x_r . ws_j / Ts                 Ps = softmax_j(s_r)
  t_gj   = (k_g . wt_j - c_j) / Tt         Pt[g] = softmax_j(t_g)     (global row g's OWN teacher row)
  u_g    = sum_j Pt[g, j] ws_j
  value  = cst * sum_r [ 2 logsumexp_j(s_r) - x_r . (u_i + u_{b+i}) / Ts ]
  dvalue/dx_r  = (cst / Ts) * ( 2 sum_j Ps[r, j] ws_j - u_i - u_{b+i} )
  dvalue/dws_j = (cst / Ts) * ( 2 sum_r Ps[r, j] x_r - sum_{g < 2b} Pt[g, j] m_g ),   m_g = sum_v x_{v b + (g mod b)}
  total  = global.value / (V - 1) + value
The teacher sees the global views only and is stop-gradient.

WHICH ROW u IS STORED BY.  simclr_dino_fwd's teacher expectation sweep fixes the rows of k and writes the split partials at the row it
fixed, so u[g] = sum_j Pt[g, j] ws_j is stored BY ROW (the pairing p(r) is applied by its readers: dino_finalize_rows and dino_combine
read u[p(r)]).  dino_reference.dino_loss_normalized returns the same u = Pt @ ws.  The local term reads the symmetric u_i + u_{b+i}.

WHICH lse_t NORMALISES A TEACHER ROW.  simclr_dino_bwd_w streams online row r beside the key of the PAIRED row and reads
row_stats[2 p(r) + 1]; the local term's teacher sweep streams global row g with its own key and must read row_stats[2 g + 1].
`lse_of='paired'` below evaluates the reference with the wrong one: the GPU test shows it falls outside the tolerance."""
import numpy as np

from tests import dino_reference as dr

LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
TILE = 64
# worst float32-emulation error (emulate() below) against float64 over every entry of ALL_CASES, relative to the reference tensor's
# largest magnitude, as tests/test_dino_multicrop_reference.py re-measures it; the tolerances of tests/test_gpu_dino_multicrop.py are
# 4x these
EMULATION_ERROR = dict(loss=2.7e-7, grad_x=2.25e-6, grad_w=5.6e-6)
TOL = {k: 4.0 * v for k, v in EMULATION_ERROR.items()}


def _image_of(rows, b, shift=0):
    return (np.arange(rows) % b + shift) % b


def local_loss_normalized(xh, ws, u, b, student_temp=0.1, grad_scale=1.0, dtype=np.float64):
    """The LOCAL share on normalised rows and GIVEN teacher expectations u [2b, D] (what the value and the query-side backward read).
    -> dict(loss = the local sum / (2 (V-1) b), rows [L b], lse [L b] in nats, Ps, grad_x [L b, D], student_w [K, D] = cst/Ts sum_r 2 Ps x_r)."""
    f = dtype
    xh, ws, u = (np.asarray(a, f) for a in (xh, ws, u))
    rows = xh.shape[0]
    assert rows % b == 0 and rows >= b and u.shape[0] == 2 * b
    L = rows // b
    img = _image_of(rows, b)
    s = (xh @ ws.T) / f(student_temp)
    ms, rs, _ = dr.softmax_stats(s)
    lse = ms + np.log1p(rs)
    Ps = np.exp(s - lse[:, None])
    uu = u[img] + u[b + img]
    l = f(2.0) * lse - (xh * uu).sum(-1) / f(student_temp)
    denom = f(2.0) * f(L + 1) * f(b)
    c = f(grad_scale) / (denom * f(student_temp))
    return dict(loss=l.sum() / denom, rows=l, lse=lse, Ps=Ps, grad_x=(f(2.0) * (Ps @ ws) - uu) * c,
                student_w=(f(2.0) * (Ps.T @ xh)) * c, c=c, L=L)


def multicrop_loss_normalized(qh, kh, xh, ws, wt, c, student_temp=0.1, teacher_temp=0.04, grad_scale=1.0, dtype=np.float64,
                              lse_of='own'):
    """The whole loss in the u / m form on normalised rows.  xh with 0 rows: L = 0, the plain DINO loss.
    lse_of='paired': the teacher rows of the local term's key-side gradient normalised with the PAIRED row's lse_t (the trap).
    -> dict(loss, global_loss (already / (V-1)), local_loss, grad_q [2b, D], grad_x [L b, D], grad_w [K, D] (the total),
    grad_w_local, grad_w_global, u, Pt, m, row_stats [L b] (local lse, base 2), global_row_stats [2b, 2] (base 2), entropy)."""
    f = dtype
    qh, kh, xh, ws, wt, c = (np.asarray(a, f) for a in (qh, kh, xh, ws, wt, c))
    b = qh.shape[0] // 2
    g = dr.dino_loss_normalized(qh, kh, ws, wt, c, student_temp, teacher_temp, grad_scale, dtype)
    L = xh.shape[0] // b
    out = dict(u=g['u'], Pt=g['Pt'], lse_t=g['lse_t'], entropy=g['entropy'],
               global_row_stats=np.stack([g['lse_s'], g['lse_t']], 1) * f(LOG2E))
    if L == 0:
        out.update(loss=g['loss'], global_loss=g['loss'], local_loss=f(0.0), grad_q=g['grad_q'], grad_x=xh, grad_w=g['grad_ws'],
                   grad_w_global=g['grad_ws'], grad_w_local=np.zeros_like(ws))
        return out
    loc = local_loss_normalized(xh, ws, g['u'], b, student_temp, grad_scale, dtype)
    m = np.zeros((b, xh.shape[1]), f)
    for v in range(L):                      # the views in the order 0, 1, ...
        m = m + xh[v * b:(v + 1) * b]
    Pt = g['Pt']
    if lse_of == 'paired':
        t = ((kh @ wt.T) - c[None, :]) / f(teacher_temp)
        Pt = np.exp(t - dr.pair(g['lse_t'])[:, None])
    else:
        assert lse_of == 'own'
    teacher_w = (Pt[:b].T @ m + Pt[b:].T @ m) * loc['c']
    share = f(1.0) / f(L + 1)
    out.update(loss=g['loss'] * share + loc['loss'], global_loss=g['loss'] * share, local_loss=loc['loss'], grad_q=g['grad_q'] * share,
               grad_x=loc['grad_x'], grad_w_global=g['grad_ws'] * share, grad_w_local=loc['student_w'] - teacher_w,
               m=m, row_stats=loc['lse'] * f(LOG2E), rows=loc['rows'], Ps=loc['Ps'])
    out['grad_w'] = out['grad_w_global'] + out['grad_w_local']
    return out


def official_loop(qh, kh, xh, ws, wt, c, student_temp=0.1, teacher_temp=0.04):
    """The official crop loop transcribed in float64 (DINOLoss.forward, ncrops = 2 + L):
        student_out = the V chunks of student_output / student_temp
        teacher_out = the 2 chunks of softmax((teacher_output - center) / temp)           (no gradient)
        total_loss, n_loss_terms = 0, 0
        for iq, q in enumerate(teacher_out):
            for v in range(len(student_out)):
                if v == iq: continue
                total_loss += mean_i(sum_j -q[i, j] log_softmax(student_out[v])[i, j]);  n_loss_terms += 1
        total_loss /= n_loss_terms"""
    qh, kh, xh, ws, wt, c = (np.asarray(a, np.float64) for a in (qh, kh, xh, ws, wt, c))
    b = qh.shape[0] // 2
    L = xh.shape[0] // b
    student_out = [qh[:b], qh[b:]] + [xh[v * b:(v + 1) * b] for v in range(L)]
    t = ((kh @ wt.T) - c[None, :]) / teacher_temp
    t = t - t.max(1, keepdims=True)
    soft = np.exp(t) / np.exp(t).sum(1, keepdims=True)
    teacher_out = [soft[:b], soft[b:]]
    total, n_terms = 0.0, 0
    for iq, q in enumerate(teacher_out):
        for v in range(len(student_out)):
            if v == iq:
                continue
            s = (student_out[v] @ ws.T) / student_temp
            ms, rs, _ = dr.softmax_stats(s)
            logp = s - (ms + np.log1p(rs))[:, None]
            total += (-(q * logp).sum(1)).mean()
            n_terms += 1
    return total / n_terms


def autograd_gradients(q, k, x, vs, vt, c, student_temp=0.1, teacher_temp=0.04, detach=True, tied=False):
    """float64 torch autograd of the official loop on RAW projections q / k [2b, D], x [L b, D] and RAW prototype variables vs / vt,
    every row normalisation inside the graph (the weight normalisation of the last layer included).  tied=True scores the teacher
    with the STUDENT's variable (the state of step 0, when the target is a copy): only then can a missing stop-gradient show, since
    the momentum teacher shares no leaf with the student otherwise.  -> (loss, grad_q, grad_x, grad_vs)."""
    import torch
    T = lambda a, rg=False: torch.tensor(np.asarray(a, np.float64), requires_grad=rg)
    l2n = lambda a: a / torch.sqrt(torch.clamp((a * a).sum(-1, keepdim=True), min=dr.EPS))
    tq, tx, tv = T(q, True), T(x, True), T(vs, True)
    b = tq.shape[0] // 2
    L = tx.shape[0] // b
    qh, xh, ws = l2n(tq), l2n(tx), l2n(tv)
    wt = ws if tied else l2n(T(vt))
    teacher = torch.softmax((l2n(T(k)) @ wt.T - T(c)) / teacher_temp, -1)
    if detach:
        teacher = teacher.detach()
    views = [qh[:b], qh[b:]] + [xh[v * b:(v + 1) * b] for v in range(L)]
    total, n_terms = 0.0, 0
    for iq in (0, 1):
        tq_rows = teacher[iq * b:(iq + 1) * b]
        for v in range(len(views)):
            if v != iq:
                total = total - (tq_rows * torch.log_softmax(views[v] @ ws.T / student_temp, -1)).sum(-1).mean()
                n_terms += 1
    loss = total / n_terms
    loss.backward()
    gx = tx.grad.numpy() if tx.grad is not None else np.zeros_like(np.asarray(x, np.float64))
    return float(loss.detach()), tq.grad.numpy(), gx, tv.grad.numpy()


# ---- the kernel cases shared by tests/test_dino_multicrop_reference.py (error budget) and tests/test_gpu_dino_multicrop.py -----------
# (b, L): one row; 6 rows; 66 rows = a 64-row tile straddling the view boundary (local AND global) and 2 row splits at K = 2; 66 rows of
# six views; 70 local rows = one ragged tile past a full one, 140 global rows = three tiles with a ragged last one and three teacher row
# splits at K = 2.  K: the smallest table, one row past a tile, 65 tiles with a ragged last one.  Every width.
MC_SHAPES = [(1, 1), (3, 2), (33, 2), (11, 6), (70, 1)]
MC_KS = [2, 65, 4097]
MC_DIMS = [64, 128, 256]
MC_CASES = [(b, L, K, D) for (b, L) in MC_SHAPES for K in MC_KS for D in MC_DIMS]
MC_TS, MC_TT = 0.1, 0.04
# the second temperature pair (0.1, 0.07) on the K = 65 cases; one near-one-hot teacher case
ALL_CASES = ([case + (MC_TT, 'plain') for case in MC_CASES] + [case + (0.07, 'plain') for case in MC_CASES if case[2] == 65]
             + [(5, 2, 65, 64, MC_TT, 'onehot')])


def case_inputs(b, L, K, D, kind='plain'):
    """-> (qh, kh [2b, D], xh [L b, D], ws, wt [K, D], c [K]) float32.  The two global views are INDEPENDENT noisy copies of an image
    row, so their teacher rows -- and their lse_t -- differ visibly; the keys are noisy copies of the online rows, the target
    prototypes a near copy of the online ones (a momentum copy), the centre non-zero and of the size of the logits' spread; the local
    rows are noisy copies of their image.  kind='onehot': target prototype g IS key g (K >= 2b), so every teacher row puts more than
    0.999 of its mass on one prototype at Tt = 0.04."""
    g = np.random.default_rng(91 + 1000 * b + 10 * L + K + D)
    unit = lambda a: dr.l2_normalize(a)[0].astype(np.float32)
    img = g.standard_normal((b, D)) / np.sqrt(D)
    noise = lambda n, s: s * g.standard_normal((n, D)) / np.sqrt(D)
    qh = unit(np.concatenate([img + noise(b, 0.8), img + noise(b, 0.8)]))
    kh = unit(qh + noise(2 * b, 0.5))
    ws = unit(g.standard_normal((K, D)))
    wt = unit(ws + noise(K, 0.1))
    c = (0.05 * g.standard_normal(K)).astype(np.float32)
    xh = unit(np.tile(img, (L, 1)) + noise(L * b, 0.7))
    if kind == 'onehot':
        assert K >= 2 * b
        wt = wt.copy()
        wt[:2 * b] = kh
    return qh, kh, xh, ws, wt, c


_REF = {}


def case_reference(b, L, K, D, Tt=MC_TT, kind='plain'):
    """The float64 reference of a case, computed once and shared (treat as read-only).  u and global_row_stats are ALSO kept rounded to
    float32 (u32, grs32): what the kernels are handed in the place of simclr_dino_fwd's outputs."""
    key = (b, L, K, D, Tt, kind)
    if key not in _REF:
        qh, kh, xh, ws, wt, c = case_inputs(b, L, K, D, kind)
        r = multicrop_loss_normalized(qh, kh, xh, ws, wt, c, MC_TS, Tt)
        r.update(qh=qh, kh=kh, xh=xh, ws=ws, wt=wt, c=c, b=b, L=L, Ts=MC_TS, Tt=Tt, u32=r['u'].astype(np.float32),
                 grs32=r['global_row_stats'].astype(np.float32))
        _REF[key] = r
    return _REF[key]


def paired_reference(b, L, K, D, Tt=MC_TT, kind='plain'):
    """grad_w_local of the case with every teacher row normalised by the PAIRED row's lse_t."""
    r = case_reference(b, L, K, D, Tt, kind)
    return multicrop_loss_normalized(r['qh'], r['kh'], r['xh'], r['ws'], r['wt'], r['c'], MC_TS, Tt, lse_of='paired')['grad_w_local']


def relerr(got, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300))


# ---- the float32 emulation ---------------------------------------------------------------------------------------------------------
def _ceil(a, b):
    return -(-a // b)


def split_plan(b, L, K):
    """Tiles per split of the three sweeps whose partials are merged in a fixed order: (student key-side sweep over the L b local rows,
    teacher key-side sweep over the 2b global rows) of csrc/dino_multicrop.hip -- about 256 workgroups each -- and the key split of
    simclr_swav_local_bwd_x's probability sweep."""
    xt, kt, gt = _ceil(L * b, TILE), _ceil(K, TILE), _ceil(2 * b, TILE)
    rtiles = _ceil(xt, max(1, min(xt, 256 // kt)))
    ttiles = _ceil(gt, max(1, min(gt, 256 // kt)))
    btiles = _ceil(kt, max(1, min(kt, 256 // xt)))
    return rtiles, ttiles, btiles


def row_splits(b, L, K):
    """(student, teacher) row splits: what ops.dino_local_row_splits returns."""
    rtiles, ttiles, _ = split_plan(b, L, K)
    return _ceil(_ceil(L * b, TILE), rtiles), _ceil(_ceil(2 * b, TILE), ttiles)


def _lse2(t2):
    """Base-2 log-sum-exp of float32 rounded logits as the statistics sweeps form it: the maximum, the NON-maximum mass summed in
    float32, then m + log1p(rest) log2(e) in double.  -> float64."""
    f = np.float32
    m = t2.max(-1)
    e = np.exp2((t2 - m[:, None]).astype(f)).astype(f)
    e[np.arange(t2.shape[0]), t2.argmax(-1)] = f(0)
    rest = e.sum(-1, dtype=f)
    return m.astype(np.float64) + np.log1p(rest.astype(np.float64)) * LOG2E


def _split_sum(P, M, tiles):
    """sum over the splits (tiles * 64 streamed rows each) of P[split].T @ M[split]: float32 partials, added in the split order."""
    f = np.float32
    acc = np.zeros((P.shape[1], M.shape[1]), f)
    for lo in range(0, P.shape[0], tiles * TILE):
        acc = (acc + (P[lo:lo + tiles * TILE].T @ M[lo:lo + tiles * TILE]).astype(f)).astype(f)
    return acc


def emulate(r, grad_scale=1.0):
    """float32 emulation of the three launches on the float32 inputs of case reference r, following the kernels: every dot product
    accumulates in float32 (one accumulator type per logit; numpy's order, not the MFMA's), the logit is the ROUNDED base-2 product
    (x . ws) (log2 e / Ts) -- for the teacher the two roundings (k . wt - c) and the product --, the probabilities are exp2(logit -
    lse) in float32 with lse rounded to float32 once (the teacher's is grs32, as the kernel is handed it), m is summed view by view,
    the split partials are float32 and merged in their fixed order, and the value finishes in double where the kernels do.
    -> dict(loss, grad_x, grad_w)."""
    f = np.float32
    xh, kh, ws, wt, c, u32, grs32 = (r[n] for n in ('xh', 'kh', 'ws', 'wt', 'c', 'u32', 'grs32'))
    b, L, K = r['b'], r['L'], ws.shape[0]
    rtiles, ttiles, btiles = split_plan(b, L, K)
    scale2s, scale2t = f(f(LOG2E) / f(r['Ts'])), f(f(LOG2E) / f(r['Tt']))
    img = _image_of(L * b, b)
    s2 = ((xh @ ws.T).astype(f) * scale2s).astype(f)
    lse_d = _lse2(s2)
    lse32 = lse_d.astype(f)
    uu = u32[img].astype(np.float64) + u32[b + img].astype(np.float64)
    rowterm = 2.0 * lse_d * LN2 - (xh.astype(np.float64) * uu).sum(-1) * (1.0 / float(f(r['Ts'])))
    loss = f(rowterm.sum() / (2.0 * (L + 1) * b))
    Ps = np.exp2((s2 - lse32[:, None]).astype(f)).astype(f)
    coeff = f(f(grad_scale) / (f(r['Ts']) * f(2) * f(L + 1) * f(b)))
    gx = _split_sum(Ps.T, ws, btiles)                                      # [L b, D]: the key splits of the probability sweep
    grad_x = (coeff * ((f(2) * gx - u32[img]).astype(f) - u32[b + img]).astype(f)).astype(f)
    m = xh[:b].copy()
    for v in range(1, L):
        m = (m + xh[v * b:(v + 1) * b]).astype(f)
    a = _split_sum(Ps, xh, rtiles)
    t2 = (((kh @ wt.T).astype(f) - c[None, :]).astype(f) * scale2t).astype(f)
    Pt = np.exp2((t2 - grs32[:, 1][:, None]).astype(f)).astype(f)
    e = _split_sum(Pt, m[np.arange(2 * b) % b], ttiles)
    grad_w = (coeff * (f(2) * a - e).astype(f)).astype(f)
    return dict(loss=loss, grad_x=grad_x, grad_w=grad_w)


def emulation_errors(b, L, K, D, Tt=MC_TT, kind='plain'):
    """Relative error of the float32 emulation of the LOCAL share against float64."""
    r = case_reference(b, L, K, D, Tt, kind)
    e = emulate(r)
    return dict(loss=relerr(e['loss'], r['local_loss']), grad_x=relerr(e['grad_x'], r['grad_x']),
                grad_w=relerr(e['grad_w'], r['grad_w_local']))
