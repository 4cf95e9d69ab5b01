"""Restatements of the cached-feature linear probe (csrc/logreg.hip, simclr_amd/logreg.py) in numpy.

  direct(...)            float64, straight from the definition, for R replicas (disjoint row shards whose sums are added)
  solve(...)             the L-BFGS solver of DESIGN.md section 30 in float64
  emulate(...)           the kernels' arithmetic: one float32 accumulator per logit in k order (every product and every addition rounded:
                         at least as many roundings as the MFMA makes), the two roundings of logit2, the per-lane (m, r) pushes and the
                         8-state and class-tile merges in the kernel's order, double finishes, G with expm1 on the label, the row parts
                         of the backward added as ((p0 + p1) + p2) + ... in float32, db from double column sums
The gate of a device value is 4 x the error of emulate() against direct() on the same inputs, never below one float32 ulp: for an array,
4 x the LARGEST elementwise emulation error, never below one ulp of the array's largest float64 magnitude (a per-element gate would
punish the element whose emulation error happens to vanish).  MUTANTS are wrong readings the comparator must reject at those gates.
"""
import functools
import hashlib

import numpy as np

LOG2E32 = np.float32(1.4426950408889634)
LN2 = 0.6931471805599453
F32 = np.float32

# ---- the case table of tests/test_gpu_logreg.py ----------------------------------------------------------------------------------
SHAPES = [(2, 64, 2),              # the floor
          (65, 64, 3),             # a one-row last row tile
          (130, 128, 65),          # one class in the last class tile
          (129, 192, 64),          # k not a multiple of 128
          (257, 2048, 1000),       # the real width with ragged classes
          (96, 8192, 10),          # the widest features
          (300, 64, 4096),         # the most classes
          (1100, 64, 5),           # row parts: simclr_logreg_row_splits > 1, the last part ragged
          (4097, 64, 897),         # the 128-wide forward tile, ragged both ways
          (40, 1024, 4096)]        # the 128-wide backward tile
L2 = {s: (1e-3 if i < 3 else 1e-4) for i, s in enumerate(SHAPES)}
FAMILIES = ('gauss', 'onehot', 'padlast')
CASES = [(n, D, C, fam) for n, D, C in SHAPES for fam in FAMILIES]
SPLIT_SHAPE = (1100, 64, 5)


def fwd_edge(n, C):
    return 128 if -(-n // 128) * -(-C // 128) >= 256 else 64


def bwd_edge(D, C):
    return 128 if -(-C // 128) * -(-D // 128) >= 256 else 64


def row_parts(n, D, C):
    """(parts, rows per part) of the backward product: the plan of csrc/logreg.hip."""
    E = bwd_edge(D, C)
    tiles = -(-C // E) * -(-D // E)
    want = 1 if tiles >= 256 else -(-256 // tiles)
    want = min(want, -(-n // 256))
    rows = -(-(-(-n // want)) // 32) * 32
    return -(-n // rows), rows


def gap_threshold(x, W):
    """Per row: 4 D 2^-24 times the row's scale max_c sum_k |x_nk W_ck| (the worst-case float32 error of a logit, four times over)."""
    scale = (np.abs(x).astype(np.float64) @ np.abs(W).astype(np.float64).T).max(1)
    return 4.0 * x.shape[1] * 2.0 ** -24 * scale


def top_gap(x, W, b):
    s = x.astype(np.float64) @ W.astype(np.float64).T + b.astype(np.float64)
    top = np.sort(s, axis=1)
    return top[:, -1] - top[:, -2]


def gap_ok(x, W, b):
    """Per row: the float64 top-1 / top-2 gap is above gap_threshold, or the row is all zero (an exact tie by construction)."""
    return (top_gap(x, W, b) > gap_threshold(x, W)) | ~np.any(np.asarray(x) != 0, axis=1)


@functools.lru_cache(maxsize=None)
def case_inputs(n, D, C, family):
    """(x [n, D], labels [n] int32, weights [n], W [C, D], b [C]) float32, read-only.  gauss: Gaussian rows, weights cycling through
    (0.5, 2, 1, 1.5) so that S != n; onehot: one dominant logit per row (the label's in three rows of four); padlast: Gaussian rows,
    every label C - 1, the last third of the rows (at least one) with weight 0.  A row whose float64 top-1 / top-2 gap is not above
    gap_threshold is redrawn.  Row 0 is the exception, in every family: its features are all zero and b_0 = b_(C-1) is the largest bias,
    so its logits are the biases in any arithmetic and classes 0 and C - 1 tie EXACTLY -- the row the tie rule decides (label 0: a hit
    under the lowest-index rule; label C - 1 in padlast: a miss)."""
    rng = np.random.RandomState(100 * FAMILIES.index(family) + 7 * n + 3 * D + C)
    W = (rng.randn(C, D) / np.sqrt(D)).astype(F32)
    b = (0.1 * rng.randn(C)).astype(F32)
    b[0] = b[C - 1] = np.abs(b).max() + F32(0.5)
    labels = rng.randint(0, C, n).astype(np.int32)
    labels[0] = 0
    weights = np.array([0.5, 2.0, 1.0, 1.5], F32)[np.arange(n) % 4]

    def draw(rows):
        x = rng.randn(len(rows), D)
        if family == 'onehot':
            dom = np.where(rows % 4 == 3, (labels[rows] + 1) % C, labels[rows])
            Wd = W[dom].astype(np.float64)
            x = 0.3 * x + 30.0 * Wd / (Wd * Wd).sum(1, keepdims=True)
        return x.astype(F32)

    rows = np.arange(n)
    x = draw(rows)
    if family == 'padlast':
        labels[:] = C - 1
        weights = np.ones(n, F32)
        weights[n - max(n // 3, 1):] = 0.0
    x[0] = 0.0
    for _ in range(200):
        bad = np.nonzero(~gap_ok(x, W, b))[0]
        if not len(bad):
            break
        x[bad] = draw(bad)
    else:
        raise AssertionError('case_inputs: rows without a top-1 gap remain')
    for a in (x, labels, weights, W, b):
        a.setflags(write=False)
    return x, labels, weights, W, b


# ---- float64, from the definition ------------------------------------------------------------------------------------------------------
def direct(x, labels, weights, W, b, l2, R=1):
    """dict(f, lse [n], hits, S, G [n, C], dW, db) in float64; rows are dealt to R replicas in contiguous shards whose sums are added in
    replica order.  dW, db and f include the l2 terms; hits is the weight of the rows whose label is the lowest-index maximum."""
    x, W, b, w = (np.asarray(a, np.float64) for a in (x, W, b, weights))
    n, C = x.shape[0], W.shape[0]
    S = sum(w[sh].sum() for sh in np.array_split(np.arange(n), R))
    loss = hits = 0.0
    dW, db = np.zeros_like(W), np.zeros_like(b)
    lse, G = np.zeros(n), np.zeros((n, C))
    for sh in np.array_split(np.arange(n), R):
        if not len(sh):
            continue
        s = x[sh] @ W.T + b
        m = s.max(1)
        lse[sh] = m + np.log(np.exp(s - m[:, None]).sum(1))
        y = np.asarray(labels)[sh]
        loss += (w[sh] * (lse[sh] - s[np.arange(len(sh)), y])).sum()
        hits += w[sh][s.argmax(1) == y].sum()
        g = np.exp(s - lse[sh][:, None])
        g[np.arange(len(sh)), y] -= 1.0
        G[sh] = g * (w[sh] / S)[:, None]
        dW += G[sh].T @ x[sh]
        db += G[sh].sum(0)
    f = loss / S + 0.5 * l2 * ((W * W).sum() + (b * b).sum())
    return dict(f=f, lse=lse, hits=hits, S=S, G=G, dW=dW + l2 * W, db=db + l2 * b)


# ---- the solver ---------------------------------------------------------------------------------------------------------------------------
class Fit:
    pass


def search_direction(g, pairs):
    """(d, g.d, pairs): -H g by the two-loop recursion over pairs = [(s, y, 1 / s.y)], oldest first, gamma = s.y / y.y of the newest; a
    result that is not a descent direction drops the history and gives -g."""
    q = g.copy()
    alphas = []
    for s, y, rho in reversed(pairs):
        a = rho * s.dot(q)
        q -= a * y
        alphas.append(a)
    if pairs:
        s, y, rho = pairs[-1]
        q *= 1.0 / (rho * y.dot(y))
    for (s, y, rho), a in zip(pairs, reversed(alphas)):
        q += (a - rho * y.dot(q)) * s
    d = -q
    gd = g.dot(d)
    if not gd < 0.0:
        pairs, d = [], -g
        gd = g.dot(d)
    return d, gd, pairs


def solve(x, labels, weights, C, l2, max_iterations=200, tolerance=1e-5, history=10, init=None, R=1):
    """L-BFGS with Armijo backtracking exactly as simclr_amd/logreg.py states it, in float64 on direct()."""
    D = x.shape[1]
    theta = np.zeros(C * D + C) if init is None else np.concatenate([np.asarray(init[0], np.float64).ravel(), np.asarray(init[1], np.float64)])

    def ev(t):
        r = direct(x, labels, weights, t[:C * D].reshape(C, D), t[C * D:], l2, R)
        return r['f'], np.concatenate([r['dW'].ravel(), r['db']]), r['hits'] / r['S']

    f, g, acc = ev(theta)
    out = Fit()
    out.evaluations, out.iterations, out.converged, out.losses = 1, 0, False, []
    pairs = []
    while True:
        if np.abs(g).max() <= tolerance * max(1.0, abs(f)):
            out.converged = True
            break
        if out.iterations >= max_iterations:
            break
        d, gd, pairs = search_direction(g, pairs)
        t = min(1.0, 1.0 / np.sqrt(g.dot(g))) if out.iterations == 0 else 1.0
        ok = False
        for _ in range(31):
            trial = theta + t * d
            ft = ev(trial)[0]
            out.evaluations += 1
            if ft <= f + 1e-4 * t * gd:
                ok = True
                break
            t *= 0.5
        if not ok:
            break
        f_new, g_new, acc = ev(trial)
        out.evaluations += 1
        s, y = trial - theta, g_new - g
        if s.dot(y) > 1e-10 * np.sqrt(s.dot(s)) * np.sqrt(y.dot(y)):
            pairs = (pairs + [(s, y, 1.0 / s.dot(y))])[-history:]
        theta, f, g = trial, f_new, g_new
        out.iterations += 1
        out.losses.append(f)
    out.W, out.b, out.loss, out.grad_norm, out.train_top_1 = theta[:C * D].reshape(C, D), theta[C * D:], f, np.abs(g).max(), acc
    return out


def toy_problem(N, D, C, separation, seed=0):
    """Class-mean clusters, standardised: (x [N, D] float32, labels int32, weights float32 -- the last three rows have weight 0)."""
    rng = np.random.RandomState(1000 + seed + N + D + C)
    means = separation * rng.randn(C, D)
    labels = (np.arange(N) % C).astype(np.int32)
    h = means[labels] + rng.randn(N, D)
    weights = np.ones(N, F32)
    weights[-3:] = 0.0
    keep = weights > 0
    mu = h[keep].mean(0)
    var = ((h[keep] - mu) ** 2).mean(0)
    return ((h - mu) / np.sqrt(var + 1e-6)).astype(F32), labels, weights


TOY_PROBLEMS = [(300, 64, 5, 1e-2, 1.0), (257, 192, 65, 1e-3, 0.5), (130, 64, 3, 1e-3, 0.1)]


# ---- the kernels' arithmetic ----------------------------------------------------------------------------------------------------------------
def _mr_push(m, r, t):
    with np.errstate(invalid='ignore', over='ignore'):
        empty, gt = np.isneginf(m), t > m
        r_gt = (r + F32(1)) * np.exp2(m - t)
        r_le = r + np.exp2(t - m)
    return np.where(empty | gt, t, m).astype(F32), np.where(empty, F32(0), np.where(gt, r_gt, r_le)).astype(F32)


def _mr_merge(m, r, m2, r2):
    with np.errstate(invalid='ignore', over='ignore'):
        e1, e2, sw = np.isneginf(m), np.isneginf(m2), m2 > m
        r_keep = r + (r2 + F32(1)) * np.exp2(m2 - m)
        r_swap = r2 + (r + F32(1)) * np.exp2(m - m2)
    mm = np.where(e2, m, np.where(e1 | sw, m2, m))
    rr = np.where(e2, r, np.where(e1, r2, np.where(sw, r_swap, r_keep)))
    return mm.astype(F32), rr.astype(F32)


def _accumulate(x, W):
    """acc[n, c] = sum_k x[n, k] W[c, k]: one float32 accumulator per logit, k ascending, product and addition rounded."""
    acc = np.zeros((x.shape[0], W.shape[0]), F32)
    for k in range(x.shape[1]):
        acc = acc + x[:, k, None] * W[None, :, k]
    return acc


MUTANTS = ('padded_columns_in_lse', 'one_over_n', 'bias_not_regularised', 'highest_index_maximum', 'label_logit_wrong_tile')


def mutant_applies(mutant, n, D, C):
    """padded_columns_in_lse needs a ragged last class tile: where C fills its tiles there is no padded column to let in."""
    return mutant != 'padded_columns_in_lse' or C % fwd_edge(n, C) != 0


def emulate(x, labels, weights, W, b, l2, mutant=None, slabs=None, share=None):
    """The device path of logreg.value_and_grad on one replica: dict(f, lse, hits, S, G, dW, db) as float64 arrays of the values the
    kernels store.  slabs: row boundaries [(o, e), ...] (default: one slab); dW and db accumulate over them in float32.  share: a dict
    that carries the accumulators and the backward product between calls on the SAME inputs (a mutant changes neither the
    accumulators nor, unless it changes G, the product)."""
    for a in (x, weights, W, b):
        assert a.dtype == F32
    n, D = x.shape
    C = W.shape[0]
    S = float(weights.astype(np.float64).sum())
    inv_S = 1.0 / (n if mutant == 'one_over_n' else S)
    slabs = slabs or [(0, n)]
    lse, G = np.zeros(n), np.zeros((n, C), F32)
    loss = hits = 0.0
    dW = db = None
    for o, e in slabs:
        r = _emulate_slab(x[o:e], labels[o:e], weights[o:e], W, b, inv_S, mutant, None if share is None else share.setdefault((o, e), {}))
        lse[o:e], G[o:e] = r['lse'], r['G']
        loss += r['loss']
        hits += r['hits']
        dW = r['dW'] if dW is None else dW + r['dW']
        db = r['db'] if db is None else db + r['db']
    W64, b64 = W.astype(np.float64), b.astype(np.float64)
    reg = (W64 * W64).sum() + (0.0 if mutant == 'bias_not_regularised' else (b64 * b64).sum())
    return dict(f=loss * inv_S + 0.5 * l2 * reg, lse=lse, hits=hits, S=S, G=G.astype(np.float64), dW=dW.astype(np.float64) + l2 * W64,
                db=db.astype(np.float64) + (0.0 if mutant == 'bias_not_regularised' else l2 * b64))


def _emulate_slab(x, labels, weights, W, b, inv_S, mutant, share=None):
    n, D = x.shape
    C = W.shape[0]
    E = fwd_edge(n, C)
    Wt = E // 32
    ntc = -(-C // E)
    cols = ntc * E
    acc = np.zeros((n, cols), F32)
    share = {} if share is None else share
    if 'acc' not in share:
        share['acc'] = _accumulate(x, W)
    acc[:, :C] = share['acc']
    bp = np.zeros(cols, F32)
    bp[:C] = b
    raw = acc + bp
    t = acc * LOG2E32 + bp * LOG2E32                                   # the two roundings of logit2 (and the one of b log2 e)
    limit = cols if mutant == 'padded_columns_in_lse' else C
    m, r = np.full(n, -np.inf, F32), np.zeros(n, F32)
    for tile in range(ntc):
        tm, tr = np.full(n, -np.inf, F32), np.zeros(n, F32)
        for wm in range(2):
            for g in range(4):
                lm, lr = np.full(n, -np.inf, F32), np.zeros(n, F32)
                for i in range(Wt):
                    for k in range(4):
                        c = tile * E + 16 * Wt * wm + 16 * i + 4 * g + k
                        if c < limit:
                            lm, lr = _mr_push(lm, lr, t[:, c])
                tm, tr = _mr_merge(tm, tr, lm, lr)
        m, r = _mr_merge(m, r, tm, tr)
    lse2 = m.astype(np.float64) + np.log2(1.0 + r.astype(np.float64))
    lse = lse2 * LN2
    rows = np.arange(n)
    lab_col = labels.astype(np.int64)
    if mutant == 'label_logit_wrong_tile' and ntc > 1:
        lab_col = (lab_col + E) % C            # the label's logit read from the next class tile (same place in the tile, wrapped)
    tl = t[rows, lab_col].astype(np.float64)
    if mutant == 'label_logit_wrong_tile' and ntc == 1:
        tl = np.full(n, -np.inf)               # a single tile: the wrong tile is no tile, the empty state stays
    w64 = weights.astype(np.float64)
    with np.errstate(invalid='ignore'):
        loss = float(np.where(w64 != 0, w64 * ((lse2 - tl) * LN2), 0.0).sum())
    best = C - 1 - np.argmax(t[:, :C][:, ::-1], axis=1) if mutant == 'highest_index_maximum' else np.argmax(t[:, :C], axis=1)
    hits = float(w64[best == labels].sum())
    d = raw[:, :C].astype(np.float64) - lse[:, None]
    ws = (w64 * inv_S).astype(F32)
    G = ws[:, None] * np.exp2((d * 1.4426950408889634).astype(F32))
    G[rows, labels] = ws * np.expm1(d[rows, labels]).astype(F32)
    G = G.astype(F32)
    P, part_rows = row_parts(n, D, C)
    key = ('dW', hashlib.sha1(G.tobytes()).digest())
    if key not in share:
        dW = None
        for p in range(P):
            a = np.zeros((C, D), F32)
            for row in range(p * part_rows, min(n, (p + 1) * part_rows)):
                a = a + G[row, :, None] * x[row, None, :]
            dW = a if dW is None else dW + a
        share[key] = dW
    dW = share[key]
    db = G.astype(np.float64).sum(0).astype(F32)
    return dict(lse=lse, G=G, loss=loss, hits=hits, dW=dW, db=db)


# ---- gates ---------------------------------------------------------------------------------------------------------------------------------
NAMES = ('f', 'lse', 'G', 'dW', 'db')


def ulp32(x):
    return float(np.spacing(F32(abs(x))))


def gates(emulated, reference):
    """Per quantity: 4 x the emulation's largest error against float64, never below one float32 ulp of the largest float64 magnitude."""
    out = {}
    for k in NAMES:
        e, r = np.asarray(emulated[k], np.float64), np.asarray(reference[k], np.float64)
        out[k] = max(4.0 * float(np.abs(e - r).max()), ulp32(float(np.abs(r).max())))
    return out


def compare(got, reference, gate):
    """{name: (largest error, ok)}: finite and within the gate; hits are compared exactly."""
    out = {}
    for k in NAMES:
        err = float(np.abs(np.asarray(got[k], np.float64) - np.asarray(reference[k], np.float64)).max())
        out[k] = (err, bool(np.isfinite(err) and err <= gate[k]))
    out['hits'] = (abs(float(got['hits']) - float(reference['hits'])), float(got['hits']) == float(reference['hits']))
    return out


@functools.lru_cache(maxsize=None)
def case(n, D, C, family):
    """(inputs, float64 reference, emulation, gates) of a table case, computed once."""
    inp = case_inputs(n, D, C, family)
    ref = direct(*inp, L2[(n, D, C)])
    emu = emulate(*inp, L2[(n, D, C)], share=_shared(n, D, C, family))
    return inp, ref, emu, gates(emu, ref)


@functools.lru_cache(maxsize=2)
def _shared(n, D, C, family):
    return {}


def mutant_results(n, D, C, family):
    """{mutant: compare(...)} of a table case at its gates; the emulations share the case's accumulators."""
    inp, ref, emu, gate = case(n, D, C, family)
    share = _shared(n, D, C, family)
    return {m: compare(emulate(*inp, L2[(n, D, C)], mutant=m, share=share), ref, gate) for m in MUTANTS}
