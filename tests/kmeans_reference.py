"""Restatements of the k-means clustering evaluation (csrc/kmeans.hip, simclr_amd/kmeans.py) in numpy.

  assign64 / update64 / finish64 / lloyd64   float64, straight from the definition, for R replicas
  nmi / ari / many_to_one / matched_brute    the four scores, written independently of simclr_amd/kmeans.py
  emulate(...)                               the kernels' arithmetic: one float32 accumulator per score in k order (every product and
                                             every addition rounded: at least as many roundings as the MFMA makes), the arg-max with
                                             the lowest-index rule, double sums in ascending row order, the centroid rounded to float32
The gate of `best` and J is 4 x the error of emulate() against float64 on the same inputs, never below one float32 ulp of 1 (the
scores of unit rows are at most 1 in magnitude, J = 1 - a weighted mean of them).  Assignments, the changed count, the kept count, the
sums and wsum are exact once the assignments are (the products w x are exact in double and the order is the reference's); c_new is
gated at one float32 ulp of 1 (the rounding of the centroid).  MUTANTS are wrong readings the comparator must reject.
"""
import functools
import itertools

import numpy as np

from tests.logreg_reference import _accumulate

F32 = np.float32
ULP1 = float(np.spacing(F32(1.0)))
TINY_NORM2 = 1e-24

SHAPES = [(1, 64, 2), (2, 64, 2),                                   # the floor
          (65, 64, 63), (64, 128, 64), (130, 64, 65),               # row and centroid tile edges; (65, ..) a last row tile of one row
          (300, 2048, 129),                                         # many k stages, three centroid tiles
          (2049, 64, 2049)]                                         # the 128-wide tile (17 x 17 >= 256), one row / one centroid ragged
WIDE_SHAPE = (2049, 64, 2049)
FAMILIES = ('gauss', 'tight', 'padlast')
CASES = [(n, D, K, fam) for n, D, K in SHAPES for fam in FAMILIES]


def tile_edge(n, K):
    return 128 if -(-n // 128) * -(-K // 128) >= 256 else 64


def unit(a):
    a = np.asarray(a, np.float64)
    return (a / np.sqrt((a * a).sum(-1, keepdims=True))).astype(F32)


# ---- float64, from the definition ------------------------------------------------------------------------------------------------------
def scores64(x, c):
    s = np.asarray(x, np.float64) @ np.asarray(c, np.float64).T
    return np.where(np.isnan(s), -np.inf, s)                        # a NaN score orders below every number


def assign64(x, c):
    """(a [n] int32, best [n] float64): the lowest index of the maximum."""
    s = scores64(x, c)
    a = s.argmax(1)                                                 # numpy returns the first maximum
    return a.astype(np.int32), s[np.arange(len(a)), a]


def gap_threshold(D):
    return 4.0 * D * 2.0 ** -24


def gap_ok(x, c, weights):
    """Per row: weight 0, or the float64 gap between the two best DISTINCT centroids exceeds 4 D 2^-24 (bitwise equal centroids give
    bitwise equal scores on the device: the tie rule decides them exactly)."""
    _, first = np.unique(np.asarray(c, F32).view(np.uint32).reshape(len(c), -1), axis=0, return_index=True)
    s = scores64(x, np.asarray(c)[np.sort(first)])
    if s.shape[1] < 2:
        return np.ones(len(s), bool)
    top = np.sort(s, axis=1)
    return (top[:, -1] - top[:, -2] > gap_threshold(np.asarray(x).shape[1])) | ~(np.asarray(weights) > 0)


def objective64(best, weights):
    w = np.asarray(weights, np.float64)
    live = w > 0
    return float((w[live] * (1.0 - best[live])).sum()), float(w[live].sum())


def update64(x, weights, a, K, sums=None, wsum=None, ignore_weights=False):
    """sums [K, D], wsum [K]: the weighted rows added in ascending row order (the stable sort of the wrapper keeps it)."""
    x = np.asarray(x, np.float64)
    sums = np.zeros((K, x.shape[1])) if sums is None else sums.copy()
    wsum = np.zeros(K) if wsum is None else wsum.copy()
    part, wpart = np.zeros_like(sums), np.zeros_like(wsum)
    for r in range(len(x)):
        w = 1.0 if ignore_weights else float(weights[r])
        if 0 <= a[r] < K and w != 0.0:
            part[a[r]] += w * x[r]
            wpart[a[r]] += w
    return sums + part, wsum + wpart


def finish64(sums, wsum, c_prev, empty_to_zero=False, unnormalised=False):
    """(c_new float32 [K, D], kept, max_k (1 - c_new_k . c_prev_k))."""
    q = (sums * sums).sum(1)
    keep = ~(wsum > 0) | ~(q > TINY_NORM2) | ~np.isfinite(q)
    with np.errstate(invalid='ignore', divide='ignore'):
        c = sums if unnormalised else sums / np.sqrt(q)[:, None]
    c = np.where(keep[:, None], 0.0 if empty_to_zero else np.asarray(c_prev, np.float64), c).astype(F32)
    shift = 1.0 - (c.astype(np.float64) * np.asarray(c_prev, np.float64)).sum(1)
    return c, int(keep.sum()), float(shift.max())


def shards(n, R):
    return np.array_split(np.arange(n), R)


def iteration64(x, weights, c, R=1):
    """One Lloyd pass over R replicas (contiguous shards whose sums are added in replica order)."""
    K = len(c)
    a, best = assign64(x, c)
    sums, wsum = np.zeros((K, x.shape[1])), np.zeros(K)
    for sh in shards(len(x), R):
        s, w = update64(x[sh], np.asarray(weights)[sh], a[sh], K)
        sums, wsum = sums + s, wsum + w
    cost, S = objective64(best, weights)
    return a, best, sums, wsum, cost / S


def lloyd64(x, weights, c0, max_iterations=50, tolerance=1e-6, R=1):
    """dict(c, J, iterations, converged, empties, Js, assigns): the loop of simclr_amd/kmeans.py on the float64 definition."""
    c = np.asarray(c0, F32)
    prev, J_prev, out = np.full(len(x), -1), None, dict(Js=[], assigns=[], centroids=[], converged=False)
    live = np.asarray(weights) > 0
    for it in range(1, max_iterations + 1):
        a, best, sums, wsum, J = iteration64(x, weights, c, R)
        c_next, kept, _ = finish64(sums, wsum, c)
        changed = int((a[live] != prev[live]).sum())
        out['Js'].append(J); out['assigns'].append(a); out['centroids'].append(c)
        out.update(c=c, J=J, iterations=it, empties=kept)
        if changed == 0 or (J_prev is not None and J_prev - J <= tolerance * max(J_prev, 1e-30)):
            out['converged'] = True
            break
        if it == max_iterations:
            break
        c, J_prev, prev = c_next, J, a
    return out


def start_rows(weights, K, seed, restart):
    """Rows (global positions) restart `restart` starts from: the first K of a permutation of the rows of weight > 0."""
    cand = np.nonzero(np.asarray(weights) > 0)[0]
    return cand[np.random.default_rng([seed, restart]).permutation(len(cand))[:K]]


def fit64(x, weights, K, seed=0, restarts=1, max_iterations=50, tolerance=1e-6, R=1):
    runs = [lloyd64(x, weights, np.asarray(x)[start_rows(weights, K, seed, r)], max_iterations, tolerance, R) for r in range(restarts)]
    best = min(range(restarts), key=lambda r: (runs[r]['J'], r))
    return dict(runs[best], restart=best, runs=runs)


# ---- the scores --------------------------------------------------------------------------------------------------------------------------
def table(a, y, K, C, weights=None):
    T = np.zeros((K, C), np.int64)
    for i in range(len(a)):
        if weights is None or weights[i] > 0:
            T[a[i], y[i]] += 1
    return T


def nmi(T):
    T = np.asarray(T, np.float64)
    N = T.sum()
    pa, pb = T.sum(1) / N, T.sum(0) / N
    h = lambda p: -sum(v * np.log(v) for v in p if v > 0)
    ha, hb = h(pa), h(pb)
    if ha == 0 and hb == 0:
        return 1.0
    mi = sum(T[i, j] / N * np.log(T[i, j] / N / (pa[i] * pb[j])) for i in range(T.shape[0]) for j in range(T.shape[1]) if T[i, j] > 0)
    return mi / ((ha + hb) / 2)


def ari(T):
    T = np.asarray(T, np.int64)
    c2 = lambda v: v * (v - 1) // 2
    N = int(T.sum())
    sij, sa, sb, tot = int(c2(T).sum()), int(c2(T.sum(1)).sum()), int(c2(T.sum(0)).sum()), c2(N)
    if tot == 0:
        return 1.0
    exp, mx = sa * sb / tot, (sa + sb) / 2
    return 1.0 if mx == exp else (sij - exp) / (mx - exp)


def many_to_one(B, E):
    hits = 0
    for k in range(B.shape[0]):
        if B[k].sum() > 0:
            hits += E[k, int(np.argmax(B[k]))]
    return hits / E.sum()


def matched_brute(E):
    K = E.shape[0]
    return max(sum(E[k, p[k]] for k in range(K)) for p in itertools.permutations(range(K))) / E.sum()


# ---- kernel cases ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_inputs(n, D, K, family):
    """(x [n, D], weights [n], c [K, D], prev [n] int32) float32 unit rows, read-only.  For K >= 3 centroid 1 is a bitwise copy of
    centroid 0 (an exact tie the lowest-index rule decides: cluster 1 stays empty).  gauss: Gaussian unit rows, weights cycling through
    (0.5, 2, 1, 1.5), row 0 = centroid 0 itself; tight: row r sits next to centroid r mod K; padlast: every row sits next to centroid
    K - 1 and the last n // 3 rows carry weight 0.  A weighted row whose gap is not above the threshold is redrawn.  prev = the
    assignment the changed count is taken against: the float64 assignment with every third row set to -1."""
    rng = np.random.RandomState(100 * FAMILIES.index(family) + 7 * n + 3 * D + K)
    c = unit(rng.randn(K, D))
    if K >= 3:
        c[1] = c[0]
    weights = np.array([0.5, 2.0, 1.0, 1.5], F32)[np.arange(n) % 4]
    if family == 'padlast':
        weights = np.ones(n, F32)
        if n // 3:
            weights[n - n // 3:] = 0.0

    def draw(rows):
        g = rng.randn(len(rows), D)
        if family == 'tight':
            g = c[rows % K].astype(np.float64) + 0.3 * g / np.sqrt(D)
        elif family == 'padlast':
            g = c[K - 1].astype(np.float64) + 0.3 * g / np.sqrt(D)
        return unit(g)

    x = draw(np.arange(n))
    if family != 'padlast':
        x[0] = c[0]
    for _ in range(200):
        bad = np.nonzero(~gap_ok(x, c, weights))[0]
        if not len(bad):
            break
        x[bad] = draw(bad)
    else:
        raise AssertionError('case_inputs: rows without a top-1 gap remain')
    prev = assign64(x, c)[0].copy()
    prev[::3] = -1
    for a in (x, weights, c, prev):
        a.setflags(write=False)
    return x, weights, c, prev


NAMES = ('assign', 'best', 'J', 'S', 'changed', 'sums', 'wsum', 'c_new', 'kept')
MUTANTS = ('ties_to_highest', 'weights_ignored', 'empty_to_zero', 'unnormalised', 'last_tile_dropped')


def _result(x, weights, c, prev, a, best, mutant=None):
    live = np.asarray(weights) > 0
    cost, S = objective64(np.asarray(best, np.float64), weights)
    K = len(c)
    sums, wsum = update64(x, weights, a, K, ignore_weights=mutant == 'weights_ignored')
    c_new, kept, shift = finish64(sums, wsum, c, empty_to_zero=mutant == 'empty_to_zero', unnormalised=mutant == 'unnormalised')
    return dict(assign=np.asarray(a), best=np.asarray(best, np.float64), J=cost / S, S=S, changed=int((np.asarray(a)[live] != prev[live]).sum()),
                sums=sums, wsum=wsum, c_new=c_new.astype(np.float64), kept=kept, shift=shift)


def _pick(s, n, K, mutant):
    """Arg-max of a score matrix under the (mutated) tie and tile rules."""
    if mutant == 'last_tile_dropped':
        E = tile_edge(n, K)
        ntc = -(-K // E)
        if ntc > 1:
            s = s[:, :(ntc - 1) * E]
    a = s.shape[1] - 1 - s[:, ::-1].argmax(1) if mutant == 'ties_to_highest' else s.argmax(1)
    return a.astype(np.int32), s[np.arange(len(a)), a]


def direct(x, weights, c, prev, mutant=None):
    """The float64 definition (or a mutant of it)."""
    a, best = _pick(scores64(x, c), len(x), len(c), mutant)
    return _result(x, weights, c, prev, a, best, mutant)


def emulate(x, weights, c, prev, mutant=None, acc=None):
    """The kernels' arithmetic (or a mutant of it); acc = the float32 accumulators, shared between mutants of one case."""
    acc = _accumulate(x, c) if acc is None else acc
    a, best = _pick(np.where(np.isnan(acc), F32(-np.inf), acc), len(x), len(c), mutant)
    return _result(x, weights, c, prev, a, best, mutant)


def gates(emulated, reference):
    g = {k: max(4.0 * float(np.abs(np.asarray(emulated[k]) - np.asarray(reference[k])).max()), ULP1) for k in ('best', 'J')}
    g['c_new'] = ULP1
    return g


def compare(got, reference, gate, weights):
    """{name: (largest error, ok)}: assignments (of the rows of weight > 0), counts, sums and wsum exact; best, J and c_new gated."""
    live = np.asarray(weights) > 0
    out = {}
    for k in NAMES:
        g, r = np.asarray(got[k], np.float64), np.asarray(reference[k], np.float64)
        if k in ('assign', 'best'):
            g, r = g[live], r[live]
        err = float(np.abs(g - r).max()) if g.size else 0.0
        out[k] = (err, bool(np.isfinite(err) and err <= gate.get(k, 0.0)))
    return out


@functools.lru_cache(maxsize=None)
def case(n, D, K, family):
    """(inputs, float64 reference, emulation, gates, float32 accumulators) of a table case, computed once."""
    inp = case_inputs(n, D, K, family)
    acc = _accumulate(inp[0], inp[2])
    ref, emu = direct(*inp), emulate(*inp, acc=acc)
    return inp, ref, emu, gates(emu, ref), acc


def mutant_applies(mutant, n, D, K, family):
    """A mutant has something to change on a case where the mutated float64 DEFINITION itself misses the case's gates."""
    inp, ref, _, gate, _ = case(n, D, K, family)
    return not all(ok for _, ok in compare(direct(*inp, mutant=mutant), ref, gate, inp[1]).values())


# ---- the planted toy of the fit tests ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planted(n=512, D=64, groups=8, noise=0.1, seed=0):
    """(x [n, D] float32 unit rows, labels int32, weights -- the last three rows have weight 0): `groups` orthogonal directions plus
    noise, row r in group r mod groups.  The tests use seed 0 with K = 8 (--kmeans_seed 0, two restarts) and seed 2 with K = 12
    (--kmeans_seed 3, one restart, one cluster left empty): on both the float64 run keeps every assignment gap above the threshold."""
    rng = np.random.RandomState(seed)
    dirs = np.linalg.qr(rng.randn(D, groups))[0].T
    labels = (np.arange(n) % groups).astype(np.int32)
    x = unit(dirs[labels] + noise * rng.randn(n, D))
    weights = np.ones(n, F32)
    weights[-3:] = 0.0
    for a in (x, labels, weights):
        a.setflags(write=False)
    return x, labels, weights


def lloyd_gaps_ok(x, weights, run):
    """Every iteration of a float64 run has its assignment gaps above the threshold."""
    return all(bool(np.all(gap_ok(x, c, weights))) for c in run['centroids'])
