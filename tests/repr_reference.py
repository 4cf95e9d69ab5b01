"""Restatements of the label-free representation diagnostics (csrc/repr.hip, metrics.representation_stats) in numpy.

z_all [2N, D]: l2-normalised rows, view a in rows [0, N), view b in rows [N, 2N).  Every function returns the four values
(align, uniform, std, rank) as a float64 array.

  direct(z_all, t)    float64, straight from the definition: explicit pairwise differences, the unbiased per-feature standard
                      deviation, eigvalsh of the covariance for the participation ratio
  gram(z_all, t)      float64, the Gram form the kernels use: distances and |C|_F^2 from G = xc xc^T
  emulate(z_all, t)   the kernels' arithmetic: the mean in double, xc ROUNDED to float32, r_a and the column sums of squares of the
                      rounded xc in double, G accumulated in float32, the epilogue and the sums in double, the final float32 store.
                      The MFMA's own order inside a 4-wide k step is not specified, so the emulation rounds every product and every
                      addition of the k-loop to float32: at least as many roundings as the device makes.
The gate of a device value is 4 x the error of emulate() against direct() on that case, never below one float32 ulp of the float64
value (the final store alone rounds by half of one): gates().  MUTANTS are wrong readings of the definition the comparator must
reject at those gates.
"""
import functools

import numpy as np

COLLAPSE = 1e-12        # tr C at or below this: PR = 0 (a definition, include/simclr_hip.h)
NAMES = ('align', 'uniform', 'std', 'rank')

# ---- the case table of tests/test_gpu_repr.py -------------------------------------------------------------------------------------
SHAPES = [(2, 64),                                  # the smallest
          (63, 64), (64, 64), (65, 128),            # the 64-tile edge
          (129, 192),                               # two 64-tiles plus one row, six k-stages
          (200, 256), (257, 64),                    # several tiles both ways
          (70, 2048), (66, 8192),                   # long k-loops
          (1409, 64), (1536, 64)]                   # the 128-wide tile (chosen from N = 1409): a last tile of one row, a full last tile
# the tile edge simclr_repr_tile_edge reports per shape: 128 where both views' tiles give >= 256 workgroups
EDGES = {(N, D): 128 if 2 * (-(-N // 128)) ** 2 >= 256 else 64 for N, D in SHAPES}
TS = (2.0, 5.0)
FAMILIES = ('gauss', 'rank5', 'clusters')
CASES = [(N, D, t, fam) for N, D in SHAPES for t in TS for fam in FAMILIES]


def normalize(h):
    h = np.asarray(h, np.float64)
    return h / np.sqrt((h * h).sum(1, keepdims=True))


@functools.lru_cache(maxsize=None)
def case_views(N, D, family):
    """float32 [2N, D], rows l2-normalised in float64 and rounded once.  gauss: correlated Gaussian views; rank5: rows in a
    5-dimensional subspace; clusters: ten tight clusters (close pairs exercise the r_a + r_b - 2 g cancellation)."""
    rng = np.random.RandomState(1000 * FAMILIES.index(family) + 7 * N + D)
    if family == 'gauss':
        a = rng.randn(N, D)
        b = 0.8 * a + 0.6 * rng.randn(N, D)
    elif family == 'rank5':
        basis = rng.randn(5, D)
        ca = rng.randn(N, 5)
        a, b = ca @ basis, (0.8 * ca + 0.6 * rng.randn(N, 5)) @ basis
    else:
        centres = normalize(rng.randn(10, D))
        which = np.arange(N) % 10
        a = centres[which] + 1e-3 * rng.randn(N, D)
        b = centres[which] + 1e-3 * rng.randn(N, D)
    z = np.concatenate([normalize(a), normalize(b)]).astype(np.float32)
    z.setflags(write=False)
    return z


def _views(z_all):
    z = np.asarray(z_all, np.float64)
    N = z.shape[0] // 2
    assert z.ndim == 2 and z.shape[0] == 2 * N and N >= 2
    return z[:N], z[N:], N


def trace_cov(z_all):
    """tr C of both views in float64 (the precondition of the device cases: far above COLLAPSE)."""
    za, zb, N = _views(z_all)
    return [float(((v - v.mean(0)) ** 2).sum() / (N - 1)) for v in (za, zb)]


def direct(z_all, t=2.0):
    za, zb, N = _views(z_all)
    D = za.shape[1]
    align = ((za - zb) ** 2).sum(1).mean()
    uniform = std = rank = 0.0
    off = ~np.eye(N, dtype=bool)
    for v in (za, zb):
        d2 = ((v[:, None, :] - v[None, :, :]) ** 2).sum(-1) if N * N * D <= 1 << 25 else \
            np.stack([((v - row) ** 2).sum(1) for row in v])
        uniform += 0.5 * np.log(np.exp(-t * d2[off]).mean())
        std += 0.5 * np.sqrt(D) * v.std(0, ddof=1).mean()
        xc = v - v.mean(0)
        if (xc * xc).sum() / (N - 1) > COLLAPSE:
            # the nonzero spectrum of C = xc^T xc / (N-1) is that of xc xc^T / (N-1): the smaller of the two matrices
            lam = np.linalg.eigvalsh((xc.T @ xc if D <= N else xc @ xc.T) / (N - 1))
            rank += 0.5 * lam.sum() ** 2 / (lam * lam).sum()
    return np.array([align, uniform, std, rank])


def _finish(pair, trs, g2s, exs, colsqs, N, D, pair_div=None, std_div=None):
    """The last launch: the four values from the per-view sums, in float64."""
    align = pair / N
    std = sum(0.5 * np.sqrt(D) * np.sqrt(c / (std_div or N - 1)).sum() / D for c in colsqs)
    rank = sum(0.0 if (tr / (N - 1) <= COLLAPSE or not g2 > 0.0) else 0.5 * tr * tr / g2 for tr, g2 in zip(trs, g2s))
    div = pair_div or N * (N - 1)
    uniform = sum(0.5 * np.log(e / div) for e in exs)
    return np.array([align, uniform, std, rank])


def gram(z_all, t=2.0):
    za, zb, N = _views(z_all)
    D = za.shape[1]
    off = ~np.eye(N, dtype=bool)
    trs, g2s, exs, colsqs = [], [], [], []
    for v in (za, zb):
        xc = v - v.mean(0)
        G = xc @ xc.T
        r = np.diag(G)
        d2 = np.maximum(r[:, None] + r[None, :] - 2.0 * G, 0.0)
        trs.append(r.sum()); g2s.append((G * G).sum()); exs.append(np.exp(-t * d2[off]).sum()); colsqs.append((xc * xc).sum(0))
    return _finish(((za - zb) ** 2).sum(), trs, g2s, exs, colsqs, N, D)


@functools.lru_cache(maxsize=None)
def _emulated_parts(key, centred=True):
    """Per view (xc64 of the rounded float32 xc, G float32-accumulated) of a table case -- independent of t, so computed once."""
    z32 = case_views(*key)
    return _parts(z32, centred)


def _parts(z32, centred=True):
    assert z32.dtype == np.float32
    N = z32.shape[0] // 2
    out = []
    for v in (z32[:N], z32[N:]):
        v64 = v.astype(np.float64)
        xc = (v64 - v64.sum(0) / N).astype(np.float32) if centred else v.copy()
        acc = np.zeros((N, N), np.float32)
        for k in range(xc.shape[1]):
            col = xc[:, k]
            acc = acc + col[:, None] * col[None, :]            # float32 product, float32 addition
        out.append((xc.astype(np.float64), acc.astype(np.float64)))
    return out


def emulate(z32, t=2.0, key=None, mutant=None):
    """The kernels' arithmetic on float32 input; `key` = (N, D, family) of a table case reuses its cached Gram emulation.
    mutant: one of MUTANTS (a wrong reading of the definition), None = the definition."""
    z32 = np.asarray(z32)
    assert z32.dtype == np.float32
    N, D = z32.shape[0] // 2, z32.shape[1]
    parts = _emulated_parts(key) if key is not None else _parts(z32)
    z64 = z32.astype(np.float64)
    pair = ((z64[:N] - z64[N:]) ** 2).sum()
    c = -float(np.float32(t)) * 1.4426950408889634
    off = ~np.eye(N, dtype=bool)
    trs, g2s, exs, colsqs = [], [], [], []
    for v, (xc, G) in enumerate(parts):
        r = (xc * xc).sum(1)
        ex = np.exp2(c * np.maximum(r[:, None] + r[None, :] - 2.0 * G, 0.0))
        trs.append(r.sum()); colsqs.append((xc * xc).sum(0))
        g2s.append((G * G)[off].sum() if mutant == 'pr_diagonal_dropped' else (G * G).sum())
        exs.append(ex.sum() if mutant == 'uniform_counts_diagonal' else ex[off].sum())
    if mutant == 'pr_uncentred':
        raw = _emulated_parts(key, False) if key is not None else _parts(z32, False)
        trs = [np.diag(G).sum() for _, G in raw]
        g2s = [(G * G).sum() for _, G in raw]
    out = _finish(pair, trs, g2s, exs, colsqs, N, D, pair_div=N * N if mutant == 'uniform_divisor_n2' else None,
                  std_div=N if mutant == 'std_divisor_n' else None)
    if mutant == 'uniform_pooled_views':
        # one pool of 2N points: the cross-view pairs, the positives among them, are counted too
        d2 = np.stack([((z64 - row) ** 2).sum(1) for row in z64])
        out[1] = np.log(np.exp2(c * d2[~np.eye(2 * N, dtype=bool)]).mean())
    return out.astype(np.float32).astype(np.float64)            # the final float32 store


# wrong readings of the definition -> the output each one changes
MUTANTS = {'uniform_counts_diagonal': 'uniform', 'uniform_divisor_n2': 'uniform', 'uniform_pooled_views': 'uniform',
           'pr_uncentred': 'rank', 'pr_diagonal_dropped': 'rank', 'std_divisor_n': 'std'}


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def gates(emulated, reference):
    """Per output: 4 x the emulation's own error against float64, never below one float32 ulp of the float64 value."""
    return np.array([max(4.0 * abs(e - r), ulp32(r)) for e, r in zip(emulated, reference)])


def compare(got, reference, gate):
    """(errors, ok) per output: |got - reference| <= gate, and finite."""
    err = np.abs(np.asarray(got, np.float64) - reference)
    return err, np.isfinite(err) & (err <= gate)


@functools.lru_cache(maxsize=None)
def case(N, D, t, family):
    """(z32, float64 reference, emulation, gates) of a table case."""
    z = case_views(N, D, family)
    ref = direct(z, t)
    emu = emulate(z, t, key=(N, D, family))
    return z, ref, emu, gates(emu, ref)


# The largest error of emulate() against direct() over CASES, per output, in float32 ulps of the float64 value (re-measured by
# tests/test_repr_reference.py; recorded in tests/golden/REPR_HAND_DERIVED.md).  The device gates are 4 x the per-case figures.
# Measured: align 0.49 (the store alone), uniform 1.89 and rank 4.37 (both at D = 8192: the float32 accumulation over 8192 k), std 0.50.
EMULATION_BUDGET_ULPS = {'align': 0.5, 'uniform': 2.0, 'std': 0.75, 'rank': 5.0}


# ---- hand cases (tests/golden/REPR_HAND_DERIVED.md) -----------------------------------------------------------------------------------
def hand_basis(N=64):
    """N = D signed basis rows, the same in both views: (0, -2t, 1, N-1)."""
    signs = np.where(np.arange(N) % 3 == 0, -1.0, 1.0)
    z = np.diag(signs).astype(np.float32)
    return np.concatenate([z, z])


def hand_antipodal(N=64, D=64):
    """Rows alternating +-e_1, view b = -view a: align 4, uniform log((N(N/2-1) + N(N/2) e^(-4t)) / (N(N-1))),
    std sqrt(N/(N-1))/sqrt(D), rank 1."""
    z = np.zeros((N, D), np.float32)
    z[:, 0] = np.where(np.arange(N) % 2 == 0, 1.0, -1.0)
    return np.concatenate([z, -z])


def hand_antipodal_values(N=64, D=64, t=2.0):
    return np.array([4.0, np.log((N * (N / 2 - 1) + N * (N / 2) * np.exp(-4.0 * t)) / (N * (N - 1))),
                     np.sqrt(N / (N - 1)) / np.sqrt(D), 1.0])


def hand_collapsed(N=48, D=64):
    """Identical rows everywhere: (0, 0, 0, 0), bitwise on the device."""
    row = normalize(np.arange(1, D + 1, dtype=np.float64)[None])[0].astype(np.float32)
    return np.tile(row, (2 * N, 1))
