"""Float64 definition, planted-spectrum generator and float32 emulation for the eigen-spectrum evaluation (simclr_amd/spectrum.py,
csrc/spectrum.hip).  numpy, and torch on the CPU for the float32 accumulation: shared by tests/test_spectrum_reference.py (CPU) and tests/test_gpu_spectrum.py (device).

  counted      a row counts when its weight is > 0 (selected, never multiplied); S = the counted rows
  mu, C        mu = (1 / S) sum h_n,   C = (1 / (S - 1)) sum (h_n - mu)(h_n - mu)^T                                  float64
  raw          what the kernel returns: sum (h_n - mu32)(h_n - mu32)^T, mu32 = fp32(mu);   C = (raw - S delta delta^T) / (S - 1)
  gates        raw: 4 x the emulation's largest elementwise error, never below one float32 ulp of the largest entry of raw;
               Frobenius: 4 x the emulation's Frobenius error, never below D x that ulp (every entry off by the floor);
               C: the raw gates over S - 1;   eigenvalues (Weyl): the Frobenius gate of C plus LAPACK_REL x lambda_1
"""
import functools

import numpy as np
import torch

F32 = np.float32
EPS64 = float(np.finfo(np.float64).eps)
COLLAPSE = 1e-12
RANKME_EPS = 1e-7
ALPHA_MIN_POINTS = 8
MAX_PART_ROWS, STAGE, WORKGROUPS = 8192, 32, 256
# largest |eigvalsh(C) - eigvalsh(P C P^T)| / lambda_1 over the cases, x 4 (tests/golden/SPECTRUM_HAND_DERIVED.md section 6)
LAPACK_REL = 4 * 4.8e-15

SHAPES = [(2, 64),            # the floor: one part, one tile
          (65, 64),           # three row parts, the last one of a single row (the smallest such n at D = 64)
          (64, 128),          # the first off-diagonal tile (64-wide: 3 tile pairs)
          (130, 192),         # 6 tile pairs, D no multiple of 128
          (8200, 128),        # the 128-wide tile on its diagonal alone, 257 row parts, the last one of 8 rows
          (300, 2048)]        # the 128-wide tile, 136 tile pairs, 3 row parts
FAMILIES = ('gauss', 'mean5', 'rank5', 'nanpad')
CASES = [(n, D, fam) for n, D in SHAPES for fam in FAMILIES]
PLANTED_SHAPE = (300, 128)


# ---- the launch plan of csrc/spectrum.hip, restated -----------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def tile_edge(n, D):
    T = D // 128
    return 128 if D % 128 == 0 and (T * (T + 1) // 2) * _cdiv(n, STAGE) >= WORKGROUPS else 64


def row_plan(n, D):
    """(part_rows, parts): enough parts that pairs x parts workgroups fill the chip, none longer than MAX_PART_ROWS, whole stages."""
    e = tile_edge(n, D)
    T = D // e
    want = max(_cdiv(WORKGROUPS, T * (T + 1) // 2), _cdiv(n, MAX_PART_ROWS))
    part_rows = max(STAGE, _cdiv(n, want) // STAGE * STAGE)      # rounded down to whole stages: never fewer parts than wanted
    return part_rows, _cdiv(n, part_rows)


def smallest_three_part_ragged_n(D=64):
    for n in range(1, 65537):
        rows, parts = row_plan(n, D)
        if parts >= 3 and n % rows:
            return n


# ---- the float64 definition ---------------------------------------------------------------------------------------------------------
def counted(weights):
    return np.asarray(weights) > 0                       # a NaN weight fails the comparison


def colsum64(x, weights):
    keep = counted(weights)
    return np.asarray(x, np.float64)[keep].sum(0), int(keep.sum())


def cov64(x, weights):
    """(C, S, mu) in float64."""
    keep = counted(weights)
    h = np.asarray(x, np.float64)[keep]
    S = h.shape[0]
    mu = h.mean(0)
    xc = h - mu
    return xc.T @ xc / (S - 1), S, mu


def raw64(x, weights, mu32):
    """sum over the counted rows of (x - mu32)(x - mu32)^T in float64: what simclr_spectrum_cov is asked for."""
    keep = counted(weights)
    xc = np.asarray(x, np.float64)[keep] - np.asarray(mu32, np.float64)
    return xc.T @ xc


def finish(raw, S, mu, mu32, divisor=None):
    """C from the kernel's sum: the exact correction of the rounded mean, then the divisor."""
    delta = np.asarray(mu, np.float64) - np.asarray(mu32, np.float64)
    return (raw - S * np.outer(delta, delta)) / (divisor if divisor is not None else S - 1)


def eig64(C):
    return np.linalg.eigvalsh(np.asarray(C, np.float64))[::-1].copy()


def scores64(lam, rank_threshold=1e-6, alpha_first=10, alpha_last=0, rankme_on_lambda=False):
    """The table of the issue, restated independently of simclr_amd/spectrum.py (loops, no shared helper)."""
    lam = sorted((float(v) for v in np.asarray(lam, np.float64).reshape(-1)), reverse=True)
    negative = sum(1 for v in lam if v < 0)
    lam = np.array([max(v, 0.0) for v in lam])
    D, tr = len(lam), float(lam.sum())
    out = {'spectrum/trace': tr, 'spectrum/dim': D, 'spectrum/negative_eigenvalues': negative}
    if tr <= COLLAPSE:
        for k in ('rankme', 'participation_ratio', 'top1_share'):
            out['eval/spectrum_' + k] = 0.0
        for k in ('numerical_rank', 'dims_90', 'dims_99'):
            out['eval/spectrum_' + k] = 0
        return out
    s = lam if rankme_on_lambda else np.sqrt(lam)
    p = s / s.sum() + RANKME_EPS
    out['eval/spectrum_rankme'] = float(np.exp(-np.sum(p * np.log(p))))
    out['eval/spectrum_participation_ratio'] = tr ** 2 / float(np.sum(lam ** 2))
    rank = sum(1 for v in lam if v > rank_threshold * lam[0])
    out['eval/spectrum_numerical_rank'] = rank
    out['eval/spectrum_top1_share'] = float(lam[0] / tr)
    for key, share in (('eval/spectrum_dims_90', 0.9), ('eval/spectrum_dims_99', 0.99)):
        run, k = 0.0, 0
        while k < D:
            run += lam[k]
            k += 1
            if run >= share * tr:
                break
        out[key] = k
    last = min(alpha_last or rank, rank)
    if last - alpha_first + 1 >= ALPHA_MIN_POINTS:
        i = np.arange(alpha_first, last + 1)
        out['eval/spectrum_alpha'] = float(-np.polyfit(np.log(i), np.log(lam[alpha_first - 1:last]), 1)[0])
    return out


def score_gates(lam, g, alpha_first=10, alpha_last=0, rank_threshold=1e-6):
    """First-order bounds, doubled, on the change of rankme and alpha when every eigenvalue moves by at most g (g far below the
    smallest eigenvalue used: the caller asserts it).  rankme = exp(H), H = -sum p log p, p_i = sigma_i / T + eps, T = sum sigma:
    dH/dsigma_j = -(1/T)(log p_j + 1) + (1/T^2) sum_i sigma_i (log p_i + 1), dsigma/dlambda = 1 / (2 sigma).
    alpha = -sum u_i log lambda_i / sum u_i^2 with u = log i - mean: |d alpha| <= sum |u_i| (g / lambda_i) / sum u_i^2."""
    lam = np.asarray(lam, np.float64)
    sig = np.sqrt(lam)
    T = sig.sum()
    p = sig / T + RANKME_EPS
    lp = np.log(p) + 1.0
    dH = np.abs(-lp / T + (sig * lp).sum() / T ** 2) / (2.0 * sig)
    rankme = float(np.exp(-(p * np.log(p)).sum()))
    rank = int((lam > rank_threshold * lam[0]).sum())
    last = min(alpha_last or rank, rank)
    u = np.log(np.arange(alpha_first, last + 1))
    u = u - u.mean()
    return {'rankme': 2.0 * rankme * float(dH.sum()) * g,
            'alpha': 2.0 * float((np.abs(u) * g / lam[alpha_first - 1:last]).sum() / (u * u).sum())}


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def planted(n, D, lam, mean=0.0, seed=0):
    """X = sqrt(n - 1) U diag(sqrt lam) V^T + mean in float64: U [n, r] has orthonormal columns orthogonal to the ones vector, V [D, r]
    orthonormal columns, so the covariance is exactly V diag(lam) V^T before the rounding to float32.  r = len(lam) <= min(n - 1, D)."""
    lam = np.asarray(lam, np.float64)
    r = len(lam)
    assert r <= min(n - 1, D)
    rng = np.random.RandomState(seed)
    U = np.linalg.qr(np.concatenate([np.ones((n, 1)), rng.randn(n, r)], 1))[0][:, 1:]
    V = np.linalg.qr(rng.randn(D, D))[0][:, :r]
    return np.sqrt(n - 1.0) * (U * np.sqrt(lam)) @ V.T + mean


def planted_harmonic(seed=0):
    """The planted lambda_i = 1 / i spectrum at PLANTED_SHAPE, as float32 rows with weight 1."""
    n, D = PLANTED_SHAPE
    x = planted(n, D, 1.0 / np.arange(1, D + 1), mean=0.5, seed=seed).astype(F32)
    return x, np.ones(n, F32)


def case_inputs(n, D, family):
    """(x [n, D] float32, weights [n] float32), read-only."""
    rng = np.random.RandomState(1000 * D + n)
    w = np.ones(n, F32)
    if family == 'gauss':
        x = rng.randn(n, D)
    elif family == 'mean5':
        x = 5.0 + 0.9 * rng.randn(n, D)
    elif family == 'rank5':
        r = min(5, n - 1)
        x = planted(n, D, np.arange(5, 0, -1.0)[:r], mean=0.5, seed=n)
    elif family == 'nanpad':
        x = rng.randn(n, D)
        off = np.arange(n) % 3 == 1
        if n > 2:
            off[n - 1] = False               # the last row counts: the last row part is never empty
        x[off] = np.nan
        x[off & (np.arange(n) % 2 == 0), ::2] = np.inf
        w[off] = 0.0
    else:
        raise ValueError(family)
    x = x.astype(F32)
    x.setflags(write=False)
    w.setflags(write=False)
    return x, w


# ---- the float32 emulation of the kernel's arithmetic ----------------------------------------------------------------------------------
MUTANTS = ('uncentred', 'lower_unwritten', 'weight_multiplied', 'divisor_s', 'last_part_dropped')


def _products32(xc32, part_rows):
    """The row parts' xc^T xc, each accumulated in float32 four rows (one MFMA k-step) at a time, as float64 arrays."""
    n, D = xc32.shape
    xt = torch.from_numpy(np.ascontiguousarray(xc32))
    out = []
    for o in range(0, n, part_rows):
        acc = torch.zeros(D, D, dtype=torch.float32)
        for k in range(o, min(n, o + part_rows), 4):
            blk = xt[k:k + 4]
            acc.addmm_(blk.t(), blk)                     # acc + the four products in float32, in place (numpy's acc += blk.T @ blk, faster)
        out.append(acc.numpy().astype(np.float64))
    return out


def _add(parts):
    """The parts in ascending order, in double."""
    total = np.zeros_like(parts[0])
    for p in parts:
        total += p
    return total


def emulate(x, weights, mutant=None, base=None):
    """dict(sums, count, mu32, raw, C, parts): the kernel's arithmetic in numpy -- the same part boundaries, float32 within a part,
    double across the parts -- with the host's finish.  `mutant` plants one of MUTANTS; `base` = the unmutated result of the same
    inputs, whose per-part products the mutants that do not touch the product reuse."""
    x = np.asarray(x, F32)
    n, D = x.shape
    keep = counted(weights)
    sums, S = colsum64(x, weights)
    mu = sums / max(S, 1)
    mu32 = mu.astype(F32)
    part_rows, _ = row_plan(n, D)
    if base is not None and mutant in ('lower_unwritten', 'divisor_s', 'last_part_dropped'):
        parts = base['parts']
    else:
        with np.errstate(invalid='ignore', over='ignore'):
            if mutant == 'weight_multiplied':
                xc = (np.asarray(weights, F32)[:, None] * (x - mu32)).astype(F32)
            elif mutant == 'uncentred':
                xc = np.where(keep[:, None], x, F32(0)).astype(F32)
            else:
                xc = np.where(keep[:, None], x - mu32, F32(0)).astype(F32)
            parts = _products32(xc, part_rows)
    raw = _add(parts[:-1] if mutant == 'last_part_dropped' and len(parts) > 1 else parts)
    if mutant == 'uncentred':                # X^T X accumulated in float32; the mean terms subtracted afterwards, exactly
        m = mu32.astype(np.float64)
        raw = raw - np.outer(m, sums) - np.outer(sums, m) + S * np.outer(m, m)
    if mutant == 'lower_unwritten':
        raw = np.triu(raw)
    C = finish(raw, S, mu, mu32, divisor=S if mutant == 'divisor_s' else None) if S >= 2 else None
    return dict(sums=sums, count=S, mu=mu, mu32=mu32, raw=raw, C=C, parts=parts)


def emulate_raw(x, weights, mu32):
    """The kernel's sum for one call (a slab, or a replica's shard) given the rounded mean of the whole bank."""
    x = np.asarray(x, F32)
    with np.errstate(invalid='ignore', over='ignore'):
        xc = np.where(counted(weights)[:, None], x - np.asarray(mu32, F32), F32(0)).astype(F32)
    return _add(_products32(xc, row_plan(*x.shape)[0]))


def reference(x, weights):
    sums, S = colsum64(x, weights)
    mu = sums / max(S, 1)
    mu32 = mu.astype(F32)
    raw = raw64(x, weights, mu32)
    return dict(sums=sums, count=S, mu=mu, mu32=mu32, raw=raw, C=finish(raw, S, mu, mu32) if S >= 2 else None)


def ulp32(v):
    return float(np.spacing(F32(abs(v))))


def gates(emulated, ref):
    D = ref['raw'].shape[0]
    d = emulated['raw'] - ref['raw']
    floor = ulp32(np.abs(ref['raw']).max())
    g = {'raw': max(4.0 * float(np.abs(d).max()), floor), 'fro': max(4.0 * float(np.linalg.norm(d)), D * floor),
         'sums': 4.0 * EPS64 * float(np.abs(ref['sums']).max())}
    if ref['count'] >= 2:
        g['C'] = g['raw'] / (ref['count'] - 1)
        g['C_fro'] = g['fro'] / (ref['count'] - 1)
    return g


def compare(got, ref, gate):
    """{name: (error, ok)} of a result dict(sums, count, raw[, C]) against the reference."""
    res = {'count': (abs(got['count'] - ref['count']), got['count'] == ref['count']),
           'sums': (float(np.abs(got['sums'] - ref['sums']).max()), bool(np.abs(got['sums'] - ref['sums']).max() <= gate['sums']))}
    d = np.asarray(got['raw'], np.float64) - ref['raw']
    ok = bool(np.isfinite(d).all())
    res['raw'] = (float(np.abs(d).max()) if ok else np.inf, ok and bool(np.abs(d).max() <= gate['raw']))
    res['fro'] = (float(np.linalg.norm(d)) if ok else np.inf, ok and bool(np.linalg.norm(d) <= gate['fro']))
    if ref['C'] is not None and got.get('C') is not None:
        dc = np.asarray(got['C'], np.float64) - ref['C']
        okc = bool(np.isfinite(dc).all())
        res['C'] = (float(np.abs(dc).max()) if okc else np.inf, okc and bool(np.abs(dc).max() <= gate['C']))
    return res


@functools.lru_cache(maxsize=None)
def case(n, D, family):
    """(inputs, reference, emulation, gates) of one case; computed once and shared (treat as read-only)."""
    x, w = case_inputs(n, D, family)
    ref, emu = reference(x, w), emulate(x, w)
    return (x, w), ref, emu, gates(emu, ref)


def mutant_applies(mutant, n, D, family):
    """The cases on which a mutant MUST be rejected (elsewhere it may or may not be).  uncentred: needs means of the size of the
    deviations; weight_multiplied: needs a weight-0 row that is not finite; last_part_dropped: needs a second row part (the families
    count the last row, so it is never empty); divisor_s and lower_unwritten: need a covariance, so every case but the one with a single
    counted row, (n = 2, nanpad), whose sum is exactly zero."""
    if mutant == 'uncentred':
        return family == 'mean5'
    if mutant == 'weight_multiplied':
        return family == 'nanpad'
    if mutant == 'last_part_dropped':
        return row_plan(n, D)[1] > 1
    return not (family == 'nanpad' and n == 2)


def error_budget(x, weights, mu32, part_rows):
    """Elementwise bound on the emulation's (and the kernel's) error: a float32 accumulation of L terms errs by at most
    (L - 1 + 1) 2^-24 sum |terms| to first order (one rounding per product, one per addition), each centred factor carries one more
    rounding (2 x 2^-24 relative), so (L + 3) 2^-24 (|xc|^T |xc|)_ab with L the longest part, x 1.01 for the higher orders."""
    keep = counted(weights)
    a = np.abs(np.asarray(x, np.float64)[keep] - np.asarray(mu32, np.float64))
    return 1.01 * (min(part_rows, len(x)) + 3) * 2.0 ** -24 * (a.T @ a)
