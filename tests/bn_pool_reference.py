"""Lattice inputs and plain references for the BatchNorm (csrc/bn.hip) and stem BN+ReLU+max-pool (csrc/pool.hip) kernel checks.

Pure torch on the CPU: shared by tests/gpu_checks.py (the GPU checks) and tests/test_bn_pool_reference.py (which pins it without a GPU).

The lattice: x, dy, residual and mask source are multiples of 1/4 in [-4, 4]; scale in {0, +-1/2, +-1, +-2, 1/4}; shift and mean
multiples of 1/4 in [-2, 2]; rstd in {1/4, 1/2, 1, 2}; c1 multiples of 1/8 in [-1/2, 1/2]; c2 in {0, 1/2, -1/4, 1/8}.  Every
intermediate of the kernels' fp32 arithmetic is then a dyadic rational that fp32 holds exactly, so neither the order of a sum nor the
contraction of a multiply-add changes a bit and a kernel is compared with tolerance ZERO.  That is checked, not assumed: every reference
below takes the dtype it evaluates in, and `assert_exact` requires the float32 evaluation to equal the float64 one bit for bit.
"""
import torch

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16

SCALES = (0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0, 0.25)
RSTDS = (0.25, 0.5, 1.0, 2.0)
C2S = (0.0, 0.5, -0.25, 0.125)


def _choice(values, n, g):
    return torch.tensor(values, dtype=F64)[torch.randint(0, len(values), (n,), generator=g)]


def quarters(shape, lim, g):
    """Multiples of 1/4 in [-lim, lim], uniform."""
    return torch.randint(-4 * lim, 4 * lim + 1, tuple(shape), generator=g).double() / 4


def lattice_params(C, g):
    """Per-channel lattice vectors (float64; exact in fp32).  Channels 1 and 2 are pinned to a zero and a negative scale so that even the
    narrowest tensors (C = 4) carry both."""
    scale = _choice(SCALES, C, g)
    if C >= 3:
        scale[1], scale[2] = 0.0, -0.5
    return dict(scale=scale, shift=quarters((C,), 2, g), mean=quarters((C,), 2, g), rstd=_choice(RSTDS, C, g),
                c1=torch.randint(-4, 5, (C,), generator=g).double() / 8, c2=_choice(C2S, C, g),
                rscale=_choice(SCALES, C, g), rshift=quarters((C,), 2, g))


def lattice(shape, seed=0, names=('x', 'dy')):
    """shape = (..., C).  Returns a dict of float64 tensors: the per-channel vectors of lattice_params and one activation-shaped tensor
    of multiples of 1/4 in [-4, 4] per name in `names`."""
    g = torch.Generator().manual_seed(seed)
    L = lattice_params(shape[-1], g)
    for n in names:
        L[n] = quarters(shape, 4, g)
    return L


def assert_survives(L, dtype):
    """Storage dtype: every lattice tensor is unchanged by the conversion (bf16: 8 significant bits)."""
    for k, v in L.items():
        assert torch.equal(v.to(dtype).double(), v), 'lattice tensor %s does not survive %s' % (k, dtype)


def assert_exact(fn, what=''):
    """fn(dtype) -> tensor or tuple/dict of tensors, evaluated in float32 and in float64: the two must agree exactly and be finite.
    Returns the float64 evaluation."""
    r32, r64 = fn(F32), fn(F64)

    def walk(a, b, path):
        if isinstance(a, dict):
            assert a.keys() == b.keys()
            for k in a:
                walk(a[k], b[k], path + '.' + str(k))
        elif isinstance(a, (tuple, list)):
            assert len(a) == len(b)
            for i, (p, q) in enumerate(zip(a, b)):
                walk(p, q, path + '[%d]' % i)
        elif a is not None:
            assert a.dtype in (F32, torch.uint8, torch.int64, torch.bool) and bool(torch.isfinite(b.double()).all()), path
            assert torch.equal(a.double(), b.double()), 'float32 evaluation of %s%s differs from float64: the lattice is not exact here' % (what, path)
    walk(r32, r64, '')
    return r64


def lattice_shares(L, ksz=3, stride=2):
    """The conditions the checks assert on their data: shares of pooling windows with a tied positive maximum / with maximum exactly 0,
    of BN outputs exactly 0 before the ReLU, of negative and of zero per-channel scales."""
    pre = L['x'] * L['scale'] + L['shift']
    out = dict(pre_zero=float((pre == 0).double().mean()), scale_neg=float((L['scale'] < 0).double().mean()),
               scale_zero=float((L['scale'] == 0).double().mean()))
    if L['x'].dim() == 4:
        taps = _window_taps(torch.relu(pre), ksz, stride)                   # [k*k, V, OH, OW, C], -inf outside the map
        best = taps.max(0).values
        ntie = (taps == best).sum(0)
        out['win_tied_pos'] = float(((best > 0) & (ntie >= 2)).double().mean())
        out['win_zero'] = float((best == 0).double().mean())
    return out


# ------------------------------------------------------------------------------------------------------------ max-pool
def same_pad(size, k, s):
    """TensorFlow 'SAME': (output size, pad before, pad after)."""
    out = -(-size // s)
    total = max((out - 1) * s + k - size, 0)
    return out, total // 2, total - total // 2


def _window_taps(act, ksz, stride):
    """act [V,H,W,C] -> [ksz*ksz, V, OH, OW, C]: tap (ky, kx) of every window in row-major tap order, -inf where the tap is off the map."""
    V, H, W, C = act.shape
    OH, pt, pb = same_pad(H, ksz, stride)
    OW, pl, pr = same_pad(W, ksz, stride)
    pad = torch.full((V, H + pt + pb, W + pl + pr, C), float('-inf'), dtype=act.dtype)
    pad[:, pt:pt + H, pl:pl + W] = act
    return torch.stack([pad[:, ky:ky + stride * (OH - 1) + 1:stride, kx:kx + stride * (OW - 1) + 1:stride]
                        for ky in range(ksz) for kx in range(ksz)])


def bnrelu_maxpool_ref(x, scale, shift, dy=None, ksz=3, stride=2, dtype=F64):
    """relu(x*scale+shift) -> max-pool(ksz, stride, SAME), written out: for every output pixel the in-bounds taps are scanned in (ky, kx)
    row-major order with a strict `>` starting from -inf, so the FIRST maximal tap wins (also in a window whose maximum is 0).
    Returns dict(y, tap[uint8, ky*ksz+kx], dact (dy routed to the winner's input pixel = the max-pool backward), dpre (dact * [pre > 0])).
    No F.max_pool2d: torch's tie rule decides nothing here."""
    x, scale, shift = x.to(dtype), scale.to(dtype), shift.to(dtype)
    V, H, W, C = x.shape
    pre = x * scale + shift
    taps = _window_taps(torch.relu(pre), ksz, stride)
    best = torch.full(taps.shape[1:], float('-inf'), dtype=dtype)
    tap = torch.zeros(taps.shape[1:], dtype=torch.int64)
    for t in range(ksz * ksz):
        upd = taps[t] > best
        best = torch.where(upd, taps[t], best)
        tap = torch.where(upd, torch.full_like(tap, t), tap)
    out = dict(y=best, tap=tap.to(torch.uint8))
    if dy is not None:
        dy = dy.to(dtype)
        OH, pt, pb = same_pad(H, ksz, stride)
        OW, pl, pr = same_pad(W, ksz, stride)
        dpad = torch.zeros(V, H + pt + pb, W + pl + pr, C, dtype=dtype)
        for t in range(ksz * ksz):
            ky, kx = divmod(t, ksz)
            dpad[:, ky:ky + stride * (OH - 1) + 1:stride, kx:kx + stride * (OW - 1) + 1:stride] += torch.where(tap == t, dy, torch.zeros_like(dy))
        out['dact'] = dpad[:, pt:pt + H, pl:pl + W].contiguous()
        out['dpre'] = out['dact'] * (pre > 0).to(dtype)
    return out


# ------------------------------------------------------------------------------------------------------------ BatchNorm
def bn_apply_ref(L, relu, res_mode, dtype=F64):
    """y = act(x*scale + shift [+ res | + res*rscale + rshift])"""
    t = lambda k: L[k].to(dtype)
    y = t('x') * t('scale') + t('shift')
    if res_mode == 1:
        y = y + t('res')
    elif res_mode == 2:
        y = y + (t('res') * t('rscale') + t('rshift'))
    return torch.relu(y) if relu else y


def bn_masked_dy(L, mask_mode, dtype=F64):
    """The gradient the BatchNorm backward sees: 0 none, 1 where mask_src > 0, 2 where x*scale+shift > 0."""
    t = lambda k: L[k].to(dtype)
    if mask_mode == 1:
        return t('dy') * (t('msk') > 0).to(dtype)
    if mask_mode == 2:
        return t('dy') * ((t('x') * t('scale') + t('shift')) > 0).to(dtype)
    return t('dy')


def bn_bwd_ref(L, dm, dtype=F64, perm=None):
    """(sum dm, sum dm*x^, dx = scale*(dm - c1 - x^*c2)) over all leading axes; perm: the order in which the rows are added."""
    t = lambda k: L[k].to(dtype)
    C = dm.shape[-1]
    dm = dm.to(dtype)
    xh = (t('x') - t('mean')) * t('rstd')
    a, b = dm.reshape(-1, C), (dm * xh).reshape(-1, C)
    if perm is not None:
        a, b = a[perm], b[perm]
    return a.sum(0), b.sum(0), t('scale') * (dm - t('c1') - xh * t('c2'))


def row_perm(rows, seed=1):
    return torch.randperm(rows, generator=torch.Generator().manual_seed(seed))


def round_to(v, dtype):
    """The exact value rounded ONCE (to nearest even) to the storage type, as float64."""
    return v.float().to(dtype).double()


def stream_rows(C, dtype):
    """Row counts of the streaming BatchNorm checks at width C: 1, 3, 37, 515 and the three around the smallest row count whose chunk count
    rows * C/EPC is a multiple of the 256 U chunks one workgroup of bn_apply / bn_bwd_apply owns (U = 2 when 256 % (C/EPC) == 0)."""
    import math
    cpr = C // (8 if dtype == torch.bfloat16 else 4)
    per_wg = 256 * (2 if 256 % cpr == 0 else 1)
    on = per_wg // math.gcd(per_wg, cpr)
    return sorted({1, 3, 37, 515} | {r for r in (on - 1, on, on + 1) if r >= 1})


# ------------------------------------------------------------------------------------------------------------ finalize
U32 = 2.0 ** -23          # one fp32 ulp, relative: a value rounded to fp32 moves by at most U32 / 2 of its magnitude


def bn_finalize_ref(sums, count, gamma, beta, mm, mv, decay, eps):
    """simclr_bn_finalize from exact sums [2, C] (float64 holding integers / dyadics exactly): mean and the biased variance in EXACT
    rational arithmetic (so the cancellation s2/count - mean^2 costs the reference nothing), everything after in float64.  decay and eps
    are taken as the fp32 values the kernel receives.  gamma / beta / mm / mv may be None.

    Returns (ref, tol): the values and, for each, the bound of |kernel - ref| that follows from the kernel's rounding steps, with
    U = 2^-23 (every fp32 rounding moves a value by <= U/2 of its magnitude; halves are rounded up to whole U, which also absorbs the
    second-order terms and the 2^-53 roundings of the fp64 steps):
      var_d  = s2/count - mean_d^2 in fp64: |var_d - var| <= 2^-51 (s2/count + mean^2) =: cancel           (three fp64 roundings;
               0 where the exact variance is below -cancel: the kernel's is then negative too and clamps to exactly 0)
      mean   = fp32(mean_d)                                             ->  1 U |mean|
      rstd   = fp32(1 / sqrt(var_d + eps))                              ->  rstd (1 U + kappa),  kappa = cancel / (var + eps)
      scale  = fp32(g * rstd)                 [rstd U/2, product U/2]   ->  |scale| (2 U + kappa)
      shift  = fp32(b - fp32(fp32(mean * g) * rstd))
               [P = mean g rstd: mean U/2, product U/2, rstd U/2, product U/2 = 2 U -> 3 U; the subtraction U/2 -> 1 U]
                                                                        ->  U (3 |P| + |shift|) + |P| kappa
      moving_mean = fp32(fp32(mm * decay) + fp32(mean * (1 - decay)))
               [first product U/2 -> 1 U; mean U/2 + product U/2 -> 2 U; the sum U/2 -> 1 U; 1 - decay is exact for decay in [1/2, 1]]
                                                                        ->  U (|mm decay| + 2 |mean (1 - decay)| + |result|)
      moving_var  likewise with fp32(var_d)                             ->  U (|mv decay| + 2 |var (1 - decay)| + |result|) + 2 cancel (1 - decay)
    A contracted multiply-add only removes roundings from these chains."""
    from fractions import Fraction
    import numpy as np
    C = sums.shape[1]
    decay = float(np.float32(decay))
    eps = float(np.float32(eps))
    omd = float(np.float32(1.0) - np.float32(decay))
    assert 0.5 <= decay <= 1.0 and omd == 1.0 - decay, 'fp32 (1 - decay) must be exact'
    mean, var, e2, vtrue = (torch.empty(C, dtype=F64) for _ in range(4))
    clamped = torch.zeros(C, dtype=torch.bool)
    cnt = Fraction(count)
    for c in range(C):
        m = Fraction(float(sums[0, c])) / cnt
        q = Fraction(float(sums[1, c])) / cnt
        v = q - m * m
        clamped[c] = v <= 0
        mean[c], var[c], e2[c], vtrue[c] = float(m), float(max(v, 0)), float(q), float(v)
    one, zero = torch.ones(C, dtype=F64), torch.zeros(C, dtype=F64)
    g = gamma.double() if gamma is not None else one
    b = beta.double() if beta is not None else zero
    rstd = 1.0 / torch.sqrt(var + eps)
    P = mean * g * rstd
    cancel = 2.0 ** -51 * (e2 + mean * mean)
    # a variance below -cancel is negative in the kernel's fp64 too: it clamps to exactly 0 and the cancellation costs nothing
    cancel = torch.where(vtrue < -cancel, torch.zeros_like(cancel), cancel)
    kappa = cancel / (var + eps)
    ref = dict(mean=mean, rstd=rstd, scale=g * rstd, shift=b - P)
    tol = dict(mean=U32 * mean.abs(), rstd=rstd * (U32 + kappa), scale=ref['scale'].abs() * (2 * U32 + kappa),
               shift=U32 * (3 * P.abs() + ref['shift'].abs()) + P.abs() * kappa)
    if mm is not None:
        ref['moving_mean'] = mm.double() * decay + mean * omd
        tol['moving_mean'] = U32 * ((mm.double() * decay).abs() + 2 * (mean * omd).abs() + ref['moving_mean'].abs())
    if mv is not None:
        ref['moving_var'] = mv.double() * decay + var * omd
        tol['moving_var'] = U32 * ((mv.double() * decay).abs() + 2 * (var * omd).abs() + ref['moving_var'].abs()) + 2 * cancel * omd
    return ref, tol, dict(clamped=clamped, kappa=kappa)


def slot_partials(nslot, C, seed=0, constant_channels=()):
    """[nslot, 2, C] fp32 partial statistics of 16 rows per slot, small integers: s1 in [-16, 16], s2 in [32, 64] (so that the variance
    at count = 16 nslot lies in [1, 4]).  constant_channels: a channel whose 16 nslot rows all hold m = fp32(1000.3) -- s1 = 16 m exactly,
    s2 = the fp32 number just BELOW 16 m^2 (a rounded-down accumulation), so that s2/count - mean^2 is negative by about 2^-24 m^2."""
    import numpy as np
    g = torch.Generator().manual_seed(seed)
    p = torch.empty(nslot, 2, C, dtype=F32)
    p[:, 0] = torch.randint(-16, 17, (nslot, C), generator=g).float()
    p[:, 1] = torch.randint(32, 65, (nslot, C), generator=g).float()
    m = np.float32(1000.3)
    s2 = np.nextafter(np.float32(16.0 * float(m) * float(m)), np.float32(0))
    assert float(s2) < 16.0 * float(m) * float(m)
    for c in constant_channels:
        p[:, 0, c] = float(np.float32(16) * m)
        p[:, 1, c] = float(s2)
    return p


# ------------------------------------------------------------------------------------------------------------ folded backward
def bn_fold_coeffs_ref(L, dtype=F64):
    """a = scale, b = -scale c2 rstd, d = scale (c2 mean rstd - c1)"""
    t = lambda k: L[k].to(dtype)
    return t('scale'), -t('scale') * t('c2') * t('rstd'), t('scale') * (t('c2') * t('mean') * t('rstd') - t('c1'))


def bn_fold_post_ref(a, b, d, t1, gw, cs, dw0, dtype=F64):
    """dw = a t1 + b gw + cs (x) d  (+ dw0)"""
    a, b, d, t1, gw, cs = (v.to(dtype) for v in (a, b, d, t1, gw, cs))
    v = a * t1 + (b * gw + d * cs[:, None])
    return v if dw0 is None else dw0.to(dtype) + v
