"""Integer-lattice inputs, plain references and the case table of the implicit-GEMM convolution checks (csrc/conv.hip, csrc/igemm_wide.h,
csrc/igemm_nwalk.h): forward, data gradient, weight gradient, the statistics / BatchNorm-backward-reduce / fused BatchNorm-apply epilogues.

Pure torch on the CPU (no device, no library call): shared by tests/gpu_checks.py (check_conv_lattice, the GPU side), by
tests/test_conv_reference.py (which pins the references and, in a dry run of the library, the kernel family every row reaches) and by
tests/test_gpu_conv_lattice.py.  The lattice helpers (assert_exact, assert_survives, round_to, lattice_params) are those of
tests/bn_pool_reference.py.

The lattice: x and dy are integers in [-2, 2], w is in {-1, 0, 1}, the accumulate operand `prev` integers in [-4, 4]; the BatchNorm
vectors of the fused epilogues come from lattice_params, their activation-shaped operands (the BatchNorm input of the data gradient's
producer, the mask source, the residual) are multiples of 1/4 in [-4, 4].  The density of w is thinned by the reduction length until
every output is an integer of magnitude <= 256 and every per-channel sum of squares stays below 2^24.  Every product and every partial
sum of the kernels -- in each of the matrix arithmetics (bf16 storage; fp32 storage with the exact fp32 MFMA, three or six bf16-piece
terms, three fp16-piece terms of 2^8 w) -- is then an integer (or a multiple of 2^-6 in the BatchNorm-backward sums) that fp32 holds
exactly, whatever the summation order, the split tail's exchange through its fp32 scratch or the weight gradient's slab sum: a kernel
is compared with these references at tolerance ZERO.  That is asserted, not assumed: `reference(case)` evaluates every output in
float32 and in float64 (assert_exact; the statistics with the rows added in a random order), checks that every operand survives its
storage type, bounds the magnitude of every order-dependent partial sum (the sum of the absolute values of its terms, in units of the
terms' common grain, stays below 2^24) and asserts floors on the shares of non-zero outputs, masked-off elements, mask arguments that
are exactly 0 and border pixels.

What the kernels compute, where that differs from the obvious (documented in include/simclr_hip.h):
  * the forward statistics are those of the fp32 accumulators on the 128-wide tiles and the eight-phase tile, and those of the
    bf16-ROUNDED outputs on the 256 x 256 instantiation of the persistent kernel (simclr_conv2d_fwd); on the lattice the two agree
    except in the two designated rounding rows (`dense`), whose outputs exceed 8 significant bits;
  * simclr_conv2d_fwd_pivoted fills its slots with sum(y - pivot), sum((y - pivot)^2), pivot = y at pixel (0, OH/2, OW/2);
    simclr_bn_reduce_slots_pivoted turns them into the raw moments; with Cout > 4096 the pivot is zero and the slots hold raw moments
    (the comment above simclr_conv2d_fwd_pivoted in csrc/conv.hip);
  * bf16 storage with a channel count of the output that is no multiple of 8 runs the non-persistent kernel (plan_igemm, odd_n);
  * simclr_conv2d_dgrad_bn accumulates sum(dm) and the raw moment sum(dm * x) and converts the latter per slot,
    (sum(dm x) - mean sum(dm)) * rstd = sum(dm * x^); mask mode 4 produces sum(dm) only (the second row of the slots is not compared);
  * simclr_conv2d_fwd_bn_apply computes act(T(conv) * scale + shift + r) from the convolution output ROUNDED to the storage type T;
  * simclr_conv2d_dgrad_ext / _bn_ext (`ext` rows) reduce over K = Cout + Cin from two operand streams, dx (+)= dm Wext[:, :Cout]^T +
    h Wext[:, Cout:]^T + bias: the data-gradient reference on the concatenated operands, w_ext thinned by Cout + Cin, an integer bias;
  * accumulate = 3 (`sparse` rows, 1x1 stride 2) stores the even (row, column) pixels and leaves every other element of dx as it was;
    accumulate = 2 adds earlier data at those even pixels only and stores elsewhere, whatever the other elements hold (SENTINEL here).
The stem chain and the Gram chain have a sibling table, tests/stem_gram_reference.py.
"""
import math
import re
import types
import zlib

import torch

from tests.bn_pool_reference import BF16, F32, F64, assert_exact, assert_survives, lattice_params, quarters, round_to, row_perm

# arithmetic -> (storage type, forward terms, backward terms): simclr_amd.ops.F32_MATMUL_TERMS
ARITH = {'bf16': (BF16, 0, 0), 'exact': (F32, 0, 0), 'bf16x3': (F32, 3, 3), 'bf16x6': (F32, 6, 6), 'bf16x6_3': (F32, 6, 3),
         'f16x3_3': (F32, 13, 3)}
DT_F32, DT_BF16 = 0, 1
PS_IN, PS_W = 0x100, 0x100000            # SIMCLR_FMT_PS_IN, SIMCLR_FMT_PS_W
F16_WSCALE = 256.0                       # 2^F16_WSCALE_LOG2: the fp16 pieces of the three-term forward hold 2^8 w
LIMIT = float(2 ** 24)
SENTINEL = 12345.0                       # what dx holds before a sparse store (finite: a leak shows as a wrong number, not as a masked compare)


def terms_field(t):
    """SIMCLR_FMT_TERMS(t)"""
    return (t + 1) << 12


def out_hw(H, W, k, s):
    """Conv2dFixedPadding: k - 1 zeros in all (pad = (k - 1) // 2 before), then a VALID convolution of stride s."""
    return (H + (k - 1) - k) // s + 1, (W + (k - 1) - k) // s + 1


def persistent_grid(M, N, narrow=False):
    """igemm_persistent_grid of csrc/conv.hip: (tile width, N-tiles, workgroups) of the 128-row persistent tile."""
    BN = 64 if (N <= 64 or narrow) else 128
    m_tiles = (M + 127) // 128
    nt = -(-N // BN)
    unit = 8 * nt
    pg = max(unit, ((3 if BN == 64 else 2) * 256 // unit) * unit)
    return BN, nt, min(pg, -(-m_tiles // 8) * unit)


def wide_grid(M, N):
    """the 256 x 256 tiles (persistent and eight-phase): (N-tiles, workgroups)"""
    nt = N // 256
    unit = 8 * nt
    return nt, min(max(unit, (256 // unit) * unit), -(-((M + 255) // 256) // 8) * unit)


def rows_for_tiles(tiles, rows_per_tile, partial=True):
    """The smallest row count with `tiles` M-tiles (partial: the last one holds a single row)."""
    return (tiles - 1) * rows_per_tile + (1 if partial else rows_per_tile)


# --------------------------------------------------------------------------------------------------------------------- references
def conv_fwd_ref(x, w, k, s, dtype=F64):
    """y[v, oy, ox, :] = sum over taps (ty, tx) of xpad[v, oy s + ty, ox s + tx, :] @ w[ty, tx]: shifted slices, written out."""
    x, w = x.to(dtype), w.to(dtype)
    V, H, W, Cin = x.shape
    pad = (k - 1) // 2
    OH, OW = out_hw(H, W, k, s)
    xp = torch.zeros(V, H + k - 1, W + k - 1, Cin, dtype=dtype)
    xp[:, pad:pad + H, pad:pad + W] = x
    y = torch.zeros(V, OH, OW, w.shape[3], dtype=dtype)
    for ty in range(k):
        for tx in range(k):
            y += xp[:, ty:ty + s * (OH - 1) + 1:s, tx:tx + s * (OW - 1) + 1:s] @ w[ty, tx]
    return y


def conv_dgrad_ref(dy, w, k, s, H, W, dtype=F64):
    """dx = conv_transpose(dy, w): every tap scatters dy @ w[ty, tx]^T to the padded pixels it read in the forward."""
    dy, w = dy.to(dtype), w.to(dtype)
    V, OH, OW, _ = dy.shape
    pad = (k - 1) // 2
    dxp = torch.zeros(V, H + k - 1, W + k - 1, w.shape[2], dtype=dtype)
    for ty in range(k):
        for tx in range(k):
            dxp[:, ty:ty + s * (OH - 1) + 1:s, tx:tx + s * (OW - 1) + 1:s] += dy @ w[ty, tx].t()
    return dxp[:, pad:pad + H, pad:pad + W].contiguous()


def conv_wgrad_ref(x, dy, k, s, dtype=F64):
    """dw[ty, tx] = (the pixels tap (ty, tx) read)^T @ dy"""
    x, dy = x.to(dtype), dy.to(dtype)
    V, H, W, Cin = x.shape
    _, OH, OW, Cout = dy.shape
    pad = (k - 1) // 2
    xp = torch.zeros(V, H + k - 1, W + k - 1, Cin, dtype=dtype)
    xp[:, pad:pad + H, pad:pad + W] = x
    dw = torch.zeros(k, k, Cin, Cout, dtype=dtype)
    for ty in range(k):
        for tx in range(k):
            dw[ty, tx] = xp[:, ty:ty + s * (OH - 1) + 1:s, tx:tx + s * (OW - 1) + 1:s].reshape(-1, Cin).t() @ dy.reshape(-1, Cout)
    return dw


def channel_sums(t, perm=None, pivot=None):
    """per-channel (sum, sum of squares) over all rows, about `pivot` if given; perm: the order in which the rows are added"""
    a = t.reshape(-1, t.shape[-1])
    if pivot is not None:
        a = a - pivot
    if perm is not None:
        a = a[perm]
    return a.sum(0), (a * a).sum(0)


def pivot_of(c, y):
    """simclr_conv2d_fwd_pivoted: y at pixel (0, OH/2, OW/2) -- zeros (raw moments in the slots) when Cout > 64 * 64, where the entry point
    leaves the pivot out (csrc/conv.hip, simclr_conv2d_fwd_pivoted: "writes zeros into pivot and raw moments into the slots")."""
    return y[0, c.OH // 2, c.OW // 2].clone() if c.Cout <= 64 * 64 else torch.zeros(c.Cout, dtype=y.dtype)


def pack_bits(m, epc):
    """bool [..., C] -> uint8 [rows, C / epc], bit e = element e of the 16-byte chunk (the layout simclr_bn_apply writes)"""
    C = m.shape[-1]
    b = m.reshape(-1, C // epc, epc).to(torch.int32)
    return (b << torch.arange(epc, dtype=torch.int32)).sum(-1).to(torch.uint8)


def mask_of(c, L, dtype=F64):
    """The ReLU mask of simclr_conv2d_dgrad_bn: mode 1 mask source > 0; 2 bn_x * scale + shift > 0; 3 / 4 the bits of the mask source."""
    if c.mode == 2:
        return (L['bnx'].to(dtype) * L['scale'].to(dtype) + L['shift'].to(dtype)) > 0
    return L['msk'] > 0


def dgrad_bn_ref(c, L, dtype=F64, perm=None):
    """dm = (dx [+ prev]) * mask; (sum dm, sum dm * x^), x^ = (bn_x - mean) * rstd -- and the same second sum the way the kernel forms it,
    (sum(dm * bn_x) - mean * sum(dm)) * rstd."""
    dx = dgrad_of(c, L, dtype)
    if c.adds:
        dx = dx + L['prev'].to(dtype)
    dm = dx * mask_of(c, L, dtype).to(dtype)
    a = dm.reshape(-1, c.Cin)
    xr = L['bnx'].to(dtype).reshape(-1, c.Cin)
    xh = (xr - L['mean'].to(dtype)) * L['rstd'].to(dtype)
    b, r = a * xh, a * xr
    if perm is not None:
        a, b, r = a[perm], b[perm], r[perm]
    s1 = a.sum(0)
    return dict(dm=dm, s1=s1, s2=b.sum(0), s2_raw=(r.sum(0) - L['mean'].to(dtype) * s1) * L['rstd'].to(dtype))


def fwd_bn_apply_ref(c, L, conv, dtype=F64):
    """act(T(conv) * scale + shift + r), r = res | res * rscale + rshift.  conv: the convolution output already rounded to T."""
    t = lambda n: L[n].to(dtype)
    z = conv.to(dtype) * t('scale') + t('shift')
    if c.res == 'plain':
        z = z + t('res')
    elif c.res == 'bn':
        z = z + (t('res') * t('rscale') + t('rshift'))
    return torch.relu(z) if c.relu else z


# --------------------------------------------------------------------------------------------------------------------- cases
_DEFAULTS = dict(k=1, s=1, env=None, fam=(), args=None, psx=False, psw=False, mode=0, acc=0, stats=False, store=True, relu=1, res=None,
                 bits=True, dense=None, tail=None, multi=False, splits=None, note='', ext=False)
OPS = ('fwd', 'fwd_pivoted', 'fwd_bn_apply', 'dgrad', 'dgrad_bn', 'wgrad')


def make_case(id, op, arith, V, H, W, Cin, Cout, **kw):
    """One row.  Cin = channels of x / dx, Cout = channels of y / dy (the ABI's names), whatever the operation.
    env: the SIMCLR_* switches of the launch; fam: the family tags (tags_of) the recorded instantiation must carry; args: template
    arguments it must name; tail: True / False = split tail planned / not; multi: some workgroup owns several M-tiles; splits: 'one' |
    'many' slabs of the weight gradient; psx / psw: dy / the weights in the pre-split (hi, lo) block format; stats: fwd with statistics;
    store=False: the statistics-only pass (y == NULL); dense: 'acc' | 'rounded' = a designated bf16 rounding row.
    ext (dgrad, dgrad_bn; 1x1 stride 1): the K-extended launch simclr_conv2d_dgrad(_bn)_ext -- L['dy'] holds [dm | h] (Cout + Cin channels),
    L['w'] the rows of w_ext [Cin][Cout + Cin], L['bias'] the bias.
    acc (data gradient): 0 store | 1 dx += | 3 (stride 2) the sparse store: only the pixel classes that receive a tap are written, the
    others keep what dx held (SENTINEL in the check) | 2 the sparse accumulate: dx holds earlier data at the even (row, column) pixels only
    -- what a 1x1 stride-2 call with accumulate = 3 from dy1 / w1 (Cout channels) left in a buffer full of SENTINEL, which is how the
    check produces it -- and SENTINEL must not leak from the other pixels."""
    assert op in OPS and arith in ARITH, (op, arith)
    bad = set(kw) - set(_DEFAULTS)
    assert not bad, bad
    d = dict(_DEFAULTS)
    d.update(kw)
    c = types.SimpleNamespace(id=id, op=op, arith=arith, V=V, H=H, W=W, Cin=Cin, Cout=Cout, **d)
    c.env = dict(c.env or {})
    c.args = dict(c.args or {})
    c.fam = tuple(c.fam)
    c.dtype, c.tf, c.tb = ARITH[arith]
    c.pad = (c.k - 1) // 2
    c.OH, c.OW = out_hw(H, W, c.k, c.s)
    c.M = V * c.OH * c.OW                 # output rows of the forward; the data gradient's GEMM has V * H * W
    c.epc = 8 if c.dtype == BF16 else 4
    assert c.acc in (0, 1) or op in ('dgrad', 'dgrad_bn'), id
    assert c.acc != 3 or c.s == 2, id
    assert c.acc != 2 or (c.k == 1 and c.s == 1 and c.dtype == F32), id
    assert not c.ext or (op in ('dgrad', 'dgrad_bn') and c.k == 1 and c.s == 1 and not c.psx), id
    c.adds = c.acc in (1, 2)                  # dx / dw += : the row has a `prev`
    c.Cy = Cout + Cin if c.ext else Cout      # channels of L['dy'] and reduction length per tap of the data gradient
    if op in ('fwd_pivoted', 'dgrad_bn'):
        c.stats = True
    return c


def _seed(c):
    return zlib.crc32(c.id.encode()) & 0x7fffffff


def _ints(shape, lim, g):
    return torch.randint(-lim, lim + 1, tuple(shape), generator=g).double()


def lattice(c):
    """The operands of a row (float64), thinned until the bounds of `reference` hold.  Deterministic in the row's id."""
    g = torch.Generator().manual_seed(_seed(c))
    L = {}
    k, Cin, Cout = c.k, c.Cin, c.Cout
    if c.dense:         # designated rounding rows: non-negative operands, per-channel weight density 1/4 ... 1 -> outputs of 9 - 10 bits
        L['x'] = torch.randint(0, 3, (c.V, c.H, c.W, Cin), generator=g).double()
        dens = (torch.arange(Cout) % 4 + 1).double() / 4
        L['w'] = (torch.rand(k, k, Cin, Cout, generator=g, dtype=F64) < dens).double()
        return L
    L['x'] = _ints((c.V, c.H, c.W, Cin), 2, g)
    L['dy'] = _ints((c.V, c.OH, c.OW, c.Cy), 2, g)
    sign = torch.randint(0, 2, (k, k, Cin, c.Cy), generator=g).double() * 2 - 1
    u = torch.rand(k, k, Cin, c.Cy, generator=g, dtype=F64)
    if c.acc == 2:          # what the sparse store of a stride-2 1x1 data gradient leaves at the even pixels (zero elsewhere: nothing is added there)
        OH2, OW2 = out_hw(c.H, c.W, 1, 2)
        L['dy1'] = _ints((c.V, OH2, OW2, Cout), 2, g)
        L['w1'] = (torch.randint(0, 2, (1, 1, Cin, Cout), generator=g).double() * 2 - 1) * (torch.rand(1, 1, Cin, Cout, generator=g, dtype=F64) < min(1.0, 6.0 / Cout)).double()
        L['prev'] = conv_dgrad_ref(L['dy1'], L['w1'], 1, 2, c.H, c.W)
    elif c.adds:
        L['prev'] = _ints((k * k * Cin, Cout) if c.op == 'wgrad' else (c.V, c.H, c.W, Cin), 4, g)
    if c.ext:
        L['bias'] = _ints((Cin,), 4, g)
    if c.op == 'dgrad_bn':
        L.update(lattice_params(Cin, g))
        L['bnx'] = quarters((c.V, c.H, c.W, Cin), 4, g)
        L['msk'] = quarters((c.V, c.H, c.W, Cin), 4, g)
    if c.op == 'fwd_bn_apply':
        L.update(lattice_params(Cout, g))
        L['res'] = quarters((c.V, c.OH, c.OW, Cout), 4, g)
    red = k * k * (c.Cy if c.op in ('dgrad', 'dgrad_bn') else Cin)
    dens = min(1.0, 12.0 / red)
    for _ in range(12):
        L['w'] = sign * (u < dens).double()
        if c.op == 'wgrad' or _bounds_ok(c, L):
            return L
        dens /= 2
    raise AssertionError('no weight density meets the bounds of %s' % c.id)


def dgrad_of(c, L, dtype=F64):
    """The data gradient before `prev`: conv_dgrad_ref, and in a K-extended row dm Wext[:, :Cout]^T + h Wext[:, Cout:]^T + bias -- the
    same reference on the concatenated operands [dm | h], plus the bias."""
    dx = conv_dgrad_ref(L['dy'], L['w'], c.k, c.s, c.H, c.W, dtype)
    return dx + L['bias'].to(dtype) if c.ext else dx


def even_pixels(c):
    """bool [1, H, W, 1]: the pixels with even row and even column -- the one class a 1x1 stride-2 data gradient has taps for."""
    m = torch.zeros(1, c.H, c.W, 1, dtype=torch.bool)
    m[:, ::2, ::2] = True
    return m


def _main_output(c, L, dtype=F64):
    if c.op in ('fwd', 'fwd_pivoted', 'fwd_bn_apply'):
        return conv_fwd_ref(L['x'], L['w'], c.k, c.s, dtype)
    if c.op == 'dgrad':
        dx = dgrad_of(c, L, dtype)
        return dx + L['prev'].to(dtype) if c.adds else dx
    if c.op == 'dgrad_bn':
        return dgrad_bn_ref(c, L, dtype)['dm']
    dw = conv_wgrad_ref(L['x'], L['dy'], c.k, c.s, dtype).reshape(c.k * c.k * c.Cin, c.Cout)
    return dw + L['prev'].to(dtype) if c.adds else dw


def _abs_sums(c, L, out):
    """Per channel, the largest order-dependent partial sum any kernel can form, in units of its grain (see `reference`)."""
    a = out.reshape(-1, out.shape[-1])
    if c.op == 'dgrad_bn':
        # sum(dm): integers.  sum(dm * x) about 0, mean * sum(dm), their difference times rstd: multiples of 2^-6 (dm integer, bn_x and
        # mean multiples of 1/4, rstd of 1/4); |.| <= sum |dm| (|x| + |mean|) * max(rstd, 1)
        xr = L['bnx'].reshape(-1, c.Cin)
        return ((a.abs() * (xr.abs() + L['mean'].abs())).sum(0) * L['rstd'].clamp_min(1.0) * 64).max()
    if c.op == 'fwd_pivoted':
        p = pivot_of(c, out)
        return torch.maximum(((a - p) ** 2).sum(0).max(), (a * a).sum(0).max())
    return (a * a).sum(0).max()


def _bounds_ok(c, L):
    out = _main_output(c, L)
    if c.op == 'dgrad_bn':          # the unmasked gradient is what the accumulators hold
        dx = dgrad_of(c, L)
        out = dx + L['prev'] if c.adds else dx
    return float(out.abs().max()) <= 256 and float(_abs_sums(c, L, out)) < LIMIT


def shares(c, L, out):
    """The shares `reference` puts floors under."""
    s = dict(nonzero=float((out != 0).double().mean()))
    if c.acc == 3 and c.k == 1:       # (among the pixels that receive a tap: the others are structural zeros, not a thin lattice)
        s['nonzero'] = float((out[:, ::2, ::2] != 0).double().mean())
    if c.op == 'dgrad_bn':
        m = mask_of(c, L)
        s['masked_off'] = float((~m).double().mean())
        dx = dgrad_of(c, L)
        s['masked_off_nonzero'] = float((~m & ((dx + L['prev'] if c.adds else dx) != 0)).double().mean())
        if c.mode == 2:
            arg = L['bnx'] * L['scale'] + L['shift']
            s['arg_zero'] = float((arg == 0).double().mean())
            s['arg_zero_live'] = int(((arg == 0) & (dx != 0)).sum())
    if c.op == 'fwd_bn_apply':
        z = fwd_bn_apply_ref(types.SimpleNamespace(res=c.res, relu=0), L, out)
        s['pre_negative'] = float((z < 0).double().mean())
        s['pre_zero'] = float((z == 0).double().mean())
    if c.k == 3:
        H, W = (c.H, c.W) if c.op in ('dgrad', 'dgrad_bn') else (c.OH, c.OW)
        s['border'] = 1.0 - max(H - 2, 0) * max(W - 2, 0) / float(H * W)
    return s


def _assert_shares(c, s, numel):
    big = numel >= 4096
    assert s['nonzero'] >= (0.25 if big else 0.05), (c.id, s)
    if c.op == 'dgrad_bn':
        assert 0.2 <= s['masked_off'] <= 0.8 or not big, (c.id, s)
        assert s['masked_off_nonzero'] > 0 or not big, (c.id, s)
        if c.mode == 2 and big:
            assert s['arg_zero'] >= 0.01 and s['arg_zero_live'] > 0, (c.id, s)
    if c.op == 'fwd_bn_apply' and big:
        assert s['pre_negative'] >= 0.1 and s['pre_zero'] >= 0.001, (c.id, s)
    if c.k == 3:
        assert s['border'] >= 0.05, (c.id, s)


def ps_roundtrip(t):
    """float64 [..., C] -> the value the pre-split (hi, lo) bf16 block format holds (tests/gpu_checks.ps_encode / ps_decode) -- imported
    lazily: gpu_checks imports the device libraries."""
    from tests import gpu_checks as gc
    return gc.ps_decode(gc.ps_encode(t.float()))[0]


def reference(c, check_ps=True):
    """Operands, expected outputs and the asserted conditions of a row.  Returns (L, want): float64 tensors; want holds `out` (y | dx |
    dm | dw as stored: rounded once to the storage type in the designated rounding rows and after the fused BatchNorm apply, exact
    everywhere else), and where the row has them s1 / s2 (the statistics), pivot, bits (uint8)."""
    L = lattice(c)
    perm = row_perm(c.V * (c.H * c.W if c.op in ('dgrad', 'dgrad_bn') else c.OH * c.OW), seed=3)

    def evaluate(dtype, perm=perm):
        out = _main_output(c, L, dtype)
        r = dict(out=out)
        if c.op == 'fwd' and c.stats:
            src = round_to(out, BF16).to(dtype) if c.dense == 'rounded' else out
            r['s1'], r['s2'] = channel_sums(src, perm)
        elif c.op == 'fwd_pivoted':
            r['pivot'] = pivot_of(c, out)
            r['p1'], r['p2'] = channel_sums(out, perm, r['pivot'])
            r['s1'], r['s2'] = channel_sums(out, perm)
        elif c.op == 'dgrad_bn':
            d = dgrad_bn_ref(c, L, dtype, perm)
            r.update(s1=d['s1'], s2=d['s2'], s2_raw=d['s2_raw'])
        elif c.op == 'fwd_bn_apply':
            conv = round_to(out, c.dtype).to(dtype)
            r['conv'] = conv
            r['out'] = fwd_bn_apply_ref(c, L, conv, dtype)
        return r

    want = assert_exact(evaluate, c.id)
    assert_exact(lambda d: evaluate(d, None), c.id + ' (rows in order)')
    if c.op == 'dgrad_bn':
        assert torch.equal(want['s2'], want['s2_raw']), c.id
        if c.mode == 4:
            want.pop('s2')
        want.pop('s2_raw')
    # storage: every operand survives its type (and, pre-split, the block format; the fp16 pieces of the forward hold 2^8 w)
    ops_ = {n: L[n] for n in ('x', 'w', 'dy', 'prev', 'bnx', 'msk', 'res', 'dy1', 'w1') if n in L and not (n == 'prev' and c.op == 'wgrad')}
    assert_survives(ops_, c.dtype)
    assert_survives({n: v for n, v in L.items() if v.dim() == 1}, F32)
    if c.dtype == F32:
        assert_survives({n: L[n] for n in ('w', 'w1') if n in L}, BF16)
        assert_survives(dict(w256=L['w'] * F16_WSCALE, x=L['x']), torch.float16)
        if c.psx and check_ps:
            assert torch.equal(ps_roundtrip(L['dy']), L['dy']), c.id
            assert c.acc != 2 or torch.equal(ps_roundtrip(L['dy1']), L['dy1']), c.id
    raw = _main_output(c, L)
    if c.dense:
        assert float((round_to(raw, BF16) != raw).double().mean()) >= 0.25, c.id       # the rounding is real
        want['out'] = round_to(raw, BF16)
        assert float(raw.abs().max()) < 2 ** 15
    elif c.op == 'fwd_bn_apply':
        assert float(raw.abs().max()) <= 256 and torch.equal(want['conv'], raw), c.id
        want['out'] = round_to(want['out'], c.dtype)
        want['bits'] = pack_bits(want['out'] > 0, c.epc)
        want.pop('conv')
    elif c.op == 'wgrad':           # dw is stored in fp32 whatever the storage type of x and dy
        assert float(raw.abs().max()) < LIMIT and torch.equal(raw, raw.round()), c.id
    else:
        assert float(raw.abs().max()) <= 256 and torch.equal(raw, raw.round()), c.id
        assert torch.equal(round_to(want['out'], BF16), want['out']), c.id
    if c.op != 'wgrad':
        assert float(_abs_sums(c, L, raw)) < LIMIT, c.id
    else:
        x, dy = L['x'].abs().reshape(-1, c.Cin), L['dy'].abs().reshape(-1, c.Cout)
        assert float(x.sum(0).max() * dy.max()) + 4 < LIMIT, c.id
    if c.op == 'dgrad_bn' and c.mode in (3, 4):
        want['mask_bits'] = pack_bits(L['msk'] > 0, c.epc)
    _assert_shares(c, shares(c, L, raw), raw.numel())
    if c.acc == 2:          # the earlier data: non-zero at some even pixel, nothing at the others
        ev = even_pixels(c)
        assert float((L['prev'] * ev != 0).double().mean()) >= 0.02 and not bool((L['prev'] * ~ev).any()), c.id
        assert float((~ev).double().mean()) > 0 or c.H * c.W == 1, c.id
    if c.acc == 3:          # the sparse store: the pixel classes without a tap keep the sentinel
        sent = float(round_to(torch.tensor([SENTINEL], dtype=F64), c.dtype))
        if c.k == 1:
            assert not bool((want['out'] * ~even_pixels(c)).any()), c.id
            want['out'] = torch.where(even_pixels(c), want['out'], torch.full_like(want['out'], sent))
    return L, want


# --------------------------------------------------------------------------------------------------------------------- the C ABI call
def launch(lib, c, P, nslot=0, stream=None):
    """The library call of a row.  P: name -> pointer (ctypes.c_void_p or None) of x, w, y, dy, dx, dw, ws, stats, pivot, scale, shift,
    mean, rstd, bnx, msk, res, rscale, rshift, bits -- real buffers on the GPU, never-dereferenced fakes in a dry run (SIMCLR_DRY_RUN=1)."""
    g = lambda n: P.get(n)
    dt = DT_BF16 if c.dtype == BF16 else DT_F32
    geo = (c.V, c.H, c.W, c.Cin, c.OH, c.OW, c.Cout, c.k, c.k, c.s, c.pad)
    fw = dt | terms_field(c.tf) | (PS_W if c.psw else 0)
    bw = dt | terms_field(c.tb) | (PS_W if c.psw else 0) | (PS_IN if c.psx else 0)
    if c.op == 'fwd':
        return lib.conv2d_fwd(g('x'), g('w'), g('y') if c.store else None, g('stats') if c.stats else None, nslot if c.stats else 0, *geo, fw, stream)
    if c.op == 'fwd_pivoted':
        return lib.conv2d_fwd_pivoted(g('x'), g('w'), g('y'), g('stats'), nslot, g('pivot'), *geo, fw, stream)
    if c.op == 'fwd_bn_apply':
        rbn = c.res == 'bn'
        return lib.conv2d_fwd_bn_apply(g('x'), g('w'), g('y'), g('scale'), g('shift'), g('res') if c.res else None, g('rscale') if rbn else None,
                                       g('rshift') if rbn else None, int(c.relu), g('bits') if c.bits else None, *geo, fw, stream)
    if c.op == 'dgrad' and c.ext:
        return lib.conv2d_dgrad_ext(g('dy'), g('h'), g('w'), g('bias'), g('dx'), int(c.acc), c.V, c.H, c.W, c.Cin, c.Cout, bw, stream)
    if c.op == 'dgrad':
        return lib.conv2d_dgrad(g('dy'), g('w'), g('dx'), int(c.acc), *geo, bw, stream)
    if c.op == 'dgrad_bn' and c.ext:
        m4 = c.mode == 4
        return lib.conv2d_dgrad_bn_ext(g('dy'), g('h'), g('w'), g('bias'), g('dx'), int(c.acc), None if m4 else g('bnx'),
                                       None if c.mode == 2 else g('msk'), g('scale') if c.mode == 2 else None,
                                       g('shift') if c.mode == 2 else None, None if m4 else g('mean'), None if m4 else g('rstd'), c.mode,
                                       g('stats'), nslot, c.V, c.H, c.W, c.Cin, c.Cout, bw, stream)
    if c.op == 'dgrad_bn':
        m4 = c.mode == 4
        return lib.conv2d_dgrad_bn(g('dy'), g('w'), g('dx'), int(c.acc), None if m4 else g('bnx'), None if c.mode == 2 else g('msk'),
                                   g('scale') if c.mode == 2 else None, g('shift') if c.mode == 2 else None, None if m4 else g('mean'),
                                   None if m4 else g('rstd'), c.mode, g('stats'), nslot, *geo, bw, stream)
    return lib.conv2d_wgrad(g('x'), g('dy'), g('dw'), int(c.acc), g('ws'), c.V, c.H, c.W, c.Cin, c.Cin, c.OH, c.OW, c.Cout, c.k, c.k, c.s,
                            c.pad, dt | terms_field(c.tb) | (PS_IN if c.psx else 0), stream)


def launch_first(lib, c, P, stream=None):
    """The call before a sparse-accumulate row (acc == 2): the 1x1 stride-2 data gradient of dy1 / w1 with accumulate = 3 into dx."""
    OH2, OW2 = out_hw(c.H, c.W, 1, 2)
    bw = DT_F32 | terms_field(c.tb) | (PS_IN if c.psx else 0)
    return lib.conv2d_dgrad(P.get('dy1'), P.get('w1'), P.get('dx'), 3, c.V, c.H, c.W, c.Cin, OH2, OW2, c.Cout, 1, 1, 2, 0, bw, stream)


POINTERS = ('x', 'w', 'y', 'dy', 'dx', 'dw', 'ws', 'stats', 'pivot', 'scale', 'shift', 'mean', 'rstd', 'bnx', 'msk', 'res', 'rscale',
            'rshift', 'bits', 'h', 'bias', 'dy1', 'w1')


# --------------------------------------------------------------------------------------------------------------------- the record
_ARGS = {
    'conv_igemm': (['T', 'MODE', 'BN', 'STATS', 'GLDS'], {}),
    'conv_igemm_persistent': (['T', 'MODE', 'BM', 'BN', 'NW', 'STAGES', 'STATS', 'BNEPI', 'EXT', 'WIN', 'FAPPLY', 'SPL', 'TAIL', 'PSB', 'FAS', 'EPS',
                               'PSX'], dict(EXT='false', WIN='false', FAPPLY='false', SPL='0', TAIL='false', PSB='false', FAS='0', EPS='0',
                                            PSX='false')),
    'conv_igemm_wide': (['MODE', 'STATS', 'BNEPI', 'FLAT'], {}),
    'conv_igemm_nwalk': (['KPT', 'FAS'], {}),
    'conv_wgrad': (['T', 'BKW', 'BNW', 'MT'], dict(MT='false')),
    'conv_wgrad_dma': (['T', 'BKW', 'BNW', 'BRM', 'STAGES', 'WK', 'WNN', 'GRAM', 'MT', 'SPL', 'PSD'],
                       dict(WK='2', WNN='2', GRAM='false', MT='false', SPL='0', PSD='0')),
    'conv_wgrad3x3_bf16': (['ST'], {}),
    'conv_wgrad3x3_f32ps': ([], {}),
}


def parse_record(rec):
    """simclr_conv2d_last_instantiation() -> (kernel, {template argument: text, defaulted ones filled in}, {field: int})"""
    m = re.match(r'\((\w+)(?:<([^>]*)>)?\)(.*)$', rec)
    assert m, rec
    kernel = m.group(1)
    names, dflt = _ARGS[kernel]
    given = [s.strip() for s in m.group(2).split(',')] if m.group(2) else []
    assert len(given) <= len(names), rec
    args = {n: (given[i] if i < len(given) else dflt[n]) for i, n in enumerate(names)}
    fields = {k_: int(v) for k_, v in re.findall(r' (\w+)=(\d+)', m.group(3))}
    return kernel, args, fields


def tags_of(c, rec):
    """The family tags of a recorded instantiation (and of the row that produced it, where the record does not say: accumulate)."""
    kernel, a, f = parse_record(rec)
    t = set()
    f32 = c.dtype == F32
    if kernel == 'conv_igemm':
        t.add('FALLBACK')
    elif kernel == 'conv_igemm_wide':
        t.add('WIDE ' + ('flat' if a['FLAT'] == 'true' else 'gathered') + (' split tail' if f['tail_parts'] >= 2 else ''))
    elif kernel == 'conv_igemm_nwalk':
        t.add('NWALK FAS%s' % a['FAS'])
    if kernel == 'conv_igemm_persistent' and a['EXT'] == 'true':
        t.add('EXT TILE%s %s%s' % (a['BM'], 'f32' if f32 else 'bf16', ' reduce' if a['BNEPI'] == 'true' else ''))
    if c.acc >= 2 and c.op in ('dgrad', 'dgrad_bn') and kernel == 'conv_igemm_persistent':
        t.add('SPARSE acc%d %s%s' % (c.acc, 'f32' if f32 else 'bf16', ' reduce' if a['BNEPI'] == 'true' else ''))
    if kernel in ('conv_igemm', 'conv_igemm_wide', 'conv_igemm_nwalk'):
        pass
    elif kernel == 'conv_igemm_persistent' and a['BM'] == '256':
        t.add('TILE256' + (' split tail' if a['TAIL'] == 'true' else ''))
        if a['FAPPLY'] == 'true':
            t.add('TILE256 fapply')
    elif kernel == 'conv_igemm_persistent':
        if a['FAPPLY'] == 'true':
            t.add(('f32 fapply SPL%s' % a['SPL']) if f32 else 'bf16 FAS%s' % a['FAS'])
        elif a['WIN'] == 'true':
            if not f32:
                t.add('TILE128 window bf16')
            elif a['MODE'] == 'MODE_FWD':
                t.add('TILE128 window f32 fwd')
            else:
                t.add('TILE128 window f32 dgrad psx' + (' reduce' if a['BNEPI'] == 'true' else ''))
        else:
            t.add('TILE128 gather BN%s' % a['BN'])
        if a['TAIL'] == 'true':
            t.add('TILE128 split tail')
        if a['EPS'] != '0':
            t.add('%s EPS%s' % ('f32' if f32 else 'bf16', a['EPS']))
    else:
        if kernel == 'conv_wgrad':
            fam = 'REG_STAGED'
        elif kernel == 'conv_wgrad3x3_bf16':
            fam = 'NINE_TAP_BF16'
        elif kernel == 'conv_wgrad3x3_f32ps':
            fam = 'NINE_TAP_F32PS'
        elif a['BKW'] == '256':
            fam = 'TILE256_F32' if a['T'] == 'float' else 'TILE256_BF16'
        else:
            fam = 'DMA_RING'
            if not f32:
                fam += ' stages %s' % a['STAGES']
        t.add(fam)
        t.add('%s acc%d splits%s' % (fam, int(c.acc), '1' if f['splits'] == 1 else '>1'))
    return t


# the families the rows must reach.  TILE256_BF16 (weight gradient) has no forcing switch -- it needs M >= 150000 -- and is left out.
# The stem and the Gram chain have their own table (tests/stem_gram_reference.py).
REQUIRED_FWD_DGRAD = ['FALLBACK', 'TILE128 gather BN64', 'TILE128 gather BN128', 'TILE128 window bf16', 'TILE128 window f32 fwd',
                      'TILE128 window f32 dgrad psx', 'TILE128 window f32 dgrad psx reduce', 'TILE128 split tail', 'TILE256',
                      'TILE256 split tail', 'WIDE flat', 'WIDE gathered', 'WIDE flat split tail', 'WIDE gathered split tail', 'NWALK FAS1',
                      'NWALK FAS2', 'bf16 EPS1', 'bf16 EPS3', 'bf16 EPS4', 'f32 EPS1', 'f32 EPS4', 'bf16 FAS0', 'bf16 FAS1', 'bf16 FAS2',
                      'f32 fapply SPL13']
WGRAD_FAMILIES = ['REG_STAGED', 'DMA_RING stages 2', 'DMA_RING stages 3', 'DMA_RING stages 4', 'DMA_RING', 'NINE_TAP_BF16', 'NINE_TAP_F32PS',
                  'TILE256_F32']
REQUIRED_WGRAD = ['%s acc%d splits%s' % (fam, acc, sp) for fam in WGRAD_FAMILIES for acc in (0, 1) for sp in ('1', '>1')]
# K-extended data gradient (EXT = true: 128-row tile in both storage types, the 256 x 256 tile in bf16; plain and with the fused reduce)
# and the sparse store / accumulate of the 1x1 stride-2 shortcut (accumulate 3 in both storage types, 2 in fp32 only)
REQUIRED_EXT = ['EXT TILE%s %s%s' % (bm, st, r) for (bm, st) in (('128', 'f32'), ('128', 'bf16'), ('256', 'bf16')) for r in ('', ' reduce')]
REQUIRED_SPARSE = ['SPARSE acc3 f32', 'SPARSE acc3 bf16', 'SPARSE acc2 f32', 'SPARSE acc2 f32 reduce']
REQUIRED = REQUIRED_FWD_DGRAD + REQUIRED_WGRAD + REQUIRED_EXT + REQUIRED_SPARSE


def check_record(c, rec):
    """The recorded instantiation names the family and the template arguments the row claims.  Returns the row's tags."""
    kernel, a, f = parse_record(rec)
    tags = tags_of(c, rec)
    assert set(c.fam) <= tags, '%s: claims %s, the record gives %s: %s' % (c.id, sorted(c.fam), sorted(tags), rec)
    for n, v in c.args.items():
        assert a.get(n) == str(v), '%s: claims %s=%s: %s' % (c.id, n, v, rec)
    if kernel.startswith('conv_igemm'):
        assert a.get('T', 'uint16_t' if c.dtype == BF16 else 'float') == ('uint16_t' if c.dtype == BF16 else 'float'), rec
        if kernel != 'conv_igemm_nwalk':
            assert a['MODE'] == ('MODE_DGRAD' if c.op in ('dgrad', 'dgrad_bn') else 'MODE_FWD'), rec
        if 'STATS' in a:
            assert a['STATS'] == ('true' if c.stats else 'false'), rec
        if 'BNEPI' in a:
            assert a['BNEPI'] == ('true' if c.op == 'dgrad_bn' else 'false'), rec
        if 'PSX' in a:
            assert a['PSX'] == ('true' if c.psx else 'false'), rec
        if c.tail is not None:
            assert (f['tail_parts'] >= 2) == bool(c.tail), '%s: split tail %s: %s' % (c.id, c.tail, rec)
        if c.multi:
            groups = f.get('n_groups', f['n_tiles']) if kernel != 'conv_igemm' else 1
            slots = f['grid'] // groups
            assert kernel != 'conv_igemm' and f['m_tiles'] > slots and f['m_tiles'] % slots != 0, '%s: no workgroup owns several tiles: %s' % (c.id, rec)
    else:
        if c.splits:
            assert (f['splits'] == 1) == (c.splits == 'one'), '%s: splits %s: %s' % (c.id, c.splits, rec)
    return tags


# --------------------------------------------------------------------------------------------------------------------- the case table
# Every row runs on the GPU (tests/test_gpu_conv_lattice.py) and, in a dry run, through the library's selection rules
# (tests/test_conv_reference.py).  Maps are non-square throughout; (7, 10) / (10, 7) are the stride-2 maps (odd and even extent per axis).
NONSQUARE = [(5, 9), (9, 5), (1, 7), (7, 1), (6, 10)]
STRIDED = [(7, 10), (10, 7)]
F32_ARITHS = ['exact', 'bf16x3', 'bf16x6', 'bf16x6_3', 'f16x3_3']
NO_WIDE = {'SIMCLR_IGEMM_WIDE': '0'}
T128 = {'SIMCLR_IGEMM_TILE': '128', 'SIMCLR_IGEMM_WIDE': '0'}
T256 = {'SIMCLR_IGEMM_TILE': '256', 'SIMCLR_IGEMM_WIDE': '0'}
WIDE = {'SIMCLR_IGEMM_WIDE': '2'}
# (V, H, W) with M = V H W rows around the tile edges
ROWS = {1: (1, 1, 1), 63: (1, 7, 9), 64: (2, 4, 8), 65: (1, 5, 13), 127: (1, 1, 127), 128: (4, 2, 16), 129: (3, 1, 43), 255: (1, 3, 85),
        256: (2, 8, 16), 257: (1, 1, 257), 1025: (1, 25, 41), 2049: (1, 3, 683), 49153: (13, 19, 199), 98400: (25, 48, 82)}


def _with(env, **more):
    d = dict(env)
    d.update(more)
    return d


def build_cases():
    rows = []

    def add(id, *a, **kw):
        rows.append(make_case(id, *a, **kw))

    # ---- geometry: every non-square map through forward (+ statistics), data gradient (store / accumulate) and weight gradient, 1x1 and 3x3
    for (H, W) in NONSQUARE + STRIDED:
        s = 2 if (H, W) in STRIDED else 1
        for k in (1, 3):
            for ar in ('bf16', 'exact', 'f16x3_3'):
                t = '%dx%d_k%d_s%d_%s' % (H, W, k, s, ar)
                add('geo_fwd_' + t, 'fwd', ar, 3, H, W, 64, 128, k=k, s=s, stats=True)
                add('geo_dgrad_' + t, 'dgrad', ar, 3, H, W, 128, 64, k=k, s=s, acc=int(H > W))
                add('geo_wgrad_' + t, 'wgrad', ar, 3, H, W, 64, 64, k=k, s=s, acc=int(H < W))
    for ar in ('bf16x3', 'bf16x6', 'bf16x6_3'):
        for (H, W, s) in ((5, 9, 1), (7, 10, 2)):
            for k in (1, 3):
                t = '%dx%d_k%d_s%d_%s' % (H, W, k, s, ar)
                add('geo_fwd_' + t, 'fwd', ar, 3, H, W, 64, 128, k=k, s=s, stats=True)
                add('geo_dgrad_' + t, 'dgrad', ar, 3, H, W, 128, 64, k=k, s=s)
                add('geo_wgrad_' + t, 'wgrad', ar, 3, H, W, 64, 64, k=k, s=s)

    # ---- FALLBACK: more than 64 N-tiles
    add('fallback_fwd_exact', 'fwd', 'exact', 2, 2, 3, 32, 8320, stats=True, fam=['FALLBACK'])
    add('fallback_fwd_bf16', 'fwd', 'bf16', 2, 2, 3, 64, 8320, stats=True, fam=['FALLBACK'])
    add('fallback_fwd_f16x3_3', 'fwd', 'f16x3_3', 2, 2, 3, 32, 8320, fam=['FALLBACK'])
    add('fallback_dgrad_exact', 'dgrad', 'exact', 2, 2, 3, 8320, 32, fam=['FALLBACK'])
    add('fallback_dgrad_bf16_acc', 'dgrad', 'bf16', 2, 3, 2, 8320, 64, acc=1, fam=['FALLBACK'])

    # ---- TILE128 gather: BN 64 / 128, every arithmetic; the narrow-tile rule's boundaries
    for ar in ['bf16'] + F32_ARITHS:
        add('gather_bn64_fwd_' + ar, 'fwd', ar, 3, 5, 9, 128, 64, stats=True, env=NO_WIDE, fam=['TILE128 gather BN64'])
        add('gather_bn128_fwd_' + ar, 'fwd', ar, 3, 9, 5, 128, 128, stats=True, env=NO_WIDE, fam=['TILE128 gather BN128'])
        add('gather_bn64_dgrad_' + ar, 'dgrad', ar, 3, 5, 9, 64, 192, env=NO_WIDE, fam=['TILE128 gather BN64'])
        add('gather_bn128_dgrad_' + ar, 'dgrad', ar, 3, 9, 5, 128, 192, acc=1, env=NO_WIDE, fam=['TILE128 gather BN128'])
    add('narrow_bf16_K64', 'fwd', 'bf16', 3, 5, 9, 64, 128, stats=True, env=NO_WIDE, fam=['TILE128 gather BN64'])
    add('narrow_bf16_K128', 'fwd', 'bf16', 3, 5, 9, 128, 128, stats=True, env=NO_WIDE, fam=['TILE128 gather BN128'])
    add('narrow_f32_dgrad_K128', 'dgrad', 'bf16x3', 3, 5, 9, 128, 128, env=NO_WIDE, fam=['TILE128 gather BN64'])
    add('narrow_f32_dgrad_K160', 'dgrad', 'bf16x3', 3, 5, 9, 128, 160, env=NO_WIDE, fam=['TILE128 gather BN128'])
    add('narrow_f32_dgrad_K128_psx', 'dgrad', 'f16x3_3', 3, 5, 9, 128, 128, psx=True, env=NO_WIDE, fam=['TILE128 gather BN64'])
    add('narrow_f32_dgrad_K160_psx', 'dgrad', 'f16x3_3', 3, 5, 9, 128, 160, psx=True, psw=True, env=NO_WIDE, fam=['TILE128 gather BN128'])

    # ---- rows around the tile edges
    for M in (1, 127, 128, 129):
        V, H, W = ROWS[M]
        for ar in ('bf16', 'exact', 'f16x3_3'):
            add('rows%d_fwd_%s' % (M, ar), 'fwd', ar, V, H, W, 64, 192, stats=True, env=NO_WIDE)
            add('rows%d_dgrad_bn_%s' % (M, ar), 'dgrad_bn', ar, V, H, W, 192, 64, mode=2, psx=ar == 'f16x3_3', env=NO_WIDE)
            add('rows%d_wgrad_%s' % (M, ar), 'wgrad', ar, V, H, W, 64, 64)
    for (V, H, W) in ((127, 1, 1), (4, 2, 16), (3, 1, 43)):          # 127 / 128 / 129 rows on the halo-window path
        add('rows%d_win_fwd_bf16' % (V * H * W), 'fwd', 'bf16', V, H, W, 64, 64, k=3, stats=True, fam=['TILE128 window bf16'])
        add('rows%d_win_dgrad_bf16' % (V * H * W), 'dgrad', 'bf16', V, H, W, 64, 64, k=3, fam=['TILE128 window bf16'])
    for M in (255, 256, 257):
        V, H, W = ROWS[M]
        add('rows%d_tile256_fwd' % M, 'fwd', 'bf16', V, H, W, 64, 256, stats=True, env=T256, fam=['TILE256'])
        add('rows%d_tile256_dgrad' % M, 'dgrad', 'bf16', V, H, W, 256, 64, env=T256, fam=['TILE256'])
        add('rows%d_wide_fwd' % M, 'fwd', 'bf16', V, H, W, 64, 256, stats=True, env=WIDE, fam=['WIDE flat'])
        add('rows%d_wide_dgrad_bn' % M, 'dgrad_bn', 'bf16', V, H, W, 256, 64, mode=2, env=WIDE, fam=['WIDE flat'])
    for M in (63, 64, 65):
        V, H, W = ROWS[M]
        add('rows%d_nwalk' % M, 'fwd_bn_apply', 'f16x3_3', V, H, W, 64, 192, res='plain', psw=M == 64, fam=['NWALK FAS1'])
        add('rows%d_nwalk_resbn' % M, 'fwd_bn_apply', 'f16x3_3', V, H, W, 128, 256, res='bn', psw=M != 64, fam=['NWALK FAS2'])

    # ---- a workgroup owns several M-tiles and the last round is partial: the smallest such M per persistent family
    V, H, W = ROWS[1025]          # 9 M-tiles of 128 rows on the 8 M-slots of a 64-N-tile grid
    assert persistent_grid(1025, 8192)[2] // 64 == 8
    add('multi_tile128_fwd', 'fwd', 'bf16', V, H, W, 64, 8192, stats=True, env=_with(NO_WIDE, SIMCLR_IGEMM_SPLIT='0'), multi=True, tail=False,
        fam=['TILE128 gather BN128'])
    add('multi_tile128_fwd_f16x3_3', 'fwd_pivoted', 'f16x3_3', V, H, W, 64, 8192, multi=True, fam=['TILE128 gather BN128'])
    add('multi_tile128_dgrad_bn_bf16', 'dgrad_bn', 'bf16', V, H, W, 8192, 64, mode=2, env=NO_WIDE, multi=True, fam=['bf16 EPS1'])
    add('multi_tile128_dgrad_bn_f32', 'dgrad_bn', 'f16x3_3', V, H, W, 8192, 64, mode=4, acc=1, psx=True, multi=True, fam=['f32 EPS4'])
    V, H, W = ROWS[98400]         # 769 M-tiles on the 768 workgroups of the 64-wide tile
    assert persistent_grid(98400, 64)[2] == 768
    add('multi_tile128_bn64_fwd', 'fwd', 'bf16', V, H, W, 64, 64, stats=True, multi=True, fam=['TILE128 gather BN64'])
    V, H, W = ROWS[2049]          # 9 M-tiles of 256 rows on the 8 M-slots of a 32-N-tile grid
    assert wide_grid(2049, 8192)[1] // 32 == 8
    add('multi_tile256_fwd', 'fwd', 'bf16', V, H, W, 64, 8192, stats=True, env=T256, multi=True, tail=False, fam=['TILE256'])
    add('multi_wide_fwd', 'fwd', 'bf16', V, H, W, 64, 8192, stats=True, env=_with(WIDE, SIMCLR_IGEMM_SPLIT='0'), multi=True, tail=False,
        fam=['WIDE flat'])
    V, H, W = ROWS[49153]         # 769 M-tiles of 64 rows on the 768 workgroups of the N-inner walk
    add('multi_nwalk', 'fwd_bn_apply', 'f16x3_3', V, H, W, 64, 192, res='plain', multi=True, fam=['NWALK FAS1'])

    # ---- split tail (shapes of tests/test_gpu_kernels.py SPLIT_TAIL_CASES: 1x1 with 16 k-steps, halo-window 3x3 split by 64-channel chunk,
    # strided 3x3 gather, the 256 x 256 tile, the mask-tensor epilogue; the row count shrunk to one round + one left-over tile by widening N)
    SP = _with(NO_WIDE, SIMCLR_IGEMM_SPLIT='1')
    V, H, W = ROWS[1025]
    add('split_tile128_fwd', 'fwd', 'bf16', V, H, W, 1024, 8192, stats=True, env=SP, tail=True, multi=True, fam=['TILE128 split tail'])
    add('split_tile128_dgrad_bn_m2', 'dgrad_bn', 'bf16', V, H, W, 8192, 1024, mode=2, env=SP, tail=True, fam=['TILE128 split tail'])
    add('split_tile128_dgrad_bn_m1', 'dgrad_bn', 'bf16', V, H, W, 8192, 1024, mode=1, env=SP, tail=True, fam=['TILE128 split tail'])
    add('split_window_fwd', 'fwd', 'bf16', V, H, W, 128, 8192, k=3, stats=True, env=SP, tail=True, fam=['TILE128 split tail', 'TILE128 window bf16'])
    add('split_window_dgrad_bn_m3_acc', 'dgrad_bn', 'bf16', V, H, W, 8192, 128, k=3, mode=3, acc=1, env=SP, tail=True,
        fam=['TILE128 split tail', 'TILE128 window bf16'])
    add('split_strided_fwd', 'fwd', 'bf16', 1, 50, 81, 128, 8192, k=3, s=2, stats=True, env=SP, tail=True, fam=['TILE128 split tail'])
    V, H, W = ROWS[2049]
    add('split_tile256_fwd', 'fwd', 'bf16', V, H, W, 1024, 8192, stats=True, env=_with(T256, SIMCLR_IGEMM_SPLIT='1'), tail=True,
        fam=['TILE256 split tail'])
    add('split_tile256_dgrad_bn_m2', 'dgrad_bn', 'bf16', V, H, W, 8192, 1024, mode=2, env=_with(T256, SIMCLR_IGEMM_SPLIT='1'), tail=True,
        fam=['TILE256 split tail'])
    add('split_wide_flat_fwd', 'fwd', 'bf16', V, H, W, 1024, 8192, stats=True, env=WIDE, tail=True, fam=['WIDE flat split tail'])
    add('split_wide_flat_dgrad', 'dgrad', 'bf16', V, H, W, 8192, 1024, env=WIDE, tail=True, fam=['WIDE flat split tail'])
    add('split_wide_gathered_fwd', 'fwd', 'bf16', V, H, W, 128, 8192, k=3, stats=True, env=WIDE, tail=True, fam=['WIDE gathered split tail'])

    # ---- TILE256 and the eight-phase tile on the non-square maps
    for (H, W) in NONSQUARE + STRIDED:
        s = 2 if (H, W) in STRIDED else 1
        for k in (1, 3):
            t = '%dx%d_k%d_s%d' % (H, W, k, s)
            flat = k == 1 and s == 1
            add('tile256_fwd_' + t, 'fwd', 'bf16', 3, H, W, 64, 256, k=k, s=s, stats=True, env=T256, fam=['TILE256'], tail=False)
            # (a strided 1x1 store ends with the zero fill of a pixel class without taps: the record names that launch)
            add('tile256_dgrad_' + t, 'dgrad', 'bf16', 3, H, W, 256, 64, k=k, s=s, acc=int(k == 3), env=T256,
                fam=['FALLBACK' if (k == 1 and s == 2) else 'TILE256'])
            add('wide_fwd_' + t, 'fwd', 'bf16', 3, H, W, 64, 256, k=k, s=s, stats=True, env=WIDE, fam=['WIDE flat' if flat else 'WIDE gathered'],
                tail=False)
            add('wide_dgrad_' + t, 'dgrad', 'bf16', 3, H, W, 256, 64, k=k, s=s, acc=int(k == 1), env=WIDE,
                fam=['WIDE flat' if flat else 'WIDE gathered'])
            if s == 1:
                add('tile256_dgrad_bn_' + t, 'dgrad_bn', 'bf16', 3, H, W, 256, 64, k=k, mode=1 + (H + k) % 4, acc=int(H > W), env=T256,
                    fam=['TILE256'])
                add('wide_dgrad_bn_' + t, 'dgrad_bn', 'bf16', 3, H, W, 256, 64, k=k, mode=1 + (W + k) % 4, acc=int(H < W), env=WIDE,
                    fam=['WIDE flat' if flat else 'WIDE gathered'])
    add('tile256_stats_only', 'fwd', 'bf16', 3, 5, 9, 64, 256, stats=True, store=False, env=T256, fam=['TILE256'])
    add('wide_stats_only', 'fwd', 'bf16', 3, 9, 5, 64, 256, stats=True, store=False, env=WIDE, fam=['WIDE flat'])

    # ---- channel edges
    for Cout in (4, 8, 68, 72, 192, 320):
        for ar in ('bf16', 'exact', 'f16x3_3'):
            for k in (1, 3):
                odd = ['FALLBACK'] if (ar == 'bf16' and Cout % 8) else []      # bf16 rows of 8-byte granules: the non-persistent kernel
                add('cout%d_fwd_k%d_%s' % (Cout, k, ar), 'fwd', ar, 2, 6, 10, 64, Cout, k=k, stats=True, env=NO_WIDE, fam=odd)
                add('cin%d_dgrad_k%d_%s' % (Cout, k, ar), 'dgrad', ar, 2, 10, 6, Cout, 64, k=k, acc=int(k == 3), env=NO_WIDE, fam=odd)
                if Cout % 8 == 0:
                    add('cout%d_wgrad_k%d_%s' % (Cout, k, ar), 'wgrad', ar, 2, 6, 10, 64, Cout, k=k)
    # (two M-tiles of the non-persistent kernel with bf16 rows of 8-byte granules)
    add('odd_n_fwd_bf16', 'fwd', 'bf16', 3, 9, 5, 64, 68, k=3, stats=True, fam=['FALLBACK'])
    add('odd_n_dgrad_bf16', 'dgrad', 'bf16', 3, 5, 9, 4, 64, k=3, acc=1, fam=['FALLBACK'])
    for Cin in (32, 96):
        for ar in F32_ARITHS:
            add('cin%d_fwd_%s' % (Cin, ar), 'fwd', ar, 2, 5, 9, Cin, 72, k=3, stats=True)
            add('cin%d_wgrad_%s' % (Cin, ar), 'wgrad', ar, 2, 9, 5, Cin, 72, k=3, fam=['REG_STAGED'])
            add('cout%d_dgrad_%s' % (Cin, ar), 'dgrad', ar, 2, 5, 9, 72, Cin, k=3)

    # ---- halo window: W = 61 / 62 (the last window width) / 63 (gathers), H = 1
    for (H, W) in ((3, 61), (3, 62), (3, 63), (1, 62)):
        win = W <= 62
        t = '%dx%d' % (H, W)
        add('win_fwd_bf16_' + t, 'fwd', 'bf16', 2, H, W, 64, 64, k=3, stats=True, fam=['TILE128 window bf16' if win else 'TILE128 gather BN64'])
        add('win_fwd_f16x3_3_' + t, 'fwd', 'f16x3_3', 2, H, W, 64, 128, k=3, stats=True, psw=H == 1,
            fam=['TILE128 window f32 fwd' if win else 'TILE128 gather BN128'])
        add('win_dgrad_bf16_' + t, 'dgrad', 'bf16', 2, H, W, 128, 64, k=3, acc=int(W == 62),
            fam=['TILE128 window bf16' if win else 'TILE128 gather BN128'])
        add('win_dgrad_psx_' + t, 'dgrad', 'bf16x3', 2, H, W, 128, 64, k=3, psx=True,
            fam=['TILE128 window f32 dgrad psx' if win else 'TILE128 gather BN128'])
        add('win_dgrad_bn_psx_' + t, 'dgrad_bn', 'f16x3_3', 2, H, W, 64, 64, k=3, psx=True, psw=H == 1, mode=2, acc=int(W == 61),
            fam=['TILE128 window f32 dgrad psx reduce' if win else 'TILE128 gather BN64'])
        add('win_dgrad_bn_bf16_' + t, 'dgrad_bn', 'bf16', 2, H, W, 64, 64, k=3, mode=2, fam=['TILE128 window bf16', 'bf16 EPS1'] if win else ['bf16 EPS1'])

    # ---- data gradient + BatchNorm-backward reduce: mask modes 1 - 4, store and accumulate; the EPS epilogues
    for mode in (1, 2, 3, 4):
        for acc in (0, 1):
            eps_b = {(2, 0): 1, (4, 0): 3, (4, 1): 4}.get((mode, acc), 0)
            eps_f = {(2, 0): 1, (4, 1): 4}.get((mode, acc), 0)
            t = 'm%d_acc%d' % (mode, acc)
            add('dgrad_bn_bf16_' + t, 'dgrad_bn', 'bf16', 3, 5, 9, 128, 64, mode=mode, acc=acc, env=NO_WIDE, args=dict(EPS=eps_b),
                fam=['bf16 EPS%d' % eps_b] if eps_b else [])
            add('dgrad_bn_bf16_k3_' + t, 'dgrad_bn', 'bf16', 3, 9, 5, 128, 64, k=3, mode=mode, acc=acc, env=NO_WIDE, fam=['TILE128 window bf16'])
            add('dgrad_bn_exact_' + t, 'dgrad_bn', 'exact', 3, 6, 10, 96, 32, mode=mode, acc=acc, args=dict(EPS=0))
            add('dgrad_bn_exact_k3_' + t, 'dgrad_bn', 'exact', 3, 7, 1, 96, 32, k=3, mode=mode, acc=acc, args=dict(EPS=0))
            add('dgrad_bn_psx_' + t, 'dgrad_bn', 'f16x3_3', 3, 9, 5, 128, 64, mode=mode, acc=acc, psx=True, psw=bool(acc), args=dict(EPS=eps_f),
                fam=['f32 EPS%d' % eps_f] if eps_f else [])
            add('dgrad_bn_psx_k3_' + t, 'dgrad_bn', 'bf16x6_3', 3, 1, 7, 128, 64, k=3, mode=mode, acc=acc, psx=True,
                fam=['TILE128 window f32 dgrad psx reduce'])
            add('dgrad_bn_bf16x3_' + t, 'dgrad_bn', 'bf16x3', 3, 5, 9, 128, 64, mode=mode, acc=acc, args=dict(EPS=0))
    add('dgrad_bn_bf16x6_m2', 'dgrad_bn', 'bf16x6', 3, 5, 9, 128, 64, mode=2, args=dict(SPL=6))
    add('dgrad_bn_bf16x6_m3_acc', 'dgrad_bn', 'bf16x6', 3, 9, 5, 128, 64, k=3, mode=3, acc=1, args=dict(SPL=6))
    add('dgrad_bn_psx_nobatch', 'dgrad_bn', 'f16x3_3', 3, 9, 5, 128, 64, mode=2, psx=True, env={'SIMCLR_F32_EPI_BATCH': '0'}, args=dict(EPS=0))
    add('dgrad_bn_psx_bn128', 'dgrad_bn', 'f16x3_3', 3, 5, 9, 128, 256, mode=2, psx=True, args=dict(EPS=1, BN=128), fam=['f32 EPS1'])
    add('dgrad_bn_psx_bn128_m4', 'dgrad_bn', 'f16x3_3', 3, 5, 9, 128, 256, mode=4, acc=1, psx=True, args=dict(EPS=4, BN=128), fam=['f32 EPS4'])

    # ---- statistics: the statistics-only pass, the pivoted forward
    for (H, W) in ((5, 9), (9, 5)):
        for k in (1, 3):
            t = '%dx%d_k%d' % (H, W, k)
            add('stats_only_' + t, 'fwd', 'bf16', 3, H, W, 64, 192, k=k, stats=True, store=False, env=NO_WIDE)
            for ar in F32_ARITHS:
                add('pivoted_%s_%s' % (t, ar), 'fwd_pivoted', ar, 3, H, W, 64, 192 if k == 1 else 64, k=k, psw=ar == 'f16x3_3' and H == 5)
    add('pivoted_7x10_s2', 'fwd_pivoted', 'f16x3_3', 3, 7, 10, 64, 72, k=3, s=2)
    add('pivoted_10x7_s2', 'fwd_pivoted', 'exact', 3, 10, 7, 32, 72, k=3, s=2)

    # ---- the two designated bf16 rounding rows (+ the eight-phase tile, whose statistics are those of the accumulators too)
    add('round_acc_tile128', 'fwd', 'bf16', 1, 5, 8, 512, 256, stats=True, dense='acc', env=T128, fam=['TILE128 gather BN128'])
    add('round_rounded_tile256', 'fwd', 'bf16', 1, 5, 8, 512, 256, stats=True, dense='rounded', env=T256, fam=['TILE256'])
    add('round_acc_wide', 'fwd', 'bf16', 1, 8, 5, 512, 256, stats=True, dense='acc', env=WIDE, fam=['WIDE flat'])

    # ---- fused BatchNorm-apply forward: bf16 FAS 0 / 1 / 2, the fp32 N-walk and its M-inner twin, the other fp32 arithmetics
    for res in (None, 'plain', 'bn'):
        for relu in (0, 1):
            t = '%s_relu%d' % (res or 'nores', relu)
            fas = (1 if res == 'plain' else 2) if (res and relu) else 0
            add('fapply_bf16_' + t, 'fwd_bn_apply', 'bf16', 3, 5, 9, 64, 192, res=res, relu=relu, env=T128, fam=['bf16 FAS%d' % fas])
            add('fapply_bf16_k3_' + t, 'fwd_bn_apply', 'bf16', 3, 9, 5, 64, 72, k=3, res=res, relu=relu, env=T128)
            add('fapply_bf16_tile256_' + t, 'fwd_bn_apply', 'bf16', 3, 6, 10, 64, 256, res=res, relu=relu, env=T256, fam=['TILE256 fapply'])
            nw = ['NWALK FAS%d' % fas] if fas else ['f32 fapply SPL13']
            add('fapply_f16x3_3_' + t, 'fwd_bn_apply', 'f16x3_3', 3, 9, 5, 64, 192, res=res, relu=relu, psw=bool(relu), fam=nw)
            add('fapply_f16x3_3_minner_' + t, 'fwd_bn_apply', 'f16x3_3', 3, 9, 5, 64, 192, res=res, relu=relu, env={'SIMCLR_IGEMM_NWALK': '0'},
                fam=['f32 fapply SPL13'])
            add('fapply_exact_' + t, 'fwd_bn_apply', 'exact', 3, 6, 10, 32, 72, res=res, relu=relu, fam=['f32 fapply SPL0'])
            add('fapply_f16x3_3_s2_' + t, 'fwd_bn_apply', 'f16x3_3', 3, 7, 10, 64, 192, s=2, res=res, relu=relu)
    add('fapply_bf16_nobits', 'fwd_bn_apply', 'bf16', 3, 5, 9, 64, 192, res='plain', bits=False, env=T128, fam=['bf16 FAS0'])
    add('fapply_bf16x6_3', 'fwd_bn_apply', 'bf16x6_3', 3, 5, 9, 64, 192, res='bn', fam=['f32 fapply SPL6'])
    add('fapply_bf16x3', 'fwd_bn_apply', 'bf16x3', 3, 9, 5, 64, 72, res='plain', fam=['f32 fapply SPL3'])
    add('fapply_bf16x6', 'fwd_bn_apply', 'bf16x6', 3, 1, 7, 96, 72, k=3, relu=0, fam=['f32 fapply SPL6'])

    # ---- weight gradient: every family with accumulate 0 / 1 and one / several slabs
    ONE, MANY = (1, 3, 9), (3, 6, 10)           # 27 rows: one reduction chunk; 180 rows: several pixel ranges
    for acc in (0, 1):
        for (sp, (V, H, W)) in (('one', ONE), ('many', MANY)):
            t = 'acc%d_%s' % (acc, sp)
            kw = dict(acc=acc, splits=sp)
            add('wgrad_reg_cin32_' + t, 'wgrad', 'exact', V, H, W, 32, 72, fam=['REG_STAGED'], **kw)
            add('wgrad_reg_cfg0_' + t, 'wgrad', 'bf16', V, H, W, 64, 128, env={'SIMCLR_WGRAD_CFG': '0'}, fam=['REG_STAGED'], **kw)
            for cfg, st in ((1, 2), (2, 3), (3, 4)):
                add('wgrad_dma_cfg%d_%s' % (cfg, t), 'wgrad', 'bf16', V, H, W, 128, 128, k=1 + 2 * (cfg == 2), s=1 + (cfg == 2),
                    env={'SIMCLR_WGRAD_CFG': str(cfg), 'SIMCLR_WGRAD_3X3': '0'}, fam=['DMA_RING stages %d' % st], **kw)
            for ar in ('exact', 'bf16x3', 'bf16x6'):
                add('wgrad_dma_%s_%s' % (ar, t), 'wgrad', ar, V, H, W, 64, 72, fam=['DMA_RING'], **kw)
            add('wgrad_dma_psx_' + t, 'wgrad', 'f16x3_3', V, H, W, 64, 96, psx=True, fam=['DMA_RING'], args=dict(PSD=1), **kw)
            V3, H3, W3 = (1, 3, 7) if sp == 'one' else (3, 9, 7)
            add('wgrad_nine_bf16_' + t, 'wgrad', 'bf16', V3, H3, W3, 64, 128, k=3, fam=['NINE_TAP_BF16'], **kw)
            add('wgrad_nine_f32ps_' + t, 'wgrad', 'bf16x3', V3, H3, W3, 128, 64, k=3, psx=True, fam=['NINE_TAP_F32PS'], **kw)
            add('wgrad_tile256_f32_' + t, 'wgrad', 'bf16x6_3', V, H, W, 256, 256, psx=True, fam=['TILE256_F32'], **kw)
    # nine-tap: W = 7 is the first eligible width, 6 keeps the per-tap ring; SIMCLR_WGRAD_3X3=0 switches it off; block-count switches
    add('wgrad_w6_bf16', 'wgrad', 'bf16', 3, 9, 6, 64, 64, k=3, fam=['DMA_RING stages 2'])
    add('wgrad_w7_bf16', 'wgrad', 'bf16', 3, 9, 7, 64, 64, k=3, fam=['NINE_TAP_BF16'])
    add('wgrad_w6_f32ps', 'wgrad', 'f16x3_3', 3, 9, 6, 64, 64, k=3, psx=True, fam=['DMA_RING'])
    add('wgrad_w7_f32ps', 'wgrad', 'f16x3_3', 3, 9, 7, 64, 64, k=3, psx=True, fam=['NINE_TAP_F32PS'])
    add('wgrad_w7_3x3_off', 'wgrad', 'bf16', 3, 9, 7, 64, 64, k=3, env={'SIMCLR_WGRAD_3X3': '0'}, fam=['DMA_RING stages 2'])
    add('wgrad_blocks64', 'wgrad', 'bf16', 3, 20, 30, 128, 256, env={'SIMCLR_WGRAD_BLOCKS': '64'}, splits='many', fam=['DMA_RING stages 2'])
    add('wgrad3_blocks8', 'wgrad', 'bf16', 3, 20, 30, 128, 128, k=3, env={'SIMCLR_WGRAD3_BLOCKS': '8'}, splits='many', fam=['NINE_TAP_BF16'])
    add('wgrad3_blocks8_f32ps', 'wgrad', 'bf16x3', 3, 30, 20, 64, 128, k=3, psx=True, env={'SIMCLR_WGRAD3_BLOCKS': '8'}, splits='many',
        fam=['NINE_TAP_F32PS'])
    # ---- K-extended data gradient: dx (+)= dm Wext[:, :Cout]^T + h Wext[:, Cout:]^T + bias, plain and with the fused reduce.  Both channel
    # counts are multiples of 8 chunks (32 fp32, 64 bf16); fp32 32 + 64 = 96 is no multiple of a 64-element k-tile.
    EXT_AR = ('bf16', 'exact', 'bf16x3', 'f16x3_3')
    ext_ch = lambda ar: [(64, 64), (64, 128), (128, 64)] if ar == 'bf16' else [(32, 32), (32, 96), (96, 32), (64, 32), (32, 64)]
    for ar in EXT_AR:
        e128 = 'EXT TILE128 ' + ('bf16' if ar == 'bf16' else 'f32')
        for i, (Cin, Cout) in enumerate(ext_ch(ar)):
            H, W = NONSQUARE[i % len(NONSQUARE)]
            t = 'cin%d_cout%d_%s' % (Cin, Cout, ar)
            add('ext_dgrad_' + t, 'dgrad', ar, 3, H, W, Cin, Cout, ext=True, acc=i % 2, env=NO_WIDE, fam=[e128], args=dict(EXT='true'))
            add('ext_dgrad_bn_' + t, 'dgrad_bn', ar, 3, W, H, Cin, Cout, ext=True, mode=1 + i % 4, acc=(i + 1) % 2, env=NO_WIDE, fam=[e128 + ' reduce'])
        Cin, Cout = ext_ch(ar)[1]
        for i, M in enumerate((1, 127, 128, 129, 255, 256, 257)):
            V, H, W = ROWS[M]
            add('ext_rows%d_dgrad_%s' % (M, ar), 'dgrad', ar, V, H, W, Cin, Cout, ext=True, acc=i % 2, env=NO_WIDE, fam=[e128])
            add('ext_rows%d_dgrad_bn_%s' % (M, ar), 'dgrad_bn', ar, V, H, W, Cout, Cin, ext=True, mode=1 + i % 4, acc=(i // 4) % 2, env=NO_WIDE,
                fam=[e128 + ' reduce'])
        Cin, Cout = ext_ch(ar)[0]
        for mode in (1, 2, 3, 4):
            for acc in (0, 1):
                H, W = NONSQUARE[(mode + acc) % len(NONSQUARE)]
                add('ext_dgrad_bn_m%d_acc%d_%s' % (mode, acc, ar), 'dgrad_bn', ar, 3, H, W, Cin, Cout, ext=True, mode=mode, acc=acc, env=NO_WIDE,
                    fam=[e128 + ' reduce'])
    # (the SIMCLR_IGEMM_TILE=256 class: bf16, 256 channels of dx)
    for i, M in enumerate((255, 256, 257)):
        V, H, W = ROWS[M]
        add('ext_rows%d_tile256_dgrad' % M, 'dgrad', 'bf16', V, H, W, 256, 64, ext=True, acc=i % 2, env=T256, fam=['EXT TILE256 bf16'])
        add('ext_rows%d_tile256_dgrad_bn' % M, 'dgrad_bn', 'bf16', V, H, W, 256, 64, ext=True, mode=2 + i, acc=(i + 1) % 2, env=T256,
            fam=['EXT TILE256 bf16 reduce'])
    add('ext_tile256_dgrad_bn_m1', 'dgrad_bn', 'bf16', 3, 6, 10, 256, 128, ext=True, mode=1, env=T256, fam=['EXT TILE256 bf16 reduce'])

    # ---- sparse store (accumulate = 3) and sparse accumulate (2) of the 1x1 stride-2 shortcut: odd and even extents per axis, so that the
    # last row / column is an even-index pixel in some rows and an odd one in others; dx channels 64 <- 32 and 32 <- 64
    SPARSE_MAPS = [(3, 7, 10), (3, 10, 7), (3, 1, 9), (3, 9, 1)] + [ROWS[M] for M in (1, 127, 128, 129)]
    for i, (V, H, W) in enumerate(SPARSE_MAPS):
        for j, ar in enumerate(('exact', 'bf16x3', 'f16x3_3')):
            Cin, Cout = ((64, 32), (32, 64))[(i + j) % 2]
            t = '%dx%dx%d_%s' % (V, H, W, ar)
            psx = ar == 'f16x3_3'
            add('sparse_store_' + t, 'dgrad', ar, V, H, W, Cin, Cout, s=2, acc=3, psx=psx, fam=['SPARSE acc3 f32'])
            add('sparse_acc_' + t, 'dgrad', ar, V, H, W, Cin, Cout, acc=2, psx=psx, fam=['SPARSE acc2 f32'])
            add('sparse_acc_bn_' + t, 'dgrad_bn', ar, V, H, W, Cin, Cout, acc=2, mode=2 if (i + j) % 2 else 4, psx=psx, fam=['SPARSE acc2 f32 reduce'])
            add('sparse_acc_bn2_' + t, 'dgrad_bn', ar, V, H, W, Cout, Cin, acc=2, mode=4 if (i + j) % 2 else 2, fam=['SPARSE acc2 f32 reduce'])
        add('sparse_store_%dx%dx%d_bf16' % (V, H, W), 'dgrad', 'bf16', V, H, W, (64, 32)[i % 2], 64, s=2, acc=3, fam=['SPARSE acc3 bf16'])

    ids = [c.id for c in rows]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return rows


CASES = build_cases()
CASE_BY_ID = {c.id: c for c in CASES}
