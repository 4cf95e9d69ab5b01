"""DropBlock (tf2/resnet.py:81-157) restated in numpy, with the noise as an INPUT, plus the stateless generator of
csrc/dropblock.hip restated in numpy.  Independent of the product code: nothing here imports simclr_amd.

Per site, net [V,H,W,C] NHWC:
    k      = min(dropblock_size, W)
    gamma  = (1 - keep_prob) * W**2 / k**2 / (W - k + 1)**2                     (Python double)
    valid  = k//2 <= i < W - (k-1)//2 on both axes
    seed   = ((1 - valid) + fp32(1 - gamma)) + u >= 1                           (fp32, in this order)
    k == W: pattern = min of seed over (H, W), shape [V,1,1,C]
    else  : pattern = k x k stride-1 SAME min-pool; output i covers inputs i-(k-1)//2 .. i+k//2 clipped to the map
    percent_ones = fp32(sum(pattern)) / fp32(size(pattern))
    out    = net / percent_ones * pattern
"""
import numpy as np

GOLDEN = 0x9E3779B97F4A7C15
_M64 = (1 << 64) - 1


def gamma_of(keep_prob, width, dropblock_size):
    k = min(dropblock_size, width)
    return k, (1.0 - keep_prob) * width**2 / k**2 / (width - k + 1)**2


def valid_centres(width, k):
    """bool [W]: the 1-D valid-centre set; the 2-D one is its outer AND."""
    i = np.arange(width)
    return (i >= k // 2) & (i < width - (k - 1) // 2)


def seed_pattern(u, keep_prob, dropblock_size):
    """u fp32 [V,H,W,C] -> float32 {0,1} [V,H,W,C]."""
    V, H, W, C = u.shape
    if H != W:
        raise ValueError('Input tensor with width!=height is not supported.')
    k, gamma = gamma_of(keep_prob, W, dropblock_size)
    v1 = valid_centres(W, k)
    valid = (v1[:, None] & v1[None, :]).astype(np.float32)[None, :, :, None]
    t = (np.float32(1) - valid) + np.float32(1.0 - gamma)          # fp32
    t = (t + u.astype(np.float32)).astype(np.float32)              # fp32 add, rounded
    return (t >= np.float32(1)).astype(np.float32)


def min_pool_same(x, k):
    """k x k stride-1 SAME min-pool over axes (1, 2) of [V,H,W,C]; window of output i: i-(k-1)//2 .. i+k//2, clipped."""
    V, H, W, C = x.shape
    back, fwd = (k - 1) // 2, k // 2
    rows = np.empty_like(x)
    for w in range(W):
        rows[:, :, w] = x[:, :, max(0, w - back):min(W, w + fwd + 1)].min(axis=2)
    out = np.empty_like(x)
    for h in range(H):
        out[:, h] = rows[:, max(0, h - back):min(H, h + fwd + 1)].min(axis=1)
    return out


def block_pattern(u, keep_prob, dropblock_size):
    """-> (pattern broadcast to [V,H,W,C] float32, ones, size) with ones / size in the reference's units (planes when k == W)."""
    V, H, W, C = u.shape
    seed = seed_pattern(u, keep_prob, dropblock_size)
    k = min(dropblock_size, W)
    if k == W:
        p = seed.min(axis=(1, 2), keepdims=True)
        ones, size = int(p.sum(dtype=np.float64)), p.size
        return np.broadcast_to(p, seed.shape).copy(), ones, size
    p = min_pool_same(seed, k)
    return p, int(p.sum(dtype=np.float64)), p.size


def percent_ones(ones, size):
    return np.float32(ones) / np.float32(size)


def apply_f32(x, pattern, ones, size):
    """fp32 `net / percent_ones * block_pattern` (true division, then the multiply)."""
    return ((x.astype(np.float32) / percent_ones(ones, size)).astype(np.float32) * pattern.astype(np.float32)).astype(np.float32)


def dropblock_f64(x, u, keep_prob, dropblock_size):
    """The whole site in float64 (pattern and percent_ones exact rationals of the counts)."""
    p, ones, size = block_pattern(u, keep_prob, dropblock_size)
    return x.astype(np.float64) / (ones / size) * p.astype(np.float64)


def relu_f32(o):
    """relu as the tail kernel defines it: o < 0 ? 0 : o (NaN and -0 pass)."""
    return np.where(o < np.float32(0), np.float32(0), o).astype(np.float32)


def tail_fwd_f32(a, pa, ca, b, pb, cb):
    return relu_f32((apply_f32(a, pa, *ca) + apply_f32(b, pb, *cb)).astype(np.float32))


def tail_bwd_f32(dout, relu_mask, pa, ca, pb, cb):
    g = np.where(relu_mask, dout.astype(np.float32), np.float32(0)).astype(np.float32)
    return apply_f32(g, pa, *ca), apply_f32(g, pb, *cb)


def pack_bits(pattern):
    """{0,1} [V,H,W,C] -> uint8 [V,H,W,C/8], bit j of a byte = channel 8*byte + j."""
    return np.packbits(pattern.astype(np.uint8), axis=-1, bitorder='little')


def unpack_bits(bits, C):
    return np.unpackbits(bits, axis=-1, bitorder='little')[..., :C]


def bf16_round(x):
    """fp32 -> the nearest bf16 value (ties to even), returned as fp32."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return (r & 0xFFFFFFFF).astype(np.uint32).view(np.float32).reshape(np.shape(x))


# ---- the generator: u of linear NHWC element i ---------------------------------------------------------------------------------
def _mix64(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over='ignore'):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def generator_uniform(key, shape):
    """u [shape] fp32: element i draws (32 bits >> 8) * 2^-24, the 32 bits = the low (i even) / high (i odd) half of
    splitmix64's output function at key + (i // 2 + 1) * GOLDEN (all arithmetic modulo 2^64)."""
    n = int(np.prod(shape))
    i = np.arange(n, dtype=np.uint64)
    with np.errstate(over='ignore'):
        r = _mix64(np.uint64(key & _M64) + (i // np.uint64(2) + np.uint64(1)) * np.uint64(GOLDEN))
    half = np.where(i % np.uint64(2) == 0, r & np.uint64(0xFFFFFFFF), r >> np.uint64(32))
    return ((half >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)).reshape(shape)


def _mix64_int(z):
    z &= _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def site_key(seed, step, replica, site):
    """The key of a site: a chain of splitmix64 mixes over (seed, step, replica, site)."""
    k = _mix64_int(int(seed) + GOLDEN)
    for v in (step, replica, site):
        k = _mix64_int(k + (int(v) + 1) * GOLDEN)
    return k
