"""Stage-by-stage references for the augmentation kernels (csrc/augment.hip) and the blur (blur1d in csrc/pool.hip).
Pure numpy on the CPU: shared by tests/gpu_checks.py (the GPU checks of tests/test_gpu_augment.py) and tests/test_augment_reference.py
(which pins it without a GPU).  TEST INFRASTRUCTURE ONLY.

* CASES.  A case is a dict {name, stage, src [b,Hs,Ws,3] uint8 | float32, sizes [b,2], params [b,views,16] float32 (what the kernel is
  given), ref_params (what the oracle is given: differs only where the kernel documents a clamp), H, W}.  Stages are isolated through the
  parameter table alone: an identity crop (crop = whole image, output size = image size) makes every bicubic weight exactly (0,1,0,0), so
  the colour stage sees the source pixels bit for bit; jitter_on = 0 and gray_on = 0 leave the resize alone.
* REFERENCE.  `oracle(case)`: oracle/augment.py in float64, record by record, laid out [b,H,W,3*views].
* FLOAT32 EMULATION.  `emulate(case, np.float32)`: the same formulas with float32 intermediates in the kernels' order of operations
  (no fused multiply-add).  E32 = max |emulate32 - oracle| is the rounding error the operation forces at working precision; the tolerance of
  a stage is 4 * max E32 over its cases (`stage_tolerance`) -- the 4 covers fma contraction, 1/s * w against w / s and summation order.
  Nothing measured on the kernels enters a tolerance.  `emulate(case, dt, mut=(...))` are the mutants the comparator has to reject.
* AMBIGUOUS COORDINATES.  The 1/1024 weight-table index of (o + 0.5) * scale - 0.5 may differ between the contracted (fma) and the
  uncontracted float32 evaluation; both are legitimate compilations.  `ambiguous_coords` lists such output coordinates; at those rows /
  columns only, `compare` also accepts the oracle evaluated with the other index.  Dyadic output sizes have none (asserted on the CPU).
* COMPARATOR.  `compare(got, case, tol)`: every element, no quantile.  Returns the project's result dicts {name, err, tol, ok, ...}.
"""
import functools
import itertools

import numpy as np

from oracle import augment as oa
from oracle import blur as oblur

P = 16
PERMS = list(itertools.permutations(range(4)))          # the 24 jitter orders (0 brightness, 1 contrast, 2 saturation, 3 hue)
F32, F64 = np.float32, np.float64
MUTANTS_AUGMENT = ('flip_hw', 'out_hw', 'view_offset', 'mean_raw', 'mean_hw1', 'order_rev', 'no_clip', 'gray_weights', 'no_wrap',
                   'no_cat_clamp', 'no_sat_clip', 'keep_oob_tap', 'index_off1')
MUTANTS_BLUR = ('blur_no_clamp', 'blur_vert_in')


def entry(name, err, tol, numel=1, nbad=None, **kw):
    d = dict(name=name, err=float(err), tol=float(tol), scale=1.0, ok=bool(err <= tol), nbad=int(err > tol) if nbad is None else int(nbad),
             numel=int(numel))
    d.update(kw)
    return d


# ---------------------------------------------------------------------------------------------------------------- bicubic taps
def in_loc(o, scale, contracted):
    """(floor, table index) of the source location of output coordinate o.  contracted: (o + 0.5) * scale - 0.5 rounded once (fma: the
    float64 product of two float32 is exact, so is the subtraction at these magnitudes), otherwise rounded after the product as well."""
    a = F32(o) + F32(0.5)
    v = F32(F64(a) * F64(scale) - 0.5) if contracted else F32(a * scale - F32(0.5))
    fl = np.floor(v)
    return int(fl), int(np.rint(F32(v - fl) * F32(1024)))


def ambiguous_coords(out_size, in_size):
    scale = F32(in_size) / F32(out_size)
    key = lambda lo: 1024 * lo[0] + lo[1]          # (k - 1, 1024) and (k, 0) are the same taps and weights
    return [o for o in range(out_size) if key(in_loc(o, scale, False)) != key(in_loc(o, scale, True))]


def _cubic32(x):
    """Keys cubic A = -0.5 at |x| <= 1 and at 1 + x, evaluated in float32 (the kernel evaluates instead of reading a table)."""
    a = F32(-0.5)
    near = ((a + F32(2)) * x - (a + F32(3))) * x * x + F32(1)
    y = x + F32(1)
    far = ((a * y - F32(5) * a) * y + F32(8) * a) * y - F32(4) * a
    return near, far


def taps(out_size, in_size, dt=F64, alt=False, mut=()):
    """oracle.augment.bicubic_taps restated with the working type as a parameter.  dt = float64, alt = False reproduces the oracle
    (pinned by tests/test_augment_reference.py); alt = True takes the contracted location."""
    idx, wts = _taps(out_size, in_size, dt, bool(alt), tuple(m for m in mut if m in ('index_off1', 'keep_oob_tap')))
    return idx.copy(), wts.copy()


@functools.lru_cache(None)
def _taps(out_size, in_size, dt, alt, mut):
    scale = F32(in_size) / F32(out_size)
    idx = np.zeros((out_size, 4), np.int64)
    wts = np.zeros((out_size, 4), dt)
    for o in range(out_size):
        loc, off = in_loc(o, scale, alt)
        if 'index_off1' in mut:
            off = min(off + 1, oa.K_TABLE)
        if dt is F64:
            w = [oa._T1[off], oa._T0[off], oa._T0[oa.K_TABLE - off], oa._T1[oa.K_TABLE - off]]
        else:
            n0, f0 = _cubic32(F32(off) * F32(1.0 / 1024))
            n1, f1 = _cubic32(F32(1024 - off) * F32(1.0 / 1024))
            w = [f0, n0, n1, f1]
        for j in range(4):
            want = loc - 1 + j
            got = min(max(want, 0), in_size - 1)
            if got != want and 'keep_oob_tap' not in mut:
                w[j] = dt(0)
            idx[o, j] = got
        s = F32(w[0]) + F32(w[1]) + F32(w[2]) + F32(w[3])
        if abs(float(s)) >= 1000.0 * float(np.finfo(np.float32).tiny):
            w = [dt(wj) / dt(s) for wj in w]
        wts[o] = w
    return idx, wts


def resize(img, H, W, dt=F64, alt_r=False, alt_c=False, mut=()):
    """img [h,w,3] of type dt -> [H,W,3]; per output pixel the kernel's order: four taps along x per source row, then the four rows."""
    iy, wy = taps(H, img.shape[0], dt, alt_r, mut)
    ix, wx = taps(W, img.shape[1], dt, alt_c, mut)
    acc = np.zeros((H, W, 3), dt)
    for a in range(4):
        row = np.zeros((H, W, 3), dt)
        rows = img[iy[:, a]]                                             # [H, w, 3]
        for c in range(4):
            row = row + wx[None, :, c, None] * rows[:, ix[:, c]]
        acc = acc + wy[:, a, None, None] * row
    assert acc.dtype == dt
    return acc


# ---------------------------------------------------------------------------------------------------------------- colour chain
def rgb_to_hsv(rgb, dt, mut=()):
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    v = np.maximum(r, np.maximum(g, b))
    rng_ = v - np.minimum(r, np.minimum(g, b))
    one, zero = dt(1), dt(0)
    s = np.where(v > 0, rng_ / np.where(v > 0, v, one), zero)
    norm = one / (dt(6) * np.where(rng_ > 0, rng_, one))
    h = np.where(r == v, norm * (g - b), np.where(g == v, norm * (b - r) + dt(2) / dt(6), norm * (r - g) + dt(4) / dt(6)))
    h = np.where(rng_ <= 0, zero, h)
    if 'no_wrap' not in mut:
        h = np.where(h < 0, h + one, h)
    return h.astype(dt), s.astype(dt), v


def hsv_to_rgb(h, s, v, dt, mut=()):
    c = s * v
    m = v - c
    dh = h * dt(6)
    cat = np.floor(dh).astype(np.int64)
    fm = np.mod(dh, dt(2))
    x = c * (dt(1) - np.abs(fm - dt(1)))
    z = np.zeros_like(c)
    cc = np.clip(cat, 0, 5)
    rr = np.choose(cc, [c, x, z, z, x, c])
    gg = np.choose(cc, [x, c, c, x, z, z])
    bb = np.choose(cc, [z, z, x, c, c, x])
    if 'no_cat_clamp' in mut:                                            # a switch without the clamp and without a default
        out = (cat < 0) | (cat > 5)
        rr, gg, bb = np.where(out, z, rr), np.where(out, z, gg), np.where(out, z, bb)
    return np.stack([rr + m, gg + m, bb + m], -1).astype(dt)


def jitter(img, p, dt, mut=()):
    """The four ops of record p in its order, each followed by the clip; the contrast mean is the double-precision mean of the image as it
    is when contrast runs, rounded to the working type (aug_color_mean)."""
    raw = img
    perm = [int(v) for v in p[6:10]]
    if 'order_rev' in mut:
        perm = perm[::-1]
    for op in perm:
        if op == 0:
            img = img * dt(p[10])
        elif op == 1:
            base = (raw if 'mean_raw' in mut else img).astype(F64).reshape(-1, 3)
            n = base.shape[0]
            mean = ((base[:-1].sum(0) if 'mean_hw1' in mut else base.sum(0)) / n).astype(dt)
            img = (img - mean) * dt(p[11]) + mean
        elif op == 2:
            h, s, v = rgb_to_hsv(img, dt, mut)
            s = s * dt(p[12])
            if 'no_sat_clip' not in mut:
                s = np.clip(s, dt(0), dt(1))
            img = hsv_to_rgb(h, s, v, dt, mut)
        else:
            h, s, v = rgb_to_hsv(img, dt, mut)
            h = h + dt(p[13]) + dt(1)
            h = h - np.floor(h)
            img = hsv_to_rgb(h, s, v, dt, mut)
        if 'no_clip' not in mut:
            img = np.clip(img, dt(0), dt(1))
        assert img.dtype == dt
    return img


def to_float(img, dt):
    img = np.asarray(img)
    if img.dtype == np.uint8:
        return img.astype(dt) * (F32(1.0 / 255.0) if dt is F32 else 1.0 / 255.0)
    return img.astype(dt)


def apply_record(image, p, H, W, dt=F64, alt_r=False, alt_c=False, mut=()):
    """oracle.augment.apply_train_params in working type dt.  Returns the pre-layout image [H,W,3] (flip applied by the caller)."""
    img = to_float(image, dt)
    y, x, h, w = (int(v) for v in p[0:4])
    img = resize(img[y:y + h, x:x + w], H, W, dt, alt_r, alt_c, mut)
    return img


def colour_record(img, p, dt, mut=()):
    if p[5] > 0:
        img = jitter(img, p, dt, mut)
    if p[14] > 0:
        wts = (0.299, 0.587, 0.114) if 'gray_weights' in mut else (0.2989, 0.5870, 0.1140)
        g = img[..., 0] * dt(wts[0]) + img[..., 1] * dt(wts[1]) + img[..., 2] * dt(wts[2])
        img = np.repeat(g[..., None], 3, -1)
    return np.clip(img, dt(0), dt(1))


def _images(case):
    src, sizes = case['src'], case['sizes']
    return [src[i, :sizes[i, 0], :sizes[i, 1]] for i in range(src.shape[0])]


def emulate(case, dt=F32, alt_r=False, alt_c=False, mut=()):
    """The three kernels on the case's reference parameters, with the kernels' flat indexing for the layout mutants."""
    H, W, p = case['H'], case['W'], case['ref_params']
    b, views = p.shape[:2]
    out = np.zeros((b, H, W, 3 * views), dt)
    for i, im in enumerate(_images(case)):
        for v in range(views):
            r = apply_record(im, p[i, v], H, W, dt, alt_r, alt_c, mut)
            if p[i, v, 4] > 0:
                if 'flip_hw' in mut:                                     # dx = H - 1 - ox in the flat index ((iv*H + oy)*W + dx)
                    flat = np.arange(H)[:, None] * W + (H - 1 - np.arange(W))[None, :]
                    ok = (flat >= 0) & (flat < H * W)
                    t = np.zeros((H * W, 3), dt)
                    t[flat[ok]] = r[ok]
                    r = t.reshape(H, W, 3)
                else:
                    r = r[:, ::-1]
            if 'out_hw' in mut:                                          # tmp written as [W][H], read as [H][W]
                r = np.ascontiguousarray(r.transpose(1, 0, 2)).reshape(H, W, 3)
            r = colour_record(r, p[i, v], dt, mut)
            o = v if 'view_offset' in mut else 3 * v
            out[i, :, :, o:o + 3] = r
    return out


def oracle(case):
    """float64 oracle/augment.py, cached in the case."""
    if '_ref' not in case:
        H, W, p = case['H'], case['W'], case['ref_params'].astype(F64)
        b, views = p.shape[:2]
        out = np.zeros((b, H, W, 3 * views))
        for i, im in enumerate(_images(case)):
            for v in range(views):
                out[i, :, :, 3 * v:3 * v + 3] = oa.apply_train_params(im, p[i, v], H, W)
        case['_ref'] = out
    return case['_ref']


def ambiguity(case):
    """Per record (rows, columns) of the OUTPUT at which the other table index is admissible (columns mirrored where flipped)."""
    if '_amb' not in case:
        H, W, p = case['H'], case['W'], case['ref_params']
        amb = {}
        for i in range(p.shape[0]):
            for v in range(p.shape[1]):
                rows = ambiguous_coords(H, int(p[i, v, 2]))
                cols = ambiguous_coords(W, int(p[i, v, 3]))
                if p[i, v, 4] > 0:
                    cols = [W - 1 - c for c in cols]
                if rows or cols:
                    amb[(i, v)] = (rows, cols)
        case['_amb'] = amb
    return case['_amb']


def ambiguous_share(case):
    """max over the records of (ambiguous rows + columns) / (H + W): the condition of a usable case is <= 0.02."""
    return max([(len(r) + len(c)) / float(case['H'] + case['W']) for r, c in ambiguity(case).values()] or [0.0])


def error_map(got, case):
    """|got - oracle| per element; at an ambiguous row / column the smaller of that and the distance to the oracle with the other index."""
    got = np.asarray(got, F64)
    err = np.abs(got - oracle(case))
    for (i, v), (rows, cols) in ambiguity(case).items():
        if '_alt' not in case:
            case['_alt'] = {}
        for ar, ac in ((True, False), (False, True), (True, True)):
            if (ar and not rows) or (ac and not cols):
                continue
            key = (i, v, ar, ac)
            if key not in case['_alt']:
                one = dict(case, src=case['src'][i:i + 1], sizes=case['sizes'][i:i + 1], ref_params=case['ref_params'][i:i + 1, v:v + 1])
                for k in ('_ref', '_amb', '_alt'):
                    one.pop(k, None)
                case['_alt'][key] = emulate(one, F64, ar, ac)[0]
            alt = np.abs(got[i, :, :, 3 * v:3 * v + 3] - case['_alt'][key])
            mask = np.zeros((case['H'], case['W'], 1), bool)
            if ar and ac:
                mask[np.ix_(rows, cols)] = True
            elif ar:
                mask[rows] = True
            else:
                mask[:, cols] = True
            e = err[i, :, :, 3 * v:3 * v + 3]
            err[i, :, :, 3 * v:3 * v + 3] = np.where(mask, np.minimum(e, alt), e)
    return err


def compare(got, case, tol, tag=''):
    """Every element of got [b,H,W,3*views] against the float64 oracle (ambiguous coordinates: either index); shape, finiteness, range."""
    name = case['name'] + tag
    p = case['ref_params']
    shape = (p.shape[0], case['H'], case['W'], 3 * p.shape[1])
    got = np.asarray(got)
    if got.shape != shape:
        return [entry(name + ' shape %s != %s' % (got.shape, shape), 1.0, 0.0)]
    g = got.astype(F64)
    if not np.isfinite(g).all():
        return [entry(name + ' non-finite output', float('inf'), tol, numel=g.size, nbad=int((~np.isfinite(g)).sum()))]
    err = error_map(g, case)
    return [entry(name + ' vs float64 oracle', err.max(), tol, numel=err.size, nbad=int((err > tol).sum())),
            entry(name + ' range [0,1]', max(-g.min(), g.max() - 1.0, 0.0), 0.0)]


def e32(case):
    return float(np.abs(emulate(case, F32).astype(F64) - oracle(case)).max())


# ---------------------------------------------------------------------------------------------------------------- case builders
SPECIAL_U8 = (
    [(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255)] +                 # primaries, secondaries
    [(g, g, g) for g in (0, 1, 32, 64, 127, 128, 200, 254, 255)] +                                         # gray ramp: range == 0, v == 0
    [(200, 200, 50), (50, 200, 200), (200, 50, 200), (255, 255, 10), (10, 255, 255), (255, 10, 255)] +     # ties at the maximum
    [(200, 50, 50), (50, 200, 50), (50, 50, 200), (255, 0, 0), (1, 0, 0), (0, 0, 1)] +                     # ties at the minimum
    [(200, 100, 101), (200, 101, 100), (100, 200, 101), (101, 200, 100), (100, 101, 200), (101, 100, 200),  # near-ties
     (200, 199, 10), (199, 200, 10), (10, 200, 199), (10, 199, 200), (199, 10, 200), (200, 10, 199)] +
    [(200, 100, 150), (250, 10, 240), (128, 0, 127), (30, 2, 29)])                                         # negative hue before the wrap
_E24, _E25 = 2.0 ** -24, 2.0 ** -25
SPECIAL_F32 = [(1.0, 0.5, 0.5 + _E24), (0.75, 0.25, 0.25 + _E25), (0.5, 0.25, 0.25 + _E25),                # hue -2e-8 .. -1e-8: wraps to exactly 1.0f
               (1.0, 0.5 + _E24, 0.5), (0.5 + _E24, 1.0, 0.5), (0.5, 0.5 + _E24, 1.0),
               (1.0 - _E24, 1.0, 1.0 - _E24), (_E24, 0.0, 0.0), (0.3, 0.3, 0.3), (0.1, 0.7, 0.7)]


def palette(H, W, seed, kind):
    """[H,W,3] uint8, or its float32 twin with the float-only near-ties added.  Specials first, random pixels after, a bright last pixel
    (a mean that drops it is off by about 1/HW)."""
    rng = np.random.default_rng(seed)
    n = H * W
    assert n >= len(SPECIAL_U8) + len(SPECIAL_F32) + 8
    px = rng.integers(0, 256, (n, 3))
    px[:len(SPECIAL_U8)] = SPECIAL_U8
    px = np.roll(px, 5 * (seed % 11), axis=0)
    px[-1] = (250, 240, 230)
    if kind == 'u8':
        return px.reshape(H, W, 3).astype(np.uint8)
    f = px.astype(F32) * F32(1.0 / 255.0)
    j = n - 1 - len(SPECIAL_F32)
    f[j:j + len(SPECIAL_F32)] = np.asarray(SPECIAL_F32, F64).astype(F32)
    f[j - 4:j] = rng.random((4, 3)).astype(F32)
    return f.reshape(H, W, 3)


def _case(name, stage, src, params, H, W, sizes=None, ref_params=None):
    src = np.ascontiguousarray(src)
    params = np.ascontiguousarray(params, F32)
    if sizes is None:
        sizes = np.tile(np.asarray(src.shape[1:3], np.int64), (src.shape[0], 1))
    return dict(name=name, stage=stage, src=src, params=params, H=H, W=W, sizes=np.asarray(sizes, np.int64),
                ref_params=params if ref_params is None else np.ascontiguousarray(ref_params, F32))


IDENTITY_SIZES = [(15, 17), (16, 16), (17, 15), (16, 32)]


@functools.lru_cache(None)
def identity_case(H, W, views, kind):
    """Identity crop with and without flip; flipped and unflipped views inside one image (b = 3, flip pattern rotates)."""
    b = 3
    src = np.stack([palette(H, W, 100 + i, kind) for i in range(b)])
    p = np.zeros((b, views, P), F32)
    p[:, :, 2], p[:, :, 3] = H, W
    for i in range(b):
        for v in range(views):
            p[i, v, 4] = (i + v) % 2
    return _case('identity %dx%d views%d %s' % (H, W, views, kind), 'identity', src, p, H, W)


def identity_expected(case):
    """The source (uint8: float32(u8) * float32(1/255)), mirrored where flip = 1, at channel offset 3*v."""
    src = to_float(case['src'], F32)
    p = case['params']
    out = np.zeros((src.shape[0], case['H'], case['W'], 3 * p.shape[1]), F32)
    for i in range(p.shape[0]):
        for v in range(p.shape[1]):
            out[i, :, :, 3 * v:3 * v + 3] = src[i][:, ::-1] if p[i, v, 4] > 0 else src[i]
    return out


def _bit(k, n, lo, hi):
    return hi if (k >> n) & 1 else lo


FACTOR_SETS = {      # record k of the 24 -> (jitter_on, brightness, contrast, saturation, hue, gray_on)
    'lo': lambda k: (1, 0.2, 0.2, 0.2, -0.2, 0),
    'hi': lambda k: (1, 1.8, 1.8, 1.8, 0.2, 0),
    'mixed': lambda k: (1, _bit(k, 0, 0.2, 1.8), _bit(k, 1, 1.8, 0.2), _bit(k, 2, 0.2, 1.8), _bit(k, 3, -0.2, 0.2), 0),
    'sat0': lambda k: (1, 1.3, 0.7, 0.0, 0.1, 0),
    'satclip': lambda k: (1, 0.9, 1.2, 5.0, -0.05, 0),
    'hues': lambda k: (1, 1.1, 0.9, 1.2, (0.0, 1.0 / 3, -1.0 / 3, 0.5)[k % 4], 0),
    'gray_half': lambda k: (1, _bit(k, 0, 0.2, 1.8), _bit(k, 1, 1.8, 0.2), _bit(k, 2, 0.2, 1.8), _bit(k, 3, -0.2, 0.2), (k // 3) % 2),
    'jitter_off': lambda k: (int(k % 3 != 0), 1.8, 0.2, 1.8, 0.2, k % 2),
    'contrast_pin': lambda k: (1, 0.5, 1.8, 0.3, 0.2, 0),             # every predecessor of contrast moves the mean visibly
}
COLOUR_SIZES = [(15, 17), (16, 16), (16, 17), (24, 40)]                # HW = 255, 256, 272, 960: aug_color_mean short, exact, multi-pass


def all_orders_params(H, W, factor_set):
    """12 images x 2 views: record k = 2 * image + view carries permutation k."""
    p = np.zeros((12, 2, P), F32)
    for k, perm in enumerate(PERMS):
        i, v = divmod(k, 2)
        jit, br, co, sa, hu, gray = FACTOR_SETS[factor_set](k)
        p[i, v] = (0, 0, H, W, (k // 2) % 2, jit) + perm + (br, co, sa, hu, gray, 0)
    return p


@functools.lru_cache(None)
def colour_case(H, W, factor_set, kind):
    src = np.stack([palette(H, W, 200 + i, kind) for i in range(12)])
    return _case('colour %dx%d %s %s' % (H, W, factor_set, kind), 'colour', src, all_orders_params(H, W, factor_set), H, W)


def colour_cases(H, W):
    return [colour_case(H, W, fs, kind) for fs in FACTOR_SETS for kind in ('u8', 'f32')]


EXACT_SIZES = [(16, 16), (16, 32)]                                     # HW a power of two: the mean of k/64 values is dyadic


@functools.lru_cache(None)
def exact_colour_case(H, W, style):
    """float32 pixels k/64, brightness and contrast in {0.5, 1.5}, saturation 1, hue 0, all 24 orders.  'gray' (r = g = b) and 'red'
    (g = b = 0) are the pixels whose HSV round trip is exact in float32: range == 0, or hue == 0 with saturation 1.  Any other colour
    loses exactness in the hue op (float32(1/3) + 1 rounds), so there is no such sub-case; tests/test_augment_reference.py proves these."""
    rng = np.random.default_rng(300 + H + W + len(style))
    src = np.zeros((12, H, W, 3), F32)
    k = rng.integers(0, 65, (12, H, W)).astype(F32) / F32(64)
    if style == 'gray':
        src[:] = k[..., None]
    else:
        src[..., 0] = k
    p = all_orders_params(H, W, 'lo')
    for r in range(24):
        i, v = divmod(r, 2)
        p[i, v, 10:15] = (_bit(r, 0, 0.5, 1.5), _bit(r, 1, 1.5, 0.5) if r % 3 else _bit(r, 1, 0.5, 1.5), 1.0, 0.0, 0)
    return _case('exact colour %dx%d %s' % (H, W, style), 'exact', src, p, H, W)


def exact_colour_cases():
    return [exact_colour_case(H, W, s) for (H, W) in EXACT_SIZES for s in ('gray', 'red')]


RESIZE_OUT_DYADIC = [(16, 32), (32, 16)]
RESIZE_OUT_OTHER = [(24, 40), (40, 24)]
_CANVAS = (64, 320)
_RESIZE_SIZES = [(64, 320), (40, 301), (50, 60), (64, 320)]
# (image, view) -> (y, x, h, w, flip): odd crop sizes 37x53 (down), 9x7 (up: border taps dropped on most pixels), 5x300, 1x1, the whole
# image; boxes on every border of their image and interior ones
_RESIZE_BOXES = [[(0, 0, 37, 53, 0), (59, 20, 5, 300, 1)],
                 [(31, 294, 9, 7, 1), (17, 100, 1, 1, 0)],
                 [(5, 3, 37, 53, 1), (0, 53, 9, 7, 0)],
                 [(0, 0, 5, 300, 0), (0, 0, 64, 320, 1)]]


def _smooth_canvas(kind, seed, b=4):
    """Noise on a smooth wave: bicubic overshoot on both sides of [0,1] and tap-to-tap differences that make a wrong index visible."""
    rng = np.random.default_rng(seed)
    Hs, Ws = _CANVAS
    yy, xx = np.mgrid[0:Hs, 0:Ws]
    out = np.zeros((b, Hs, Ws, 3), np.uint8)
    for i in range(b):
        wave = 127 + 120 * np.sin(yy / (3.0 + i) + xx / (5.0 + 2 * i))[..., None] * np.array([1.0, 0.6, -0.8])
        out[i] = np.clip(0.6 * wave + 0.4 * rng.integers(0, 256, (Hs, Ws, 3)), 0, 255).astype(np.uint8)
    if kind == 'u8':
        return out
    return (out.astype(F32) * F32(1.0 / 255.0) + (rng.random(out.shape).astype(F32) - F32(0.5)) * F32(1.0 / 512)).clip(0, 1).astype(F32)


@functools.lru_cache(None)
def resize_case(H, W, kind):
    src = _smooth_canvas(kind, 400)
    p = np.zeros((4, 2, P), F32)
    for i in range(4):
        for v in range(2):
            p[i, v, 0:5] = _RESIZE_BOXES[i][v]
    return _case('resize ->%dx%d %s' % (H, W, kind), 'resize', src, p, H, W, sizes=_RESIZE_SIZES)


@functools.lru_cache(None)
def eval_case(H, W, kind):
    """preprocess_for_eval's central crop: the box comes from the oracle here and from data_util.center_crop_boxes on the device side."""
    src = _smooth_canvas(kind, 401)
    p = np.zeros((4, 1, P), F32)
    for i, (h, w) in enumerate(_RESIZE_SIZES):
        p[i, 0, 0:4] = oa.center_crop_box(h, w, H, W, 0.875)
    return _case('eval centre crop ->%dx%d %s' % (H, W, kind), 'resize', src, p, H, W, sizes=_RESIZE_SIZES)


@functools.lru_cache(None)
def ambiguous_case(axis, kind):
    """The rule in use: 24 x 40 from a whole-image crop of 2092 rows (output row 23 may take either index) or of 4749 columns (output
    column 34; flipped in view 1, so column 5 there).  One coordinate of H + W = 64 is 1.6 %."""
    rng = np.random.default_rng(450)
    hs, ws = (2092, 8) if axis == 'rows' else (8, 4749)
    src = rng.integers(0, 256, (1, hs, ws, 3), dtype=np.uint8)
    if kind == 'f32':
        src = rng.random((1, hs, ws, 3)).astype(F32)
    p = np.zeros((1, 2, P), F32)
    p[0, :, 2], p[0, :, 3], p[0, 1, 4] = hs, ws, 1
    return _case('resize ambiguous %s ->24x40 %s' % (axis, kind), 'resize', src, p, 24, 40)


def ambiguous_cases():
    return [ambiguous_case(axis, kind) for axis in ('rows', 'cols') for kind in ('u8', 'f32')]


def resize_cases():
    return [f(H, W, kind) for (H, W) in RESIZE_OUT_DYADIC + RESIZE_OUT_OTHER for kind in ('u8', 'f32') for f in (resize_case, eval_case)]


def pack(case):
    """A uint8 case as packed records: (bytes, table [b,3] = (offset, height, width))."""
    assert case['src'].dtype == np.uint8
    recs = [np.ascontiguousarray(im).reshape(-1) for im in _images(case)]
    offs = np.cumsum([0] + [r.size for r in recs])[:-1]
    table = np.stack([offs, case['sizes'][:, 0], case['sizes'][:, 1]], 1).astype(np.int64)
    return np.concatenate(recs), table


def clamp_box(y, x, h, w, Hs, Ws):
    """The clamp aug_crop_resize_flip_ragged documents."""
    cy, cx = min(max(y, 0), Hs - 1), min(max(x, 0), Ws - 1)
    return cy, cx, min(max(h, 1), Hs - cy), min(max(w, 1), Ws - cx)


@functools.lru_cache(None)
def clamp_case(H, W):
    """Ragged records whose crop boxes overhang their image by at most 8 rows / columns on each side, or have h = 0 / w = 0."""
    sizes = [(20, 30), (33, 21), (12, 40), (25, 25)]
    rng = np.random.default_rng(500)
    src = np.zeros((4, 40, 40, 3), np.uint8)
    for i, (h, w) in enumerate(sizes):
        src[i, :h, :w] = rng.integers(0, 200, (h, w, 3))                 # the filler around the records is 255: never a pixel value
    boxes = [[(-5, -8, 15, 20, 0), (10, 12, 18, 26, 1)],                 # negative origin; y+h > height and x+w > width
             [(30, 15, 0, 6, 0), (-3, 4, 44, 0, 1)],                     # h = 0; overhang at both ends in y, w = 0
             [(4, 36, 8, 12, 1), (11, -2, 9, 50, 0)],                    # x+w > width; y+h > height by 8, both ends in x
             [(0, 0, 25, 25, 0), (24, 24, 8, 8, 1)]]                     # a valid box beside a corner one
    p = np.zeros((4, 2, P), F32)
    ref = np.zeros((4, 2, P), F32)
    for i in range(4):
        for v in range(2):
            y, x, h, w, fl = boxes[i][v]
            p[i, v, 0:5] = (y, x, h, w, fl)
            ref[i, v, 0:5] = clamp_box(y, x, h, w, *sizes[i]) + (fl,)
            assert max(-y, -x, y + h - sizes[i][0], x + w - sizes[i][1]) <= 8
    return _case('ragged clamp ->%dx%d' % (H, W), 'resize', src, p, H, W, sizes=sizes, ref_params=ref)


STAGE_CASES = {
    'colour': lambda: [c for (H, W) in COLOUR_SIZES for c in colour_cases(H, W)],
    'resize': lambda: resize_cases() + ambiguous_cases() + [clamp_case(16, 32), clamp_case(24, 40)],
}


@functools.lru_cache(None)
def stage_e32(stage):
    """{case name: E32} of every case of the stage."""
    return {c['name']: e32(c) for c in STAGE_CASES[stage]()}


# max E32 per stage as measured by stage_e32 / blur_e32 (tests/golden/AUGMENT_STAGES.md): recorded so that a GPU test does not spend
# seconds on re-deriving them; tests/test_augment_reference.py re-measures and fails if a recorded value is not the measured one.
# Nothing here was measured on a kernel.
E32_RECORDED = {'colour': 4.607e-06, 'resize': 3.564e-07, 'blur': 1.713e-07}


def stage_tolerance(stage):
    return 4.0 * E32_RECORDED[stage]


# ---------------------------------------------------------------------------------------------------------------- blur
BLUR_SIZES = [(40, 3, 40), (3, 40, 3), (3, 40, 40), (45, 20, 45), (7, 9, 7)]     # (H, W, the `height` that sizes the filter)
BLUR_SIGMAS = {1: [(0.1,), (2.0,)], 2: [(0.1, 2.0)], 3: [(2.0, 0.1, 1.0)]}


@functools.lru_cache(None)
def blur_case(H, W, height, k, sigmas, select):
    """x [b,H,W,3k] float32 in [-0.1, 1.1]; select: 'none', 'all' or 'mixed' (per view and image)."""
    b = 3
    rng = np.random.default_rng(600 + 7 * H + W + k)
    x = (rng.random((b, H, W, 3 * k)) * 1.2 - 0.1).astype(F32)
    if select == 'mixed':
        sel = np.asarray([[(i + v) % 2 for i in range(b)] for v in range(k)], F32)
    else:
        sel = np.full((k, b), float(select == 'all'), F32)
    return dict(name='blur %dx%d height%d k%d sigma%s %s' % (H, W, height, k, '/'.join('%g' % s for s in sigmas), select), stage='blur',
                x=x, height=height, sigmas=tuple(sigmas), sel=sel)


def blur_cases(H, W, height):
    return [blur_case(H, W, height, k, sg, select) for k in (1, 2, 3) for sg in BLUR_SIGMAS[k] for select in ('none', 'all', 'mixed')]


def gaussian_filter(radius, sigma, dt):
    x = np.arange(-radius, radius + 1).astype(dt)
    f = np.exp(-(x * x) / (dt(2) * dt(sigma) * dt(sigma)))
    return (f / f.sum()).astype(dt)


def blur_emulate(case, dt=F32, mut=()):
    """blur1d twice in working type dt with the kernel's flat addressing: a tap that is not clamped reads the neighbouring row."""
    x = case['x'].astype(dt)
    b, H, W, C = x.shape
    r = int((case['height'] // 10) / 2)
    K = 2 * r + 1
    filt = np.stack([gaussian_filter(r, s, dt) for s in case['sigmas']])             # [k, K]
    n, y, xx, c = np.indices(x.shape)
    e = np.arange(x.size).reshape(x.shape)
    view = c // 3

    def one_pass(src, vert):
        flat = src.reshape(-1)
        pos, lim, step = (y, H, W * C) if vert else (xx, W, C)
        acc = np.zeros(x.shape, dt)
        for t in range(K):
            idx = e + (t - r) * step
            ok = ((idx >= 0) & (idx < x.size)) if 'blur_no_clamp' in mut else ((pos + t - r >= 0) & (pos + t - r < lim))
            acc = acc + filt[view, t] * np.where(ok, flat[np.clip(idx, 0, x.size - 1)], dt(0))
        return acc
    hb = one_pass(x, False)
    vb = one_pass(x if 'blur_vert_in' in mut else hb, True)
    out = np.clip(np.where(case['sel'][view, n] != 0, vb, x), dt(0), dt(1))
    assert out.dtype == dt
    return out


def blur_oracle(case):
    if '_ref' not in case:
        x = case['x']
        k = x.shape[3] // 3
        ref = oblur.batch_random_blur([x[..., 3 * i:3 * i + 3] for i in range(k)], case['height'], case['sigmas'], case['sel'])
        case['_ref'] = np.concatenate(ref, axis=3)
    return case['_ref']


def blur_compare(got, case, tol):
    got = np.asarray(got)
    if got.shape != case['x'].shape:
        return [entry(case['name'] + ' shape', 1.0, 0.0)]
    g = got.astype(F64)
    if not np.isfinite(g).all():
        return [entry(case['name'] + ' non-finite output', float('inf'), tol)]
    err = np.abs(g - blur_oracle(case))
    res = [entry(case['name'] + ' vs float64 oracle', err.max(), tol, numel=err.size, nbad=int((err > tol).sum()))]
    if not case['sel'].any():                                            # nothing selected: the clipped input, bit for bit
        want = np.clip(case['x'], F32(0), F32(1))
        res.append(entry(case['name'] + ' bitwise clip(input)', float((got != want).sum()), 0.0, numel=got.size))
    return res


def all_blur_cases():
    return [c for (H, W, hh) in BLUR_SIZES for c in blur_cases(H, W, hh)]


@functools.lru_cache(None)
def blur_e32():
    return {c['name']: float(np.abs(blur_emulate(c, F32).astype(F64) - blur_oracle(c)).max()) for c in all_blur_cases()}


def blur_tolerance():
    return 4.0 * E32_RECORDED['blur']
