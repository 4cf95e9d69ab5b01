"""References for solarization in the blur's last pass (blur1d<true, true> in csrc/pool.hip, simclr_batch_blur_solarize).
Pure numpy on the CPU, on top of tests/augment_reference.py's blur cases, float32 emulation and float64 oracle: shared by
tests/test_gpu_aug_recipe.py and tests/test_aug_recipe_reference.py (which pins it without a GPU).  TEST INFRASTRUCTURE ONLY.

* CASES.  A case is a blur case (x [b,H,W,3k], sigmas, sel [k,b]) plus a coin table `coin` [k,b] of 0/1 and a threshold `t`.
  The rule: after the clip, v -> 1 - v where coin[view, image] is set and v >= t.
* REFERENCE.  `oracle(case)`: the rule in float64 on `blur_oracle`.  `emulate(case)`: the rule in float32 on `blur_emulate`.
* TOLERANCE.  4 x the largest |emulate32 - oracle| over the GPU cases (`E32_RECORDED`, re-measured by the CPU test): the project's
  convention.  Nothing measured on a kernel enters it.
* THRESHOLD GUARD.  At t != 0.5 the map jumps by |1 - 2t| at v = t, so an element whose float64 pre-solarize value lies within the
  tolerance of t may legitimately land on either side.  At such an element -- on a solarized image, nowhere else -- `compare` accepts
  the distance to either branch; the share of such elements is reported and capped at 1 % of the case.  At t = 0.5 the map is
  continuous and there is no guard.  An `exact` case (dyadic pixels, nothing blurred) is compared bit for bit with no guard: these
  tell `>=` from `>`, and (at t = 0, with pixels outside [0, 1]) clip-then-solarize from solarize-then-clip.
* MUTANTS.  `mutant(case, name)`: float64 outputs of five wrong kernels the comparator has to reject.
"""
import functools

import numpy as np

from oracle import blur as oblur
from tests import augment_reference as ar

F32, F64 = np.float32, np.float64
PATTERNS = ('none', 'all', 'mixed', 'views')
THRESHOLDS = (0.5, 0.25, 0.75)
SELECTS = ('none', 'all', 'mixed')
MUTANTS = ('gt', 'before_clip', 'before_blur', 'coin_transposed', 'coin_view_a')
GUARD_CAP = 0.01

# max |float32 emulation - float64 oracle| over all_cases(), elements on which the two take different branches left out (they lie within
# the blur's own E32 of the threshold): measured by measured_e32(), written down in tests/golden/AUG_RECIPE.md, re-measured by
# tests/test_aug_recipe_reference.py.  Nothing here was measured on a kernel.
E32_RECORDED = 1.713e-07


def tolerance():
    return 4.0 * E32_RECORDED


def coin_table(k, b, pattern):
    """[k, b] of 0/1.  'mixed': per (view, image), crossing the blur's own 'mixed' selector ((i + v) % 2) so that blurred and unblurred
    images occur with and without solarization; 'views': rows that differ between the views (and from their transpose)."""
    if pattern == 'none':
        return np.zeros((k, b), F32)
    if pattern == 'all':
        return np.ones((k, b), F32)
    if pattern == 'mixed':
        return np.asarray([[(i + 1) % 2 for i in range(b)] for v in range(k)], F32)
    assert pattern == 'views'
    base = [1.0] * (b - 1) + [0.0]
    return np.asarray([np.roll(base, v) for v in range(k)], F32)


@functools.lru_cache(None)
def case(H, W, height, k, sigmas, select, pattern, t):
    base = ar.blur_case(H, W, height, k, sigmas, select)
    return dict(name='%s solarize %s t%g' % (base['name'], pattern, t), blur=base, coin=coin_table(k, base['x'].shape[0], pattern),
                t=float(t), exact=False)


def cases(H, W, height):
    """One of augment_reference.BLUR_SIZES: views 1, 2, 3 (sigma sets as the blur's), selectors none / all / mixed, the four coin
    patterns, the three thresholds."""
    return [case(H, W, height, k, sg, select, pattern, t) for k in (1, 2, 3) for sg in ar.BLUR_SIGMAS[k] for select in SELECTS
            for pattern in PATTERNS for t in THRESHOLDS]


def all_cases():
    return [c for (H, W, hh) in ar.BLUR_SIZES for c in cases(H, W, hh)]


@functools.lru_cache(None)
def dyadic_case(H=7, W=9, k=2, t=0.25, lo=0, hi=64):
    """Pixels j/64 (j = lo .. hi, every value present, 64 t among them), nothing blurred (K = 1 filter, zero selectors), mixed
    coins: the clip and 1 - v are exact, the expected table is bitwise and holds elements equal to the threshold, which must invert.
    lo < 0 < 64 < hi with t = 0: pixels the clip moves.  Clip-then-solarize and solarize-then-clip differ only there: for t > 0 both
    send u < 0 to 0 and u > 1 to 0, at t = 0 the clipped 0 inverts to 1 while the unclipped u < 0 does not."""
    b = 3
    rng = np.random.default_rng(700 + H + W + k)
    j = rng.integers(lo, hi + 1, (b, H, W, 3 * k))
    j.reshape(-1)[:hi - lo + 1] = np.arange(lo, hi + 1)
    j[..., 0] = np.where(np.arange(W)[None, None, :] % 3 == 0, int(round(64 * t)), j[..., 0])   # a stripe AT the threshold in every image of view a
    x = (j.astype(F32) / F32(64)).astype(F32)
    base = dict(name='dyadic %dx%d k%d [%d,%d]/64' % (H, W, k, lo, hi), stage='blur', x=x, height=10, sigmas=(1.0,) * k, sel=np.zeros((k, b), F32))
    return dict(name=base['name'] + ' solarize mixed t%g' % t, blur=base, coin=coin_table(k, b, 'mixed'), t=float(t), exact=True)


def exact_cases():
    return [dyadic_case(), dyadic_case(t=0.0, lo=-4, hi=68)]


def _coin_mask(c, coin=None):
    """coin[view, image] broadcast to [b,H,W,3k]."""
    x = c['blur']['x']
    coin = c['coin'] if coin is None else coin
    n, _, _, ch = np.indices(x.shape)
    return coin[ch // 3, n] != 0


def solarize(v, mask, t, dt, strict=False):
    """The rule in working type dt."""
    v = v.astype(dt)
    hit = mask & ((v > dt(t)) if strict else (v >= dt(t)))
    out = np.where(hit, dt(1) - v, v)
    assert out.dtype == dt
    return out


def oracle(c):
    if '_ref' not in c:
        c['_ref'] = solarize(ar.blur_oracle(c['blur']), _coin_mask(c), c['t'], F64)
    return c['_ref']


def emulate(c, dt=F32):
    return solarize(ar.blur_emulate(c['blur'], dt), _coin_mask(c), c['t'], dt)


def _unclipped(c, x=None):
    """The blur of the case before its clip, float64 (oracle/blur.py's own steps)."""
    base = c['blur']
    x = base['x'].astype(F64) if x is None else x
    out = np.zeros_like(x)
    for v, (sigma, sel) in enumerate(zip(base['sigmas'], base['sel'])):
        img = x[..., 3 * v:3 * v + 3]
        s = np.asarray(sel, F64).reshape(-1, 1, 1, 1)
        out[..., 3 * v:3 * v + 3] = oblur.gaussian_blur(img, base['height'] // 10, sigma) * s + img * (1 - s)
    return out


def mutant(c, name):
    """float64 output of a wrong kernel."""
    mask, t = _coin_mask(c), c['t']
    pre = ar.blur_oracle(c['blur'])
    k, b = c['coin'].shape
    if name == 'gt':                                   # > instead of >=
        return solarize(pre, mask, t, F64, strict=True)
    if name == 'before_clip':                          # solarize, then clip
        return np.clip(solarize(_unclipped(c), mask, t, F64), 0.0, 1.0)
    if name == 'before_blur':                          # solarize the input, then blur and clip
        return np.clip(_unclipped(c, solarize(c['blur']['x'], mask, t, F64)), 0.0, 1.0)
    if name == 'coin_transposed':                      # the table read as [b, nviews]: element n * nviews + view
        flat = c['coin'].reshape(-1)
        wrong = np.asarray([[flat[n * k + v] for n in range(b)] for v in range(k)], F32)
        return solarize(pre, _coin_mask(c, wrong), t, F64)
    assert name == 'coin_view_a'                       # view a's coin applied to every view
    return solarize(pre, _coin_mask(c, np.repeat(c['coin'][:1], k, 0)), t, F64)


def guard(c, tol):
    """The elements compare() may judge against either branch: on a solarized image, float64 pre-solarize value within tol of t != 0.5."""
    if c['t'] == 0.5 or c['exact']:
        return np.zeros(c['blur']['x'].shape, bool)
    return _coin_mask(c) & (np.abs(ar.blur_oracle(c['blur']) - c['t']) <= tol)


def guard_share(c, tol):
    return float(guard(c, tol).mean())


def error_map(got, c, tol):
    got = np.asarray(got, F64)
    err = np.abs(got - oracle(c))
    g = guard(c, tol)
    if g.any():
        pre = ar.blur_oracle(c['blur'])
        other = np.where(pre >= c['t'], pre, 1.0 - pre)              # the branch the oracle did not take
        err = np.where(g, np.minimum(err, np.abs(got - other)), err)
    return err


def compare(got, c, tol):
    """Every element of got against the float64 oracle; result dicts {name, err, tol, ok, ...} as augment_reference's."""
    name = c['name']
    got = np.asarray(got)
    if got.shape != c['blur']['x'].shape:
        return [ar.entry(name + ' shape', 1.0, 0.0)]
    g = got.astype(F64)
    if not np.isfinite(g).all():
        return [ar.entry(name + ' non-finite output', float('inf'), tol)]
    if c['exact']:
        want = expected_exact(c)
        return [ar.entry(name + ' bitwise the expected table', float((got != want).sum()), 0.0, numel=got.size)]
    err = error_map(g, c, tol)
    return [ar.entry(name + ' vs float64 oracle', err.max(), tol, numel=err.size, nbad=int((err > tol).sum())),
            ar.entry(name + ' guarded share', guard_share(c, tol), GUARD_CAP),
            ar.entry(name + ' range [0,1]', max(-g.min(), g.max() - 1.0, 0.0), 0.0)]


def expected_exact(c):
    """The table of an exact case: clip, then the rule, in float32 -- every step exact on its pixels (asserted by the CPU test)."""
    x = np.clip(c['blur']['x'], F32(0), F32(1))
    return solarize(x, _coin_mask(c), c['t'], F32)


def e32(c):
    """max |emulate32 - oracle| of a case, elements on which float32 and float64 take different branches left out."""
    pre32 = ar.blur_emulate(c['blur'], F32)
    pre64 = ar.blur_oracle(c['blur'])
    same = (pre32 >= F32(c['t'])) == (pre64 >= c['t'])
    err = np.abs(emulate(c, F32).astype(F64) - oracle(c))
    keep = same | ~_coin_mask(c) | (c['t'] == 0.5)
    return float(err[keep].max()), int((~keep).sum())


@functools.lru_cache(None)
def measured_e32():
    """{case name: (E32, elements left out)} over all_cases()."""
    return {c['name']: e32(c) for c in all_cases()}
