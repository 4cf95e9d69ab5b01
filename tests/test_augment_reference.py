"""CPU tests that go with tests/test_gpu_augment.py: the case builders, the float32 emulation, the exactness claims and the comparator
of tests/augment_reference.py, pinned without a GPU.  The comparator has to accept the float32 emulation of the oracle on every case
at the tolerance derived from it, and to reject every listed mutant of that emulation on at least one case."""
import numpy as np
import pytest

from oracle import augment as oa
from tests import augment_reference as R

F32, F64 = np.float32, np.float64


def _ok(results):
    return all(r['ok'] for r in results)


# ---------------------------------------------------------------------------------------------------------------- restatements
@pytest.mark.parametrize('out_size,in_size', [(16, 37), (32, 53), (16, 9), (32, 7), (16, 5), (32, 300), (16, 1), (24, 37), (40, 300)])
def test_taps_restate_the_oracle(out_size, in_size):
    idx, wts = R.taps(out_size, in_size, F64)
    oidx, owts = oa.bicubic_taps(out_size, in_size)
    assert np.array_equal(idx, oidx) and np.array_equal(wts, owts)


def test_float64_emulation_is_the_oracle():
    """The alternative-index references come from emulate(.., float64): it must be the oracle to float64 rounding."""
    for case in (R.colour_case(15, 17, 'mixed', 'u8'), R.colour_case(16, 17, 'gray_half', 'f32'), R.resize_case(24, 40, 'u8'),
                 R.eval_case(16, 32, 'f32'), R.clamp_case(16, 32)):
        assert np.abs(R.emulate(case, F64) - R.oracle(case)).max() < 1e-12, case['name']


def test_blur_emulation_in_float64_is_the_oracle():
    for case in R.blur_cases(40, 3, 40) + R.blur_cases(3, 40, 40) + R.blur_cases(7, 9, 7):
        assert np.abs(R.blur_emulate(case, F64) - R.blur_oracle(case)).max() < 1e-14, case['name']


# ---------------------------------------------------------------------------------------------------------------- exactness claims
@pytest.mark.parametrize('H,W', R.IDENTITY_SIZES)
def test_identity_crop_weights_are_exactly_0100(H, W):
    for n in (H, W):
        for dt in (F32, F64):
            idx, wts = R.taps(n, n, dt)
            assert np.array_equal(wts, np.tile(np.asarray([0, 1, 0, 0], dt), (n, 1)))
            assert np.array_equal(idx[:, 1], np.arange(n))
        assert R.ambiguous_coords(n, n) == []
    for kind in ('u8', 'f32'):
        for views in (1, 2, 3):
            case = R.identity_case(H, W, views, kind)
            want = R.identity_expected(case)
            assert np.array_equal(R.emulate(case, F32), want)
            flips = case['params'][:, :, 4]
            assert views == 1 or all(0 < flips[i].sum() < views for i in range(flips.shape[0]))    # mixed inside every image


def test_identity_sources_sit_on_the_colour_branches():
    for kind in ('u8', 'f32'):
        px = R.to_float(R.palette(15, 17, 3, kind), F32).reshape(-1, 3)
        h, s, v = R.rgb_to_hsv(px, F32)
        r, g, b = px.T
        assert ((v == 0).any() and ((v > 0) & (s == 0)).any() and (s == 1).any())
        assert ((r == v) & (g == v) & (b < v)).any() and ((g == v) & (b == v) & (r < v)).any() and ((r == v) & (b == v) & (g < v)).any()
        for first in ((r == v) & (g < v) & (b < v), (g == v) & (r < v) & (b < v), (b == v) & (r < v) & (g < v)):
            assert first.any()
        hneg = R.rgb_to_hsv(px, F32, mut=('no_wrap',))[0]
        assert (hneg < -0.01).any()
        if kind == 'f32':
            assert (h == 1.0).any() and ((hneg < 0) & (hneg > -1e-7)).any()      # a tiny negative hue wraps to exactly 1.0f: dh == 6


def test_dyadic_outputs_have_no_ambiguous_coordinate():
    for out in (16, 32):
        for n in range(1, 520):
            assert R.ambiguous_coords(out, n) == [], (out, n)
    for case in R.resize_cases() + [R.clamp_case(16, 32)]:
        if case['H'] in (16, 32) and case['W'] in (16, 32):
            assert R.ambiguity(case) == {}, case['name']


def test_ambiguous_share_of_the_chosen_cases():
    """Condition, not measurement: at most 2 % of H + W rows and columns of any record may take either index."""
    for case in R.STAGE_CASES['resize']():
        assert R.ambiguous_share(case) <= 0.02, (case['name'], R.ambiguity(case))


def test_exact_colour_sub_cases_are_exact():
    for case in R.exact_colour_cases():
        e = R.emulate(case, F32)
        assert np.array_equal(e.astype(F64), R.oracle(case)), case['name']
        # and they are no fixed point: brightness and contrast move most pixels, the clip is reached on both sides
        src = R.identity_expected(case)
        assert (e != src)[src != 0].mean() > 0.5 and (e == 0).any() and (e == 1).any()
        # one pixel dropped from the mean is a bitwise difference
        assert not np.array_equal(R.emulate(case, F32, mut=('mean_hw1',)), e)


def test_a_general_colour_has_no_exact_sub_case():
    """Why the exact sub-cases are gray and red only: a green pixel on the lattice already differs after the hue op with delta 0."""
    case = R.exact_colour_case(16, 16, 'red')
    green = dict(case, src=np.ascontiguousarray(case['src'][..., [1, 0, 2]]), name='green')
    for k in ('_ref', '_amb', '_alt'):
        green.pop(k, None)
    assert not np.array_equal(R.emulate(green, F32).astype(F64), R.oracle(green))


def test_contrast_mean_depends_on_every_predecessor_set():
    """contrast_pin: the contrast mean of a record differs by far more than the tolerance between any two sets of ops before contrast."""
    case = R.colour_case(16, 16, 'contrast_pin', 'f32')
    img = R.to_float(case['src'][0], F64)
    means = {}
    for perm in R.PERMS:
        pre = frozenset(perm[:perm.index(1)])
        p = case['params'][0, 0].astype(F64)
        x = img
        for op in perm[:perm.index(1)]:
            x = oa.color_jitter_given(x, [op], p[10], p[11], p[12], p[13])
        means.setdefault(pre, []).append(x.mean((0, 1)))
    assert len(means) == 8
    reps = [np.mean(v, 0) for v in means.values()]
    gaps = [np.abs(a - b).max() for i, a in enumerate(reps) for b in reps[i + 1:]]
    assert min(gaps) > 100 * R.stage_tolerance('colour') / 0.8


# ---------------------------------------------------------------------------------------------------------------- tolerances
def test_tolerances_come_from_the_float32_emulation():
    """The recorded E32 of a stage is the largest |float32 emulation - float64 oracle| over that stage's cases, re-measured here."""
    measured = {'colour': max(R.stage_e32('colour').values()), 'resize': max(R.stage_e32('resize').values()),
                'blur': max(R.blur_e32().values())}
    for stage in ('colour', 'resize'):
        for name, e in sorted(R.stage_e32(stage).items()):
            print('  E32 %-50s %.3e' % (name, e))
    for stage, e in measured.items():
        print('E32 %-7s measured %.4e recorded %.4e tolerance %.4e' % (stage, e, R.E32_RECORDED[stage], 4 * R.E32_RECORDED[stage]))
    # colour and resize are IEEE arithmetic only: the same on every machine.  The blur's filter goes through exp: 10 % for another libm.
    assert abs(measured['colour'] / R.E32_RECORDED['colour'] - 1) < 1e-3
    assert abs(measured['resize'] / R.E32_RECORDED['resize'] - 1) < 1e-3
    assert abs(measured['blur'] / R.E32_RECORDED['blur'] - 1) < 0.1
    assert R.stage_tolerance('colour') == 4 * R.E32_RECORDED['colour'] and R.blur_tolerance() == 4 * R.E32_RECORDED['blur']


# ---------------------------------------------------------------------------------------------------------------- the comparator
def _all_augment_cases():
    ident = [R.identity_case(H, W, views, kind) for (H, W) in R.IDENTITY_SIZES for views in (1, 2, 3) for kind in ('u8', 'f32')]
    return ident + R.STAGE_CASES['colour']() + R.STAGE_CASES['resize']() + R.exact_colour_cases()


def _tol(case):
    return {'identity': 0.0, 'exact': 0.0, 'colour': R.stage_tolerance('colour'), 'resize': R.stage_tolerance('resize')}[case['stage']]


def _verdict(case, out):
    """What the GPU test would conclude from `out`: identity and exact cases are bitwise, the others go through compare."""
    if case['stage'] == 'identity':
        return np.array_equal(out, R.identity_expected(case))
    if case['stage'] == 'exact':
        return np.array_equal(np.asarray(out, F64), R.oracle(case))
    return _ok(R.compare(out, case, _tol(case)))


def test_comparator_accepts_the_float32_emulation_on_every_case():
    for case in _all_augment_cases():
        assert _verdict(case, R.emulate(case, F32)), case['name']
    for case in R.all_blur_cases():
        assert _ok(R.blur_compare(R.blur_emulate(case, F32), case, R.blur_tolerance())), case['name']


def test_comparator_accepts_either_index_only_at_ambiguous_coordinates():
    """The cases with an ambiguous row / column: the contracted evaluation passes, the same values at another column do not."""
    assert R.ambiguous_coords(24, 2092) == [23] and R.ambiguous_coords(40, 4749) == [34]
    tol = R.stage_tolerance('resize')
    for kind in ('u8', 'f32'):
        case = R.ambiguous_case('rows', kind)
        assert R.ambiguity(case) == {(0, 0): ([23], []), (0, 1): ([23], [])} and R.ambiguous_share(case) <= 0.02
        plain, other = R.emulate(case, F32), R.emulate(case, F32, alt_r=True)
        assert np.abs(plain.astype(F64) - other)[:, 23].max() > 10 * tol and np.array_equal(plain[:, :23], other[:, :23])
        assert _ok(R.compare(plain, case, tol)) and _ok(R.compare(other, case, tol))
        case = R.ambiguous_case('cols', kind)
        assert R.ambiguity(case) == {(0, 0): ([], [34]), (0, 1): ([], [5])} and R.ambiguous_share(case) <= 0.02
        plain, other = R.emulate(case, F32), R.emulate(case, F32, alt_c=True)
        assert np.abs(plain.astype(F64) - other).max() > 10 * tol                      # the two indices are far apart ...
        assert _ok(R.compare(plain, case, tol)) and _ok(R.compare(other, case, tol))   # ... and both are accepted there,
        moved = plain.copy()
        moved[0, :, 20, 0:3] = other[0, :, 34, 0:3]
        assert not _ok(R.compare(moved, case, tol))                                    # but nowhere else:
        mixed = plain.copy()
        mixed[0, :, 5, 0:3] = other[0, :, 5, 3:6]                                      # view 0 has its ambiguous column at 34, not at 5
        assert not _ok(R.compare(mixed, case, tol))


@pytest.mark.parametrize('mutant', R.MUTANTS_AUGMENT)
def test_comparator_rejects_mutant(mutant):
    stages = ('identity', 'resize') if mutant in ('flip_hw', 'out_hw', 'view_offset', 'keep_oob_tap', 'index_off1') else ('colour', 'exact')
    cases = [case for case in _all_augment_cases() if case['stage'] in stages]
    caught = [case['name'] for case in cases if not _verdict(case, R.emulate(case, F32, mut=(mutant,)))]
    print('%s: caught by %d cases, e.g. %s' % (mutant, len(caught), caught[:3]))
    assert caught, 'no case catches mutant ' + mutant


@pytest.mark.parametrize('mutant', R.MUTANTS_BLUR)
def test_blur_comparator_rejects_mutant(mutant):
    caught = [case['name'] for case in R.all_blur_cases()
              if not _ok(R.blur_compare(R.blur_emulate(case, F32, mut=(mutant,)), case, R.blur_tolerance()))]
    print('%s: caught by %d cases, e.g. %s' % (mutant, len(caught), caught[:3]))
    assert caught, 'no case catches mutant ' + mutant


def test_each_stage_catches_its_own_mutants():
    """Not only somewhere: the shape and view mutants at the non-square identity sizes, the colour mutants in the colour stage at every
    HW, the resize mutants in the resize stage."""
    for (H, W) in ((15, 17), (17, 15), (16, 32)):
        case = R.identity_case(H, W, 2, 'u8')
        for m in ('flip_hw', 'out_hw', 'view_offset', 'index_off1'):
            assert not _verdict(case, R.emulate(case, F32, mut=(m,))), (m, case['name'])
    for (H, W) in R.COLOUR_SIZES:
        for m in ('mean_raw', 'mean_hw1', 'order_rev', 'no_clip', 'gray_weights', 'no_wrap', 'no_sat_clip'):
            assert any(not _verdict(c, R.emulate(c, F32, mut=(m,))) for c in R.colour_cases(H, W)), (m, H, W)
        assert any(not _verdict(c, R.emulate(c, F32, mut=('no_cat_clamp',))) for c in R.colour_cases(H, W) if c['src'].dtype == F32)
    for (H, W) in R.RESIZE_OUT_DYADIC + R.RESIZE_OUT_OTHER:
        for kind in ('u8', 'f32'):
            case = R.resize_case(H, W, kind)
            for m in ('keep_oob_tap', 'index_off1', 'flip_hw', 'out_hw', 'view_offset'):
                assert not _verdict(case, R.emulate(case, F32, mut=(m,))), (m, case['name'])


def test_clamp_case_overhangs_stay_small_and_clamped_boxes_fit():
    for case in (R.clamp_case(16, 32), R.clamp_case(24, 40)):
        assert not np.array_equal(case['params'], case['ref_params'])
        for i, (h, w) in enumerate(case['sizes']):
            for v in range(2):
                y, x, ch, cw = case['ref_params'][i, v, 0:4].astype(int)
                assert 0 <= y and 0 <= x and ch >= 1 and cw >= 1 and y + ch <= h and x + cw <= w
        packed, table = R.pack(case)
        assert packed.size == int((3 * case['sizes'][:, 0] * case['sizes'][:, 1]).sum()) and packed.max() < 255
