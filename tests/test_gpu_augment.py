"""GPU parity tests (pytest -m gpu) of the augmentation kernels (csrc/augment.hip: crop + bicubic resize + flip, the contrast mean, the
jitter chain, grayscale; canvas and ragged front ends) and of the blur (blur1d in csrc/pool.hip), one stage at a time.  A stage is isolated
through the public parameter table alone: an identity crop hands the colour stage the source pixels bit for bit, jitter_on = 0 leaves the
resize alone.  Every element is compared with the float64 oracle (oracle/augment.py, oracle/blur.py); no quantile.  Tolerances are not
chosen: identity crops and the dyadic colour sub-cases are bitwise, every other stage gets 4 x the error of the float32 emulation of the
oracle on that stage's cases, measured on the CPU (tests/augment_reference.py; values in tests/golden/AUGMENT_STAGES.md).  Outputs land in
guarded buffers.  tests/test_augment_reference.py pins cases, emulation and comparator without a GPU and shows that the comparator
rejects fourteen mutants (H / W swaps, view offset, contrast mean, order, clips, hue wrap, tap handling, blur clamps)."""
import pytest

from tests import augment_reference as R

pytestmark = pytest.mark.gpu


def _assert(results):
    for r in results:
        print('%-4s %-96s err=%.3e tol=%.3e' % ('ok' if r['ok'] else 'FAIL', r['name'], r['err'], r['tol']))
    bad = [r for r in results if not r['ok']]
    assert not bad, '\n'.join('%s err=%.3e tol=%.3e' % (r['name'], r['err'], r['tol']) for r in bad)


@pytest.mark.parametrize('views', [1, 2, 3])
@pytest.mark.parametrize('H,W', R.IDENTITY_SIZES)
def test_identity_crop_and_flip_are_bitwise(H, W, views):
    """15x17, 16x16, 17x15, 16x32: the source (uint8: float32(u8) * float32(1/255)), mirrored where flip = 1, at channel offset 3v of
    [b,H,W,3*views]; flipped and unflipped views inside one image.  Canvas (both source types) and ragged front end."""
    from tests import gpu_checks as gc
    _assert(gc.check_augment_identity(H, W, views))


@pytest.mark.parametrize('H,W', R.COLOUR_SIZES)
def test_colour_stage_all_orders_and_factor_sets(H, W):
    """HW = 255, 256, 272, 960 (aug_color_mean: a short, an exact and several 256-thread passes).  12 images x 2 views carry the 24 jitter
    orders once each, at the factor sets of augment_reference.FACTOR_SETS: the extremes of strength 1, saturation 0 and 5 (clipped), hue
    0 / +-1/3 / 0.5, grayscale on half of the records, jitter off with and without grayscale, and contrast_pin (the mean moves with every
    predecessor of contrast); palette pixels on every branch of rgb_to_hsv / hsv_to_rgb."""
    from tests import gpu_checks as gc
    _assert(gc.check_augment_colour(H, W))


def test_colour_exact_sub_cases_are_bitwise():
    from tests import gpu_checks as gc
    _assert(gc.check_augment_exact_colour())


@pytest.mark.parametrize('kind', ['u8', 'f32'])
@pytest.mark.parametrize('H,W', R.RESIZE_OUT_DYADIC + R.RESIZE_OUT_OTHER)
def test_resize_stage(H, W, kind):
    """Crops 37x53, 9x7, 5x300, 1x1 and a whole 64x320 image to 16x32 / 32x16 (no ambiguous coordinate) and 24x40 / 40x24; boxes on every
    border and interior, per-image sizes below the canvas, flips; the eval centre crop; at 24x40 also the two crops that do have an
    ambiguous row / column."""
    from tests import gpu_checks as gc
    _assert(gc.check_augment_resize(H, W, kind))


@pytest.mark.parametrize('H,W', R.RESIZE_OUT_DYADIC + R.RESIZE_OUT_OTHER)
def test_ragged_front_end_matches_oracle_and_canvas(H, W):
    """The uint8 resize and eval cases from packed records: against the oracle, bitwise the canvas path (torch.equal of
    two_view_batch_ragged and two_view_batch), and the colour stage (24 orders) behind the ragged front end."""
    from tests import gpu_checks as gc
    _assert(gc.check_augment_ragged(H, W))


@pytest.mark.parametrize('H,W', [(16, 32), (24, 40)])
def test_ragged_clamps(H, W):
    """Crop boxes with a negative origin, y+h > height, x+w > width, h = 0 or w = 0 equal the oracle on the clamped box; a device table
    whose record overruns the packed bytes gives zeros for that image only.  The records sit between 64 KiB of filler."""
    from tests import gpu_checks as gc
    _assert(gc.check_augment_ragged_clamps(H, W))


@pytest.mark.parametrize('H,W,height', R.BLUR_SIZES)
def test_blur_cases(H, W, height):
    """40x3 and 3x40 with the 5-tap filter of height 40 (wider than the short side: both ends of the filter are cut at one pixel), 3x40 and
    7x9 with their own 1-tap filter, 45x20; views 1, 2, 3; selectors none (bitwise the clipped input), all, mixed."""
    from tests import gpu_checks as gc
    _assert(gc.check_blur_cases(H, W, height))
