"""GPU parity tests (pytest -m gpu) of the stem chain and the Gram chain on exact integer lattices, the sibling of
tests/test_gpu_conv_lattice.py (which holds the K-extended and the sparse data-gradient rows): every output is compared with a float64
reference at tolerance ZERO, with no element exempted, and lives in a guarded buffer (gpu_checks._guarded) whose guard bands are checked.

`stem` rows (stem_gram_reference.STEM_CASES, gpu_checks.check_stem_lattice): simclr_pack_views / simclr_pack_views_ps (the packed tensor with
its zero ring and zero 4th channel, the bf16 hi / lo split), simclr_prep_weights mode 2, simclr_stem_conv_fwd with BOTH rows of the
statistics at simclr_stem_stats_slots + 5 (spare slots stay zero), 1 and 3 slots, the weight gradient through simclr_conv2d_wgrad with
pixpitch = 4 + simclr_unpack_stem_dw and through simclr_presplit_packed + simclr_stem_wgrad_ps, each with accumulate 0 and 1.  7x7 stride 2,
3x3 stride 1 and 2; output rows 1, 127 / 128 / 129, 257; maps 9x17, 17x9, 1x15, 15x1, 10x7; Cout 32 ... 192, fp32 4 and 68 (forward runs,
the weight gradient is refused: asserted); pre-split OW 1 / 31 / 32 / 33 / 65, one and several chunks per split, ring depth 2 and 3.  The
persistent-loop tail (more than 2048 M-tiles) needs 306 456 rows and stays with the Gaussian test of tests/test_gpu_kernels.py.

`gram` rows (GRAM_CASES, GEMM_CASES): simclr_conv2d_gram on a workspace of exactly simclr_conv2d_gram_workspace_bytes, simclr_small_gemm_nt_f32
and simclr_bn_sums_from_gram (cs32 and cs64 entry), K = 64 / 128 (fp32 exact, six bf16 terms) and 64 / 128 / 256 (bf16), M = 1 and around
the reduction chunk the library plans (br - 1, br, br + 1, 3 br + 1), one row per kernel shape with several chunks per split and an
uneven last split; the helper GEMM alone in both tile branches with M, N that are no multiples of the tile."""
import pytest

from tests.stem_gram_reference import GEMM_CASES, GRAM_CASES, STEM_CASES

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _exact_f32_matmul():
    from simclr_amd import ops
    ops.set_f32_matmul('exact')
    yield
    ops.set_f32_matmul('exact')


def _assert(results):
    bad = [r for r in results if not r['ok']]
    for r in bad:
        print('FAIL %-90s err=%.3e nbad=%d of %d' % (r['name'], r['err'], r.get('nbad', 0), r.get('numel', 0)))
    assert not bad, '\n'.join('%s err=%.3e tol=%.3e' % (r['name'], r['err'], r['tol']) for r in bad)


@pytest.mark.parametrize('case', STEM_CASES, ids=lambda c: c.id)
def test_stem_lattice_bitwise(case):
    from tests import gpu_checks as gc
    _assert(gc.check_stem_lattice(case))


@pytest.mark.parametrize('case', GRAM_CASES, ids=lambda c: c.id)
def test_gram_lattice_bitwise(case):
    from tests import gpu_checks as gc
    _assert(gc.check_gram_lattice(case))


@pytest.mark.parametrize('case', GEMM_CASES, ids=lambda c: c.id)
def test_small_gemm_lattice_bitwise(case):
    from tests import gpu_checks as gc
    _assert(gc.check_small_gemm_lattice(case))
