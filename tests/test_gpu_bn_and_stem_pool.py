"""GPU parity tests (pytest -m gpu) of the BatchNorm kernels (csrc/bn.hip) and the stem BN+ReLU+max-pool family (csrc/pool.hip) on exact
lattices: inputs on which every intermediate of the kernels' fp32 arithmetic is exactly representable (tests/bn_pool_reference.py), so that
each kernel, called through the C ABI, is compared with a float64 reference of the same operation at tolerance ZERO -- one dropped row,
one wrong tap or one chunk read from the neighbouring channel is a non-zero error however large the tensor.  Every check first asserts on
the CPU that the float32 evaluation of its reference equals the float64 one.  The only non-zero tolerance is simclr_bn_finalize's against
float64 (division and square root): ulp bounds derived from its rounding steps in bn_pool_reference.bn_finalize_ref.  The check bodies
live in tests/gpu_checks.py; tests/test_bn_pool_reference.py pins the references without a GPU."""
import pytest
import torch

from tests.bn_pool_reference import stream_rows

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
DTYPES = [F32, BF]


@pytest.fixture(autouse=True)
def _exact_f32_matmul():
    """simclr_set_f32_matmul is process-wide: every test starts (and leaves) the library in the exact fp32 mode."""
    from simclr_amd import ops
    from simclr_amd.flags import FLAGS
    ops.set_f32_matmul('exact')
    yield
    FLAGS.update(f32_matmul='exact')
    ops.set_f32_matmul('exact')


def _assert(results):
    for r in results:
        print('%-4s %-78s err=%.3e tol=%.3e' % ('ok' if r['ok'] else 'FAIL', r['name'], r['err'], r['tol']))
    bad = [r for r in results if not r['ok']]
    assert not bad, '\n'.join('%s err=%.3e tol=%.3e' % (r['name'], r['err'], r['tol']) for r in bad)


# ---------------------------------------------------------------------------------------------------------------- streaming kernels
# 16-byte chunks per row C/EPC = 1, 6, 12, 24 (fp32 96: the pre-split output without the two-chunk form), 48, 256 (the last width with two
# chunks per thread), 512, and 1536 / 768 (bn_bwd_reduce walks its columns in several passes of 256); rows: stream_rows
STREAM_C = {F32: [4, 24, 48, 96, 192, 1024, 2048, 6144], BF: [8, 48, 96, 384, 2048, 4096, 6144]}
STREAM_CASES = [(rows, C, dt) for dt in DTYPES for C in STREAM_C[dt] for rows in stream_rows(C, dt)]


@pytest.mark.parametrize('rows,C,dtype', STREAM_CASES)
def test_bn_apply_and_backward_bitwise_on_lattice(rows, C, dtype):
    """bn_apply (ReLU on / off; no / plain / BatchNorm'd residual; relu_bits), bn_bwd_reduce and bn_bwd_apply (mask modes 0, 1, 2; dmasked
    written and NULL; the pre-split output at fp32 C = 96, 192, 1024), every output in a guarded buffer."""
    from tests import gpu_checks as gc
    _assert(gc.check_bn_stream_lattice(rows, C, dtype))


@pytest.mark.parametrize('rows,C,dtype', [(515, 192, F32), (515, 384, BF), (37, 2048, F32)])
def test_bn_bwd_reduce_with_fewer_and_more_slots_than_workgroups(rows, C, dtype):
    """nslot in {1, 3, grid - 1}: the atomics branch; {grid, grid + 5}: one store per slot, the five spare slots stay zero.  The third case
    has two column passes per workgroup."""
    from tests import gpu_checks as gc
    _assert(gc.check_bn_bwd_reduce_slot_counts(rows, C, dtype))


# ---------------------------------------------------------------------------------------------------------------- slots and finalize
@pytest.mark.parametrize('C', [8, 40, 64, 2048])
@pytest.mark.parametrize('nslot', [1, 31, 32, 33, 127, 128, 129, 160, 768])
def test_slot_reduction_and_finalize_kernels(nslot, C):
    """32 slot lanes, four slots per lane and trip of the unrolled walk: 1 .. 33 leave the unrolled loop out, 127 / 128 / 129 sit around its
    first full trip, 160 = one trip and one more slot per lane, 768 = six trips; C = 40 half-fills the second 32-channel workgroup."""
    from tests import gpu_checks as gc
    _assert(gc.check_bn_slot_kernels(nslot, C))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('K,N', [(5, 40), (5, 300), (64, 40), (64, 300)])
def test_bn_fold_helpers_bitwise_on_lattice(K, N, dtype):
    from tests import gpu_checks as gc
    _assert(gc.check_bn_fold_lattice(K, N, dtype))


# ---------------------------------------------------------------------------------------------------------------- stem pool family
STEM_SHAPES = [(2, 6, 10, 64), (3, 7, 5, 128), (1, 9, 16, 192), (2, 1, 1, 64), (1, 2, 3, 256), (2, 15, 15, 64)]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('V,H,W,C', STEM_SHAPES)
def test_stem_pool_family_bitwise_on_lattice(V, H, W, C, dtype):
    """3 x 3 stride 2 on non-square maps of both parities, a one-pixel map and every stem width: pooled value, the tap id of every window,
    the whole max-pool backward, the fused reduce / apply (pre-split where fp32), the un-fused sequence, want_arg=False.  C = 192:
    bn_bwd_reduce_pool refuses (256 is no multiple of its chunks per row) without launching; apply and the un-fused path still match."""
    from tests import gpu_checks as gc
    _assert(gc.check_stem_pool_lattice(V, H, W, C, dtype))


# (2, 9, 9, 1024) with 5 x 5 stride 3: 18 pooled pixels < 21 workgroups -- the one way into bn_bwd_reduce_pool<float>, which 3 x 3 stride 2
# never reaches (tests/test_bn_pool_reference.py::test_fp32_stem_reduce_always_walks_the_pooled_pixels); (3, 1) at C = 192: the division
# by a chunk count that is no power of two in bn_bwd_apply_pool<float>
GENERIC_WINDOWS = [(2, 7, 9, 64, 2, 2), (2, 7, 9, 64, 3, 1), (2, 7, 9, 64, 5, 3), (2, 7, 9, 192, 3, 1), (2, 9, 9, 1024, 5, 3)]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('V,H,W,C,ksz,stride', GENERIC_WINDOWS)
def test_stem_pool_family_generic_windows(V, H, W, C, ksz, stride, dtype):
    """The loop forms of maxpool_bwd, maxpool_gather and bn_bwd_apply_pool, which the 3 x 3 stride-2 stem pool bypasses."""
    from tests import gpu_checks as gc
    _assert(gc.check_stem_pool_lattice(V, H, W, C, dtype, ksz=ksz, stride=stride))


# ---------------------------------------------------------------------------------------------------------------- ResNet-D shortcut pool
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('C', [8, 192])
@pytest.mark.parametrize('H,W,stride', [(7, 4, 2), (5, 8, 2), (7, 4, 1), (4, 7, 1)])
def test_avgpool2_on_non_square_maps(H, W, stride, C, dtype):
    from tests import gpu_checks as gc
    _assert(gc.check_avgpool2(2, H, C, stride, dtype, W=W))
