"""GPU parity tests (pytest -m gpu) of the selective-kernel unit and the small head kernels of csrc/pool.hip: each kernel, called through
the C ABI, against a float64 reference of the same operation at the shapes and edges the product reaches (tf2/resnet.py:217-277 for the
SK unit, tf2/objective.py:27-32 + tf2/metrics.py:49-55 for the supervised loss).  The check bodies live in tests/gpu_checks.py."""
import pytest
import torch

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


# ---------------------------------------------------------------------------------------------------------------- SK kernels
# (V, H, W, f, lpitch, gpitch); None = the unpadded pitch (2f, f)
SK_PRODUCT = [(4, 7, 7, 512, None, None), (3, 14, 14, 256, None, None), (2, 28, 28, 128, None, None),
              (2, 56, 56, 64, None, None)]          # HW = 3136: the longest serial sums of sk_pool_fwd / sk_mix_bwd_logits in any supported model
SK_PITCH = [(3, 4, 4, 72, 192, 128), (3, 5, 5, 8, 64, 64)]
SK_EDGES = [(3, 5, 3, 64, None, None), (3, 1, 1, 64, None, None), (1, 7, 7, 64, None, None), (130, 3, 3, 64, None, None)]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('V,H,W,f,lpitch,gpitch', SK_PRODUCT + SK_PITCH + SK_EDGES)
def test_sk_kernels_vs_float64(V, H, W, f, lpitch, gpitch, dtype):
    from tests import gpu_checks as gc
    _assert(gc.check_sk_kernels(V, H, W, f, lpitch, gpitch, dtype))


def test_sk_kernels_four_channels_f32_and_bf16_refusal():
    """f = 4: one 16-byte chunk per stream in fp32.  In bf16 a chunk holds 8 channels, so sk_mix_fwd and sk_mix_bwd_streams refuse f = 4
    with an argument error instead of launching."""
    from simclr_amd import ops
    from simclr_amd._lib import SimclrHipError
    from tests import gpu_checks as gc
    _assert(gc.check_sk_kernels(3, 5, 5, 4, 64, 64, F32))
    a = torch.zeros(2, 3, 3, 8, device='cuda', dtype=BF)
    l = torch.zeros(2, 64, device='cuda', dtype=BF)
    dout = torch.zeros(2, 3, 3, 4, device='cuda', dtype=BF)
    dg = torch.zeros(2, 64, device='cuda', dtype=BF)
    with pytest.raises(SimclrHipError, match='sk_mix_fwd: bad f/lpitch'):
        ops.sk_mix_fwd(a, l, 4)
    with pytest.raises(SimclrHipError, match='sk_mix_bwd_streams: bad shape'):
        ops.sk_mix_bwd_streams(l, dout, dg, 4)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('logits', ['equal', 'saturated'])
@pytest.mark.parametrize('V,H,W,f,lpitch,gpitch', [(4, 7, 7, 64, None, None), (3, 4, 4, 72, 192, 128)])
def test_sk_kernels_equal_and_saturated_logits(V, H, W, f, lpitch, gpitch, logits, dtype):
    """'equal': l0 == l1, the mix is exactly 0.5.  'saturated': logit differences of +-30, +-100, +-200 -- __expf over- and underflows, the
    mix must come out 0 / 1, every gradient finite."""
    from tests import gpu_checks as gc
    _assert(gc.check_sk_kernels(V, H, W, f, lpitch, gpitch, dtype, logits=logits))


# ---------------------------------------------------------------------------------------------------------------- SK layer
# seeds chosen on the CPU so that no BatchNorm pre-activation of the float64 reference lies within 1e-5 * max of zero (check_sk_layer
# asserts it): nothing in the comparison depends on which side of zero a rounding error falls
SK_LAYER_CASES = [(3, 14, 64, 64, 2, 4), (3, 8, 64, 64, 1, 10), (4, 7, 64, 64, 1, 11)]      # margins 2.7e-5, 2.7e-5, 2.3e-5


@pytest.mark.parametrize('f32_matmul', ['exact', 'f16x3_3'])
@pytest.mark.parametrize('V,H,Cin,f,stride,seed', SK_LAYER_CASES)
def test_sk_layer_vs_float64_oracle(V, H, Cin, f, stride, seed, f32_matmul):
    from tests import gpu_checks as gc
    _assert(gc.check_sk_layer(V, H, Cin, f, stride, f32_matmul=f32_matmul, seed=seed))


# ---------------------------------------------------------------------------------------------------------------- pooling
@pytest.mark.parametrize('V,H,C', [(4, 7, 2048), (2, 56, 64)])
def test_global_avgpool_fp32_means_of_bf16_activations(V, H, C):
    from tests import gpu_checks as gc
    _assert(gc.check_avgpool_f32_from_bf16(V, H, C))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('V,H,C', [(4, 7, 2048), (3, 5, 64)])
def test_global_avgpool_bwd_masked(V, H, C, dtype):
    from tests import gpu_checks as gc
    _assert(gc.check_avgpool_bwd_mask(V, H, C, dtype))


# ---------------------------------------------------------------------------------------------------------------- supervised head
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('nclass,cpad', [(10, 16), (1000, 1008)])
@pytest.mark.parametrize('rows,label_rows', [(1, 1), (5, 5), (63, 63), (2, 1), (10, 5), (126, 63)])
def test_bias_softmax_xent_rows_and_views(rows, label_rows, nclass, cpad, dtype):
    """Single view (label_rows == rows) and two views (label_rows == rows / 2); row counts that do not fill the four rows of a workgroup."""
    from tests import gpu_checks as gc
    _assert(gc.check_xent(rows, label_rows, nclass, cpad, dtype))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('nclass,cpad,mode', [(10, 16, 'zero'), (1000, 1008, 'zero'), (1000, 1008, 'tie_cross'), (1000, 1008, 'tie_same'),
                                              (10, 16, 'large'), (1000, 1008, 'large')])
def test_bias_softmax_xent_ties_and_large_logits(nclass, cpad, mode, dtype):
    """All logits zero (a zero-initialised logits layer on its first step): loss log(nclass), accuracy = the share of rows with label 0,
    because tf.argmax returns the first maximum.  Two-way ties across lanes and inside a lane: the lower column wins.  Logits of
    magnitude 80: everything finite."""
    from tests import gpu_checks as gc
    _assert(gc.check_xent(63, 63, nclass, cpad, dtype, mode=mode))
    _assert(gc.check_xent(10, 5, nclass, cpad, dtype, gscale=0.5, mode=mode))


@pytest.mark.parametrize('dtype', DTYPES)
def test_bias_softmax_xent_gscale(dtype):
    from tests import gpu_checks as gc
    _assert(gc.check_xent(10, 5, 1000, 1008, dtype, gscale=0.5))
    _assert(gc.check_xent(5, 5, 10, 16, dtype, gscale=0.5))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('cvalid,C', [(10, 16), (1000, 1008)])
@pytest.mark.parametrize('rows', [1, 15, 17, 1000])
def test_colsum(rows, cvalid, C, dtype):
    from tests import gpu_checks as gc
    _assert(gc.check_colsum(rows, C, cvalid, dtype))


# ---------------------------------------------------------------------------------------------------------------- elementwise helpers
def test_cast_is_round_to_nearest_even_on_every_class_of_value():
    from tests import gpu_checks as gc
    _assert(gc.check_cast_classes())


@pytest.mark.parametrize('n', [1, 255, 256, 257, (1 << 20) + 3])
def test_cast_sizes_and_sentinel(n):
    from tests import gpu_checks as gc
    _assert(gc.check_cast_sizes(n))


@pytest.mark.parametrize('n', [1, 255, 256, 257, (1 << 20) + 3])
def test_axpy_f32_is_one_fma_per_element(n):
    from tests import gpu_checks as gc
    _assert(gc.check_axpy(n))


@pytest.mark.parametrize('n', [1, 1023, 1024, 1025, (1 << 18) + 7, 2048000])
def test_l2_loss_f32(n):
    from tests import gpu_checks as gc
    _assert(gc.check_l2_loss(n))


@pytest.mark.parametrize('n', [1, 5, 16])
def test_accumulate_scalars(n):
    from tests import gpu_checks as gc
    _assert(gc.check_accumulate_scalars(n))


def test_empty_launches_touch_nothing_and_bad_colsum_shapes_are_refused():
    from simclr_amd import ops
    from simclr_amd._lib import DT_F32, SimclrHipError, lib
    from tests import gpu_checks as gc
    _assert(gc.check_empty_launches())
    x = torch.ones(4, 16, device='cuda')
    out = torch.full((16,), 7.5, device='cuda')
    for rows, C, cvalid in [(0, 16, 10), (4, 16, 0), (4, 16, 17), (4, 16, -1)]:
        rc = lib()._dll.simclr_colsum(ops._p(x), rows, C, cvalid, ops._p(out), 0, DT_F32, ops._s())
        assert rc == 1 and 'colsum: bad shape' in lib().last_error(), (rows, C, cvalid, rc, lib().last_error())
    with pytest.raises(SimclrHipError, match='colsum: bad shape'):
        ops.colsum(x, 17, out)
    torch.cuda.synchronize()
    assert bool((out == 7.5).all())
