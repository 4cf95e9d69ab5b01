"""CPU tests that go with tests/test_gpu_bn_and_stem_pool.py: the explicit max-pool reference and the lattice generator of
tests/bn_pool_reference.py, pinned without a GPU."""
import pytest
import torch
import torch.nn.functional as F

from tests import bn_pool_reference as R

# every (window, stride, V, H, W) the GPU module pools at
POOL_SHAPES = [(3, 2, 2, 6, 10), (3, 2, 3, 7, 5), (3, 2, 1, 9, 16), (3, 2, 2, 1, 1), (3, 2, 1, 2, 3), (3, 2, 2, 15, 15),
               (2, 2, 2, 7, 9), (3, 1, 2, 7, 9), (5, 3, 2, 7, 9), (5, 3, 2, 4, 5)]


@pytest.mark.parametrize('ksz,stride,V,H,W', POOL_SHAPES)
def test_explicit_maxpool_equals_float64_autograd_on_tie_free_data(ksz, stride, V, H, W):
    """Random float64 data has no tied positive maxima; a window of zeros may tie, but its gradient is masked by the ReLU either way.  So the
    pooled value and the gradient wrt the BatchNorm output are those of relu -> pad(-inf) -> F.max_pool2d."""
    C = 5
    g = torch.Generator().manual_seed(ksz * 100 + H)
    x = torch.randn(V, H, W, C, generator=g, dtype=torch.float64)
    scale = torch.randn(C, generator=g, dtype=torch.float64)
    shift = 0.3 * torch.randn(C, generator=g, dtype=torch.float64)
    OH, pt, pb = R.same_pad(H, ksz, stride)
    OW, pl, pr = R.same_pad(W, ksz, stride)
    # dy on a dyadic grid: a pixel that wins several windows adds their gradients, and the order of that sum must not matter below
    dy = torch.randint(-64, 65, (V, OH, OW, C), generator=g).double() / 8
    pre = (x * scale + shift).permute(0, 3, 1, 2).requires_grad_(True)
    pooled = F.max_pool2d(F.pad(F.relu(pre), (pl, pr, pt, pb), value=float('-inf')), ksz, stride)
    assert tuple(pooled.shape) == (V, C, OH, OW)
    pooled.backward(dy.permute(0, 3, 1, 2))
    ref = R.bnrelu_maxpool_ref(x, scale, shift, dy, ksz, stride)
    assert torch.equal(ref['y'], pooled.detach().permute(0, 2, 3, 1))
    assert torch.equal(ref['dpre'], pre.grad.permute(0, 2, 3, 1))
    assert int(ref['tap'].max()) < ksz * ksz
    # the routed gradient loses nothing: every pooled element hands its dy to exactly one input pixel
    assert torch.equal(ref['dact'].sum((1, 2)), dy.sum((1, 2)))


def test_explicit_maxpool_ties_on_a_hand_written_map():
    """4 x 5 map, one channel, scale 1, shift 0, 3 x 3 stride 2 SAME: OH, OW = 2, 3 with pad_t = 0 (one row below), pad_l = 1.
         x =  1  3  0  0 -1         window (oy, ox) covers rows 2 oy .. 2 oy + 2, columns 2 ox - 1 .. 2 ox + 1
              3  2 -2  0  0
              0  3  0 -1 -3
              5  5  0  0  0
    (0,0): columns -1..1 -> in-bounds taps kx = 1, 2; the maximum 3 sits at (0,1) tap 2, (1,0) tap 4, (2,1) tap 8: the first, tap 2, wins.
    (0,1): interior window, columns 1..3: 3 at (0,1) tap 0 and (2,1) tap 6 -> tap 0.
    (0,2): columns 3..5, all values <= 0 -> ReLU output all 0: the first in-bounds tap, (0,3) = tap 0, wins.
    (1,0): edge window, rows 2..4 (row 4 off the map), columns -1..1: relu = [0 3 / 5 5]: 5 at (3,0) tap 4 and (3,1) tap 5 -> tap 4.
    (1,1): rows 2..3, columns 1..3: [3 0 0 / 5 0 0] -> 5 at (3,1) tap 3.
    (1,2): rows 2..3, columns 3..4: all zero -> first in-bounds tap (2,3) = tap 0."""
    x = torch.tensor([[1., 3, 0, 0, -1], [3, 2, -2, 0, 0], [0, 3, 0, -1, -3], [5, 5, 0, 0, 0]], dtype=torch.float64).view(1, 4, 5, 1)
    dy = torch.tensor([[1., 2, 4], [8, 16, 32]], dtype=torch.float64).view(1, 2, 3, 1)
    one, zero = torch.ones(1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)
    ref = R.bnrelu_maxpool_ref(x, one, zero, dy)
    assert ref['y'].view(2, 3).tolist() == [[3., 3., 0.], [5., 5., 0.]]
    assert ref['tap'].view(2, 3).tolist() == [[2, 0, 0], [4, 3, 0]]
    # dact: (0,1) receives windows (0,0) and (0,1): 1 + 2; (0,3) the all-zero window (0,2): 4; (3,0) window (1,0): 8; (3,1) window (1,1): 16;
    # (2,3) the all-zero window (1,2): 32
    want_dact = [[0., 3, 0, 4, 0], [0, 0, 0, 0, 0], [0, 0, 0, 32, 0], [8, 16, 0, 0, 0]]
    assert ref['dact'].view(4, 5).tolist() == want_dact
    # dpre: the ReLU kills what went to pixels with x <= 0 -- the two all-zero windows give no gradient
    want_dpre = [[0., 3, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [8, 16, 0, 0, 0]]
    assert ref['dpre'].view(4, 5).tolist() == want_dpre
    # a negative scale mirrors the map: the winners are now the most negative x
    neg = R.bnrelu_maxpool_ref(x, -one, zero, dy)
    assert neg['y'].view(2, 3).tolist() == [[0., 2., 3.], [0., 1., 3.]]
    assert neg['tap'].view(2, 3).tolist() == [[1, 4, 7], [1, 2, 1]]


@pytest.mark.parametrize('shape', [(3, 9, 14, 192), (2, 6, 10, 64), (3, 7, 5, 128), (1, 9, 16, 192), (1, 2, 3, 256), (2, 15, 15, 64),
                                   (2, 7, 9, 64)])
def test_lattice_meets_its_conditions(shape):
    L = R.lattice(shape, seed=0, names=('x', 'dy'))
    R.assert_survives(L, torch.float32)
    R.assert_survives(L, torch.bfloat16)
    s = R.lattice_shares(L)
    assert s['win_tied_pos'] >= 0.05 and s['win_zero'] >= 0.05, s
    assert s['pre_zero'] >= 0.01 and s['scale_neg'] >= 0.01 and s['scale_zero'] >= 0.01, s
    # the BatchNorm output and the ReLU output fit bf16 exactly (what makes the bf16 kernels tie as the fp32 ones do)
    pre = L['x'] * L['scale'] + L['shift']
    assert torch.equal(pre.bfloat16().double(), pre)


def test_lattice_references_are_exact_in_float32():
    """x*scale+shift, the two BatchNorm-backward sums in a random row order and scale*(dm - c1 - x^*c2): float32 == float64 bit for bit."""
    L = R.lattice((3, 9, 14, 192), seed=0, names=('x', 'dy', 'res', 'msk'))
    perm = R.row_perm(3 * 9 * 14)
    for relu in (False, True):
        for res_mode in (0, 1, 2):
            R.assert_exact(lambda d: R.bn_apply_ref(L, relu, res_mode, d), 'bn_apply')
    for mode in (0, 1, 2):
        R.assert_exact(lambda d: R.bn_bwd_ref(L, R.bn_masked_dy(L, mode, d), d, perm), 'bn_bwd')
    R.assert_exact(lambda d: R.bnrelu_maxpool_ref(L['x'], L['scale'], L['shift'], None, 3, 2, d), 'maxpool')


def test_narrow_and_single_pixel_lattices_still_carry_zero_and_negative_scales():
    for shape in [(1, 4), (37, 8), (2, 1, 1, 64)]:
        s = R.lattice_shares(R.lattice(shape, seed=0))
        assert s['scale_neg'] >= 0.01 and s['scale_zero'] >= 0.01, (shape, s)
    # one tap per window: nothing can tie, but a window is zero whenever its pixel is
    s = R.lattice_shares(R.lattice((2, 1, 1, 64), seed=0))
    assert s['win_tied_pos'] == 0.0 and s['win_zero'] >= 0.05


def test_fp32_stem_reduce_always_walks_the_pooled_pixels():
    """simclr_bn_bwd_reduce_pool takes the walk over the pooled pixels (bn_bwd_reduce_pool_out) for fp32 storage whenever there are at
    least as many pooled pixels as workgroups.  With the 3 x 3 stride-2 stem pool that always holds (a workgroup owns >= 8 input pixels,
    a pooled pixel stands for <= 4), so no such call reaches bn_bwd_reduce_pool<float>; a 5 x 5 stride-3 window at C = 1024 does."""
    from simclr_amd import _lib
    slots = _lib.lib().bn_bwd_pool_slots
    for C in (4, 64, 128, 256, 1024):
        for V in (1, 2, 3, 64):
            for H in (1, 2, 3, 7, 16, 112):
                for W in (1, 2, 5, 9, 112):
                    OH, OW = R.same_pad(H, 3, 2)[0], R.same_pad(W, 3, 2)[0]
                    assert V * OH * OW >= slots(V * H * W, C, _lib.DT_F32), (V, H, W, C)
    assert 2 * R.same_pad(9, 5, 3)[0] ** 2 < slots(2 * 9 * 9, 1024, _lib.DT_F32)
