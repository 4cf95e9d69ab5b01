"""CPU tests of the DropBlock restatement (tests/dropblock_reference.py), of the flags, and of the construction of a network with
DropBlock sites.  The hand cases were worked out on paper from tf2/resnet.py:81-157."""
import numpy as np
import pytest
import torch

from tests import dropblock_reference as dr


def _hand_noise():
    u = np.full((1, 6, 6, 1), 0.999, np.float32)
    u[0, 2, 2, 0] = 0.0
    return u


@pytest.mark.parametrize('k, dropped, ones', [(2, (1, 2), 32), (3, (1, 3), 27), (4, (0, 3), 20)])
def test_hand_cases_6x6(k, dropped, ones):
    """6x6 map, one channel, keep_prob 0.9, every u = 0.999 except u[2,2] = 0: one seed at (2,2) drops rows / cols dropped[0]..dropped[1]."""
    p, n, size = dr.block_pattern(_hand_noise(), 0.9, k)
    want = np.ones((6, 6), np.float32)
    want[dropped[0]:dropped[1] + 1, dropped[0]:dropped[1] + 1] = 0
    assert np.array_equal(p[0, :, :, 0], want)
    assert (n, size) == (ones, 36)
    assert dr.percent_ones(n, size) == np.float32(ones) / np.float32(36)
    x = np.arange(36, dtype=np.float32).reshape(1, 6, 6, 1) - 7
    y = dr.apply_f32(x, p, n, size)
    assert np.array_equal(y, (x / (np.float32(ones) / np.float32(36))) * want[None, :, :, None])


def test_hand_case_block_covers_the_map():
    """3x3 map, V = 2, C = 2, dropblock_size 7 (clipped to 3), keep_prob 0.5: the only valid centre is (1,1); a zero there in plane
    (v=1, c=0) drops that whole plane.  The pattern is [V,1,1,C]: percent_ones = 3/4, not 27/36."""
    u = np.full((2, 3, 3, 2), 0.999, np.float32)
    u[1, 1, 1, 0] = 0.0
    k, gamma = dr.gamma_of(0.5, 3, 7)
    assert k == 3 and gamma == 0.5
    p, n, size = dr.block_pattern(u, 0.5, 7)
    assert np.array_equal(p[:, 0, 0, :], np.array([[1, 1], [0, 1]], np.float32))
    assert np.all(p == p[:, :1, :1, :])
    assert (n, size) == (3, 4) and dr.percent_ones(n, size) == np.float32(0.75)
    # a zero away from the centre is not a seed
    u2 = np.full((2, 3, 3, 2), 0.999, np.float32)
    u2[0, 0, 0, 1] = 0.0
    assert dr.block_pattern(u2, 0.5, 7)[1:] == (4, 4)


def test_valid_centres_odd_and_even():
    assert dr.valid_centres(7, 3).tolist() == [False, True, True, True, True, True, False]
    assert dr.valid_centres(6, 2).tolist() == [False, True, True, True, True, True]            # k//2 = 1, (k-1)//2 = 0
    assert dr.valid_centres(6, 4).tolist() == [False, False, True, True, True, False]          # 2 <= i < 5
    assert dr.valid_centres(7, 7).tolist() == [False, False, False, True, False, False, False]
    assert dr.valid_centres(4, 4).tolist() == [False, False, True, False]
    for w, k in [(6, 2), (7, 3), (6, 4), (14, 7), (56, 7), (4, 3)]:
        assert dr.valid_centres(w, k).sum() == w - k + 1           # every block lies inside the map


def test_gamma_formula():
    assert dr.gamma_of(0.9, 14, 7) == (7, (1.0 - 0.9) * 196 / 49 / 64)
    assert dr.gamma_of(0.75, 8, 3) == (3, 0.25 * 64 / 9 / 36)
    assert dr.gamma_of(0.9, 7, 9) == (7, (1.0 - 0.9) * 49 / 49 / 1)       # size clipped to the width
    assert dr.gamma_of(1.0, 8, 3)[1] == 0.0
    # the product's copy of the formula and its fp32 constant
    from simclr_amd import ops
    for kp, w, s in [(0.9, 14, 7), (0.75, 8, 3), (0.9, 7, 9), (0.9, 6, 2)]:
        assert ops.dropblock_gamma(kp, w, s) == dr.gamma_of(kp, w, s)
        assert np.float32(ops.dropblock_keep_thresh(dr.gamma_of(kp, w, s)[1])) == np.float32(1.0 - dr.gamma_of(kp, w, s)[1])


@pytest.mark.parametrize('hw, k', [(6, 2), (8, 3), (8, 4), (7, 5), (14, 7), (5, 4)])
def test_min_pool_against_torch_max_pool(hw, k):
    """-max_pool2d(-x) with TF's SAME padding written out: (k-1)//2 before, k//2 after (asymmetric for even k), padded with the
    identity of the max."""
    rng = np.random.default_rng(hw * 10 + k)
    x = (rng.random((3, hw, hw, 5)) < 0.8).astype(np.float32)
    t = torch.from_numpy(-x).permute(0, 3, 1, 2)
    t = torch.nn.functional.pad(t, ((k - 1) // 2, k // 2, (k - 1) // 2, k // 2), value=float('-inf'))
    want = (-torch.nn.functional.max_pool2d(t, k, stride=1)).permute(0, 2, 3, 1).numpy()
    assert np.array_equal(dr.min_pool_same(x, k), want)


def test_restatement_against_torch_end_to_end():
    rng = np.random.default_rng(3)
    u = rng.random((2, 8, 8, 16), dtype=np.float32)
    p, n, size = dr.block_pattern(u, 0.75, 3)
    k, gamma = dr.gamma_of(0.75, 8, 3)
    i = torch.arange(8)
    v1 = (i >= k // 2) & (i < 8 - (k - 1) // 2)
    valid = (v1[:, None] & v1[None, :]).float()[None, :, :, None]
    seed = ((1 - valid + torch.tensor(1 - gamma, dtype=torch.float32) + torch.from_numpy(u)) >= 1).float()
    t = torch.nn.functional.pad((-seed).permute(0, 3, 1, 2), (1, 1, 1, 1), value=float('-inf'))
    want = (-torch.nn.functional.max_pool2d(t, 3, stride=1)).permute(0, 2, 3, 1)
    assert np.array_equal(p, want.numpy())
    assert n == int(want.sum()) and size == want.numel()
    assert 0 < n < size


def test_bit_packing_round_trip_and_generator_range():
    rng = np.random.default_rng(0)
    p = (rng.random((2, 3, 3, 24)) < 0.5).astype(np.float32)
    b = dr.pack_bits(p)
    assert b.shape == (2, 3, 3, 3) and b.dtype == np.uint8
    assert b[1, 2, 0, 1] == sum(int(p[1, 2, 0, 8 + j]) << j for j in range(8))
    assert np.array_equal(dr.unpack_bits(b, 24), p.astype(np.uint8))
    u = dr.generator_uniform(dr.site_key(0, 0, 0, 0), (4, 7, 7, 64))
    assert u.dtype == np.float32 and u.min() >= 0 and u.max() < 1 and abs(float(u.mean()) - 0.5) < 0.01
    assert np.array_equal(u, dr.generator_uniform(dr.site_key(0, 0, 0, 0), (4, 7, 7, 64)))
    keys = {dr.site_key(*a) for a in [(0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)]}
    assert len(keys) == 5
    # the product's key derivation is the restated one
    from simclr_amd.resnet import dropblock_key
    for a in [(0, 0, 0, 0), (7, 123456, 3, 35), (2 ** 40, 5, 0, 1)]:
        assert dropblock_key(*a) == dr.site_key(*a)
    assert np.array_equal(dr.bf16_round(np.array([1.0, 1.00390625, 1.01171875], np.float32)),
                          np.array([1.0, 1.0, 1.015625], np.float32))         # ties to even, both directions


def test_flag_parsing_and_startup_errors():
    from simclr_amd.flags import FLAGS, check_dropblock_flags, parse_dropblock_keep_probs
    try:
        FLAGS.reset()
        assert (FLAGS.dropblock_keep_probs, FLAGS.dropblock_size, FLAGS.dropblock_seed) == ('', None, 0)
        assert check_dropblock_flags() == (None, None)
        FLAGS.parse(['--dropblock_keep_probs=none,None,0.9,0.75', '--dropblock_size=7', '--dropblock_seed', '5'])
        assert check_dropblock_flags() == ([None, None, 0.9, 0.75], 7) and FLAGS.dropblock_seed == 5
        assert parse_dropblock_keep_probs('1,1.0, 1 ,none') == [None, None, None, None]
        FLAGS.parse(['--dropblock_keep_probs=1,1,1,1'])
        assert check_dropblock_flags() == ([None] * 4, None)            # nothing active: no size needed
        for bad in ('0.9', '0.9,0.9,0.9', '0.9,0.9,0.9,0.9,0.9', 'a,b,c,d', '0,1,1,1', '1,1,1,1.5', '1,1,1,-0.1'):
            with pytest.raises(ValueError):
                parse_dropblock_keep_probs(bad)
        FLAGS.parse(['--dropblock_keep_probs=1,1,0.9,0.9'])
        with pytest.raises(ValueError, match='dropblock_size'):
            check_dropblock_flags()
        FLAGS.parse(['--dropblock_keep_probs=1,1,0.9,0.9', '--dropblock_size=0'])
        with pytest.raises(ValueError, match='dropblock_size'):
            check_dropblock_flags()
        # the step function checks them before any device work, as main() does
        from simclr_amd import run
        FLAGS.parse(['--dropblock_keep_probs=1,1,0.9,0.9'])
        with pytest.raises(ValueError, match='dropblock_size'):
            run.make_single_step(None, None, None, all_metrics={})
    finally:
        FLAGS.reset()


def _names(layer):
    return [(v.name, tuple(v.value.shape)) for v in layer.variables]


def test_network_with_dropblock_constructs_on_cpu():
    """Fails on a build without the feature: an active keep probability raised NotImplementedError."""
    from simclr_amd import model as model_lib
    from simclr_amd import resnet
    from simclr_amd.flags import FLAGS
    from simclr_amd.resnet import RT, DropBlock
    try:
        FLAGS.reset(); FLAGS.update(use_blur=False); RT.reset()
        net = resnet.resnet(50, 1, dropblock_keep_probs=[None, None, 0.9, 0.9], dropblock_size=7)
        per_group = [[b.dropblock for b in g.layers] for g in net.block_groups]
        assert all(d is None for g in per_group[:2] for d in g)
        sites = [s for g in per_group[2:] for d in g for s in d]
        assert len(sites) == 4 * (6 + 3) and all(isinstance(s, DropBlock) for s in sites)
        assert [s.site for s in sites] == list(range(36))                  # ordinals in construction order
        assert all((s.keep_prob, s.dropblock_size, s.data_format) == (0.9, 7, 'channels_last') for s in sites)
        d = DropBlock(0.8, 5, 'channels_last')
        assert (d.keep_prob, d.dropblock_size, d.site) == (0.8, 5, 36) and d.saved is None
        with pytest.raises(ValueError):
            resnet.resnet(50, 1, dropblock_keep_probs=[None, None, 0.9, 0.9])          # no size
        with pytest.raises(ValueError):
            resnet.resnet(50, 1, dropblock_keep_probs=[0.9, 0.9], dropblock_size=7)   # tf2/resnet.py:546-547
        # ResidualBlock discards the arguments (tf2/resnet.py:323-324)
        RT.reset()
        r18 = resnet.resnet(18, 1, dropblock_keep_probs=[0.9] * 4, dropblock_size=3)
        assert RT.counters.get('drop_block', 0) == 0 and len(r18.block_groups) == 4
        # Model with the flags set
        FLAGS.parse(['--dropblock_keep_probs=none,none,0.9,0.9', '--dropblock_size=7', '--nouse_blur']); RT.reset()
        m = model_lib.Model(1000)
        assert RT.counters['drop_block'] == 36 and RT.counters['bottleneck_block'] == 16 and RT.counters['conv2d'] == 53
        assert m.resnet_model.block_groups[3].layers[2].dropblock[3].site == 35
        # selective-kernel blocks carry the sites too
        FLAGS.update(sk_ratio=0.0625); RT.reset()
        m = model_lib.Model(1000)
        assert RT.counters['drop_block'] == 36 and RT.counters['sk__conv2d'] == 16
    finally:
        FLAGS.reset(); RT.reset()


def test_inactive_keep_probs_build_todays_layers():
    from simclr_amd import model as model_lib
    from simclr_amd import resnet
    from simclr_amd.flags import FLAGS
    from simclr_amd.resnet import RT

    def layer_list(layer, out):
        out.append(type(layer).__name__)
        for l in layer.sublayers():
            layer_list(l, out)
        return out

    try:
        built = []
        for kw in (dict(), dict(dropblock_keep_probs=[None] * 4, dropblock_size=7), dict(dropblock_keep_probs=[1.0] * 4, dropblock_size=7),
                   dict(dropblock_keep_probs=[1.0, None, 1.0, None])):
            FLAGS.reset(); FLAGS.update(use_blur=False); RT.reset()
            net = resnet.resnet(50, 1, **kw)
            built.append((layer_list(net, []), dict(RT.counters)))
            assert all(b.dropblock is None for g in net.block_groups for b in g.layers)
        assert all(b == built[0] for b in built[1:])
        assert 'DropBlock' not in built[0][0] and 'drop_block' not in built[0][1]
        counters = []
        for argv in ([], ['--dropblock_keep_probs=1,1,1,1'], ['--dropblock_keep_probs=none,none,none,none', '--dropblock_size=7']):
            FLAGS.reset(); FLAGS.parse(argv + ['--nouse_blur']); RT.reset()
            RT.device = torch.device('cpu')
            m = model_lib.Model(1000)
            m.build_variables()
            counters.append((dict(RT.counters), _names(m)))
        assert counters[1] == counters[0] and counters[2] == counters[0]
    finally:
        FLAGS.reset(); RT.reset()
