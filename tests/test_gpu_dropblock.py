"""GPU tests of DropBlock (csrc/dropblock.hip, resnet.DropBlock, the DropBlock route of resnet.BottleneckBlock) against the numpy
restatement tests/dropblock_reference.py and a float64 torch-autograd restatement of the block."""
import ctypes
import json
import math
import os
import shutil
import tempfile
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import dropblock_reference as dr
from tests.gpu_checks import DEV

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ops():
    from simclr_amd import ops
    return ops


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------------------------ mask kernel, supplied noise
MASK_SHAPES = [(2, 6, 6, 8, 2, .9), (2, 8, 8, 64, 3, .75), (2, 8, 8, 72, 4, .75), (3, 7, 7, 64, 7, .9), (2, 7, 7, 64, 9, .9),
               (2, 4, 4, 64, 3, .9), (1, 14, 14, 256, 7, .9), (1, 56, 56, 64, 7, .9)]


def _run_mask(u, size, keep):
    bits, count = _ops().dropblock_mask(u.shape, keep, size, noise=torch.from_numpy(u).to(DEV))
    torch.cuda.synchronize()
    return bits.cpu().numpy(), [int(c) for c in count.cpu()]


@pytest.mark.parametrize('V, H, W, C, size, keep', MASK_SHAPES)
def test_mask_kernel_equals_the_restatement(V, H, W, C, size, keep):
    u = np.random.default_rng(V * 1000 + H * 10 + size).random((V, H, W, C), dtype=np.float32)
    p, ones, total = dr.block_pattern(u, keep, size)
    bits, count = _run_mask(u, size, keep)
    print('dropblock_mask %r: kept %d of %d (%.1f %%)' % ((V, H, W, C, size, keep), ones, total, 100.0 * ones / total))
    assert 0 < ones < total
    assert total == (V * C if min(size, W) == W else V * H * W * C)
    assert bits.shape == (V, H, W, C // 8) and np.array_equal(bits, dr.pack_bits(p))
    assert count == [ones, total]


def _fence_noise(keep, W, size):
    """Noise values around the decision t + u >= 1, t = fp32(1 - gamma): g = fp32(gamma) and its two fp32 neighbours, and the values
    that separate the rounded fp32 add from any other evaluation.  u0 = 1 - t is exact in fp32 (Sterbenz), so t + u0 == 1.  Below 1 the
    fp32 spacing is 2^-24: t + (u0 - 2^-24) == 1 - 2^-24 exactly (dropped); t + (u0 - 2^-25) is a tie that rounds to the even 1.0
    (kept, though the exact sum is below 1); the neighbour of u0 towards 0 gives an exact sum just below 1 that rounds to 1.0 (kept);
    the neighbour of u0 - 2^-25 towards 0 gives a sum below the tie (dropped)."""
    _, gamma = dr.gamma_of(keep, W, size)
    g = np.float32(gamma)
    t = np.float32(1.0 - gamma)
    u0 = np.float32(1) - t
    tie = u0 - np.float32(2.0 ** -25)
    vals = np.array([g, np.nextafter(g, np.float32(0)), np.nextafter(g, np.float32(1)),
                     u0, np.nextafter(u0, np.float32(0)), np.nextafter(u0, np.float32(1)), u0 - np.float32(2.0 ** -24),
                     tie, np.nextafter(tie, np.float32(0))], np.float32)
    keeps = ((t + vals).astype(np.float32) >= np.float32(1))
    return vals, keeps, t


def test_mask_kernel_compares_in_fp32_with_greater_or_equal():
    """Noise on the fence (see _fence_noise): only the rounded fp32 add followed by >= reproduces the restatement."""
    V, H, W, C, size, keep = 2, 8, 8, 64, 3, .75
    vals, keeps, t = _fence_noise(keep, W, size)
    assert np.float64(t) + np.float64(vals[3]) == 1.0 and keeps[3]                       # equality is kept: >=, not >
    assert np.float64(t) + np.float64(vals[4]) < 1.0 and keeps[4]                        # the add is rounded to fp32 first
    assert np.float64(t) + np.float64(vals[7]) < 1.0 and keeps[7] and not keeps[8]       # the tie goes to the even 1.0
    assert not keeps[6] and keeps.any() and not keeps.all()
    rng = np.random.default_rng(5)
    u = vals[rng.integers(0, len(vals), (V, H, W, C))]
    seed = dr.seed_pattern(u, keep, size)
    assert 0 < seed.sum() < seed.size                       # the values do fall on both sides
    p, ones, total = dr.block_pattern(u, keep, size)
    bits, count = _run_mask(u, size, keep)
    assert np.array_equal(bits, dr.pack_bits(p)) and count == [ones, total]


def test_refusals():
    from simclr_amd._lib import SimclrHipError, lib
    ops = _ops()
    with pytest.raises(ValueError, match='width!=height'):
        ops.dropblock_mask((2, 6, 8, 8), 0.9, 3, device=DEV)
    with pytest.raises(SimclrHipError, match='multiple of 8'):
        ops.dropblock_mask((2, 6, 6, 12), 0.9, 3, device=DEV)
    L = lib()
    x = torch.zeros(2, 6, 6, 12, device=DEV)
    b = torch.zeros(2, 6, 6, 2, device=DEV, dtype=torch.uint8)
    c = torch.ones(2, device=DEV, dtype=torch.int64)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    with pytest.raises(SimclrHipError, match='multiple of 8'):
        L.dropblock_apply(P(x), P(b), P(c), P(x), 72, 12, 0, None)
    with pytest.raises(SimclrHipError, match='null argument'):
        L.dropblock_mask(None, 0, 2, 6, 6, 8, 3, ctypes.c_float(0.9), None, None, None)
    with pytest.raises(SimclrHipError, match='width!=height'):
        L.dropblock_mask(None, 0, 2, 6, 8, 8, 3, ctypes.c_float(0.9), P(b), P(c), None)
    with pytest.raises(SimclrHipError, match='does not fit'):
        L.dropblock_mask(None, 0, 1, 200, 200, 8, 3, ctypes.c_float(0.9), P(b), P(c), None)
    with pytest.raises(SimclrHipError, match='null argument'):
        L.dropblock_apply(None, None, None, None, 72, 16, 0, None)
    with pytest.raises(SimclrHipError, match='null argument'):
        L.dropblock_tail_fwd(None, None, None, None, None, None, None, None, 72, 16, 0, None)
    with pytest.raises(SimclrHipError, match='null argument'):
        L.dropblock_tail_bwd(None, None, None, None, None, None, None, None, 72, 16, 0, None)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ generator
def _generated(shape, keep, size, key):
    bits, count = _ops().dropblock_mask(shape, keep, size, key=key, device=DEV)
    torch.cuda.synchronize()
    return bits.cpu().numpy(), [int(c) for c in count.cpu()]


@pytest.mark.parametrize('shape, size, keep', [((2, 14, 14, 256), 7, .9), ((2, 8, 8, 72), 4, .75), ((3, 7, 7, 64), 7, .5)])
def test_generator_equals_the_numpy_restatement(shape, size, keep):
    key = dr.site_key(3, 17, 1, 5)
    p, ones, total = dr.block_pattern(dr.generator_uniform(key, shape), keep, size)
    bits, count = _generated(shape, keep, size, key)
    assert np.array_equal(bits, dr.pack_bits(p)) and count == [ones, total] and 0 < ones < total
    again, count2 = _generated(shape, keep, size, key)
    assert np.array_equal(again, bits) and count2 == count                     # no state


def test_generator_key_and_seed_statistics():
    from simclr_amd.resnet import dropblock_key
    shape, size, keep = (2, 14, 14, 256), 7, .9
    base = dict(seed=3, step=17, replica=1, site=5)
    ref, _ = _generated(shape, keep, size, dropblock_key(**base))
    for name in base:
        other, _ = _generated(shape, keep, size, dropblock_key(**dict(base, **{name: base[name] + 1})))
        assert not np.array_equal(other, ref), 'changing %s left the pattern unchanged' % name
    # the seeds themselves: at dropblock_size 1 the pattern IS the seed pattern and gamma' = 1 - keep'; keep' = 1 - gamma makes the
    # kernel compare the same draws with the same fp32 constant as the k = 7 site does at its valid centres
    k, gamma = dr.gamma_of(keep, 14, size)
    keep1 = 1.0 - gamma
    assert np.float32(1.0 - dr.gamma_of(keep1, 14, 1)[1]) == np.float32(1.0 - gamma)
    key = dropblock_key(**base)
    seeds, _ = _generated(shape, keep1, 1, key)
    seeds = dr.unpack_bits(seeds, 256)
    v1 = dr.valid_centres(14, k)
    at_centres = seeds[:, v1][:, :, v1]
    want = dr.seed_pattern(dr.generator_uniform(key, shape), keep, size)[:, v1][:, :, v1]
    assert np.array_equal(at_centres, want.astype(np.uint8))
    n = at_centres.size
    assert n == 2 * 8 * 8 * 256
    dropped = 1.0 - at_centres.mean()
    sd = math.sqrt(gamma * (1 - gamma) / n)
    print('dropped share %.6f, gamma %.6f, %.2f standard deviations (n = %d)' % (dropped, gamma, (dropped - gamma) / sd, n))
    assert abs(dropped - gamma) <= 5 * sd


# ------------------------------------------------------------------------------------------------ apply and tail kernels
STREAM_SHAPES = [(2, 8, 8, 64), (1, 7, 7, 256), (3, 5, 5, 72)]       # the last: 1350 / 675 chunks, no multiple of a workgroup's 512


def _random_site(shape, rng, keep):
    p = (rng.random(shape) < keep).astype(np.float32)
    ones = int(p.sum())
    bits = torch.from_numpy(dr.pack_bits(p)).to(DEV)
    count = torch.tensor([ones, p.size], dtype=torch.int64, device=DEV)
    return p, (ones, p.size), bits, count


def _storage(x, dtype):
    """numpy fp32 -> (device tensor in `dtype` storage, the fp32 values it holds)."""
    t = torch.from_numpy(x).to(DEV).to(dtype)
    return t, t.float().cpu().numpy()


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('shape', STREAM_SHAPES)
def test_apply_kernel(shape, dtype):
    ops = _ops()
    rng = np.random.default_rng(sum(shape))
    p, cnt, bits, count = _random_site(shape, rng, 0.8)
    xt, x = _storage(rng.standard_normal(shape).astype(np.float32), dtype)
    want = dr.apply_f32(x, p, *cnt)
    if dtype == torch.bfloat16:
        want = dr.bf16_round(want)
    got = ops.dropblock_apply(xt, bits, count)
    torch.cuda.synchronize()
    assert got.dtype == dtype and _bits_equal(got.float().cpu().numpy(), want)
    assert (want == 0).any() and (want != 0).any()


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('shape', STREAM_SHAPES)
def test_tail_kernels(shape, dtype):
    ops = _ops()
    rng = np.random.default_rng(sum(shape) + 1)
    pa, ca, bits_a, count_a = _random_site(shape, rng, 0.8)
    pb, cb, bits_b, count_b = _random_site(shape, rng, 0.7)
    at, a = _storage(rng.standard_normal(shape).astype(np.float32), dtype)
    bt, b = _storage(rng.standard_normal(shape).astype(np.float32), dtype)
    dt_, dout = _storage(rng.standard_normal(shape).astype(np.float32), dtype)
    want = dr.tail_fwd_f32(a, pa, ca, b, pb, cb)
    if dtype == torch.bfloat16:
        want = dr.bf16_round(want)
    out, rb = ops.dropblock_tail_fwd(at, bits_a, count_a, bt, bits_b, count_b)
    torch.cuda.synchronize()
    assert _bits_equal(out.float().cpu().numpy(), want)
    # the ReLU bits: one byte per 16-byte chunk of the output, bit e = element e of the chunk (simclr_bn_apply's format)
    epc = 16 // out.element_size()
    mask = want > 0
    chunks = mask.reshape(-1, epc)
    want_bits = (chunks * (1 << np.arange(epc))).sum(axis=1).astype(np.uint8).reshape(-1, shape[-1] // epc)
    assert rb.dtype == torch.uint8 and np.array_equal(rb.cpu().numpy(), want_bits)
    out2, none = ops.dropblock_tail_fwd(at, bits_a, count_a, bt, bits_b, count_b, want_bits=False)
    assert none is None and torch.equal(out2, out)
    wda, wdb = dr.tail_bwd_f32(dout, mask, pa, ca, pb, cb)
    if dtype == torch.bfloat16:
        wda, wdb = dr.bf16_round(wda), dr.bf16_round(wdb)
    da, db = ops.dropblock_tail_bwd(dt_, rb, bits_a, count_a, bits_b, count_b)
    torch.cuda.synchronize()
    assert _bits_equal(da.float().cpu().numpy(), wda) and _bits_equal(db.float().cpu().numpy(), wdb)


def test_dropblock_layer_forward_backward_and_release():
    from simclr_amd.flags import FLAGS
    from simclr_amd.resnet import RT, Act, DropBlock
    FLAGS.reset(); RT.reset(); RT.device = torch.device(DEV)
    try:
        FLAGS.update(dropblock_seed=9)
        layer = DropBlock(0.75, 3, 'channels_last')
        x = torch.randn(2, 8, 8, 64, device=DEV)
        assert layer(Act(x), False).t is x and layer.saved is None              # inference: the input itself, nothing launched
        y = layer(Act(x), True)
        bits, count = layer.saved['bits'], layer.saved['count']
        key = dr.site_key(9, 0, 0, layer.site)
        p, ones, total = dr.block_pattern(dr.generator_uniform(key, tuple(x.shape)), 0.75, 3)
        assert np.array_equal(bits.cpu().numpy(), dr.pack_bits(p)) and [int(c) for c in count.cpu()] == [ones, total]
        assert _bits_equal(y.t.cpu().numpy(), dr.apply_f32(x.cpu().numpy(), p, ones, total))
        dy = torch.randn_like(x)
        dx = layer.backward(dy)
        assert layer.saved is None and _bits_equal(dx.cpu().numpy(), dr.apply_f32(dy.cpu().numpy(), p, ones, total))
        layer(Act(x), True)
        layer.release()
        assert layer.saved is None
        with pytest.raises(ValueError, match='width!=height'):
            layer(Act(torch.zeros(2, 6, 8, 64, device=DEV)), True)
        off = DropBlock(1.0, 3)
        assert off(Act(x), True).t is x
    finally:
        FLAGS.reset(); RT.reset()


# ------------------------------------------------------------------------------------------------ the block, against float64 autograd
def _block64(b, x, filters, strides, use_projection, sites):
    """BottleneckBlock.call (tf2/resnet.py:478-487) on the float64 builder's layers; sites: four (pattern NCHW, percent_ones) or None."""
    def drop(t, s):
        return t if s is None else t / s[1] * s[0]
    sites = sites or [None] * 4
    b.scope.append(b.namer('bottleneck_block'))
    shortcut = b._shortcut(x, 4 * filters, strides) if use_projection else x
    shortcut = drop(shortcut, sites[0])
    x = drop(b.batch_norm_relu(b.conv2d_fixed_padding(x, filters, 1, 1)), sites[1])
    if b.cfg.sk_ratio > 0:
        x = b.sk_conv2d(x, filters, strides)
    else:
        x = b.batch_norm_relu(b.conv2d_fixed_padding(x, filters, 3, strides))
    x = drop(x, sites[2])
    x = b.batch_norm_relu(b.conv2d_fixed_padding(x, 4 * filters, 1, 1), relu=False, init_zero=True)
    x = drop(x, sites[3])
    b.scope.pop()
    return F.relu(x + shortcut)


def _rel_l2(got, ref):
    return float((got.double().cpu() - ref).norm() / ref.norm())


BLOCK_VARIANTS = {'identity': dict(cin=256, strides=1, use_projection=False, sk_ratio=0.0),
                  'projection_s2': dict(cin=128, strides=2, use_projection=True, sk_ratio=0.0),
                  'identity_sk': dict(cin=256, strides=1, use_projection=False, sk_ratio=0.0625)}


def _run_block(variant, keep_prob, params, state, x, dy):
    """The product block (training, fp32 storage, exact fp32 MFMA) on the given variables; returns (tensors, sites) with sites = the four
    (pattern NCHW float64, ones / size) the layers drew, or None."""
    from simclr_amd import ops
    from simclr_amd.flags import FLAGS
    from simclr_amd.resnet import RT, Act, BottleneckBlock, join_wgrad_stream
    v = BLOCK_VARIANTS[variant]
    FLAGS.reset()
    FLAGS.update(compute_dtype='f32', f32_matmul='exact', sk_ratio=v['sk_ratio'], dropblock_seed=4)
    RT.reset()
    RT.device = torch.device(DEV)
    try:
        blk = BottleneckBlock(64, v['strides'], use_projection=v['use_projection'], dropblock_keep_prob=keep_prob, dropblock_size=3)
        blk.is_final = True                 # a block on its own: no consuming block folds its tail
        xd, dyd = x.to(DEV), dy.to(DEV)
        ops.begin_step(DEV)
        blk(Act(xd), True)                  # builds the variables
        ops.end_step()
        byname = {t.name: t for t in blk.variables}
        allv = dict(params); allv.update(state)
        assert sorted(byname) == sorted(allv), (sorted(byname), sorted(allv))
        for k, t in byname.items():
            t.value.copy_(allv[k].to(DEV))
        RT.weights_version += 1
        ops.begin_step(DEV)
        out = blk(Act(xd), True)
        sites = None
        if keep_prob is not None:
            assert blk._on_dropblock_route and blk.tail_info() is None and not blk.fused_tail and not blk._foldable()
            sites = []
            for d in blk.dropblock:
                bits, (ones, size) = d.saved['bits'].cpu().numpy(), [int(c) for c in d.saved['count'].cpu()]
                pat = dr.unpack_bits(bits, bits.shape[-1] * 8).astype(np.float64)
                assert size == pat.size and ones == int(pat.sum()) and 0 < ones < size
                sites.append((torch.from_numpy(pat).permute(0, 3, 1, 2), ones / size))
        else:
            assert blk.dropblock is None
        dx, partial = blk.backward(dyd)
        join_wgrad_stream()
        torch.cuda.synchronize()
        assert partial is None
        if keep_prob is not None:
            assert all(d.saved is None for d in blk.dropblock)
        got = OrderedDict(out=out.t, dx=dx)
        for k in params:
            got['d ' + k] = byname[k].grad
        assert all(t is not None and bool(torch.isfinite(t).all()) for t in got.values())
        return got, sites
    finally:
        ops.end_step()
        ops.set_f32_matmul('exact')
        FLAGS.reset(); RT.reset()


@pytest.mark.parametrize('variant', list(BLOCK_VARIANTS))
def test_block_against_float64_autograd(variant):
    """BottleneckBlock(filters=64), V = 4, 8x8, keep_prob .75, size 3, fp32 storage with exact fp32 matrix arithmetic, training mode, random
    BatchNorm gammas / betas: output, dx and every variable's gradient against a float64 autograd restatement that takes the block's
    own patterns and percent_ones as constants.  Tolerance: the same block with keep_prob=None (the code path without the feature)
    against the same restatement gives the error of this arithmetic; the DropBlock run may reach 4x that, per tensor (four more
    roundings per path, un-fused BatchNorm backward kernels in place of the fused ones).  Both go to profiles/dropblock_parity.json."""
    from oracle.model_torch import Builder, Config
    v = BLOCK_VARIANTS[variant]
    cfg = Config(sk_ratio=v['sk_ratio'])
    gx = torch.Generator().manual_seed(11)
    x = torch.randn(4, 8, 8, v['cin'], generator=gx)
    b0 = Builder(cfg, seed=2, randomize_bn=True)
    with torch.no_grad():
        o0 = _block64(b0, x.permute(0, 3, 1, 2), 64, v['strides'], v['use_projection'], None)
    dy = torch.randn(tuple(o0.permute(0, 2, 3, 1).shape), generator=gx)
    params, state = b0.params, b0.state

    def reference(sites):
        p = OrderedDict((k, t.double().requires_grad_(True)) for k, t in params.items())
        s = OrderedDict((k, t.double()) for k, t in state.items())
        b = Builder(cfg, params=p, state=s, dtype=torch.float64)
        xi = x.double().permute(0, 3, 1, 2).requires_grad_(True)
        out = _block64(b, xi, 64, v['strides'], v['use_projection'], sites)
        (out * dy.double().permute(0, 3, 1, 2)).sum().backward()
        r = OrderedDict(out=out.detach().permute(0, 2, 3, 1), dx=xi.grad.permute(0, 2, 3, 1))
        for k, t in p.items():
            r['d ' + k] = t.grad
        return r

    got0, _ = _run_block(variant, None, params, state, x, dy)
    ref0 = reference(None)
    base = {k: _rel_l2(got0[k], ref0[k]) for k in ref0}
    got1, sites = _run_block(variant, 0.75, params, state, x, dy)
    ref1 = reference(sites)
    err = {k: _rel_l2(got1[k], ref1[k]) for k in ref1}
    for k in err:
        print('dropblock_block %-14s %-80s err=%.3e  keep_prob=None err=%.3e  ratio=%.2f' % (variant, k, err[k], base[k], err[k] / base[k]))
    path = os.path.join(ROOT, 'profiles', 'dropblock_parity.json')
    try:
        doc = json.load(open(path))
    except (OSError, ValueError):
        doc = {}
    doc[variant] = {k: dict(dropblock_rel_l2=err[k], no_dropblock_rel_l2=base[k]) for k in err}
    doc['_about'] = ('tests/test_gpu_dropblock.py::test_block_against_float64_autograd: relative L2 error against float64 autograd of '
                     'BottleneckBlock(64) with keep_prob=.75 / size 3 and of the same block with keep_prob=None; gate: 4x per tensor')
    with open(path, 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True)
    bad = {k: (err[k], base[k]) for k in err if not err[k] <= 4 * base[k]}
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ the network
_NET = {}


def _net_inputs():
    if 'inputs' not in _NET:
        g = torch.Generator().manual_seed(21)
        feats = [torch.rand(8, 32, 32, 6, generator=g).to(DEV) for _ in range(2)]
        labs = [{'labels': F.one_hot(torch.randint(0, 10, (8,), generator=g), 10).float().to(DEV)} for _ in range(2)]
        _NET['inputs'] = (feats, labs)
    return _NET['inputs']


def _fresh(argv, build=False):
    from simclr_amd import model as model_lib
    from simclr_amd.flags import FLAGS
    from simclr_amd.resnet import RT
    from simclr_amd.run import make_single_step
    FLAGS.reset()
    FLAGS.parse(['--resnet_depth=50', '--image_size=32', '--train_batch_size=8', '--nouse_blur', '--compute_dtype=f32'] + argv)
    RT.reset()
    RT.device = torch.device(DEV)
    RT.seed = 1234
    model = model_lib.Model(10)
    if build:
        with torch.no_grad():
            model(torch.zeros(2, 32, 32, 6, device=DEV), training=True)           # builds the variables (a restore needs them)
    opt = model_lib.build_optimizer(0.1)
    return model, opt, make_single_step(model, opt, None)


def _snapshot(model, opt):
    snap = {v.name: v.value.clone() for v in model.variables}
    snap.update({'momentum/' + v.name: opt.get_slot(v, 'Momentum').clone() for v in model._flat_order})
    return snap


def _sites(model):
    return [d for g in model.resnet_model.block_groups for b in g.layers if b.dropblock for d in b.dropblock]


DROP_ARGV = ['--dropblock_keep_probs=none,none,0.9,0.9', '--dropblock_size=3', '--dropblock_seed=2']


def _base_run():
    """Two steps with DropBlock in groups 3 and 4; a checkpoint is written after the first."""
    if 'base' in _NET:
        return _NET['base']
    from simclr_amd.checkpoint import Checkpoint, CheckpointManager
    from simclr_amd.flags import FLAGS
    from simclr_amd.resnet import RT
    feats, labs = _net_inputs()
    try:
        model, opt, step = _fresh(DROP_ARGV)
        losses, counts = [], []
        d = tempfile.mkdtemp(prefix='simclr_dropblock_')
        for i in range(2):
            out = step(feats[i], labs[i])
            torch.cuda.synchronize()
            losses.append(float(out['total_loss'].reshape(-1)[0]))
            grads = [v.grad for v in model._flat_order if v.grad is not None]
            assert len(grads) > 100 and all(bool(torch.isfinite(g).all()) for g in grads)
            counts.append([[int(c) for c in s.last_count.cpu()] for s in _sites(model)])
            if i == 0:
                CheckpointManager(Checkpoint(model=model, optimizer=opt), d, max_to_keep=2).save()
        _NET['base'] = dict(losses=losses, counts=counts, snap=_snapshot(model, opt), dir=d)
    finally:
        FLAGS.reset(); RT.reset()
    return _NET['base']


def test_network_two_steps_finite_and_repeatable():
    from simclr_amd.flags import FLAGS
    from simclr_amd.resnet import RT
    base = _base_run()
    assert all(math.isfinite(l) for l in base['losses'])
    assert len(base['counts'][0]) == 36
    assert all(0 < ones <= size for step in base['counts'] for ones, size in step)
    assert any(ones < size for ones, size in base['counts'][0])
    assert base['counts'][0] != base['counts'][1]                               # the step enters the key
    feats, labs = _net_inputs()
    try:
        model, opt, step = _fresh(DROP_ARGV)
        for i in range(2):
            step(feats[i], labs[i])
        torch.cuda.synchronize()
        snap = _snapshot(model, opt)
        counts = [[int(c) for c in s.last_count.cpu()] for s in _sites(model)]
    finally:
        FLAGS.reset(); RT.reset()
    assert counts == base['counts'][1]
    diff = [k for k in base['snap'] if not torch.equal(base['snap'][k], snap[k])]
    assert not diff, diff[:5]


def test_network_resume_continues_bitwise():
    from simclr_amd.checkpoint import try_restore_from_checkpoint
    from simclr_amd.flags import FLAGS
    from simclr_amd.resnet import RT
    base = _base_run()
    feats, labs = _net_inputs()
    try:
        model, opt, step = _fresh(DROP_ARGV, build=True)
        try_restore_from_checkpoint(model, opt, base['dir'])
        assert opt.iterations == 1
        step(feats[1], labs[1])
        torch.cuda.synchronize()
        snap = _snapshot(model, opt)
        counts = [[int(c) for c in s.last_count.cpu()] for s in _sites(model)]
    finally:
        FLAGS.reset(); RT.reset()
        shutil.rmtree(base['dir'], ignore_errors=True)
    assert counts == base['counts'][1]
    diff = [k for k in base['snap'] if not torch.equal(base['snap'][k], snap[k])]
    assert not diff, diff[:5]


def test_keep_probs_of_one_step_like_the_default():
    from simclr_amd.flags import FLAGS
    from simclr_amd.resnet import RT
    feats, labs = _net_inputs()
    snaps = []
    try:
        for argv in ([], ['--dropblock_keep_probs=1,1,1,1']):
            model, opt, step = _fresh(argv)
            assert not _sites(model)
            for i in range(2):
                step(feats[i], labs[i])
            torch.cuda.synchronize()
            snaps.append(_snapshot(model, opt))
    finally:
        FLAGS.reset(); RT.reset()
    diff = [k for k in snaps[0] if not torch.equal(snaps[0][k], snaps[1][k])]
    assert not diff, diff[:5]
