"""BYOL on the device (pytest -m gpu): the kernels of csrc/byol.hip through the C ABI and simclr_amd.ops against the restatement
tests/byol_reference.py (loss: float64; moving average: float32, bitwise), then the target network, the predictor, the step, run.main end
to end (metrics, resume, what other modes read from its checkpoint) and two replicas over gloo.

Gates: those of tests/test_gpu_barlow.py for the same arithmetic -- loss and cosine 1e-5 relative, gradients 2e-4 of the reference tensor's
maximum.  The moving average and everything that is a copy is compared bitwise."""
import ctypes
import glob
import json
import math
import os
import shutil
import socket

import numpy as np
import pytest
import torch

from tests.byol_reference import byol_loss, ema_f32, one_minus_tau_f32
from tests.gpu_checks import DEV, _res, structured_images

pytestmark = pytest.mark.gpu
GATE_LOSS, GATE_GRAD = 1e-5, 2e-4
B, SIZE, NCLS = 16, 32, 4


@pytest.fixture(autouse=True)
def _exact_f32_matmul():
    from simclr_amd import ops
    from simclr_amd.flags import FLAGS
    from simclr_amd.resnet import RT
    ops.set_f32_matmul('exact')
    yield
    FLAGS.reset()
    RT.reset()
    ops.set_f32_matmul('exact')


def _assert(results):
    for r in results:
        print('%-4s %-86s err=%.3e tol=%.3e' % ('ok' if r['ok'] else 'FAIL', r['name'], r['err'], r['tol']))
    bad = [r for r in results if not r['ok']]
    assert not bad, '\n'.join('%s err=%.3e tol=%.3e' % (r['name'], r['err'], r['tol']) for r in bad)


def _np(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


# ---------------------------------------------------------------------------------------------------------------- loss kernels
def _qt(b, D, seed):
    g = np.random.default_rng(seed)
    q = (g.standard_normal((2 * b, D)) * g.uniform(0.2, 5.0, (2 * b, 1))).astype(np.float32)
    t = (g.standard_normal((2 * b, D)) * g.uniform(0.2, 5.0, (2 * b, 1))).astype(np.float32)
    return q, t


@pytest.mark.parametrize('D', [64, 320, 8192])
@pytest.mark.parametrize('b', [1, 3, 5, 70])
def test_loss_kernels_vs_float64(b, D):
    """Odd row counts, partner rows in another workgroup, a wave with idle lanes (D = 64), the widest row; one zero q row; both scales;
    a second call is bitwise the first."""
    from simclr_amd import ops
    q, t = _qt(b, D, 100 * b + D)
    q[2 * b - 1] = 0.0                                    # the eps branch: finite loss, gradient 2e6 (qhat - that) / b
    qd, td = torch.from_numpy(q).to(DEV), torch.from_numpy(t).to(DEV)
    out, stats = ops.byol_fwd(qd, td)
    out = out.clone()
    res = []
    for scale in (1.0, 0.5):
        ref = byol_loss(q, t, grad_scale=scale)
        dq = ops.byol_bwd(qd, td, stats, scale)
        res += [_res('byol_grad b=%d D=%d scale=%g' % (b, D, scale), dq, ref['grad'], GATE_GRAD),
                _res('byol_grad zero row b=%d D=%d scale=%g' % (b, D, scale), dq[2 * b - 1], ref['grad'][2 * b - 1], GATE_GRAD)]
    res += [_res('byol_loss b=%d D=%d' % (b, D), out[0], ref['loss'], GATE_LOSS), _res('byol_cosine b=%d D=%d' % (b, D), out[1], ref['cosine'], 0, GATE_LOSS)]
    out2, stats2 = ops.byol_fwd(qd, td)
    dq2 = ops.byol_bwd(qd, td, stats2, 0.5)
    torch.cuda.synchronize()
    assert torch.equal(out2, out) and torch.equal(stats2, stats) and torch.equal(dq2, dq)
    assert bool(torch.isfinite(dq).all()) and float(dq[2 * b - 1].abs().max()) > 1e3 / b
    _assert(res)


@pytest.mark.parametrize('D', [64, 2048])
def test_near_converged_loss_keeps_its_digits(D):
    """t = q + 1e-3 randn: the loss is ~1e-6.  2 - 2 cos in fp32 misses this gate by orders of magnitude (tests/test_byol_reference.py);
    the kernel sums squared differences in double."""
    from simclr_amd import ops
    b = 16
    g = np.random.default_rng(D)
    q = g.standard_normal((2 * b, D)).astype(np.float32)
    t = np.roll((q + 1e-3 * g.standard_normal((2 * b, D))).astype(np.float32), b, axis=0)     # row r pairs with row r + b
    ref = byol_loss(q, t)
    assert 1e-7 < ref['loss'] < 1e-4
    qd, td = torch.from_numpy(q).to(DEV), torch.from_numpy(t).to(DEV)
    out, stats = ops.byol_fwd(qd, td)
    dq = ops.byol_bwd(qd, td, stats, 1.0)
    torch.cuda.synchronize()
    _assert([_res('byol_near_converged_loss D=%d' % D, out[0], ref['loss'], GATE_LOSS),
             _res('byol_near_converged_cosine D=%d' % D, out[1], ref['cosine'], 0, GATE_LOSS),
             _res('byol_near_converged_grad D=%d' % D, dq, ref['grad'], GATE_GRAD)])


def test_refusals_return_the_error_code_and_launch_nothing():
    from simclr_amd import ops
    from simclr_amd._lib import SimclrHipError, lib
    q, t = torch.zeros(8, 64, device=DEV), torch.ones(8, 64, device=DEV)
    out = torch.full((2,), 7.0, device=DEV)
    stats, rows = torch.full((8 * 4,), 7.0, device=DEV, dtype=torch.float64), torch.full((8 * 2,), 7.0, device=DEV, dtype=torch.float64)
    dq = torch.full((8, 64), 7.0, device=DEV)
    P = lambda x: ctypes.c_void_p(x.data_ptr())
    raw = lib()._dll
    cases = [(P(q), P(t), 4, 100), (P(q), P(t), 4, 32), (P(q), P(t), 4, 8256), (P(q), P(t), 0, 64), (P(q), P(t), -1, 64),
             (None, P(t), 4, 64), (P(q), None, 4, 64)]
    for a, c, b, D in cases:
        assert raw.simclr_byol_fwd(a, c, b, D, P(out), P(stats), P(rows), None) == 1, (b, D)
        assert 'byol_fwd' in lib().last_error()
        assert raw.simclr_byol_bwd(a, c, b, D, P(stats), 1.0, P(dq), None) == 1, (b, D)
    assert raw.simclr_byol_fwd(P(q), P(t), 4, 64, None, P(stats), P(rows), None) == 1
    assert raw.simclr_byol_bwd(P(q), P(t), 4, 64, None, 1.0, P(dq), None) == 1
    assert raw.simclr_byol_bwd(P(q), P(t), 4, 64, P(stats), 1.0, None, None) == 1
    tab = torch.zeros(3, dtype=torch.int64, device=DEV)
    assert raw.simclr_ema_multi_tensor(None, 1, P(tab), 1, 0.5, None) == 1
    assert raw.simclr_ema_multi_tensor(P(tab), 1, None, 1, 0.5, None) == 1
    assert raw.simclr_ema_multi_tensor(P(tab), 0, P(tab), 1, 0.5, None) == 1
    assert raw.simclr_ema_multi_tensor(P(tab), 1, P(tab), 0, 0.5, None) == 1
    assert raw.simclr_ema_multi_tensor(P(tab), 1, P(tab), 1, 1.5, None) == 1
    with pytest.raises(SimclrHipError, match='byol_fwd'):
        lib().byol_fwd(P(q), P(t), 0, 64, P(out), P(stats), P(rows), None)
    with pytest.raises(ValueError, match='one shape'):
        ops.byol_fwd(q, torch.zeros(8, 128, device=DEV))
    with pytest.raises(ValueError, match='multiples of 64'):
        ops.byol_fwd(torch.zeros(8, 100, device=DEV), torch.zeros(8, 100, device=DEV))
    with pytest.raises(ValueError, match='one size'):
        ops.EmaTables().run([torch.zeros(4, device=DEV)], [torch.zeros(5, device=DEV)], 0.5)
    torch.cuda.synchronize()
    for x in (out, stats, rows, dq):
        assert bool((x == 7.0).all())                     # nothing was written


# ---------------------------------------------------------------------------------------------------------------- EMA kernel
@pytest.mark.parametrize('tau', [0.996, 1.0, 0.0])
def test_ema_kernel_is_the_float32_restatement_bit_for_bit(tau):
    """Tensors below, at and above the 8192-element chunk, tails that are no multiple of 4, one tensor whose pointer is only 4-byte aligned
    (the scalar path); then a second launch on the first one's output."""
    from simclr_amd import ops
    g = np.random.default_rng(11)
    sizes = [1, 3, 8191, 8192, 8193, 3 * 8192 + 5, 8195]
    t_np = [(g.standard_normal(n) * g.uniform(0.1, 30.0)).astype(np.float32) for n in sizes]
    o_np = [(g.standard_normal(n) * g.uniform(0.1, 30.0)).astype(np.float32) for n in sizes]
    store = torch.from_numpy(np.concatenate([[0.0], t_np[-1]]).astype(np.float32)).to(DEV)
    ts = [torch.from_numpy(x).to(DEV) for x in t_np[:-1]] + [store[1:]]          # x[1:]: 4-byte aligned
    os_ = [torch.from_numpy(x).to(DEV) for x in o_np]
    assert ts[-1].data_ptr() % 16 == 4 and all(x.data_ptr() % 16 == 0 for x in ts[:-1] + os_)
    omt = float(np.float32(1.0 - tau))
    tables = ops.EmaTables()
    tables.run(ts, os_, omt)
    torch.cuda.synchronize()
    want = [ema_f32(a, c, omt) for a, c in zip(t_np, o_np)]
    for n, got, w in zip(sizes, ts, want):
        assert _np(got).tobytes() == w.tobytes(), 'first launch, %d elements' % n
    assert float(store[0]) == 0.0
    if tau == 1.0:
        assert all(_np(got).tobytes() == a.tobytes() for got, a in zip(ts, t_np))
    tables.run(ts, os_, omt)
    torch.cuda.synchronize()
    for n, got, w, c in zip(sizes, ts, want, o_np):
        assert _np(got).tobytes() == ema_f32(w, c, omt).tobytes(), 'second launch, %d elements' % n
    assert all(_np(got).tobytes() == c.tobytes() for got, c in zip(os_, o_np))       # the online side is read only


def test_ema_of_equal_tensors_changes_nothing():
    from simclr_amd import ops
    x = torch.randn(20000, generator=torch.Generator().manual_seed(2)).to(DEV) * 1e3
    t = x.clone()
    ops.EmaTables().run([t], [x], float(np.float32(0.004)))
    torch.cuda.synchronize()
    assert torch.equal(t, x)


# ---------------------------------------------------------------------------------------------------------------- target network
def _flags(**kw):
    from simclr_amd.flags import FLAGS
    FLAGS.reset()
    kw.setdefault('proj_out_dim', 64)
    kw.setdefault('byol_pred_hidden_dim', 128)
    kw.setdefault('contrastive_loss', 'byol')
    kw.setdefault('use_blur', False)
    FLAGS.update(resnet_depth=18, image_size=SIZE, compute_dtype='f32', f32_matmul='exact', train_batch_size=B, train_mode='pretrain',
                 train_steps=10, **kw)
    return FLAGS


def _fresh_runtime():
    from simclr_amd.resnet import RT
    RT.reset()
    RT.device = torch.device(DEV)
    return RT


def _batch(n=B, seed=31):
    g = torch.Generator().manual_seed(seed)
    images = structured_images(n, SIZE, 2, g)
    ids = torch.randint(0, NCLS, (n,), generator=g)
    return images, ids


def _build(steps=10, strategy=None, lr=0.1):
    from simclr_amd import model as model_lib
    from simclr_amd.run import make_single_step
    model = model_lib.Model(NCLS)
    target = model_lib.TargetNetwork(model, steps)
    opt = model_lib.build_optimizer(lr)
    return model, target, opt, make_single_step(model, opt, strategy, target=target)


def _values(variables):
    return {v.name: v.value.detach().clone() for v in variables}


def test_target_is_a_bitwise_copy_and_the_online_model_is_the_ntxent_model():
    from simclr_amd import model as model_lib
    _flags(contrastive_loss='ntxent')
    _fresh_runtime()
    plain = model_lib.Model(NCLS)
    plain(torch.zeros(2, SIZE, SIZE, 3, device=DEV), training=False)
    plain_values = _values(plain.variables)
    _flags()
    _fresh_runtime()
    model, target, opt, step = _build()
    online = _values(model.variables)
    assert [n for n in online if 'prediction_head' not in n] == list(plain_values)
    assert all(torch.equal(online[n], plain_values[n]) for n in plain_values)
    assert sum('prediction_head' in n for n in online) == 6
    tv = _values(target.variables)
    assert list(tv) == [n for n in plain_values if 'head_supervised' not in n] and len(tv) > 60
    assert all(torch.equal(tv[n], online[n]) for n in tv)
    # nothing of the target trains
    names = {v.name for v in model.trainable_variables}
    assert target.model.trainable_variables == [] and target.model.supervised_head is None and target.model.prediction_head is None
    assert all(id(v) not in {id(o) for o in model.variables} for v in target.variables)
    assert all(v.value.data_ptr() not in {o.value.data_ptr() for o in model.variables} for v in target.variables)
    assert any('prediction_head' in n for n in names)


def test_one_step_moves_the_target_by_the_moving_average_and_touches_nothing_else_of_it():
    """EMA after a step (bitwise), isolation (no gradient, no slot, no weight decay), no activation kept, the metric set."""
    from simclr_amd import model as model_lib
    FLAGS = _flags()
    _fresh_runtime()
    model, target, opt, step = _build(steps=10)
    assert sorted(step.metrics) == ['train/byol_cosine', 'train/contrast_loss', 'train/supervised_acc', 'train/supervised_loss',
                                    'train/total_loss', 'train/weight_decay']
    before_t, before_o = _values(target.variables), _values(model.variables)
    images, ids = _batch()
    out = step(images.to(DEV), {'labels': torch.nn.functional.one_hot(ids, NCLS).float().to(DEV)})
    torch.cuda.synchronize()
    after_o = _values(model.variables)
    omt = one_minus_tau_f32(0, 10, FLAGS.byol_tau_base)
    assert omt == np.float32(1.0 - 0.996)
    trained = {v.name for v in model.trainable_variables}
    moved = changed = own = 0
    for v in target.variables:
        if v.name in trained:
            # (zero-initialised last gammas cut the residual branches at step 0: the variables inside them have an exactly zero gradient)
            changed += int(not torch.equal(after_o[v.name], before_o[v.name]))
            want = ema_f32(_np(before_t[v.name]), _np(after_o[v.name]), omt)
            assert _np(v.value).tobytes() == want.tobytes(), v.name
            moved += int(not torch.equal(v.value, before_t[v.name]))
        else:
            # the target's own statistics: no average touches them, its training forward moved them
            assert 'moving_' in v.name
            assert not torch.equal(v.value, before_t[v.name]), v.name
            own += 1
    assert changed >= 20 and moved == changed and own >= 40
    # isolation
    assert all(v.grad is None for v in target.variables)
    assert all(id(v) not in opt._slots for v in target.variables) and len(opt._slots) == len(model.trainable_variables)
    flat = {id(v) for v in model._flat_order}
    assert all(id(v) not in flat for v in target.variables)
    for v in model.variables:                  # the step's weight decay was formed on the values before it
        v.value.copy_(before_o[v.name])
    wd_before = model_lib.add_weight_decay(model, adjust_per_optimizer=True)
    torch.cuda.synchronize()
    assert float(out['weight_decay']) == float(wd_before) and float(wd_before) > 0.0
    # nothing kept
    for l in model_lib._all_layers(target.model):
        for a in ('saved', 'out', 'relu_bits'):
            assert getattr(l, a, None) is None, (type(l).__name__, a)
    assert target.model.resnet_model.endpoints == {} and target.model.resnet_model._final is None
    # metrics
    con = out['con_loss']
    m = step.metrics
    assert m['train/byol_cosine'].result() == float(con.cosine) and m['train/contrast_loss'].result() == float(con.value)
    assert -1.0 <= float(con.cosine) <= 1.0 and 0.0 <= float(con.value) <= 8.0
    assert abs(float(con.value) - 2.0 * (2.0 - 2.0 * float(con.cosine))) <= 1e-4
    assert out['logits_con'] is None
    assert all(bool(torch.isfinite(x).all()) for x in after_o.values())
    assert all(bool(torch.isfinite(v.value).all()) for v in target.variables)


def test_step_with_the_imagenet_stem():
    """64 px: the 7x7 stem with BN + ReLU + max-pool fused, which a frozen stem runs without keeping the pooling tap ids -- the path the
    target takes at 224 px.  The moving average after the step is again the restatement's, bit for bit."""
    from simclr_amd.flags import FLAGS
    _flags()
    FLAGS.update(image_size=64, train_batch_size=8)
    _fresh_runtime()
    model, target, opt, step = _build(steps=10)
    rm = target.model.resnet_model
    assert not rm.cifar_stem and not rm.stem_trainable and model.resnet_model.stem_trainable
    before_t = _values(target.variables)
    g = torch.Generator().manual_seed(5)
    images = structured_images(8, 64, 2, g).to(DEV)
    ids = torch.randint(0, NCLS, (8,), generator=g)
    out = step(images, {'labels': torch.nn.functional.one_hot(ids, NCLS).float().to(DEV)})
    torch.cuda.synchronize()
    assert rm._pool is None and rm.endpoints == {} and rm.stem_conv.saved is None and rm.stem_bn.saved is None
    assert math.isfinite(float(out['con_loss'].value)) and -1.0 <= float(out['con_loss'].cosine) <= 1.0
    online = {v.name: v for v in model.variables}
    trained = {v.name for v in model.trainable_variables}
    omt = one_minus_tau_f32(0, 10, FLAGS.byol_tau_base)
    for v in target.variables:
        assert bool(torch.isfinite(v.value).all()), v.name
        if v.name in trained:
            assert _np(v.value).tobytes() == ema_f32(_np(before_t[v.name]), _np(online[v.name].value), omt).tobytes(), v.name


def test_both_networks_see_the_same_blurred_pixels(monkeypatch):
    from simclr_amd import model as model_lib
    _flags(use_blur=True)
    _fresh_runtime()
    model, target, opt, step = _build()
    seen = []
    orig = model_lib.PackedInput

    def packed(images, *a, **kw):
        seen.append(images.detach().clone())
        return orig(images, *a, **kw)
    monkeypatch.setattr(model_lib, 'PackedInput', packed)
    images, ids = _batch()
    images = images.to(DEV)
    step(images, {'labels': torch.nn.functional.one_hot(ids, NCLS).float().to(DEV)})
    torch.cuda.synchronize()
    assert len(seen) == 2 and torch.equal(seen[0], seen[1])
    assert not torch.equal(seen[0], images)               # and they are blurred


def _fresh_frozen_copy(target):
    """A newly built frozen model of the target's configuration, loaded with the target's master weights."""
    from simclr_amd import model as model_lib
    from simclr_amd.flags import FLAGS
    from simclr_amd.resnet import RT
    with FLAGS.override(**model_lib.target_flag_values()), RT.fresh_names():
        fresh = model_lib.Model(0)
        fresh.trainable = False
        fresh.resnet_model.stem_trainable = False
        fresh(torch.zeros(2, SIZE, SIZE, 3, device=DEV), training=False)
        fresh.release()
    src = {v.name: v.value for v in target.variables}
    for v in fresh.variables:
        v.value.copy_(src[v.name])
    RT.weights_version += 1             # a change of unknown scope: every compute copy in the process is rebuilt from its master
    return fresh


def test_target_compute_copies_follow_the_moving_average():
    """After two steps the target's output is that of a freshly built frozen model holding the target's master weights -- not that of
    its step-0 compute copies."""
    from simclr_amd import model as model_lib
    from simclr_amd.flags import FLAGS
    _flags(byol_tau_base=0.5)                              # a large step of the average: stale copies could not hide in the rounding
    _fresh_runtime()
    model, target, opt, step = _build(lr=0.5)
    images, ids = _batch()
    labels = {'labels': torch.nn.functional.one_hot(ids, NCLS).float().to(DEV)}
    fixed = _batch(seed=77)[0].to(DEV)
    y0 = target(fixed).clone()
    for _ in range(2):
        step(images.to(DEV), labels)
    y_target = target(fixed).clone()
    torch.cuda.synchronize()
    fresh = _fresh_frozen_copy(target)
    with FLAGS.override(**model_lib.target_flag_values()):
        y_fresh, _ = fresh(fixed, training=True, blur=False)
    torch.cuda.synchronize()
    assert torch.equal(y_target, y_fresh)
    assert not torch.equal(y_target, y0)


# ---------------------------------------------------------------------------------------------------------------- predictor
@pytest.mark.parametrize('hidden', [64, 128])
def test_predictor_vs_float64_autograd(hidden):
    from simclr_amd import model as model_lib
    from simclr_amd import ops
    _flags(byol_pred_hidden_dim=hidden)
    _fresh_runtime()
    model = model_lib.Model(NCLS)
    g = torch.Generator().manual_seed(hidden)
    x = torch.randn(2 * B, 64, generator=g)
    dq = torch.randn(2 * B, 64, generator=g) * 0.1
    ops.begin_step(torch.device(DEV))
    q = model.predict(x.to(DEV), training=True)
    l0, l1 = model.prediction_head.linear_layers
    # the initial kernels (stddev 0.01) scaled up, so that the BatchNorm's epsilon does not dominate its variance
    l0.kernel.value.mul_(30.0)
    l1.kernel.value.mul_(30.0)
    from simclr_amd.resnet import RT
    RT.weights_version += 1
    q = model.predict(x.to(DEV), training=True).clone()
    d_proj = model.backward_predictor(dq.to(DEV)).clone()
    ops.end_step()
    torch.cuda.synchronize()
    assert tuple(l0.kernel.shape) == (64, hidden) and tuple(l1.kernel.shape) == (hidden, 64) and l1.bias is None and l0.bias is None
    xr = x.double().requires_grad_(True)
    w0 = l0.kernel.value.detach().cpu().double().requires_grad_(True)
    w1 = l1.kernel.value.detach().cpu().double().requires_grad_(True)
    gamma = torch.ones(hidden, dtype=torch.float64, requires_grad=True)
    beta = torch.zeros(hidden, dtype=torch.float64, requires_grad=True)
    y = xr @ w0
    yh = (y - y.mean(0)) / torch.sqrt(y.var(0, unbiased=False) + 1e-5) * gamma + beta
    qr = torch.relu(yh) @ w1
    qr.backward(dq.double())
    _assert([_res('predictor_q hidden=%d' % hidden, q, qr, GATE_GRAD), _res('predictor_d_proj hidden=%d' % hidden, d_proj, xr.grad, GATE_GRAD),
             _res('predictor_dw0 hidden=%d' % hidden, l0.kernel.grad, w0.grad, GATE_GRAD),
             _res('predictor_dw1 hidden=%d' % hidden, l1.kernel.grad, w1.grad, GATE_GRAD),
             _res('predictor_dgamma hidden=%d' % hidden, l0.bn_relu.gamma.grad, gamma.grad, GATE_GRAD),
             _res('predictor_dbeta hidden=%d' % hidden, l0.bn_relu.beta.grad, beta.grad, GATE_GRAD)])


# ---------------------------------------------------------------------------------------------------------------- step
def _capture(setattr_fn, model):
    """Records what the step hands the loss and what it hands the predictor's backward (the layer below the loss)."""
    from simclr_amd import objective as obj_lib
    box = {}
    orig_loss, orig_backward = obj_lib.add_byol_loss, model.backward_predictor

    def loss_fn(online, target, *a, **kw):
        box['q'], box['t'] = online.detach().clone(), target.detach().clone()
        box['loss'] = orig_loss(online, target, *a, **kw)
        return box['loss']

    def backward(dq):
        box['dq'] = dq.detach().clone()
        return orig_backward(dq)
    setattr_fn(obj_lib, 'add_byol_loss', loss_fn)
    setattr_fn(model, 'backward_predictor', backward)
    return box


@pytest.mark.parametrize('head_mode,width', [('nonlinear', 64), ('none', 512)])
def test_step_hands_the_predictor_the_reference_gradient(monkeypatch, head_mode, width):
    _flags(proj_head_mode=head_mode)
    _fresh_runtime()
    model, target, opt, step = _build()
    box = _capture(monkeypatch.setattr, model)
    images, ids = _batch()
    out = step(images.to(DEV), {'labels': torch.nn.functional.one_hot(ids, NCLS).float().to(DEV)})
    torch.cuda.synchronize()
    assert tuple(box['q'].shape) == tuple(box['t'].shape) == (2 * B, width)
    ref = byol_loss(_np(box['q']), _np(box['t']))
    con = out['con_loss']
    _assert([_res('step_loss', con.value, ref['loss'], GATE_LOSS), _res('step_cosine', con.cosine, ref['cosine'], 0, GATE_LOSS),
             _res('step_dq', box['dq'], ref['grad'], GATE_GRAD)])
    assert step.metrics['train/byol_cosine'].result() == float(con.cosine)
    assert all(bool(torch.isfinite(v.value).all()) for v in model.variables + target.variables)


# ---------------------------------------------------------------------------------------------------------------- run.main
ARGS = ['--dataset=synthetic', '--resnet_depth=18', '--image_size=32', '--train_batch_size=8', '--use_blur=False', '--compute_dtype=f32',
        '--checkpoint_steps=2', '--train_steps=3', '--mode=train', '--proj_out_dim=64', '--byol_pred_hidden_dim=64']


def test_run_main_trains_logs_and_resumes_bitwise(tmp_path, capsys):
    from simclr_amd import run
    from simclr_amd.checkpoint import INDEX_NAME
    from simclr_amd.flags import FLAGS
    args = ARGS + ['--contrastive_loss=byol']
    full_dir, again_dir = str(tmp_path / 'full'), str(tmp_path / 'again')
    FLAGS.reset()
    run.main(args + ['--model_dir=' + full_dir])
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith('{') and 'train/byol_cosine' in l]
    assert lines and lines[0]['step'] == 2
    for k in ('train/contrast_loss', 'train/byol_cosine', 'train/total_loss'):
        assert math.isfinite(lines[0][k]), (k, lines[0])
    assert -1.0 <= lines[0]['train/byol_cosine'] <= 1.0
    assert not any(k in lines[0] for k in ('train/contrast_entropy', 'train/contrast_acc', 'train/align_loss', 'train/bt_on_diag',
                                           'train/contrast_positives'))
    full = torch.load(os.path.join(full_dir, 'ckpt-3.pt'), map_location='cpu')
    target_names = [n for n in full['model'] if n.startswith('target/')]
    assert len(target_names) > 60 and all(n[len('target/'):] in full['model'] for n in target_names)
    assert sum('prediction_head' in n for n in full['model']) == 6
    assert any(not torch.equal(full['model'][n], full['model'][n[len('target/'):]]) for n in target_names)
    assert not any(n.startswith('target/') for n in full['optimizer']['slots'])
    os.makedirs(again_dir)
    shutil.copy(os.path.join(full_dir, 'ckpt-2.pt'), os.path.join(again_dir, 'ckpt-2.pt'))
    with open(os.path.join(again_dir, INDEX_NAME), 'w') as f:
        json.dump({'model_checkpoint_path': 'ckpt-2.pt', 'all_model_checkpoint_paths': ['ckpt-2.pt']}, f)
    FLAGS.reset()
    run.main(args + ['--model_dir=' + again_dir])
    again = torch.load(os.path.join(again_dir, 'ckpt-3.pt'), map_location='cpu')
    assert sorted(again['model']) == sorted(full['model'])
    assert all(torch.equal(again['model'][n], full['model'][n]) for n in full['model'])
    assert all(torch.equal(again['optimizer']['slots'][n], full['optimizer']['slots'][n]) for n in full['optimizer']['slots'])
    assert again['optimizer']['iterations'] == full['optimizer']['iterations'] == 3
    assert len(glob.glob(os.path.join(again_dir, 'ckpt-*.pt'))) == 2


def test_other_modes_read_a_byol_checkpoint_as_a_plain_one_and_other_losses_write_no_new_names(tmp_path, monkeypatch, capsys):
    """run.main itself: --train_mode=finetune --checkpoint=<BYOL file> starts from the online encoder and builds no target network;
    --mode=eval with --knn_eval reads the file with --contrastive_loss=byol still on the command line (the predictor is constructed and
    never built); an ntxent run's checkpoint has none of the new names."""
    from simclr_amd import checkpoint as ckpt_lib
    from simclr_amd import model as model_lib
    from simclr_amd import run
    from simclr_amd.flags import FLAGS
    byol_dir, plain_dir, ft_dir = str(tmp_path / 'byol'), str(tmp_path / 'plain'), str(tmp_path / 'ft')
    FLAGS.reset()
    run.main(ARGS + ['--contrastive_loss=byol', '--train_steps=2', '--model_dir=' + byol_dir])
    FLAGS.reset()
    run.main(ARGS + ['--train_steps=2', '--model_dir=' + plain_dir])
    plain = torch.load(os.path.join(plain_dir, 'ckpt-2.pt'), map_location='cpu')
    assert not any(n.startswith('target/') or 'prediction_head' in n for n in plain['model'])
    path = os.path.join(byol_dir, 'ckpt-2.pt')
    held = torch.load(path, map_location='cpu')['model']
    extra = {n for n in held if n.startswith('target/') or 'prediction_head' in n}
    assert len(extra) > 60

    # fine-tuning from that file
    seen = {}
    orig = ckpt_lib.try_restore_from_checkpoint

    def restore(model, *a, **kw):
        manager, status = orig(model, *a, **kw)
        seen['model'], seen['status'] = model, status
        seen['values'] = {v.name: v.value.detach().cpu().clone() for v in model.variables}
        return manager, status

    def no_target(*a, **kw):
        raise AssertionError('a target network was built outside BYOL pretraining')
    monkeypatch.setattr(ckpt_lib, 'try_restore_from_checkpoint', restore)
    monkeypatch.setattr(model_lib, 'TargetNetwork', no_target)
    FLAGS.reset()
    run.main(['--dataset=synthetic', '--resnet_depth=18', '--image_size=32', '--train_batch_size=8', '--compute_dtype=f32', '--mode=train',
              '--train_mode=finetune', '--contrastive_loss=byol', '--proj_out_dim=64', '--train_steps=1', '--checkpoint_steps=1',
              '--checkpoint=' + path, '--model_dir=' + ft_dir])
    assert isinstance(seen['model'], model_lib.Model) and seen['model'].prediction_head is None
    enc = [n for n in seen['values'] if n.startswith('model/resnet/')]
    assert len(enc) > 60 and all(torch.equal(seen['values'][n], held[n]) for n in enc)
    assert any(not torch.equal(held[n], held['target/' + n]) for n in enc)            # the online values, not the target's
    assert extra <= set(seen['status'].unused_in_checkpoint)
    assert not any(n.startswith('model/resnet/') for n in seen['status'].unused_in_checkpoint)
    written = torch.load(os.path.join(ft_dir, 'ckpt-1.pt'), map_location='cpu')['model']
    assert not any(n.startswith('target/') or 'prediction_head' in n for n in written)
    monkeypatch.setattr(ckpt_lib, 'try_restore_from_checkpoint', orig)

    # evaluation and the k-NN evaluation of that run's directory, the loss flag left on
    capsys.readouterr()
    FLAGS.reset()
    result = run.main(['--dataset=synthetic', '--resnet_depth=18', '--image_size=32', '--eval_batch_size=8', '--eval_steps=1',
                       '--compute_dtype=f32', '--mode=eval', '--contrastive_loss=byol', '--proj_out_dim=64', '--byol_pred_hidden_dim=64',
                       '--knn_eval=True', '--knn_k=5', '--model_dir=' + byol_dir])
    assert result['global_step'] == 2
    for k in ('eval/label_top_1_accuracy', 'eval/knn_top_1_accuracy'):
        assert 0.0 <= result[k] <= 1.0, (k, result)


# ---------------------------------------------------------------------------------------------------------------- two replicas
KEEP = 4096        # leading elements of every variable the replicas report


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _weights(variables):
    return {v.name: _np(v.value.reshape(-1)[:KEEP]).copy() for v in variables}


def _worker(rank, world, port, q):
    try:
        import torch.distributed as dist
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        torch.cuda.set_device(0)
        dist.init_process_group('gloo', rank=rank, world_size=world)
        from simclr_amd import comm, ops
        ops.set_f32_matmul('exact')
        FLAGS = _flags()
        FLAGS.update(train_batch_size=world * B)
        RT = _fresh_runtime()
        strategy = comm.Strategy()
        RT.strategy = strategy
        model, target, opt, step = _build(strategy=strategy)
        attrs = {}
        box = _capture(lambda o, name, v: (attrs.setdefault((id(o), name), (o, name, getattr(o, name))), setattr(o, name, v)), model)
        images, ids = _batch(world * B, seed=51)
        out = step(images[rank * B:(rank + 1) * B].to(DEV), {'labels': ids[rank * B:(rank + 1) * B].to(DEV)})
        torch.cuda.synchronize()
        res = dict(q=_np(box['q']), t=_np(box['t']), dq=_np(box['dq']), loss=float(out['con_loss'].value),
                   cosine=float(out['con_loss'].cosine), weights=_weights(model.variables), target=_weights(target.variables))
        for o, name, v in attrs.values():
            setattr(o, name, v)
        dist.destroy_process_group()
        q.put((rank, 'ok', res))
    except Exception:  # noqa
        import traceback
        q.put((rank, 'FAIL', traceback.format_exc()))


def test_two_replica_step_vs_the_one_replica_step_on_the_gathered_batch():
    """Two gloo ranks sharing one GPU.  Each rank's loss and the gradient it hands its predictor equal the restatement on its OWN blocks
    with grad_scale 1 / 2 (no collective in the loss); the mean of the two loss values, the online weights and the target weights after
    the step agree with ONE replica's step on the gathered batch within the gradient gate."""
    import torch.multiprocessing as mp
    os.environ['SIMCLR_PEER_STATS'] = '0'          # the statistics travel over gloo (the peer-mapped exchange has its own tests)
    os.environ['SIMCLR_SHARE_GPU'] = '1'
    try:
        ctx = mp.get_context('spawn')
        q = ctx.Queue()
        port = _free_port()
        procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
        for p in procs:
            p.start()
        res = [q.get(timeout=600) for _ in procs]
        for p in procs:
            p.join(timeout=60)
    finally:
        os.environ.pop('SIMCLR_PEER_STATS', None)
        os.environ.pop('SIMCLR_SHARE_GPU', None)
    assert all(r[1] == 'ok' for r in res), res
    boxes = [r[2] for r in sorted(res, key=lambda r: r[0])]
    out = []
    for r, b in enumerate(boxes):
        ref = byol_loss(b['q'], b['t'], grad_scale=0.5)
        out += [_res('two_replica_loss rank %d' % r, b['loss'], ref['loss'], GATE_LOSS),
                _res('two_replica_cosine rank %d' % r, b['cosine'], ref['cosine'], 0, GATE_LOSS),
                _res('two_replica_dq rank %d' % r, b['dq'], ref['grad'], GATE_GRAD)]
    # one replica, the gathered batch, the same initial weights (the initialisation is a function of the seed alone)
    FLAGS = _flags()
    FLAGS.update(train_batch_size=2 * B)
    _fresh_runtime()
    model, target, opt, step = _build()
    images, ids = _batch(2 * B, seed=51)
    one = step(images.to(DEV), {'labels': ids.to(DEV)})
    torch.cuda.synchronize()
    after, after_t = _weights(model.variables), _weights(target.variables)
    out.append(_res('two_replica_loss_mean vs one replica', 0.5 * (boxes[0]['loss'] + boxes[1]['loss']), float(one['con_loss'].value), GATE_GRAD))
    def atol(name, ref):
        # ONE statistic is mathematically zero: the predictor's first dense layer reads the projection head's last BatchNorm, which has
        # no ReLU and beta = 0 at step 0, so every column of its input sums to zero over the (global) batch and so does every column of
        # its output.  Its moving mean is rounding noise (~1e-9), and a gate relative to that would compare noise with noise: it is
        # gated against the spread of the activations it averages, sqrt(moving variance) of the same layer.
        if not ('prediction_head' in name and name.endswith('moving_mean:0')):
            return 0.0            # every other variable, the target's included: the gradient gate alone
        return GATE_GRAD * float(np.sqrt(np.abs(ref[name.replace('moving_mean', 'moving_variance')]).max()))
    for r, b in enumerate(boxes):
        for name in sorted(after):
            out.append(_res('two_replica_weights rank %d %s' % (r, name), b['weights'][name], after[name], GATE_GRAD, atol(name, after)))
        for name in sorted(after_t):
            out.append(_res('two_replica_target rank %d %s' % (r, name), b['target'][name], after_t[name], GATE_GRAD, atol(name, after_t)))
    _assert(out)
