"""DINO self-distillation on the device (pytest -m gpu): the kernels of csrc/dino.hip through the C ABI and simclr_amd.ops against the
float64 restatement tests/dino_reference.py, then the prototype head, the target network with its centre, the step, run.main end to
end (metrics, resume, what other modes read from its checkpoint) and two replicas over gloo.

Gates: the project's for this arithmetic (tests/test_gpu_moco.py) -- loss and entropy 1e-5 relative, gradients 2e-4 of the reference
tensor's maximum; tests/test_dino_reference.py shows that no case of CASES needs the 4x-emulation rule.  Copies and repeated calls are
compared bitwise."""
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

from tests.byol_reference import ema_f32
from tests.dino_reference import (CASES, GATE_GRAD, GATE_LOSS, case_gates, case_inputs, center_blend_f32, center_update, dino_loss,
                                  dino_loss_normalized, l2_normalize, last_layer_frozen, teacher_temp)
from tests.gpu_checks import DEV, _res, structured_images

pytestmark = pytest.mark.gpu
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


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)


# ---------------------------------------------------------------------------------------------------------------- loss kernels
def _run_kernels(qh, kh, ws, wt, c, Ts, Tt, scales=(1.0, 0.5), tag='', gates=None):
    """Forward, both backward sweeps at every scale and a second call (bitwise) against the float64 restatement on the same float32
    rows."""
    from simclr_amd import ops
    gates = gates or {}
    gate = lambda name, project: gates.get(name, (project,))[0]
    qd, kd, wsd, wtd, cd = _dev(qh), _dev(kh), _dev(ws), _dev(wt), _dev(c)
    out, stats, u, wsp = ops.dino_fwd(qd, kd, wsd, wtd, cd, Ts, Tt)
    out, u = out.clone(), u.clone()
    res = []
    for scale in scales:
        ref = dino_loss_normalized(qh, kh, ws, wt, c, Ts, Tt, grad_scale=scale)
        dq = ops.dino_bwd_q(qd, wsd, u, Ts, stats, scale, wsp)
        dw = ops.dino_bwd_w(qd, kd, wsd, wtd, cd, Ts, Tt, stats, scale, wsp)
        res += [_res('dino_grad_q %s scale=%g' % (tag, scale), dq, ref['grad_q'], gate('grad_q', GATE_GRAD)),
                _res('dino_grad_ws %s scale=%g' % (tag, scale), dw, ref['grad_ws'], gate('grad_ws', GATE_GRAD))]
    log2e = 1.4426950408889634
    res += [_res('dino_loss %s' % tag, out[0], ref['loss'], gate('loss', GATE_LOSS)),
            _res('dino_entropy %s' % tag, out[1], ref['entropy'], gate('entropy', GATE_LOSS)),
            _res('dino_u %s' % tag, u, ref['u'], gate('u', GATE_GRAD)),
            _res('dino_lse_s %s' % tag, stats[:, 0], ref['lse_s'] * log2e, GATE_LOSS),
            _res('dino_lse_t %s' % tag, stats[:, 1], ref['lse_t'] * log2e, GATE_LOSS)]
    out2, stats2, u2, wsp2 = ops.dino_fwd(qd, kd, wsd, wtd, cd, Ts, Tt)
    dq2 = ops.dino_bwd_q(qd, wsd, u2, Ts, stats2, scales[-1], wsp2)
    dw2 = ops.dino_bwd_w(qd, kd, wsd, wtd, cd, Ts, Tt, stats2, scales[-1], wsp2)
    torch.cuda.synchronize()
    assert torch.equal(out2, out) and torch.equal(stats2, stats) and torch.equal(u2, u), 'a second forward is not bitwise the first'
    assert torch.equal(dq2, dq) and torch.equal(dw2, dw), 'a second backward is not bitwise the first'
    for x in (out, u, dq, dw, stats):
        assert bool(torch.isfinite(x).all())
    return res, ref, out, dq, dw


@pytest.mark.parametrize('b,K,D,Ts,Tt', CASES)
def test_kernels_vs_float64(b, K, D, Ts, Tt):
    from simclr_amd import ops
    qh, kh, ws, wt, c = case_inputs(b, K, D, Ts, Tt)
    assert np.abs(c).max() > 0.0                                           # a non-zero centre
    if K == 4097:
        assert ops.dino_key_splits(2 * b, K) > 1 and K % 64 != 0          # several key splits, the last tile ragged
    if (b, K) == (33, 2):
        # the smallest b whose key-side sweep has more than one row split: 2b > 64 rows against one prototype tile
        assert ops.dino_row_splits(2 * b, K) == 2 and ops.dino_row_splits(2 * (b - 1), K) == 1
    res, ref, _, _, _ = _run_kernels(qh, kh, ws, wt, c, Ts, Tt, tag='b=%d K=%d D=%d Ts=%g Tt=%g' % (b, K, D, Ts, Tt),
                                     gates=case_gates(b, K, D, Ts, Tt))
    assert 0.0 < ref['loss'] and np.abs(ref['grad_q']).max() > 0.0 and np.abs(ref['grad_ws']).max() > 0.0
    _assert(res)


def test_splits_follow_the_shape():
    from simclr_amd import ops
    assert ops.dino_key_splits(2, 2) == 1 and ops.dino_key_splits(2, 64) == 1 and ops.dino_key_splits(2, 65) == 2
    assert ops.dino_key_splits(1024, 65536) > 1
    assert ops.dino_row_splits(64, 2) == 1 and ops.dino_row_splits(66, 2) == 2 and ops.dino_row_splits(1024, 65536) == 1
    for two_n, K in ((0, 64), (3, 64), (2, 1)):
        with pytest.raises(ValueError, match='even two_n'):
            ops.dino_key_splits(two_n, K)
        with pytest.raises(ValueError, match='even two_n'):
            ops.dino_row_splits(two_n, K)


def near_one_hot():
    """K = 65, Tt = 0.04: prototype 7 of the target table equals row 0's key, so that row's best logit leads the rest by ~ 1 / Tt."""
    b, K, D = 3, 65, 64
    qh, kh, ws, wt, c = case_inputs(b, K, D, 0.1, 0.04)
    wt = wt.copy()
    wt[7] = kh[0]
    return qh, kh, ws, wt, np.zeros(K, np.float32)


def test_near_one_hot_teacher_entropy_keeps_its_digits():
    qh, kh, ws, wt, c = near_one_hot()
    res, ref, out, _, _ = _run_kernels(qh, kh, ws, wt, c, 0.1, 0.04, tag='near one-hot')
    assert ref['row_entropy'][0] < 1e-4 * ref['row_entropy'][1:].min()      # the row the entropy metric exists to show
    assert math.isfinite(float(out[1])) and float(out[1]) > 0.0
    _assert(res)
    # that row alone: a batch whose every key is the prototype
    kh1 = np.repeat(kh[:1], 2, axis=0)
    res1, ref1, out1, _, _ = _run_kernels(qh[:2], kh1, ws, wt, c, 0.1, 0.04, tag='one-hot rows only')
    assert 0.0 < ref1['entropy'] < 1e-6
    _assert(res1)


def test_identical_networks_have_zero_gradient():
    """Student = teacher (same rows, same prototypes, Ts = Tt, c = 0): every view's teacher distribution is its own student
    distribution when both views are the same rows -- the loss is the teacher entropy and both gradients vanish."""
    b, K, D = 33, 200, 64
    g = np.random.default_rng(5)
    half = l2_normalize(g.standard_normal((b, D)))[0].astype(np.float32)
    qh = np.concatenate([half, half])
    ws = l2_normalize(g.standard_normal((K, D)))[0].astype(np.float32)
    c = np.zeros(K, np.float32)
    from simclr_amd import ops
    qd, wd, cd = _dev(qh), _dev(ws), _dev(c)
    out, stats, u, wsp = ops.dino_fwd(qd, qd, wd, wd, cd, 0.1, 0.1)
    dq = ops.dino_bwd_q(qd, wd, u, 0.1, stats, 1.0, wsp)
    dw = ops.dino_bwd_w(qd, qd, wd, wd, cd, 0.1, 0.1, stats, 1.0, wsp)
    ref = dino_loss_normalized(qh, qh, ws, ws, c, 0.1, 0.1)
    assert abs(ref['loss'] - ref['entropy']) < 1e-12 and np.abs(ref['grad_q']).max() < 1e-15
    # the scale a gradient of this shape has when the two sides differ: the teacher at another temperature
    other = dino_loss_normalized(qh, qh, ws, ws, c, 0.1, 0.04)
    _assert([_res('identical loss == entropy', out[0], ref['entropy'], GATE_LOSS), _res('identical entropy', out[1], ref['entropy'], GATE_LOSS),
             _res('identical grad_q ~ 0', dq, ref['grad_q'], 0, GATE_GRAD * np.abs(other['grad_q']).max()),
             _res('identical grad_ws ~ 0', dw, ref['grad_ws'], 0, GATE_GRAD * np.abs(other['grad_ws']).max())])


@pytest.mark.parametrize('K', [200, 4097])
def test_center_kernel_vs_the_column_mean(K):
    """w^t . kbar against the float64 column mean of the logits, then the fp32 blend bit for bit on the kernel's own fp32 dot product."""
    from simclr_amd import ops
    D, rows, m = 128, 70, 0.9
    g = np.random.default_rng(K)
    kh = l2_normalize(g.standard_normal((rows, D)) + 0.3)[0].astype(np.float32)
    wt = l2_normalize(g.standard_normal((K, D)))[0].astype(np.float32)
    c0 = (0.05 * g.standard_normal(K)).astype(np.float32)
    kbar = ops.dino_key_mean(_dev(kh), rows)
    col_mean = (kh.astype(np.float64) @ wt.astype(np.float64).T).mean(0)
    assert np.abs(_np(kbar) - kh.astype(np.float64).mean(0)).max() <= 1e-15
    # m = 0: the centre becomes the rounded dot product itself, c + 1 * (x - c) in fp32
    bound = D * 2.0 ** -24 * np.abs(col_mean).max()
    c = _dev(np.zeros(K, np.float32))
    ops.dino_center(_dev(wt), kbar, c, 0.0)
    x = _np(c).copy()
    assert np.abs(x - col_mean).max() <= bound, (np.abs(x - col_mean).max(), bound)
    # the blend on that fp32 dot product, and the whole update against the restatement
    c = _dev(c0)
    ops.dino_center(_dev(wt), kbar, c, m)
    assert _np(c).tobytes() == center_blend_f32(c0, x, m).tobytes()
    want = center_update(c0, wt, kh, m)
    assert np.abs(_np(c) - want).max() <= bound + 2.0 ** -24 * np.abs(want).max()
    c2 = _dev(c0)
    ops.dino_center(_dev(wt), ops.dino_key_mean(_dev(kh), rows), c2, m)
    torch.cuda.synchronize()
    assert torch.equal(c, c2)


def test_refusals_return_the_error_code_and_launch_nothing():
    from simclr_amd import ops
    from simclr_amd._lib import SimclrHipError, lib
    q, k = torch.zeros(8, 64, device=DEV), torch.ones(8, 64, device=DEV)
    ws, wt, c = torch.ones(16, 64, device=DEV), torch.ones(16, 64, device=DEV), torch.zeros(16, device=DEV)
    kbar = torch.zeros(64, device=DEV, dtype=torch.float64)
    out = torch.full((2,), 7.0, device=DEV)
    stats, dq, u, dw = (torch.full(s, 7.0, device=DEV) for s in ((8, 2), (8, 64), (8, 64), (16, 64)))
    cen = torch.full((16,), 7.0, device=DEV)
    wsp = torch.full((lib().dino_workspace_bytes(8, 16, 64) // 4,), 7.0, device=DEV)
    P = lambda x, off=0: ctypes.c_void_p(x.data_ptr() + off)
    F = ctypes.c_float
    raw = lib()._dll
    nan = float('nan')
    ok = dict(q=P(q), k=P(k), ws=P(ws), wt=P(wt), c=P(c), two_n=8, K=16, D=64, Ts=0.1, Tt=0.04, w=P(wsp))
    bad = [dict(D=100), dict(D=32), dict(D=512), dict(two_n=0), dict(two_n=1), dict(two_n=7), dict(two_n=-2), dict(K=1), dict(K=0),
           dict(K=-1), dict(Ts=0.0), dict(Ts=-0.5), dict(Ts=nan), dict(Tt=0.0), dict(Tt=-1.0), dict(Tt=nan), dict(q=None), dict(k=None),
           dict(ws=None), dict(wt=None), dict(c=None), dict(w=None), dict(q=P(q, 4), two_n=6), dict(k=P(k, 8), two_n=6),
           dict(ws=P(ws, 4), K=15), dict(wt=P(wt, 8), K=15), dict(w=P(wsp, 4))]
    for change in bad:
        a = dict(ok, **change)
        only_teacher = bool(set(change) & {'Tt', 'k', 'wt', 'c'})        # the query-side backward reads none of these
        assert raw.simclr_dino_fwd(a['q'], a['k'], a['ws'], a['wt'], a['c'], a['two_n'], a['K'], a['D'], F(a['Ts']), F(a['Tt']), P(out),
                                   P(stats), P(u), a['w'], None) == 1, change
        assert 'dino_fwd' in lib().last_error()
        assert raw.simclr_dino_bwd_w(a['q'], a['k'], a['ws'], a['wt'], a['c'], a['two_n'], a['K'], a['D'], F(a['Ts']), F(a['Tt']),
                                     P(stats), F(1.0), P(dw), a['w'], None) == 1, change
        assert 'dino_bwd_w' in lib().last_error()
        if not only_teacher:
            assert raw.simclr_dino_bwd_q(a['q'], a['ws'], P(u), a['two_n'], a['K'], a['D'], F(a['Ts']), P(stats), F(1.0), P(dq), a['w'],
                                         None) == 1, change
            assert 'dino_bwd_q' in lib().last_error()
    a = ok
    assert raw.simclr_dino_fwd(a['q'], a['k'], a['ws'], a['wt'], a['c'], 8, 16, 64, F(0.1), F(0.04), None, P(stats), P(u), a['w'], None) == 1
    assert raw.simclr_dino_fwd(a['q'], a['k'], a['ws'], a['wt'], a['c'], 8, 16, 64, F(0.1), F(0.04), P(out), None, P(u), a['w'], None) == 1
    assert raw.simclr_dino_fwd(a['q'], a['k'], a['ws'], a['wt'], a['c'], 8, 16, 64, F(0.1), F(0.04), P(out), P(stats), None, a['w'], None) == 1
    assert raw.simclr_dino_bwd_q(a['q'], a['ws'], None, 8, 16, 64, F(0.1), P(stats), F(1.0), P(dq), a['w'], None) == 1
    assert raw.simclr_dino_bwd_q(a['q'], a['ws'], P(u), 8, 16, 64, F(0.1), None, F(1.0), P(dq), a['w'], None) == 1
    assert raw.simclr_dino_bwd_q(a['q'], a['ws'], P(u), 6, 16, 64, F(0.1), P(stats), F(1.0), P(dq, 4), a['w'], None) == 1
    assert raw.simclr_dino_bwd_w(a['q'], a['k'], a['ws'], a['wt'], a['c'], 8, 16, 64, F(0.1), F(0.04), None, F(1.0), P(dw), a['w'], None) == 1
    assert raw.simclr_dino_bwd_w(a['q'], a['k'], a['ws'], a['wt'], a['c'], 8, 16, 64, F(0.1), F(0.04), P(stats), F(1.0), None, a['w'], None) == 1
    # the centre: another D, K < 2, a momentum outside [0, 1] or NaN, null / misaligned pointers
    for wt_p, kb_p, c_p, K, D, m in ((P(wt), P(kbar), P(cen), 16, 100, 0.9), (P(wt), P(kbar), P(cen), 1, 64, 0.9),
                                     (P(wt), P(kbar), P(cen), 16, 64, -0.1), (P(wt), P(kbar), P(cen), 16, 64, 1.5),
                                     (P(wt), P(kbar), P(cen), 16, 64, nan), (None, P(kbar), P(cen), 16, 64, 0.9),
                                     (P(wt), None, P(cen), 16, 64, 0.9), (P(wt), P(kbar), None, 16, 64, 0.9),
                                     (P(wt, 4), P(kbar), P(cen), 15, 64, 0.9), (P(wt), P(kbar, 4), P(cen), 16, 64, 0.9)):
        assert raw.simclr_dino_center(wt_p, kb_p, c_p, K, D, F(m), None) == 1, (K, D, m)
        assert 'dino_center' in lib().last_error()
    for two_n, K, D in ((8, 16, 100), (0, 16, 64), (7, 16, 64), (8, 1, 64)):
        assert lib().dino_workspace_bytes(two_n, K, D) == 0
    assert lib().dino_key_splits(7, 16) == 0 and lib().dino_key_splits(8, 1) == 0 and lib().dino_row_splits(8, 1) == 0
    with pytest.raises(SimclrHipError, match='dino_fwd'):
        lib().dino_fwd(P(q), P(k), P(ws), P(wt), P(c), 7, 16, 64, 0.1, 0.04, P(out), P(stats), P(u), P(wsp), None)
    z100 = torch.zeros(8, 100, device=DEV)
    with pytest.raises(ValueError, match='widths 64/128/256'):
        ops.dino_fwd(z100, z100, torch.zeros(4, 100, device=DEV), torch.zeros(4, 100, device=DEV), torch.zeros(4, device=DEV), 0.1, 0.04)
    with pytest.raises(ValueError, match='K >= 2'):
        ops.dino_fwd(q, k, ws[:1], wt[:1], c[:1], 0.1, 0.04)
    with pytest.raises(ValueError, match='teacher temperature'):
        ops.dino_fwd(q, k, ws, wt, c, 0.1, nan)
    with pytest.raises(ValueError, match='student temperature'):
        ops.dino_bwd_q(q, ws, u, 0.0, stats, 1.0, wsp)
    with pytest.raises(ValueError, match='workspace is smaller'):
        ops.dino_bwd_w(q, k, ws, wt, c, 0.1, 0.04, stats, 1.0, torch.zeros(4, device=DEV))
    with pytest.raises(ValueError, match='row_stats'):
        ops.dino_bwd_q(q, ws, u, 0.1, torch.zeros(8, 4, device=DEV), 1.0, wsp)
    with pytest.raises(ValueError, match=r'momentum must lie in \[0, 1\]'):
        ops.dino_center(wt, kbar, cen, 1.5)
    torch.cuda.synchronize()
    for x in (out, stats, dq, u, dw, wsp, cen):
        assert bool((x == 7.0).all())                     # nothing was written


# ---------------------------------------------------------------------------------------------------------------- layers
K_STEP, SPE = 200, 2          # prototypes of the small network; steps per epoch of its schedules


def _fresh_runtime():
    from simclr_amd.resnet import RT
    RT.reset()
    RT.device = torch.device(DEV)
    return RT


def _flags(**kw):
    from simclr_amd.flags import FLAGS
    FLAGS.reset()
    kw.setdefault('proj_out_dim', 64)
    kw.setdefault('contrastive_loss', 'dino')
    kw.setdefault('use_blur', False)
    kw.setdefault('dino_out_dim', K_STEP)
    kw.setdefault('dino_momentum', 0.9)
    kw.setdefault('dino_freeze_last_layer_epochs', 0)
    kw.setdefault('train_batch_size', B)
    FLAGS.update(resnet_depth=18, image_size=SIZE, compute_dtype='f32', f32_matmul='exact', train_mode='pretrain', train_steps=10, **kw)
    return FLAGS


def _batch(n=B, seed=31):
    g = torch.Generator().manual_seed(seed)
    images = structured_images(n, SIZE, 2, g)
    ids = torch.randint(0, NCLS, (n,), generator=g)
    return images, ids


def _build(steps=10, strategy=None, lr=0.1):
    from simclr_amd import model as model_lib
    from simclr_amd.flags import FLAGS
    from simclr_amd.run import make_single_step
    model = model_lib.Model(NCLS)
    target = model_lib.TargetNetwork(model, steps, center=model_lib.DinoCenter(FLAGS.dino_out_dim), steps_per_epoch=SPE)
    opt = model_lib.build_optimizer(lr)
    return model, target, opt, make_single_step(model, opt, strategy, target=target)


def _values(variables):
    return {v.name: v.value.detach().clone() for v in variables}


def test_prototype_head_forward_and_backward_vs_float64_autograd():
    """b = 3, K = 200, D = 64: the normalised rows, and through add_dino_loss the gradient of the RAW variable and of the raw online
    projection, against the restatement (itself pinned to float64 autograd in tests/test_dino_reference.py)."""
    from simclr_amd import model as model_lib
    from simclr_amd import objective as obj_lib
    _flags()
    _fresh_runtime()
    b, K, D = 3, 200, 64
    g = np.random.default_rng(8)
    head = model_lib.PrototypeHead(K)
    head.build(D)
    assert head.kernel.name == 'prototype_head/kernel:0' and head.kernel.shape == (K, D) and head.trainable_variables == [head.kernel]
    head.kernel.value.copy_(_dev(g.standard_normal((K, D)) * (0.5 + g.random((K, 1)))))       # rows of many norms
    vs = _np(head.kernel.value)
    q, k = g.standard_normal((2 * b, D)).astype(np.float32), g.standard_normal((2 * b, D)).astype(np.float32)
    vt = g.standard_normal((K, D)).astype(np.float32)
    c = (0.05 * g.standard_normal(K)).astype(np.float32)
    wt = _dev(l2_normalize(vt)[0])
    ws = head()
    res = [_res('prototype_head rows', ws, l2_normalize(vs)[0], 0, 1e-6)]
    head.saved = None
    for scale in (1.0, 0.5):
        ref = dino_loss(q, k, vs, _np(wt), c, 0.1, 0.04, grad_scale=scale)
        loss = obj_lib.add_dino_loss(_dev(q), _dev(k), head, wt, _dev(c), 0.1, 0.04)
        dq = loss.backward(scale)
        assert head.saved is None
        res += [_res('layer grad_q scale=%g' % scale, dq, ref['grad_q'], GATE_GRAD),
                _res('layer grad_vs scale=%g' % scale, head.kernel.grad, ref['grad_vs'], GATE_GRAD)]
    res += [_res('layer loss', loss.value, ref['loss'], GATE_LOSS), _res('layer entropy', loss.entropy, ref['entropy'], GATE_LOSS),
            _res('layer keys', loss.keys, ref['kh'], 0, 1e-6)]
    # frozen: no key-side launch, the gradient slot keeps what it held
    before = head.kernel.grad.clone()
    loss = obj_lib.add_dino_loss(_dev(q), _dev(k), head, wt, _dev(c), 0.1, 0.04, update_prototypes=False)
    dq2 = loss.backward(0.5)
    torch.cuda.synchronize()
    assert torch.equal(dq2, dq) and torch.equal(head.kernel.grad, before) and head.saved is None
    _assert(res)


def _capture(setattr_fn, model, target, opt):
    """Records what the step hands the loss (with the centre and the target prototypes as the loss saw them), what the loss hands the
    projection head's backward, the centre at the moment of the backward, and the prototype gradient the optimizer is handed."""
    from simclr_amd import objective as obj_lib
    box = {}
    orig_loss, orig_backward, orig_apply = obj_lib.add_dino_loss, model.backward, opt.apply_gradients

    def loss_fn(online, tgt, prototypes, wt, center, *a, **kw):
        box.update(q=online.detach().clone(), t=tgt.detach().clone(), wt=wt.detach().clone(), center=center.detach().clone(),
                   vs=prototypes.kernel.value.detach().clone(), Ts=kw.get('student_temp'), Tt=kw.get('teacher_temp'),
                   update=kw.get('update_prototypes'))
        box['loss'] = orig_loss(online, tgt, prototypes, wt, center, *a, **kw)
        return box['loss']

    def backward(d_proj, *a, **kw):
        box['d_proj'] = d_proj.detach().clone()
        box['center_at_backward'] = target.center.value.detach().clone()
        return orig_backward(d_proj, *a, **kw)

    def apply(pairs, *a, **kw):
        pairs = list(pairs)
        box['applied'] = [v.name for _, v in pairs]
        box['proto_grad'] = model.prototype_head.kernel.grad.detach().clone()
        return orig_apply(pairs, *a, **kw)
    setattr_fn(obj_lib, 'add_dino_loss', loss_fn)
    setattr_fn(model, 'backward', backward)
    setattr_fn(opt, 'apply_gradients', apply)
    return box


def test_step_matches_the_restatement_on_the_pre_step_centre_and_target(monkeypatch):
    """The gradients are those of the loss taken with the centre and the target as they stood BEFORE the step; afterwards the centre is
    the restatement's update from the target prototypes the forward used."""
    FLAGS = _flags(dino_center_momentum=0.5)
    _fresh_runtime()
    model, target, opt, step = _build()
    assert model.prediction_head is None and model.variables[-1].name == 'model/prototype_head/kernel:0'
    assert sorted(step.metrics) == ['train/contrast_loss', 'train/dino_teacher_entropy', 'train/supervised_acc', 'train/supervised_loss',
                                    'train/total_loss', 'train/weight_decay']
    online0 = _values(model.variables)
    tv = _values(target.variables)
    assert len(tv) > 60 and 'model/prototype_head/kernel:0' in tv and all(torch.equal(tv[n], online0[n]) for n in tv)
    # a non-zero centre, and target prototypes that differ from the online ones: the pre-step state the gradients must be taken with
    g = np.random.default_rng(3)
    c0 = (0.05 * g.standard_normal(K_STEP)).astype(np.float32)
    target.center.value.copy_(_dev(c0))
    tproto = [v for v in target.variables if v.name == 'model/prototype_head/kernel:0'][0]
    tproto.value.add_(_dev(0.003 * g.standard_normal((K_STEP, 64))))
    vt0 = _np(tproto.value).copy()
    box = _capture(monkeypatch.setattr, model, target, opt)
    images, ids = _batch()
    labels = {'labels': torch.nn.functional.one_hot(ids, NCLS).float().to(DEV)}
    out = step(images.to(DEV), labels)
    torch.cuda.synchronize()
    assert tuple(box['q'].shape) == tuple(box['t'].shape) == (2 * B, 64) and box['update'] is True
    assert box['Ts'] == 0.1 and box['Tt'] == float(np.float32(0.04))
    assert _np(box['center']).tobytes() == c0.tobytes() and _np(box['center_at_backward']).tobytes() == c0.tobytes()
    assert _np(box['vs']).tobytes() == _np(online0['model/prototype_head/kernel:0']).tobytes()
    ref = dino_loss(_np(box['q']), _np(box['t']), _np(box['vs']), vt0, c0, 0.1, 0.04)
    con = out['con_loss']
    res = [_res('step_loss', con.value, ref['loss'], GATE_LOSS), _res('step_entropy', con.entropy, ref['entropy'], GATE_LOSS),
           _res('step_wt', box['wt'], ref['wt'], 0, 1e-6), _res('step_d_proj', box['d_proj'], ref['grad_q'], GATE_GRAD),
           _res('step_prototype_grad', box['proto_grad'], ref['grad_vs'], GATE_GRAD)]
    assert 'model/prototype_head/kernel:0' in box['applied']
    assert step.metrics['train/dino_teacher_entropy'].result() == float(con.entropy) and step.metrics['train/contrast_loss'].result() == float(con.value)
    assert out['logits_con'] is None
    # the centre: from the PRE-update target prototypes and the mean key, in the kernel's float32 blend
    want = center_update(c0, ref['wt'], ref['kh'], 0.5)
    bound = 64 * 2.0 ** -24 * np.abs(ref['kh'] @ ref['wt'].T).max() + 2.0 ** -23 * np.abs(want).max()
    res.append(_res('step_centre', target.center.value, want, 0, bound))
    assert not np.array_equal(_np(target.center.value), c0)
    # the target moved by 1 - tau_0 towards the stepped online weights (prototypes included), in the float32 arithmetic of the kernel
    from simclr_amd import model as model_lib
    omt = np.float32(1.0 - model_lib.byol_tau(0, 10, 0.9))
    after_o = _values(model.variables)
    trained = {v.name for v in model.trainable_variables}
    moved = 0
    for v in target.variables:
        if v.name in trained:
            before = vt0 if v is tproto else _np(tv[v.name])
            assert _np(v.value).tobytes() == ema_f32(before, _np(after_o[v.name]), omt).tobytes(), v.name
            moved += int(not np.array_equal(_np(v.value), before))
    assert moved >= 20 and not torch.equal(after_o['model/prototype_head/kernel:0'], online0['model/prototype_head/kernel:0'])
    assert all(v.grad is None for v in target.variables + target.center.variables)
    assert all(id(v) not in opt._slots for v in target.variables + target.center.variables)
    _assert(res)
    assert all(bool(torch.isfinite(v.value).all()) for v in model.variables + target.variables + target.center.variables)


def test_target_network_prototypes_freeze_and_thaw(monkeypatch):
    """freeze = 1 epoch of 2 steps: during steps 0 and 1 the prototypes are bitwise unchanged on both sides (no gradient, no weight
    decay, no momentum slot) while everything else trains and the centre moves; step 2 changes them on both sides.  The target keeps
    nothing after a call."""
    from simclr_amd import model as model_lib
    FLAGS = _flags(dino_freeze_last_layer_epochs=1)
    _fresh_runtime()
    model, target, opt, step = _build()
    name = 'model/prototype_head/kernel:0'
    proto = model.prototype_head.kernel
    tproto = [v for v in target.variables if v.name == name][0]
    p0 = proto.value.clone()
    assert torch.equal(tproto.value, p0)                                     # step 0: the target is the online copy, prototypes included
    box = _capture(monkeypatch.setattr, model, target, opt)
    images, ids = _batch()
    labels = {'labels': torch.nn.functional.one_hot(ids, NCLS).float().to(DEV)}
    others0 = _values([v for v in model.trainable_variables if v is not proto])
    for s in (0, 1):
        centre_before = target.center.value.clone()
        step(images.to(DEV), labels)
        torch.cuda.synchronize()
        assert box['update'] is False and name not in box['applied'], s
        assert torch.equal(proto.value, p0) and torch.equal(tproto.value, p0), s
        assert id(proto) not in opt._slots
        assert not torch.equal(target.center.value, centre_before)
        assert all(getattr(l, 'saved', None) is None for l in model_lib._all_layers(target.model))      # nothing kept after a call
    assert sum(int(not torch.equal(v.value, others0[v.name])) for v in model.trainable_variables if v is not proto) >= 20
    step(images.to(DEV), labels)                                             # optimizer step 2: the first one past the freeze
    torch.cuda.synchronize()
    assert box['update'] is True and name in box['applied']
    assert not torch.equal(proto.value, p0) and not torch.equal(tproto.value, p0)
    assert id(proto) in opt._slots and bool(torch.isfinite(proto.value).all())


# ---------------------------------------------------------------------------------------------------------------- run.main
ARGS = ['--dataset=synthetic', '--resnet_depth=18', '--image_size=32', '--train_batch_size=8', '--use_blur=False', '--compute_dtype=f32',
        '--checkpoint_steps=2', '--train_steps=3', '--mode=train', '--proj_out_dim=64', '--dino_out_dim=200', '--dino_momentum=0.9',
        '--dino_freeze_last_layer_epochs=0']


def test_run_main_trains_logs_resumes_bitwise_and_other_modes_read_the_file(tmp_path, capsys):
    """Three steps with a checkpoint after two: the run resumed from ckpt-2 writes a ckpt-3 bitwise equal to the uninterrupted one, the
    centre and the target prototypes included.  Then --mode=eval --knn_eval and a one-step fine-tune read the file as a plain
    pretraining checkpoint."""
    from simclr_amd import run
    from simclr_amd.checkpoint import INDEX_NAME
    from simclr_amd.flags import FLAGS
    args = ARGS + ['--contrastive_loss=dino']
    full_dir, again_dir, ft_dir = str(tmp_path / 'full'), str(tmp_path / 'again'), str(tmp_path / 'ft')
    FLAGS.reset()
    run.main(args + ['--model_dir=' + full_dir])
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith('{') and 'train/dino_teacher_entropy' in l]
    assert lines and lines[0]['step'] == 2
    for k in ('train/contrast_loss', 'train/dino_teacher_entropy', 'train/total_loss'):
        assert math.isfinite(lines[0][k]), (k, lines[0])
    assert 0.0 < lines[0]['train/dino_teacher_entropy'] <= math.log(200) + 1e-4 and lines[0]['train/contrast_loss'] > 0.0
    assert not any(k in lines[0] for k in ('train/contrast_entropy', 'train/contrast_acc', 'train/byol_cosine', 'train/align_loss'))
    full = torch.load(os.path.join(full_dir, 'ckpt-3.pt'), map_location='cpu')
    target_names = [n for n in full['model'] if n.startswith('target/')]
    assert len(target_names) > 60 and all(n[len('target/'):] in full['model'] for n in target_names)
    name = 'model/prototype_head/kernel:0'
    assert tuple(full['model'][name].shape) == tuple(full['model']['target/' + name].shape) == (200, 64)
    assert not torch.equal(full['model'][name], full['model']['target/' + name])
    assert tuple(full['model']['dino/center'].shape) == (200,) and float(full['model']['dino/center'].abs().max()) > 0.0
    assert name in full['optimizer']['slots']
    assert not any(n.startswith('target/') or n.startswith('dino/') for n in full['optimizer']['slots'])
    two = torch.load(os.path.join(full_dir, 'ckpt-2.pt'), map_location='cpu')['model']
    assert not torch.equal(two['dino/center'], full['model']['dino/center']) and not torch.equal(two[name], full['model'][name])
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

    # evaluation and the k-NN evaluation of that run's directory, the loss flag left on
    capsys.readouterr()
    FLAGS.reset()
    result = run.main(['--dataset=synthetic', '--resnet_depth=18', '--image_size=32', '--eval_batch_size=8', '--eval_steps=1',
                       '--compute_dtype=f32', '--mode=eval', '--contrastive_loss=dino', '--proj_out_dim=64', '--knn_eval=True',
                       '--knn_k=5', '--model_dir=' + full_dir])
    assert result['global_step'] == 3
    for k in ('eval/label_top_1_accuracy', 'eval/knn_top_1_accuracy'):
        assert 0.0 <= result[k] <= 1.0, (k, result)
    # one fine-tuning step from the file: the online encoder, no target, no centre, no prototypes in what it writes
    FLAGS.reset()
    path = os.path.join(full_dir, 'ckpt-3.pt')
    run.main(['--dataset=synthetic', '--resnet_depth=18', '--image_size=32', '--train_batch_size=8', '--compute_dtype=f32', '--mode=train',
              '--train_mode=finetune', '--contrastive_loss=dino', '--proj_out_dim=64', '--train_steps=1', '--checkpoint_steps=1',
              '--checkpoint=' + path, '--model_dir=' + ft_dir])
    written = torch.load(os.path.join(ft_dir, 'ckpt-1.pt'), map_location='cpu')['model']
    assert not any(n.startswith('target/') or n.startswith('dino/') or 'prototype_head' in n for n in written)
    enc = [n for n in written if n.startswith('model/resnet/')]
    assert len(enc) > 60 and all(n in full['model'] for n in enc)


# ---------------------------------------------------------------------------------------------------------------- two replicas
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    try:
        import torch.distributed as dist
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        torch.cuda.set_device(0)
        dist.init_process_group('gloo', rank=rank, world_size=world)
        from simclr_amd import comm, ops
        ops.set_f32_matmul('exact')
        _flags(train_batch_size=world * B)
        RT = _fresh_runtime()
        strategy = comm.Strategy()
        RT.strategy = strategy
        model, target, opt, step = _build(strategy=strategy)
        attrs = {}
        box = _capture(lambda o, name, v: (attrs.setdefault((id(o), name), (o, name, getattr(o, name))), setattr(o, name, v)),
                       model, target, opt)
        images, ids = _batch(world * B, seed=51)
        out = step(images[rank * B:(rank + 1) * B].to(DEV), {'labels': ids[rank * B:(rank + 1) * B].to(DEV)})
        torch.cuda.synchronize()
        res = dict(q=_np(box['q']), t=_np(box['t']), d_proj=_np(box['d_proj']), vs=_np(box['vs']), wt=_np(box['wt']),
                   proto_grad=_np(box['proto_grad']), loss=float(out['con_loss'].value), entropy=float(out['con_loss'].entropy),
                   center=_np(target.center.value).copy())
        for o, name, v in attrs.values():
            setattr(o, name, v)
        dist.destroy_process_group()
        q.put((rank, 'ok', res))
    except Exception:  # noqa
        import traceback
        q.put((rank, 'FAIL', traceback.format_exc()))


def test_two_replica_step_vs_the_restatement_on_the_gathered_batch():
    """Two gloo ranks sharing one GPU.  Each rank's loss is the restatement's on its own rows and the mean of the two is the
    restatement's on the gathered batch; the prototype gradient the optimizer is handed (after the gradient synchronisation summed the
    two shares) is the gathered batch's on both ranks; both centres are bitwise equal and are the gathered batch's."""
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
    assert boxes[0]['vs'].tobytes() == boxes[1]['vs'].tobytes() and boxes[0]['wt'].tobytes() == boxes[1]['wt'].tobytes()
    assert boxes[0]['center'].tobytes() == boxes[1]['center'].tobytes()
    vs = boxes[0]['vs']
    c0 = np.zeros(K_STEP, np.float32)
    cat = lambda name: np.concatenate([boxes[0][name][:B], boxes[1][name][:B], boxes[0][name][B:], boxes[1][name][B:]])
    whole = dino_loss(cat('q'), cat('t'), vs, vs, c0, 0.1, 0.04)               # step 0: the target prototypes are the online copy
    want_c = center_update(c0, whole['wt'], whole['kh'], 0.9)
    bound = 64 * 2.0 ** -24 * np.abs(whole['kh'] @ whole['wt'].T).max() + 2.0 ** -23 * np.abs(want_c).max()
    out = [_res('two_replica_loss_mean vs the gathered batch', 0.5 * (boxes[0]['loss'] + boxes[1]['loss']), whole['loss'], GATE_LOSS),
           _res('two_replica_entropy_mean vs the gathered batch', 0.5 * (boxes[0]['entropy'] + boxes[1]['entropy']), whole['entropy'], GATE_LOSS),
           _res('two_replica_centre vs the gathered batch', boxes[0]['center'], want_c, 0, bound)]
    for r, b in enumerate(boxes):
        ref = dino_loss(b['q'], b['t'], vs, vs, c0, 0.1, 0.04, grad_scale=0.5)
        idx = np.concatenate([np.arange(r * B, (r + 1) * B), 2 * B + np.arange(r * B, (r + 1) * B)])
        out += [_res('two_replica_loss rank %d' % r, b['loss'], ref['loss'], GATE_LOSS),
                _res('two_replica_d_proj rank %d' % r, b['d_proj'], ref['grad_q'], GATE_GRAD),
                _res('two_replica_d_proj rank %d vs the gathered batch' % r, b['d_proj'], whole['grad_q'][idx], GATE_GRAD),
                _res('two_replica_prototype_grad rank %d vs the gathered batch' % r, b['proto_grad'], whole['grad_vs'], GATE_GRAD)]
    _assert(out)
