"""SwAV on the device (pytest -m gpu): the kernels of csrc/swav.hip through the C ABI and simclr_amd.ops against the float64 restatement
tests/swav_reference.py -- the Sinkhorn-Knopp potentials, then the loss and both gradients on the REFERENCE's alpha (so that a Sinkhorn
error cannot hide a loss error) -- then add_swav_loss, the step, freeze and thaw, run.main end to end and two replicas over gloo.

Gates: the project's for this arithmetic -- loss and entropy 1e-5 relative, gradients and u 2e-4 of the reference tensor's maximum
(tests/test_swav_reference.py shows that no case of LOSS_CASES needs the 4x-emulation rule); alpha: ALPHA_TOL nats absolute = 4x the worst
float32-emulation error of the restatement over SINK_CASES (tests/golden/SWAV_HAND_DERIVED.md, "Error budget").  Repeated calls are
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

from tests.gpu_checks import DEV, _res, structured_images
from tests.swav_reference import (ALPHA_TOL, GATE_GRAD, GATE_LOSS, LOSS_CASES, SINK_CASES, autograd_gradients, case_gates, case_inputs,
                                  gates_of_inputs, l2_normalize_bwd, loss_case_inputs, sinkhorn_potentials, swav_loss,
                                  swav_loss_normalized)

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


# ---------------------------------------------------------------------------------------------------------------- the Sinkhorn
@pytest.mark.parametrize('N,K,D,eps,iters,concentrated', SINK_CASES)
def test_sinkhorn_vs_float64(N, K, D, eps, iters, concentrated):
    from simclr_amd import ops
    z, w = case_inputs(N, K, D, concentrated)
    if K == 4097:
        assert ops.swav_key_splits(2 * N, K) > 1 and K % 64 != 0          # several key splits of the row sweep, the last tile ragged
    if (N, K) == (33, 2):
        assert ops.swav_row_splits(2 * N, K) == 2                          # two row splits of the column sweep
    if (N, K) == (70, 63):
        assert ops.swav_row_splits(2 * N, K) == 3
    want, _ = sinkhorn_potentials(z, w, eps, iters)
    if concentrated:
        assert want.max() - want.min() > 15.0
    zd, wd = _dev(z), _dev(w)
    alpha = ops.swav_sinkhorn(zd, wd, eps, iters)
    again = ops.swav_sinkhorn(zd, wd, eps, iters)
    torch.cuda.synchronize()
    assert tuple(alpha.shape) == (2, K) and bool(torch.isfinite(alpha).all())
    assert torch.equal(alpha, again), 'a second Sinkhorn is not bitwise the first'
    _assert([_res('swav_alpha N=%d K=%d D=%d eps=%g I=%d%s' % (N, K, D, eps, iters, ' concentrated' if concentrated else ''), alpha, want,
                  0, ALPHA_TOL)])


def test_sinkhorn_sixteen_iterations_and_one_row_per_view():
    """I = 16 (the largest) on a small case, and N = 1: alpha_j = -ln K - L_gj exactly, the code uniform."""
    from simclr_amd import ops
    z, w = case_inputs(24, 6, 64)
    want, _ = sinkhorn_potentials(z, w, 0.05, 16)
    res = [_res('swav_alpha I=16', ops.swav_sinkhorn(_dev(z), _dev(w), 0.05, 16), want, 0, ALPHA_TOL)]
    z, w = case_inputs(1, 200, 128)
    alpha = _np(ops.swav_sinkhorn(_dev(z), _dev(w), 0.05, 3)).astype(np.float64)
    t = z.astype(np.float64) @ w.astype(np.float64).T / 0.05 + alpha
    res.append(_res('N=1: L + alpha is constant in j', t - t.mean(1, keepdims=True), np.zeros_like(t), 0, 2 * ALPHA_TOL))
    _assert(res)


def test_splits_follow_the_shape():
    from simclr_amd import ops
    assert ops.swav_key_splits(2, 2) == 1 and ops.swav_key_splits(2, 64) == 1 and ops.swav_key_splits(2, 65) == 2
    assert ops.swav_key_splits(1024, 65536) > 1
    assert ops.swav_row_splits(64, 2) == 1 and ops.swav_row_splits(66, 2) == 2 and ops.swav_row_splits(1024, 65536) == 1
    for rows, K in ((0, 64), (3, 64), (2, 1), (2, 1048577)):
        with pytest.raises(ValueError, match='even row count'):
            ops.swav_key_splits(rows, K)
        with pytest.raises(ValueError, match='even row count'):
            ops.swav_row_splits(rows, K)


# ---------------------------------------------------------------------------------------------------------------- loss kernels
def _run_kernels(qh, w, alpha, T, eps, scales=(1.0, 0.5), tag='', gates=None):
    """Forward, both backward sweeps at every scale and a second call (bitwise) against the float64 restatement on the same float32
    rows and the same float32 alpha."""
    from simclr_amd import ops
    gates = gates or {}
    gate = lambda name, project: gates.get(name, (project,))[0]
    qd, wd, ad = _dev(qh), _dev(w), _dev(alpha)
    out, stats, u, wsp = ops.swav_fwd(qd, wd, ad, T, eps)
    out, u = out.clone(), u.clone()
    res = []
    for scale in scales:
        ref = swav_loss_normalized(qh, w, alpha, T, eps, grad_scale=scale)
        dq = ops.swav_bwd_q(qd, wd, u, T, stats, scale, wsp)
        dw = ops.swav_bwd_w(qd, wd, ad, T, eps, stats, scale, wsp)
        res += [_res('swav_grad_q %s scale=%g' % (tag, scale), dq, ref['grad_q'], gate('grad_q', GATE_GRAD)),
                _res('swav_grad_w %s scale=%g' % (tag, scale), dw, ref['grad_w'], gate('grad_w', GATE_GRAD))]
    log2e = 1.4426950408889634
    res += [_res('swav_loss %s' % tag, out[0], ref['loss'], gate('loss', GATE_LOSS)),
            _res('swav_entropy %s' % tag, out[1], ref['entropy'], gate('entropy', GATE_LOSS)),
            _res('swav_u %s' % tag, u, ref['u'], gate('u', GATE_GRAD)),
            # (relative to the largest logit: with one row per view the code's log-sum-exp is a zero formed from logits of size 1 / eps)
            _res('swav_lse_s %s' % tag, stats[:, 0], ref['lse_s'] * log2e, 0, GATE_LOSS * log2e * ref['smax']),
            _res('swav_lse_t %s' % tag, stats[:, 1], ref['lse_t'] * log2e, 0, GATE_LOSS * log2e * ref['tmax'])]
    out2, stats2, u2, wsp2 = ops.swav_fwd(qd, wd, ad, T, eps)
    dq2 = ops.swav_bwd_q(qd, wd, u2, T, stats2, scales[-1], wsp2)
    dw2 = ops.swav_bwd_w(qd, wd, ad, T, eps, stats2, scales[-1], wsp2)
    torch.cuda.synchronize()
    assert torch.equal(out2, out) and torch.equal(stats2, stats) and torch.equal(u2, u), 'a second forward is not bitwise the first'
    assert torch.equal(dq2, dq) and torch.equal(dw2, dw), 'a second backward is not bitwise the first'
    for x in (out, u, dq, dw, stats):
        assert bool(torch.isfinite(x).all())
    return res, ref, out, dq, dw


@pytest.mark.parametrize('b,K,D,T,eps,concentrated', LOSS_CASES)
def test_kernels_vs_float64(b, K, D, T, eps, concentrated):
    from simclr_amd import ops
    qh, w, alpha = loss_case_inputs(b, K, D, T, eps, concentrated)
    assert np.abs(alpha[0] - alpha[1]).max() > 0.0                          # two different views' potentials
    if K == 4097:
        assert ops.swav_key_splits(2 * b, K) > 1 and K % 64 != 0
    if (b, K) == (33, 2):
        assert ops.swav_row_splits(2 * b, K) == 2 and ops.swav_row_splits(2 * (b - 1), K) == 1
    res, ref, _, _, _ = _run_kernels(qh, w, alpha, T, eps, tag='b=%d K=%d D=%d T=%g eps=%g' % (b, K, D, T, eps),
                                     gates=case_gates(b, K, D, T, eps, concentrated))
    assert 0.0 < ref['loss'] and np.abs(ref['grad_q']).max() > 0.0 and np.abs(ref['grad_w']).max() > 0.0
    _assert(res)


def near_one_hot():
    """K = 65, eps = 0.03: prototype 7 equals row 0, so that row's best code logit leads the rest by ~ 0.6 / eps nats."""
    b, K, D = 3, 65, 64
    qh, w = case_inputs(b, K, D)
    w = w.copy()
    w[7] = qh[0]
    alpha = (0.05 * np.random.default_rng(2).standard_normal((2, K))).astype(np.float32)
    return qh, w, alpha


def test_near_one_hot_code_entropy_keeps_its_digits():
    qh, w, alpha = near_one_hot()
    res, ref, out, _, _ = _run_kernels(qh, w, alpha, 0.1, 0.03, tag='near one-hot', gates=gates_of_inputs(qh, w, alpha, 0.1, 0.03))
    # rows 0 and b (the other view of the same sample, which stays close to it): the rows the entropy metric exists to show
    assert ref['row_entropy'][[0, 3]].max() < 1e-4 * ref['row_entropy'][[1, 2, 4, 5]].min()
    assert math.isfinite(float(out[1])) and float(out[1]) > 0.0
    _assert(res)
    # that row alone: a batch whose every row is the prototype.  T = 1, so that the STUDENT is not one-hot as well: at T = 0.1 the loss
    # itself would be the 6e-3 left of logsumexp(s) - q . u / T, two numbers near 10, which is not what this case is about
    q1 = np.repeat(qh[:1], 2, axis=0)
    res1, ref1, out1, _, _ = _run_kernels(q1, w, alpha, 1.0, 0.03, tag='one-hot rows only', gates=gates_of_inputs(q1, w, alpha, 1.0, 0.03))
    assert 0.0 < ref1['entropy'] < 1e-5 and ref1['loss'] > 1.0
    _assert(res1)


def test_alpha_is_read_per_view_and_for_the_paired_row():
    """The kernels fed alpha[::-1] must MISS the reference on the right alpha: the per-view indexing is observable.  b = 33 puts the view
    boundary inside a 64-row workgroup."""
    from simclr_amd import ops
    b, K, D, T, eps = 33, 63, 256, 0.1, 0.05
    qh, w, alpha = loss_case_inputs(b, K, D, T, eps)
    ref = swav_loss_normalized(qh, w, alpha, T, eps)
    qd, wd = _dev(qh), _dev(w)
    for name, a, expect_ok in (('right', alpha, True), ('swapped', alpha[::-1].copy(), False)):
        ad = _dev(a)
        out, stats, u, wsp = ops.swav_fwd(qd, wd, ad, T, eps)
        dq = ops.swav_bwd_q(qd, wd, u, T, stats, 1.0, wsp)
        dw = ops.swav_bwd_w(qd, wd, ad, T, eps, stats, 1.0, wsp)
        for r in (_res('u (%s alpha)' % name, u, ref['u'], GATE_GRAD), _res('grad_q (%s alpha)' % name, dq, ref['grad_q'], GATE_GRAD),
                  _res('grad_w (%s alpha)' % name, dw, ref['grad_w'], GATE_GRAD)):
            print(r['name'], r['err'], r['tol'])
            assert r['ok'] == expect_ok, r
    # the key-side sweep alone on the swapped alpha, with the statistics of the RIGHT alpha: only its own indexing is wrong
    ad = _dev(alpha)
    out, stats, u, wsp = ops.swav_fwd(qd, wd, ad, T, eps)
    dw = ops.swav_bwd_w(qd, wd, _dev(alpha[::-1].copy()), T, eps, stats, 1.0, wsp)
    assert not _res('grad_w (swapped in the key-side sweep only)', dw, ref['grad_w'], GATE_GRAD)['ok']


def test_refusals_return_the_error_code_and_launch_nothing():
    from simclr_amd import ops
    from simclr_amd._lib import SimclrHipError, lib
    q, w, al = torch.zeros(8, 64, device=DEV), torch.ones(16, 64, device=DEV), torch.zeros(2, 16, device=DEV)
    out = torch.full((2,), 7.0, device=DEV)
    stats, dq, u, dw, alpha = (torch.full(s, 7.0, device=DEV) for s in ((8, 2), (8, 64), (8, 64), (16, 64), (2, 16)))
    wsp = torch.full((lib().swav_workspace_bytes(8, 16, 64) // 4,), 7.0, device=DEV)
    P = lambda x, off=0: ctypes.c_void_p(x.data_ptr() + off)
    F = ctypes.c_float
    raw = lib()._dll
    nan = float('nan')
    ok = dict(q=P(q), w=P(w), a=P(al), rows=8, K=16, D=64, T=0.1, eps=0.05, ws=P(wsp), I=3)
    bad = [dict(D=100), dict(D=32), dict(D=512), dict(rows=0), dict(rows=1), dict(rows=7), dict(rows=-2), dict(K=1), dict(K=0), dict(K=-1),
           dict(K=1048577), dict(T=0.0), dict(T=-0.5), dict(T=nan), dict(eps=0.0), dict(eps=-1.0), dict(eps=nan), dict(q=None), dict(w=None),
           dict(a=None), dict(ws=None), dict(q=P(q, 4), rows=6), dict(w=P(w, 4), K=15), dict(ws=P(wsp, 4)), dict(I=0), dict(I=17), dict(I=-1)]
    for change in bad:
        a = dict(ok, **change)
        keys = set(change)
        if not keys & {'T', 'a', 'I'}:
            assert raw.simclr_swav_sinkhorn(a['q'], a['w'], a['rows'], a['K'], a['D'], F(a['eps']), a['I'], P(alpha), a['ws'], None) == 1, change
            assert 'swav_sinkhorn' in lib().last_error()
        if keys & {'I'}:
            assert raw.simclr_swav_sinkhorn(a['q'], a['w'], a['rows'], a['K'], a['D'], F(a['eps']), a['I'], P(alpha), a['ws'], None) == 1, change
            assert 'iters must lie in [1, 16]' in lib().last_error()
            continue
        assert raw.simclr_swav_fwd(a['q'], a['w'], a['a'], a['rows'], a['K'], a['D'], F(a['T']), F(a['eps']), P(out), P(stats), P(u), a['ws'],
                                   None) == 1, change
        assert 'swav_fwd' in lib().last_error()
        assert raw.simclr_swav_bwd_w(a['q'], a['w'], a['a'], a['rows'], a['K'], a['D'], F(a['T']), F(a['eps']), P(stats), F(1.0), P(dw),
                                     a['ws'], None) == 1, change
        assert 'swav_bwd_w' in lib().last_error()
        if not keys & {'eps', 'a'}:                                         # the query-side backward reads neither
            assert raw.simclr_swav_bwd_q(a['q'], a['w'], P(u), a['rows'], a['K'], a['D'], F(a['T']), P(stats), F(1.0), P(dq), a['ws'],
                                         None) == 1, change
            assert 'swav_bwd_q' in lib().last_error()
    a = ok
    assert raw.simclr_swav_sinkhorn(a['q'], a['w'], 8, 16, 64, F(0.05), 3, None, a['ws'], None) == 1
    assert raw.simclr_swav_fwd(a['q'], a['w'], a['a'], 8, 16, 64, F(0.1), F(0.05), None, P(stats), P(u), a['ws'], None) == 1
    assert raw.simclr_swav_fwd(a['q'], a['w'], a['a'], 8, 16, 64, F(0.1), F(0.05), P(out), None, P(u), a['ws'], None) == 1
    assert raw.simclr_swav_fwd(a['q'], a['w'], a['a'], 8, 16, 64, F(0.1), F(0.05), P(out), P(stats), None, a['ws'], None) == 1
    assert raw.simclr_swav_bwd_q(a['q'], a['w'], None, 8, 16, 64, F(0.1), P(stats), F(1.0), P(dq), a['ws'], None) == 1
    assert raw.simclr_swav_bwd_q(a['q'], a['w'], P(u), 8, 16, 64, F(0.1), None, F(1.0), P(dq), a['ws'], None) == 1
    assert raw.simclr_swav_bwd_q(a['q'], a['w'], P(u), 6, 16, 64, F(0.1), P(stats), F(1.0), P(dq, 4), a['ws'], None) == 1
    assert raw.simclr_swav_bwd_w(a['q'], a['w'], a['a'], 8, 16, 64, F(0.1), F(0.05), None, F(1.0), P(dw), a['ws'], None) == 1
    assert raw.simclr_swav_bwd_w(a['q'], a['w'], a['a'], 8, 16, 64, F(0.1), F(0.05), P(stats), F(1.0), None, a['ws'], None) == 1
    for rows, K, D in ((8, 16, 100), (0, 16, 64), (7, 16, 64), (8, 1, 64), (8, 1048577, 64)):
        assert lib().swav_workspace_bytes(rows, K, D) == 0
    assert lib().swav_key_splits(7, 16) == 0 and lib().swav_key_splits(8, 1) == 0 and lib().swav_row_splits(8, 1) == 0
    with pytest.raises(SimclrHipError, match='swav_fwd'):
        lib().swav_fwd(P(q), P(w), P(al), 7, 16, 64, 0.1, 0.05, P(out), P(stats), P(u), P(wsp), None)
    with pytest.raises(ValueError, match='widths 64/128/256'):
        ops.swav_sinkhorn(torch.zeros(8, 100, device=DEV), torch.zeros(4, 100, device=DEV))
    with pytest.raises(ValueError, match='workspace is smaller'):
        ops.swav_bwd_w(q, w, al, 0.1, 0.05, stats, 1.0, torch.zeros(4, device=DEV))
    with pytest.raises(ValueError, match='row_stats'):
        ops.swav_bwd_q(q, w, u, 0.1, torch.zeros(8, 4, device=DEV), 1.0, wsp)
    torch.cuda.synchronize()
    for x in (out, stats, dq, u, dw, wsp, alpha):
        assert bool((x == 7.0).all())                     # nothing was written


# ---------------------------------------------------------------------------------------------------------------- layers
K_STEP, SPE = 200, 2          # prototypes of the small network; steps per epoch of the freeze


def _fresh_runtime():
    from simclr_amd.resnet import RT
    RT.reset()
    RT.device = torch.device(DEV)
    return RT


def _flags(**kw):
    from simclr_amd.flags import FLAGS
    FLAGS.reset()
    kw.setdefault('proj_out_dim', 64)
    kw.setdefault('contrastive_loss', 'swav')
    kw.setdefault('use_blur', False)
    kw.setdefault('swav_num_prototypes', K_STEP)
    kw.setdefault('swav_freeze_prototypes_epochs', 0)
    kw.setdefault('train_batch_size', B)
    FLAGS.update(resnet_depth=18, image_size=SIZE, compute_dtype='f32', f32_matmul='exact', train_mode='pretrain', train_steps=10, **kw)
    return FLAGS


def _batch(n=B, seed=31):
    g = torch.Generator().manual_seed(seed)
    images = structured_images(n, SIZE, 2, g)
    ids = torch.randint(0, NCLS, (n,), generator=g)
    return images, ids


def _build(strategy=None, lr=0.1):
    from simclr_amd import model as model_lib
    from simclr_amd.run import make_single_step
    model = model_lib.Model(NCLS)
    opt = model_lib.build_optimizer(lr)
    return model, opt, make_single_step(model, opt, strategy, steps_per_epoch=SPE)


def _values(variables):
    return {v.name: v.value.detach().clone() for v in variables}


def test_add_swav_loss_vs_float64_through_the_prototype_head():
    """b = 33, K = 200, D = 64, the Sinkhorn on the device: the loss, the code entropy, alpha, the gradient of the raw online projection
    and the gradient of the RAW prototype variable against the restatement (itself pinned to float64 autograd with the codes detached)."""
    from simclr_amd import model as model_lib
    from simclr_amd import objective as obj_lib
    _flags()
    _fresh_runtime()
    b, K, D = 33, 200, 64
    g = np.random.default_rng(8)
    head = model_lib.PrototypeHead(K)
    head.build(D)
    assert head.kernel.name == 'prototype_head/kernel:0' and head.kernel.shape == (K, D)
    head.kernel.value.copy_(_dev(g.standard_normal((K, D)) * (0.5 + g.random((K, 1)))))       # rows of many norms
    vs = _np(head.kernel.value)
    a = g.standard_normal((b, D))
    q = np.concatenate([a, a + 0.5 * g.standard_normal((b, D))]).astype(np.float32)
    res = []
    for scale in (1.0, 0.5):
        ref = swav_loss(q, vs, 0.1, 0.05, 3, grad_scale=scale)
        loss = obj_lib.add_swav_loss(_dev(q), head, 0.1, 0.05, 3)
        dq = loss.backward(scale)
        assert head.saved is None
        res += [_res('layer grad_q scale=%g' % scale, dq, ref['grad_q'], GATE_GRAD),
                _res('layer grad_v scale=%g' % scale, head.kernel.grad, ref['grad_v'], GATE_GRAD)]
    res += [_res('layer loss', loss.value, ref['loss'], GATE_LOSS), _res('layer entropy', loss.entropy, ref['entropy'], GATE_LOSS),
            _res('layer alpha', loss.alpha, ref['alpha'], 0, ALPHA_TOL)]
    # frozen: no key-side launch, the gradient slot keeps what it held
    before = head.kernel.grad.clone()
    loss = obj_lib.add_swav_loss(_dev(q), head, 0.1, 0.05, 3, update_prototypes=False)
    dq2 = loss.backward(0.5)
    torch.cuda.synchronize()
    assert torch.equal(dq2, dq) and torch.equal(head.kernel.grad, before) and head.saved is None
    _assert(res)


def _capture(setattr_fn, model, opt):
    """Records what the step hands the loss, what the Sinkhorn is handed and returns, what the loss hands the projection head's backward
    and the prototype gradient the optimizer is handed."""
    from simclr_amd import objective as obj_lib
    from simclr_amd import ops
    box = {}
    orig_loss, orig_backward, orig_apply, orig_sink = obj_lib.add_swav_loss, model.backward, opt.apply_gradients, ops.swav_sinkhorn

    def loss_fn(online, prototypes, *a, **kw):
        box.update(q=online.detach().clone(), T=kw.get('temperature'), eps=kw.get('epsilon'), iters=kw.get('sinkhorn_iterations'),
                   update=kw.get('update_prototypes'))
        box['loss'] = orig_loss(online, prototypes, *a, **kw)
        box['vs'] = prototypes.kernel.value.detach().clone()      # (the head builds its variable at its first call; the optimizer comes later)
        return box['loss']

    def sink(z_all, w, *a, **kw):
        box.update(z_all=z_all.detach().clone(), w=w.detach().clone())
        box['alpha'] = orig_sink(z_all, w, *a, **kw)
        return box['alpha']

    def backward(d_proj, *a, **kw):
        box['d_proj'] = d_proj.detach().clone()
        return orig_backward(d_proj, *a, **kw)

    def apply(pairs, *a, **kw):
        pairs = list(pairs)
        box['applied'] = [v.name for _, v in pairs]
        g = model.prototype_head.kernel.grad
        box['proto_grad'] = None if g is None else g.detach().clone()
        return orig_apply(pairs, *a, **kw)
    setattr_fn(obj_lib, 'add_swav_loss', loss_fn)
    setattr_fn(ops, 'swav_sinkhorn', sink)
    setattr_fn(model, 'backward', backward)
    setattr_fn(opt, 'apply_gradients', apply)
    return box


def test_step_gradients_are_those_of_the_detached_code_loss(monkeypatch):
    _flags()
    _fresh_runtime()
    model, opt, step = _build()
    assert model.prediction_head is None and model.prototype_head.num_prototypes == K_STEP
    assert sorted(step.metrics) == ['train/contrast_loss', 'train/supervised_acc', 'train/supervised_loss', 'train/swav_code_entropy',
                                    'train/total_loss', 'train/weight_decay']
    box = _capture(monkeypatch.setattr, model, opt)
    images, ids = _batch()
    labels = {'labels': torch.nn.functional.one_hot(ids, NCLS).float().to(DEV)}
    out = step(images.to(DEV), labels)
    torch.cuda.synchronize()
    assert model.variables[-1].name == 'model/prototype_head/kernel:0'
    assert tuple(box['q'].shape) == (2 * B, 64) and box['update'] is True
    assert (box['T'], box['eps'], box['iters']) == (0.1, 0.05, 3)
    ref = swav_loss(_np(box['q']), _np(box['vs']), 0.1, 0.05, 3)
    con = out['con_loss']
    res = [_res('step_loss', con.value, ref['loss'], GATE_LOSS), _res('step_entropy', con.entropy, ref['entropy'], GATE_LOSS),
           _res('step_alpha', box['alpha'], ref['alpha'], 0, ALPHA_TOL), _res('step_z_all', box['z_all'], ref['qh'], 0, 1e-6),
           _res('step_d_proj', box['d_proj'], ref['grad_q'], GATE_GRAD),
           _res('step_prototype_grad', box['proto_grad'], ref['grad_v'], GATE_GRAD)]
    # ... and NOT those of the loss differentiated through the Sinkhorn
    _, gq_full, _ = autograd_gradients(ref['qh'], ref['w'], 0.1, 0.05, 3, detach=False)
    miss = _res('step_d_proj vs the gradient through the Sinkhorn', _through_the_normalisation(ref, box, gq_full), ref['grad_q'], GATE_GRAD)
    assert not miss['ok']
    assert 'model/prototype_head/kernel:0' in box['applied']
    assert step.metrics['train/swav_code_entropy'].result() == float(con.entropy) and step.metrics['train/contrast_loss'].result() == float(con.value)
    assert out['logits_con'] is None and 0.0 < float(con.entropy) <= math.log(K_STEP) + 1e-4
    _assert(res)
    assert all(bool(torch.isfinite(v.value).all()) for v in model.variables)


def _through_the_normalisation(ref, box, grad_qhat):
    """The non-detached gradient carried through the row normalisation of the captured projections (float64)."""
    q = _np(box['q']).astype(np.float64)
    return l2_normalize_bwd(ref['qh'], (q * q).sum(-1, keepdims=True), grad_qhat)


def test_prototypes_freeze_and_thaw(monkeypatch):
    """freeze = 1 epoch of 2 steps: during steps 0 and 1 the prototypes are bitwise unchanged (no gradient, no weight decay, no momentum
    slot) while everything else trains; step 2 changes them."""
    _flags(swav_freeze_prototypes_epochs=1)
    _fresh_runtime()
    model, opt, step = _build()
    name = 'model/prototype_head/kernel:0'
    box = _capture(monkeypatch.setattr, model, opt)
    images, ids = _batch()
    labels = {'labels': torch.nn.functional.one_hot(ids, NCLS).float().to(DEV)}
    # the variables exist before step 0, as run.main makes them exist before a restore: a forward in inference mode, the prototypes last
    model(torch.zeros(2, SIZE, SIZE, 3, device=DEV), training=False)
    model.release()
    model.prototype_head.build(64)
    proto = model.prototype_head.kernel
    p0 = proto.value.clone()
    assert 0.005 < float(p0.std()) < 0.015 and model.variables[-1] is proto
    others0 = None
    for s in (0, 1):
        step(images.to(DEV), labels)
        torch.cuda.synchronize()
        assert model.prototype_head.kernel is proto
        assert box['update'] is False and name not in box['applied'], s
        assert torch.equal(proto.value, p0), s
        assert id(proto) not in opt._slots
        if others0 is None:
            others0 = _values([v for v in model.trainable_variables if v is not proto])
    assert sum(int(not torch.equal(v.value, others0[v.name])) for v in model.trainable_variables if v is not proto) >= 20
    step(images.to(DEV), labels)                                             # optimizer step 2: the first one past the freeze
    torch.cuda.synchronize()
    assert box['update'] is True and name in box['applied']
    assert not torch.equal(proto.value, p0)
    assert id(proto) in opt._slots and bool(torch.isfinite(proto.value).all())


# ---------------------------------------------------------------------------------------------------------------- run.main
ARGS = ['--dataset=synthetic', '--resnet_depth=18', '--image_size=32', '--train_batch_size=8', '--use_blur=False', '--compute_dtype=f32',
        '--checkpoint_steps=2', '--train_steps=3', '--mode=train', '--proj_out_dim=64', '--swav_num_prototypes=200',
        '--swav_freeze_prototypes_epochs=0']


def test_run_main_trains_logs_resumes_bitwise_and_other_modes_read_the_file(tmp_path, capsys):
    """Three steps with a checkpoint after two: the run resumed from ckpt-2 writes a ckpt-3 bitwise equal to the uninterrupted one.  Then
    --mode=eval --knn_eval and a one-step fine-tune read the file as a plain pretraining checkpoint."""
    from simclr_amd import run
    from simclr_amd.checkpoint import INDEX_NAME
    from simclr_amd.flags import FLAGS
    args = ARGS + ['--contrastive_loss=swav']
    full_dir, again_dir, ft_dir = str(tmp_path / 'full'), str(tmp_path / 'again'), str(tmp_path / 'ft')
    FLAGS.reset()
    run.main(args + ['--model_dir=' + full_dir])
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith('{') and 'train/swav_code_entropy' in l]
    assert lines and lines[0]['step'] == 2
    for k in ('train/contrast_loss', 'train/swav_code_entropy', 'train/total_loss'):
        assert math.isfinite(lines[0][k]), (k, lines[0])
    assert 0.0 < lines[0]['train/swav_code_entropy'] <= math.log(200) + 1e-4 and lines[0]['train/contrast_loss'] > 0.0
    assert not any(k in lines[0] for k in ('train/contrast_entropy', 'train/contrast_acc', 'train/dino_teacher_entropy'))
    full = torch.load(os.path.join(full_dir, 'ckpt-3.pt'), map_location='cpu')
    name = 'model/prototype_head/kernel:0'
    assert tuple(full['model'][name].shape) == (200, 64) and name in full['optimizer']['slots']
    assert not any(n.startswith('target/') or n.startswith('dino/') or n.startswith('moco/') for n in full['model'])
    two = torch.load(os.path.join(full_dir, 'ckpt-2.pt'), map_location='cpu')['model']
    assert not torch.equal(two[name], full['model'][name])
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
                       '--compute_dtype=f32', '--mode=eval', '--contrastive_loss=swav', '--proj_out_dim=64', '--knn_eval=True',
                       '--knn_k=5', '--model_dir=' + full_dir])
    assert result['global_step'] == 3
    for k in ('eval/label_top_1_accuracy', 'eval/knn_top_1_accuracy'):
        assert 0.0 <= result[k] <= 1.0, (k, result)
    # one fine-tuning step from the file: the online encoder, no prototypes in what it writes
    FLAGS.reset()
    path = os.path.join(full_dir, 'ckpt-3.pt')
    run.main(['--dataset=synthetic', '--resnet_depth=18', '--image_size=32', '--train_batch_size=8', '--compute_dtype=f32', '--mode=train',
              '--train_mode=finetune', '--contrastive_loss=swav', '--proj_out_dim=64', '--train_steps=1', '--checkpoint_steps=1',
              '--checkpoint=' + path, '--model_dir=' + ft_dir])
    written = torch.load(os.path.join(ft_dir, 'ckpt-1.pt'), map_location='cpu')['model']
    assert not any('prototype_head' in n for n in written)
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
        model, opt, step = _build(strategy=strategy)
        attrs = {}
        box = _capture(lambda o, name, v: (attrs.setdefault((id(o), name), (o, name, getattr(o, name))), setattr(o, name, v)), model, opt)
        images, ids = _batch(world * B, seed=51)
        out = step(images[rank * B:(rank + 1) * B].to(DEV), {'labels': ids[rank * B:(rank + 1) * B].to(DEV)})
        torch.cuda.synchronize()
        res = dict(q=_np(box['q']), d_proj=_np(box['d_proj']), vs=_np(box['vs']), w=_np(box['w']), z_all=_np(box['z_all']),
                   alpha=_np(box['alpha']), proto_grad=_np(box['proto_grad']), loss=float(out['con_loss'].value),
                   entropy=float(out['con_loss'].entropy))
        for o, name, v in attrs.values():
            setattr(o, name, v)
        dist.destroy_process_group()
        q.put((rank, 'ok', res))
    except Exception:  # noqa
        import traceback
        q.put((rank, 'FAIL', traceback.format_exc()))


def test_two_replica_step_vs_the_one_replica_sinkhorn_and_the_gathered_batch():
    """Two gloo ranks sharing one GPU.  Both ranks' alpha is bitwise the alpha ONE replica computes on the gathered batch; each rank's
    loss is the restatement's on its own rows under that alpha and the mean of the two is the restatement's on the gathered batch; the
    row gradients are the gathered batch's slices and the prototype gradient the optimizer is handed (after the gradient synchronisation
    summed the two shares) is the gathered batch's on both ranks."""
    import torch.multiprocessing as mp
    from simclr_amd import ops
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
    for name in ('vs', 'w', 'z_all', 'alpha'):
        assert boxes[0][name].tobytes() == boxes[1][name].tobytes(), name
    vs = boxes[0]['vs']
    cat = lambda name: np.concatenate([boxes[0][name][:B], boxes[1][name][:B], boxes[0][name][B:], boxes[1][name][B:]])
    whole = swav_loss(cat('q'), vs, 0.1, 0.05, 3)
    assert boxes[0]['z_all'].shape == (4 * B, 64) and np.abs(boxes[0]['z_all'] - whole['qh']).max() <= 1e-6      # view-major
    # one replica, the gathered batch: the same launches in the same order
    one = ops.swav_sinkhorn(_dev(boxes[0]['z_all']), _dev(boxes[0]['w']), 0.05, 3)
    torch.cuda.synchronize()
    assert _np(one).tobytes() == boxes[0]['alpha'].tobytes(), 'the two-replica alpha is not bitwise the one-replica alpha'
    out = [_res('two_replica_alpha vs the gathered batch', boxes[0]['alpha'], whole['alpha'], 0, ALPHA_TOL),
           _res('two_replica_loss_mean vs the gathered batch', 0.5 * (boxes[0]['loss'] + boxes[1]['loss']), whole['loss'], GATE_LOSS),
           _res('two_replica_entropy_mean vs the gathered batch', 0.5 * (boxes[0]['entropy'] + boxes[1]['entropy']), whole['entropy'],
                GATE_LOSS)]
    for r, b in enumerate(boxes):
        ref = swav_loss(b['q'], vs, 0.1, 0.05, 3, grad_scale=0.5, z_all=whole['qh'])
        idx = np.concatenate([np.arange(r * B, (r + 1) * B), 2 * B + np.arange(r * B, (r + 1) * B)])
        out += [_res('two_replica_loss rank %d' % r, b['loss'], ref['loss'], GATE_LOSS),
                _res('two_replica_d_proj rank %d' % r, b['d_proj'], ref['grad_q'], GATE_GRAD),
                _res('two_replica_d_proj rank %d vs the gathered batch' % r, b['d_proj'], whole['grad_q'][idx], GATE_GRAD),
                _res('two_replica_prototype_grad rank %d vs the gathered batch' % r, b['proto_grad'], whole['grad_v'], GATE_GRAD)]
    _assert(out)
