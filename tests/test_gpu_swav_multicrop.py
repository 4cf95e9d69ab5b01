"""SwAV multi-crop on the GPU: the kernels of csrc/swav_multicrop.hip against the float64 restatement (tests/swav_multicrop_reference.py)
on the shared cases -- alpha, u and the global row_stats are the REFERENCE's, rounded to float32 once, never the kernel's own --, the
pairing of local rows with their image, repeat calls, refusals; add_swav_local_loss through the prototype head; the two-pass step at three
shapes; run.main (bitwise resume, the other modes, L = 0 against no flag); two replicas over gloo.

Tolerances: the kernels are held to 4 x the worst float32-emulation error of the restatement over the cases (swav_multicrop_reference.TOL,
re-measured on the CPU by tests/test_swav_multicrop_reference.py).  The layer and step tests read alpha from the device Sinkhorn, whose own
error budget is ALPHA_TOL; they are held to the project's gates for this arithmetic (GATE_LOSS / GATE_GRAD of tests/swav_reference.py), as
the same quantities are in tests/test_gpu_swav.py."""
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

from tests import swav_multicrop_reference as mr
from tests.gpu_checks import DEV, _res, structured_images
from tests.swav_reference import ALPHA_TOL, GATE_GRAD, GATE_LOSS, l2_normalize, l2_normalize_bwd, sinkhorn_potentials

pytestmark = pytest.mark.gpu
NCLS = 4


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


# ---------------------------------------------------------------------------------------------------------------- the kernels
def _launch(r, L, scale=1.0):
    from simclr_amd import ops
    x, w, u, z, al, grs = (_dev(r[k]) for k in ('xh', 'w', 'u32', 'qh', 'alpha', 'grs32'))
    out, stats, wsp = ops.swav_local_fwd(x, w, u, L, mr.MC_T)
    dx = ops.swav_local_bwd_x(x, w, u, L, mr.MC_T, stats, scale, wsp)
    dw = ops.swav_local_bwd_w(x, z, w, al, L, mr.MC_T, mr.MC_EPS, stats, grs, scale, wsp)
    torch.cuda.synchronize()
    return out, stats, dx, dw


@pytest.mark.parametrize('b,L,K,D', mr.MC_CASES)
def test_kernels_vs_float64(b, L, K, D):
    """Loss, row statistics, dx and dw against float64 within 4 x the float32-emulation error; a second call is bitwise the first; the
    reference with every local row paired to the NEXT image misses the same tolerances by more than 100 x (b > 1)."""
    r = mr.case_reference(b, L, K, D)
    tag = 'b=%d L=%d K=%d D=%d ' % (b, L, K, D)
    out, stats, dx, dw = _launch(r, L)
    res = [_res(tag + 'loss', out[0:1], r['local_loss'], mr.TOL['loss']), _res(tag + 'row_stats', stats, r['row_stats'], mr.TOL['row_stats']),
           _res(tag + 'grad_x', dx, r['grad_x'], mr.TOL['grad_x']), _res(tag + 'grad_w', dw, r['grad_w_local'], mr.TOL['grad_w'])]
    again = _launch(r, L)
    for name, a, c in zip(('loss', 'row_stats', 'grad_x', 'grad_w'), (out, stats, dx, dw), again):
        assert torch.equal(a, c), tag + name + ': a second call is not bitwise the first'
    half = _launch(r, L, scale=0.5)
    res += [_res(tag + 'grad_x scale=0.5', half[2], 0.5 * r['grad_x'], mr.TOL['grad_x']),
            _res(tag + 'grad_w scale=0.5', half[3], 0.5 * r['grad_w_local'], mr.TOL['grad_w'])]
    if b > 1:
        s = mr.multicrop_loss_normalized(r['qh'], r['xh'], r['w'], r['alpha'], mr.MC_T, mr.MC_EPS, shift=1)
        for name, got, ref in (('loss', out[0:1], s['local_loss']), ('grad_x', dx, s['grad_x']), ('grad_w', dw, s['grad_w_local'])):
            miss = _res(tag + name + ' vs the mis-paired reference', got, ref, mr.TOL[name])
            print('     %-86s err=%.3e tol=%.3e' % (miss['name'], miss['err'], miss['tol']))
            assert miss['err'] > 100.0 * miss['tol'], miss
    _assert(res)


def test_splits_follow_the_shape():
    """The cases reach several key splits of the statistics sweep and several row splits of both key-side sweeps."""
    from simclr_amd import ops
    assert ops.swav_local_key_splits(1, 1, 4097) == 65 and ops.swav_local_key_splits(70, 1, 4097) >= 2
    assert ops.swav_local_key_splits(33, 2, 2) == 1
    assert ops.swav_local_row_splits(33, 2, 2) == (2, 2)           # 66 local rows, 66 global rows: two 64-row tiles each
    assert ops.swav_local_row_splits(70, 1, 65) == (2, 3)          # 70 local rows, 140 global rows
    assert ops.swav_local_row_splits(11, 6, 4097) == (2, 1)
    assert ops.swav_local_row_splits(1, 1, 2) == (1, 1)
    with pytest.raises(ValueError, match='swav_local'):
        ops.swav_local_key_splits(4, 9, 16)


def test_refusals_return_the_error_code_and_launch_nothing():
    from simclr_amd import ops
    from simclr_amd._lib import lib
    b, L, K, D = 4, 2, 16, 64
    x, z, w, u, al = (torch.zeros(s, device=DEV) for s in ((L * b, D), (2 * b, D), (K, D), (2 * b, D), (2, K)))
    out = torch.full((1,), 7.0, device=DEV)
    stats, grs, dx, dw = (torch.full(s, 7.0, device=DEV) for s in ((L * b,), (2 * b, 2), (L * b, D), (K, D)))
    wsp = torch.full((lib().swav_local_workspace_bytes(b, L, K, D) // 4,), 7.0, device=DEV)
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    F = ctypes.c_float
    raw = lib()._dll
    nan = float('nan')
    ok = dict(x=P(x), z=P(z), w=P(w), u=P(u), a=P(al), b=b, L=L, K=K, D=D, T=0.1, eps=0.05, ws=P(wsp), st=P(stats), grs=P(grs),
              out=P(out), dx=P(dx), dw=P(dw))
    bad = [dict(D=100), dict(D=32), dict(D=512), dict(b=0), dict(b=-3), dict(L=0), dict(L=9), dict(L=-1), dict(K=1), dict(K=0),
           dict(K=1048577), dict(T=0.0), dict(T=-0.5), dict(T=nan), dict(eps=0.0), dict(eps=nan), dict(x=None), dict(w=None), dict(u=None),
           dict(z=None), dict(a=None), dict(ws=None), dict(st=None), dict(grs=None), dict(out=None), dict(dx=None), dict(dw=None),
           dict(x=P(x, 4)), dict(w=P(w, 4)), dict(u=P(u, 4)), dict(z=P(z, 4)), dict(ws=P(wsp, 4)), dict(dx=P(dx, 4)), dict(dw=P(dw, 4))]
    for change in bad:
        a = dict(ok, **change)
        keys = set(change)
        if not keys & {'eps', 'z', 'a', 'grs', 'dx', 'dw'}:
            assert raw.simclr_swav_local_fwd(a['x'], a['w'], a['u'], a['b'], a['L'], a['K'], a['D'], F(a['T']), a['out'], a['st'], a['ws'],
                                             None) == 1, change
            assert 'swav_local_fwd' in lib().last_error()
        if not keys & {'eps', 'z', 'a', 'grs', 'out', 'dw'}:
            assert raw.simclr_swav_local_bwd_x(a['x'], a['w'], a['u'], a['b'], a['L'], a['K'], a['D'], F(a['T']), a['st'], F(1.0), a['dx'],
                                               a['ws'], None) == 1, change
            assert 'swav_local_bwd_x' in lib().last_error()
        if not keys & {'u', 'out', 'dx'}:
            assert raw.simclr_swav_local_bwd_w(a['x'], a['z'], a['w'], a['a'], a['b'], a['L'], a['K'], a['D'], F(a['T']), F(a['eps']),
                                               a['st'], a['grs'], F(1.0), a['dw'], a['ws'], None) == 1, change
            assert 'swav_local_bwd_w' in lib().last_error()
    for args in ((b, L, K, 100), (0, L, K, D), (b, 0, K, D), (b, 9, K, D), (b, L, 1, D), (b, L, 1048577, D)):
        assert lib().swav_local_workspace_bytes(*args) == 0
    assert lib().swav_local_key_splits(0, 1, 16) == 0 and lib().swav_local_row_splits(4, 9, 16) == 0
    assert lib().swav_local_code_row_splits(4, 1, 1) == 0
    with pytest.raises(ValueError, match='local views lies in'):
        ops.swav_local_fwd(x, w, u, 9, 0.1)
    with pytest.raises(ValueError, match='global block'):
        ops.swav_local_fwd(x, w, u[:6], L, 0.1)
    with pytest.raises(ValueError, match='widths 64/128/256'):
        ops.swav_local_fwd(torch.zeros(8, 100, device=DEV), torch.zeros(4, 100, device=DEV), torch.zeros(8, 100, device=DEV), 2, 0.1)
    with pytest.raises(ValueError, match='workspace is smaller'):
        ops.swav_local_bwd_x(x, w, u, L, 0.1, stats, 1.0, torch.zeros(4, device=DEV))
    with pytest.raises(ValueError, match='row_stats'):
        ops.swav_local_bwd_x(x, w, u, L, 0.1, torch.zeros(L * b, 2, device=DEV), 1.0, wsp)
    with pytest.raises(ValueError, match='must be > 0'):
        ops.swav_local_fwd(x, w, u, L, 0.0)
    torch.cuda.synchronize()
    for t in (out, stats, grs, dx, dw, wsp):
        assert bool((t == 7.0).all())                     # nothing was written


# ---------------------------------------------------------------------------------------------------------------- layers
K_STEP, SPE = 200, 2          # prototypes of the small network; steps per epoch of the freeze


def _fresh_runtime():
    from simclr_amd.resnet import RT
    RT.reset()
    RT.device = torch.device(DEV)
    return RT


def _flags(image_size=32, batch=16, **kw):
    from simclr_amd.flags import FLAGS
    FLAGS.reset()
    kw.setdefault('proj_out_dim', 64)
    kw.setdefault('contrastive_loss', 'swav')
    kw.setdefault('use_blur', False)
    kw.setdefault('swav_num_prototypes', K_STEP)
    kw.setdefault('swav_freeze_prototypes_epochs', 0)
    FLAGS.update(resnet_depth=18, image_size=image_size, compute_dtype='f32', f32_matmul='exact', train_mode='pretrain', train_steps=10,
                 train_batch_size=batch, **kw)
    return FLAGS


def _batch(n, size, local, L, seed=31):
    g = torch.Generator().manual_seed(seed)
    images = structured_images(n, size, 2, g)
    ids = torch.randint(0, NCLS, (n,), generator=g)
    locs = structured_images(n, local, L, g)
    return images, locs, ids


def _build(strategy=None, lr=0.1):
    from simclr_amd import model as model_lib
    from simclr_amd.run import make_single_step
    model = model_lib.Model(NCLS)
    opt = model_lib.build_optimizer(lr)
    return model, opt, make_single_step(model, opt, strategy, steps_per_epoch=SPE)


def _reference(q, x, vs, grad_scale=1.0, z_all=None):
    """The float64 reference on captured RAW projections q [2b, D], x [L b, D] and the raw prototype variable vs: the Sinkhorn on the
    normalised global rows (or the gathered z_all), the u / m form, the gradients carried through the three row normalisations."""
    qh, ssq = l2_normalize(q)
    xh, ssx = l2_normalize(x)
    w, ssw = l2_normalize(vs)
    alpha, _ = sinkhorn_potentials(qh if z_all is None else z_all, w, 0.05, 3)
    r = mr.multicrop_loss_normalized(qh, xh, w, alpha, 0.1, 0.05, grad_scale)
    r.update(alpha=alpha, qh=qh, grad_q_raw=l2_normalize_bwd(qh, ssq, r['grad_q']), grad_x_raw=l2_normalize_bwd(xh, ssx, r['grad_x']),
             grad_v=l2_normalize_bwd(w, ssw, r['grad_w']), grad_v_local=l2_normalize_bwd(w, ssw, r['grad_w_local']),
             grad_v_global=l2_normalize_bwd(w, ssw, r['grad_w_global']))
    return r


def test_add_swav_local_loss_vs_float64_through_the_prototype_head():
    """b = 33, L = 2, K = 200, D = 64, the Sinkhorn and the global loss on the device: the local value, the gradient of the raw local
    projections and the gradient of the RAW prototype variable (student and code term together) against the restatement."""
    from simclr_amd import model as model_lib
    from simclr_amd import objective as obj_lib
    _flags()
    _fresh_runtime()
    b, L, K, D = 33, 2, 200, 64
    g = np.random.default_rng(8)
    head = model_lib.PrototypeHead(K)
    head.build(D)
    head.kernel.value.copy_(_dev(g.standard_normal((K, D)) * (0.5 + g.random((K, 1)))))       # rows of many norms
    vs = _np(head.kernel.value)
    a = g.standard_normal((b, D))
    q = np.concatenate([a, a + 0.5 * g.standard_normal((b, D))]).astype(np.float32)
    x = (np.tile(a, (L, 1)) + 0.7 * g.standard_normal((L * b, D))).astype(np.float32) * 3.0
    res = []
    for scale in (1.0, 0.5):
        ref = _reference(q, x, vs, grad_scale=scale)
        gl = obj_lib.add_swav_loss(_dev(q), head, 0.1, 0.05, 3)
        gl.backward(scale / (L + 1))
        loc = obj_lib.add_swav_local_loss(_dev(x), gl, head, 0.1)
        dx = loc.backward(scale)
        assert head.saved is None
        res += [_res('layer grad_x scale=%g' % scale, dx, ref['grad_x_raw'], GATE_GRAD),
                _res('layer grad_v (local share) scale=%g' % scale, head.kernel.grad, ref['grad_v_local'], GATE_GRAD)]
    res += [_res('layer local loss', loc.value, ref['local_loss'], GATE_LOSS), _res('layer alpha', gl.alpha, ref['alpha'], 0, ALPHA_TOL)]
    # frozen: neither key-side launch, the gradient slot keeps what it held
    before = head.kernel.grad.clone()
    loc = obj_lib.add_swav_local_loss(_dev(x), gl, head, 0.1, update_prototypes=False)
    dx2 = loc.backward(0.5)
    torch.cuda.synchronize()
    assert torch.equal(dx2, dx) and torch.equal(head.kernel.grad, before) and head.saved is None
    with pytest.raises(ValueError, match='L views of the 33 images'):
        obj_lib.add_swav_local_loss(_dev(x[:40]), gl, head, 0.1)
    _assert(res)


# ---------------------------------------------------------------------------------------------------------------- the step
def _capture(setattr_fn, model, opt):
    """Records the projections both loss calls are handed, what they hand the model's backward and the prototype gradient the optimizer
    is handed."""
    from simclr_amd import objective as obj_lib
    box = {'d_proj': []}
    orig_g, orig_l, orig_backward, orig_apply = obj_lib.add_swav_loss, obj_lib.add_swav_local_loss, model.backward, opt.apply_gradients

    def global_fn(online, prototypes, *a, **kw):
        box.update(q=online.detach().clone(), update=kw.get('update_prototypes'))
        box['global'] = orig_g(online, prototypes, *a, **kw)
        box['vs'] = prototypes.kernel.value.detach().clone()
        return box['global']

    def local_fn(local_online, global_loss, prototypes, *a, **kw):
        assert global_loss is box['global']
        box.update(x=local_online.detach().clone(), local_update=kw.get('update_prototypes'))
        box['vs_b'] = prototypes.kernel.value.detach().clone()
        box['local'] = orig_l(local_online, global_loss, prototypes, *a, **kw)
        return box['local']

    def backward(d_proj, *a, **kw):
        box['d_proj'].append(d_proj.detach().clone())
        return orig_backward(d_proj, *a, **kw)

    def apply(pairs, *a, **kw):
        pairs = list(pairs)
        box['applied'] = [v.name for _, v in pairs]
        g = model.prototype_head.kernel.grad
        box['proto_grad'] = None if g is None else g.detach().clone()
        box['flat'] = model._flat_grads.detach().clone()
        return orig_apply(pairs, *a, **kw)
    setattr_fn(obj_lib, 'add_swav_loss', global_fn)
    setattr_fn(obj_lib, 'add_swav_local_loss', local_fn)
    setattr_fn(model, 'backward', backward)
    setattr_fn(opt, 'apply_gradients', apply)
    return box


# image_size, local size, L, batch: 32 / 16; 32 / 24 with six views -- pass B has MORE convolution rows than pass A (6 * 24^2 > 2 * 32^2),
# which a buffer sized by the first shape seen does not survive; 128 / 96: the real local shape on the 7x7 stem
STEP_SHAPES = [(32, 16, 2, 16), (32, 24, 6, 8), (128, 96, 2, 4)]


@pytest.mark.parametrize('size,local,L,batch', STEP_SHAPES)
def test_two_pass_step_vs_float64_on_its_own_projections(monkeypatch, size, local, L, batch):
    """The prototype gradient the optimizer is handed is dW_A / (V - 1) + dW_B of the float64 reference on the projections the step
    itself produced (it is dW_B alone if pass B overwrites pass A, and misses by the whole of dW_A); the total loss, both row
    gradients; the supervised head's gradient is pass A's alone (not doubled by the add)."""
    _flags(image_size=size, batch=batch, swav_local_crops=L, swav_local_crop_size=local)
    _fresh_runtime()
    model, opt, step = _build()
    box = _capture(monkeypatch.setattr, model, opt)
    images, locs, ids = _batch(batch, size, local, L)
    labels = {'labels': torch.nn.functional.one_hot(ids, NCLS).float().to(DEV)}
    out = step((images.to(DEV), locs.to(DEV)), labels)
    torch.cuda.synchronize()
    assert tuple(box['q'].shape) == (2 * batch, 64) and tuple(box['x'].shape) == (L * batch, 64)
    assert box['update'] is True and box['local_update'] is True and torch.equal(box['vs'], box['vs_b'])
    ref = _reference(_np(box['q']), _np(box['x']), _np(box['vs']))
    con = out['con_loss']
    assert len(box['d_proj']) == 2
    res = [_res('step total loss', con.value, ref['loss'], GATE_LOSS),
           _res('step global value', box['global'].value, ref['global_loss'] * (L + 1), GATE_LOSS),
           _res('step local value', box['local'].value, ref['local_loss'], GATE_LOSS),
           _res('step alpha', con.alpha, ref['alpha'], 0, ALPHA_TOL),
           _res('step d_proj pass A', box['d_proj'][0], ref['grad_q_raw'], GATE_GRAD),
           _res('step d_proj pass B', box['d_proj'][1], ref['grad_x_raw'], GATE_GRAD),
           _res('step prototype grad = dW_A / (V-1) + dW_B', box['proto_grad'], ref['grad_v'], GATE_GRAD)]
    for part in ('grad_v_local', 'grad_v_global'):
        miss = _res('step prototype grad vs %s alone' % part, box['proto_grad'], ref[part], GATE_GRAD)
        assert not miss['ok'], miss
    assert step.metrics['train/contrast_loss'].result() == float(con.value)
    assert step.metrics['train/swav_code_entropy'].result() == float(con.entropy)
    assert 'model/prototype_head/kernel:0' in box['applied']
    sup = model.supervised_head.linear_layer.kernel
    assert bool((sup.grad != 0).any()) and bool(torch.isfinite(box['flat']).all())
    _assert(res)
    assert all(bool(torch.isfinite(v.value).all()) for v in model.variables)
    # a second step on the same buffers (the larger pass-B shape has been seen now)
    out2 = step((images.to(DEV), locs.to(DEV)), labels)
    torch.cuda.synchronize()
    assert math.isfinite(float(out2['con_loss'].value)) and float(out2['con_loss'].value) != float(con.value)


def test_supervised_head_gradient_is_pass_a_alone(monkeypatch):
    """With the same global views, the supervised head's gradient of a multi-crop step is bitwise the plain swav step's: the head is
    trained in pass A only and the saved buffer is added onto zeros."""
    grads = []
    for L in (0, 2):
        _flags(swav_local_crops=L, swav_local_crop_size=16)
        _fresh_runtime()
        model, opt, step = _build()
        box = _capture(monkeypatch.setattr, model, opt)
        images, locs, ids = _batch(16, 32, 16, 2)
        labels = {'labels': torch.nn.functional.one_hot(ids, NCLS).float().to(DEV)}
        step((images.to(DEV), locs.to(DEV)) if L else images.to(DEV), labels)
        torch.cuda.synchronize()
        k = model.supervised_head.linear_layer.kernel
        off = model._flat_offsets[[id(v) for v in model._flat_order].index(id(k))]
        grads.append(box['flat'][off:off + k.numel()].clone())
    assert torch.equal(grads[0], grads[1]) and bool((grads[0] != 0).any())


def test_frozen_prototypes_stay_bitwise_unchanged(monkeypatch):
    _flags(swav_local_crops=2, swav_local_crop_size=16, swav_freeze_prototypes_epochs=1)
    _fresh_runtime()
    model, opt, step = _build()
    name = 'model/prototype_head/kernel:0'
    box = _capture(monkeypatch.setattr, model, opt)
    images, locs, ids = _batch(16, 32, 16, 2)
    labels = {'labels': torch.nn.functional.one_hot(ids, NCLS).float().to(DEV)}
    model(torch.zeros(2, 32, 32, 3, device=DEV), training=False)
    model.release()
    model.prototype_head.build(64)
    proto = model.prototype_head.kernel
    p0 = proto.value.clone()
    for s in (0, 1):
        step((images.to(DEV), locs.to(DEV)), labels)
        torch.cuda.synchronize()
        assert box['update'] is False and box['local_update'] is False and name not in box['applied'], s
        assert torch.equal(proto.value, p0) and id(proto) not in opt._slots, s
    step((images.to(DEV), locs.to(DEV)), labels)
    torch.cuda.synchronize()
    assert box['update'] is True and box['local_update'] is True and name in box['applied']
    assert not torch.equal(proto.value, p0) and bool(torch.isfinite(proto.value).all())


# ---------------------------------------------------------------------------------------------------------------- run.main
ARGS = ['--dataset=synthetic', '--resnet_depth=18', '--image_size=32', '--train_batch_size=8', '--use_blur=False', '--compute_dtype=f32',
        '--checkpoint_steps=2', '--train_steps=3', '--mode=train', '--proj_out_dim=64', '--swav_num_prototypes=200',
        '--swav_freeze_prototypes_epochs=0', '--contrastive_loss=swav']


def _same(a, b):
    assert sorted(a['model']) == sorted(b['model'])
    assert all(torch.equal(a['model'][n], b['model'][n]) for n in a['model'])
    assert all(torch.equal(a['optimizer']['slots'][n], b['optimizer']['slots'][n]) for n in a['optimizer']['slots'])
    assert a['optimizer']['iterations'] == b['optimizer']['iterations']


def test_run_main_resumes_bitwise_and_other_modes_read_the_file(tmp_path, capsys):
    from simclr_amd import run
    from simclr_amd.checkpoint import INDEX_NAME
    from simclr_amd.flags import FLAGS
    args = ARGS + ['--swav_local_crops=2', '--swav_local_crop_size=16']
    full_dir, again_dir, ft_dir = str(tmp_path / 'full'), str(tmp_path / 'again'), str(tmp_path / 'ft')
    FLAGS.reset()
    run.main(args + ['--model_dir=' + full_dir])
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith('{') and 'train/swav_code_entropy' in l]
    assert lines and lines[0]['step'] == 2
    for k in ('train/contrast_loss', 'train/swav_code_entropy', 'train/total_loss'):
        assert math.isfinite(lines[0][k]), (k, lines[0])
    full = torch.load(os.path.join(full_dir, 'ckpt-3.pt'), map_location='cpu')
    os.makedirs(again_dir)
    shutil.copy(os.path.join(full_dir, 'ckpt-2.pt'), os.path.join(again_dir, 'ckpt-2.pt'))
    with open(os.path.join(again_dir, INDEX_NAME), 'w') as f:
        json.dump({'model_checkpoint_path': 'ckpt-2.pt', 'all_model_checkpoint_paths': ['ckpt-2.pt']}, f)
    FLAGS.reset()
    run.main(args + ['--model_dir=' + again_dir])
    again = torch.load(os.path.join(again_dir, 'ckpt-3.pt'), map_location='cpu')
    _same(again, full)
    assert again['optimizer']['iterations'] == 3 and len(glob.glob(os.path.join(again_dir, 'ckpt-*.pt'))) == 2
    # evaluation, the k-NN evaluation and one fine-tuning step read the file; both ignore the multi-crop flags
    capsys.readouterr()
    FLAGS.reset()
    result = run.main(['--dataset=synthetic', '--resnet_depth=18', '--image_size=32', '--eval_batch_size=8', '--eval_steps=1',
                       '--compute_dtype=f32', '--mode=eval', '--contrastive_loss=swav', '--proj_out_dim=64', '--knn_eval=True',
                       '--knn_k=5', '--swav_local_crops=2', '--swav_local_crop_size=16', '--model_dir=' + full_dir])
    assert result['global_step'] == 3
    for k in ('eval/label_top_1_accuracy', 'eval/knn_top_1_accuracy'):
        assert 0.0 <= result[k] <= 1.0, (k, result)
    FLAGS.reset()
    run.main(['--dataset=synthetic', '--resnet_depth=18', '--image_size=32', '--train_batch_size=8', '--compute_dtype=f32', '--mode=train',
              '--train_mode=finetune', '--contrastive_loss=swav', '--proj_out_dim=64', '--train_steps=1', '--checkpoint_steps=1',
              '--swav_local_crops=2', '--swav_local_crop_size=16', '--checkpoint=' + os.path.join(full_dir, 'ckpt-3.pt'),
              '--model_dir=' + ft_dir])
    written = torch.load(os.path.join(ft_dir, 'ckpt-1.pt'), map_location='cpu')['model']
    assert not any('prototype_head' in n for n in written)


def test_run_main_without_local_crops_is_the_run_without_the_flag(tmp_path):
    from simclr_amd import run
    from simclr_amd.flags import FLAGS
    a_dir, b_dir, c_dir = str(tmp_path / 'a'), str(tmp_path / 'b'), str(tmp_path / 'c')
    short = [x for x in ARGS if not x.startswith('--train_steps')] + ['--train_steps=2']
    FLAGS.reset()
    run.main(short + ['--model_dir=' + a_dir])
    FLAGS.reset()
    run.main(short + ['--swav_local_crops=0', '--swav_local_crop_size=16', '--swav_local_crop_min_scale=0.2',
                      '--swav_local_crop_max_scale=0.3', '--model_dir=' + b_dir])
    a = torch.load(os.path.join(a_dir, 'ckpt-2.pt'), map_location='cpu')
    _same(a, torch.load(os.path.join(b_dir, 'ckpt-2.pt'), map_location='cpu'))
    FLAGS.reset()
    run.main(short + ['--swav_local_crops=2', '--swav_local_crop_size=16', '--model_dir=' + c_dir])
    c = torch.load(os.path.join(c_dir, 'ckpt-2.pt'), map_location='cpu')
    name = 'model/prototype_head/kernel:0'
    assert not torch.equal(a['model'][name], c['model'][name])
    with pytest.raises(ValueError, match='swav_local_crops belongs to'):
        FLAGS.reset()
        run.main([x for x in short if not x.startswith('--contrastive_loss')] + ['--contrastive_loss=dino', '--swav_local_crops=2'])


# ---------------------------------------------------------------------------------------------------------------- two replicas
B2, L2, LOCAL2 = 8, 2, 16


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
        _flags(batch=world * B2, swav_local_crops=L2, swav_local_crop_size=LOCAL2)
        RT = _fresh_runtime()
        strategy = comm.Strategy()
        RT.strategy = strategy
        model, opt, step = _build(strategy=strategy)
        attrs = {}
        box = _capture(lambda o, name, v: (attrs.setdefault((id(o), name), (o, name, getattr(o, name))), setattr(o, name, v)), model, opt)
        images, locs, ids = _batch(world * B2, 32, LOCAL2, L2, seed=51)
        sl = slice(rank * B2, (rank + 1) * B2)
        out = step((images[sl].to(DEV), locs[sl].to(DEV)), {'labels': torch.nn.functional.one_hot(ids[sl], NCLS).float().to(DEV)})
        torch.cuda.synchronize()
        res = dict(q=_np(box['q']), x=_np(box['x']), vs=_np(box['vs']), alpha=_np(box['global'].alpha),
                   proto_grad=_np(box['proto_grad']), local=float(box['local'].value), total=float(out['con_loss'].value))
        for o, name, v in attrs.values():
            setattr(o, name, v)
        dist.destroy_process_group()
        q.put((rank, 'ok', res))
    except Exception:  # noqa
        import traceback
        q.put((rank, 'FAIL', traceback.format_exc()))


def test_two_replica_step_vs_the_gathered_batch():
    """Two gloo ranks sharing one GPU.  alpha is bitwise the alpha ONE replica computes on the gathered global rows; each rank's local
    value is the restatement's on its own rows under that alpha -- its share of the one-replica loss on the gathered batch, whose value
    is the mean of the two; the prototype gradient after the ONE all-reduce is the gathered batch's on both ranks."""
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
    assert boxes[0]['vs'].tobytes() == boxes[1]['vs'].tobytes() and boxes[0]['alpha'].tobytes() == boxes[1]['alpha'].tobytes()
    vs = boxes[0]['vs']
    q_all = np.concatenate([boxes[0]['q'][:B2], boxes[1]['q'][:B2], boxes[0]['q'][B2:], boxes[1]['q'][B2:]])
    x_all = np.concatenate([boxes[r]['x'][v * B2:(v + 1) * B2] for v in range(L2) for r in range(2)])
    whole = _reference(q_all, x_all, vs)
    # one replica, the gathered batch: the same normalisations and the same launches in the same order
    zd, _ = ops.l2norm_fwd(_dev(q_all))
    wd, _ = ops.l2norm_fwd(_dev(vs))
    one = ops.swav_sinkhorn(zd, wd, 0.05, 3)
    torch.cuda.synchronize()
    assert _np(one).tobytes() == boxes[0]['alpha'].tobytes(), 'the two-replica alpha is not bitwise the one-replica alpha'
    out = [_res('two_replica alpha vs the gathered batch', boxes[0]['alpha'], whole['alpha'], 0, ALPHA_TOL),
           _res('two_replica local mean vs the gathered batch', 0.5 * (boxes[0]['local'] + boxes[1]['local']), whole['local_loss'],
                GATE_LOSS),
           _res('two_replica total mean vs the gathered batch', 0.5 * (boxes[0]['total'] + boxes[1]['total']), whole['loss'], GATE_LOSS)]
    for r, bx in enumerate(boxes):
        ref = _reference(bx['q'], bx['x'], vs, z_all=whole['qh'])
        out += [_res('two_replica local value rank %d' % r, bx['local'], ref['local_loss'], GATE_LOSS),
                _res('two_replica total value rank %d' % r, bx['total'], ref['loss'], GATE_LOSS),
                _res('two_replica prototype grad rank %d vs the gathered batch' % r, bx['proto_grad'], whole['grad_v'], GATE_GRAD)]
    _assert(out)
