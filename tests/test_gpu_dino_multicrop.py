"""DINO multi-crop on the GPU: simclr_dino_local_bwd_w (csrc/dino_multicrop.hip) and the loss-agnostic local sweeps it sits beside,
against the float64 restatement (tests/dino_multicrop_reference.py) on the shared cases -- u and the global row_stats are the
REFERENCE's, rounded to float32 once, never simclr_dino_fwd's own --, the split queries, repeat calls, the paired-lse_t miss, refusals;
add_dino_local_loss through the prototype head; the two-pass step; run.main (bitwise resume, L = 0 against no flag, the other modes);
two replicas over gloo.

Tolerances: the kernels are held to 4 x the worst float32-emulation error over the cases (dino_multicrop_reference.TOL, re-measured
on the CPU by tests/test_dino_multicrop_reference.py).  The layer and step tests run simclr_dino_fwd on the device, whose u and
row_stats carry that family's own error; they are held to the project's gates for this arithmetic (GATE_LOSS / GATE_GRAD of
tests/dino_reference.py), as the same quantities are in tests/test_gpu_dino.py."""
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

from tests import dino_multicrop_reference as mr
from tests import swav_multicrop_reference as smr
from tests.byol_reference import ema_f32
from tests.dino_reference import GATE_GRAD, GATE_LOSS, center_update, l2_normalize, l2_normalize_bwd
from tests.gpu_checks import DEV, _res, structured_images

pytestmark = pytest.mark.gpu
NCLS = 4
# the local row_stats are simclr_swav_local_fwd's output: the tolerance that family's own test holds them to
STATS_TOL = smr.TOL['row_stats']


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
def _launch(r, scale=1.0):
    from simclr_amd import ops
    x, k, ws, wt, c, u, grs = (_dev(r[n]) for n in ('xh', 'kh', 'ws', 'wt', 'c', 'u32', 'grs32'))
    L = r['L']
    out, stats, wsp = ops.swav_local_fwd(x, ws, u, L, r['Ts'])
    dx = ops.swav_local_bwd_x(x, ws, u, L, r['Ts'], stats, scale, wsp)
    dw = ops.dino_local_bwd_w(x, k, ws, wt, c, L, r['Ts'], r['Tt'], stats, grs, scale)
    torch.cuda.synchronize()
    return out, stats, dx, dw


@pytest.mark.parametrize('b,L,K,D,Tt,kind', mr.ALL_CASES)
def test_kernels_vs_float64(b, L, K, D, Tt, kind):
    """The local value, dx and the key-side gradient against float64 within 4 x the float32-emulation error; the local row_stats are
    lse_s in the base-2 domain; a second call is bitwise the first; the reference whose teacher rows are normalised with the PAIRED
    row's lse_t falls outside the grad_w tolerance."""
    r = mr.case_reference(b, L, K, D, Tt, kind)
    tag = 'b=%d L=%d K=%d D=%d Tt=%g %s ' % (b, L, K, D, Tt, kind)
    out, stats, dx, dw = _launch(r)
    res = [_res(tag + 'loss', out[0:1], r['local_loss'], mr.TOL['loss']), _res(tag + 'row_stats (lse_s, base 2)', stats, r['row_stats'], STATS_TOL),
           _res(tag + 'grad_x', dx, r['grad_x'], mr.TOL['grad_x']), _res(tag + 'grad_w', dw, r['grad_w_local'], mr.TOL['grad_w'])]
    again = _launch(r)
    for name, a, c in zip(('loss', 'row_stats', 'grad_x', 'grad_w'), (out, stats, dx, dw), again):
        assert torch.equal(a, c), tag + name + ': a second call is not bitwise the first'
    half = _launch(r, scale=0.5)
    res += [_res(tag + 'grad_x scale=0.5', half[2], 0.5 * r['grad_x'], mr.TOL['grad_x']),
            _res(tag + 'grad_w scale=0.5', half[3], 0.5 * r['grad_w_local'], mr.TOL['grad_w'])]
    miss = _res(tag + 'grad_w vs the reference with the paired lse_t', dw, mr.paired_reference(b, L, K, D, Tt, kind), mr.TOL['grad_w'])
    print('     %-86s err=%.3e tol=%.3e' % (miss['name'], miss['err'], miss['tol']))
    assert miss['err'] > 100.0 * miss['tol'], miss
    _assert(res)


def test_splits_follow_the_shape():
    """The cases reach several row splits of both key-side sweeps, and the queries agree with the restatement's plan."""
    from simclr_amd import ops
    assert ops.dino_local_row_splits(33, 2, 2) == (2, 2)           # 66 local rows, 66 global rows: two 64-row tiles each
    assert ops.dino_local_row_splits(70, 1, 2) == (2, 3)           # 70 local rows, 140 global rows
    assert ops.dino_local_row_splits(70, 1, 65) == (2, 3)
    assert ops.dino_local_row_splits(11, 6, 4097) == (2, 1)
    assert ops.dino_local_row_splits(1, 1, 2) == (1, 1)
    assert ops.dino_local_row_splits(512, 6, 65536) == (1, 1)
    for b, L, K, _ in mr.MC_CASES:
        assert ops.dino_local_row_splits(b, L, K) == mr.row_splits(b, L, K), (b, L, K)
    with pytest.raises(ValueError, match='dino_local'):
        ops.dino_local_row_splits(4, 9, 16)


def test_refusals_return_the_error_code_and_launch_nothing():
    from simclr_amd import ops
    from simclr_amd._lib import lib
    b, L, K, D = 4, 2, 16, 64
    x, k, ws, wt, c = (torch.zeros(s, device=DEV) for s in ((L * b, D), (2 * b, D), (K, D), (K, D), (K,)))
    stats, grs, dw = (torch.full(s, 7.0, device=DEV) for s in ((L * b,), (2 * b, 2), (K, D)))
    wsp = torch.full((lib().dino_local_workspace_bytes(b, L, K, D) // 4,), 7.0, device=DEV)
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    F = ctypes.c_float
    raw = lib()._dll
    nan = float('nan')
    ok = dict(x=P(x), k=P(k), ws=P(ws), wt=P(wt), c=P(c), b=b, L=L, K=K, D=D, Ts=0.1, Tt=0.04, st=P(stats), grs=P(grs), dw=P(dw), w=P(wsp))
    bad = [dict(D=100), dict(D=32), dict(D=512), dict(b=0), dict(b=-3), dict(L=0), dict(L=9), dict(L=-1), dict(K=1), dict(K=0),
           dict(K=1048577), dict(Ts=0.0), dict(Ts=-0.5), dict(Ts=nan), dict(Tt=0.0), dict(Tt=-1.0), dict(Tt=nan), dict(x=None),
           dict(k=None), dict(ws=None), dict(wt=None), dict(c=None), dict(st=None), dict(grs=None), dict(dw=None), dict(w=None),
           dict(x=P(x, 4)), dict(k=P(k, 4)), dict(ws=P(ws, 4)), dict(wt=P(wt, 8)), dict(dw=P(dw, 4)), dict(w=P(wsp, 4)),
           dict(grs=P(grs, 4)), dict(c=P(c, 2)), dict(st=P(stats, 2))]
    for change in bad:
        a = dict(ok, **change)
        assert raw.simclr_dino_local_bwd_w(a['x'], a['k'], a['ws'], a['wt'], a['c'], a['b'], a['L'], a['K'], a['D'], F(a['Ts']), F(a['Tt']),
                                           a['st'], a['grs'], F(1.0), a['dw'], a['w'], None) == 1, change
        assert 'dino_local_bwd_w' in lib().last_error()
    for args in ((b, L, K, 100), (0, L, K, D), (b, 0, K, D), (b, 9, K, D), (b, L, 1, D), (b, L, 1048577, D)):
        assert lib().dino_local_workspace_bytes(*args) == 0
    assert lib().dino_local_row_splits(0, 1, 16) == 0 and lib().dino_local_row_splits(4, 9, 16) == 0
    assert lib().dino_local_teacher_row_splits(4, 1, 1) == 0
    real_stats, real_grs = torch.zeros(L * b, device=DEV), torch.zeros(2 * b, 2, device=DEV)
    with pytest.raises(ValueError, match='local views lies in'):
        ops.dino_local_bwd_w(x, k, ws, wt, c, 9, 0.1, 0.04, real_stats, real_grs, 1.0)
    with pytest.raises(ValueError, match='global block'):
        ops.dino_local_bwd_w(x, k[:6], ws, wt, c, L, 0.1, 0.04, real_stats, real_grs, 1.0)
    with pytest.raises(ValueError, match='widths 64/128/256'):
        ops.dino_local_bwd_w(torch.zeros(8, 100, device=DEV), torch.zeros(8, 100, device=DEV), torch.zeros(4, 100, device=DEV),
                             torch.zeros(4, 100, device=DEV), torch.zeros(4, device=DEV), 2, 0.1, 0.04, real_stats, real_grs, 1.0)
    with pytest.raises(ValueError, match='workspace is smaller'):         # a short workspace
        ops.dino_local_bwd_w(x, k, ws, wt, c, L, 0.1, 0.04, real_stats, real_grs, 1.0, torch.zeros(4, device=DEV))
    with pytest.raises(ValueError, match='row_stats'):
        ops.dino_local_bwd_w(x, k, ws, wt, c, L, 0.1, 0.04, torch.zeros(L * b, 2, device=DEV), real_grs, 1.0)
    with pytest.raises(ValueError, match='row_stats'):
        ops.dino_local_bwd_w(x, k, ws, wt, c, L, 0.1, 0.04, real_stats, torch.zeros(2 * b, device=DEV), 1.0)
    with pytest.raises(ValueError, match='teacher temperature'):
        ops.dino_local_bwd_w(x, k, ws, wt, c, L, 0.1, nan, real_stats, real_grs, 1.0)
    with pytest.raises(ValueError, match='student temperature'):
        ops.dino_local_bwd_w(x, k, ws, wt, c, L, 0.0, 0.04, real_stats, real_grs, 1.0)
    torch.cuda.synchronize()
    for t in (stats, grs, dw, wsp):
        assert bool((t == 7.0).all())                     # nothing was written


# ---------------------------------------------------------------------------------------------------------------- layers
K_STEP, SPE = 200, 2          # prototypes of the small network; steps per epoch of its schedules


def _fresh_runtime():
    from simclr_amd.resnet import RT
    RT.reset()
    RT.device = torch.device(DEV)
    return RT


def _flags(image_size=32, batch=16, **kw):
    from simclr_amd.flags import FLAGS
    FLAGS.reset()
    kw.setdefault('proj_out_dim', 64)
    kw.setdefault('contrastive_loss', 'dino')
    kw.setdefault('use_blur', False)
    kw.setdefault('dino_out_dim', K_STEP)
    kw.setdefault('dino_momentum', 0.9)
    kw.setdefault('dino_freeze_last_layer_epochs', 0)
    FLAGS.update(resnet_depth=18, image_size=image_size, compute_dtype='f32', f32_matmul='exact', train_mode='pretrain', train_steps=10,
                 train_batch_size=batch, **kw)
    return FLAGS


def _batch(n, size, local, L, seed=31):
    g = torch.Generator().manual_seed(seed)
    images = structured_images(n, size, 2, g)
    ids = torch.randint(0, NCLS, (n,), generator=g)
    locs = structured_images(n, local, L, g)
    return images, locs, ids


def _build(strategy=None, lr=0.1, steps=10):
    from simclr_amd import model as model_lib
    from simclr_amd.flags import FLAGS
    from simclr_amd.run import make_single_step
    model = model_lib.Model(NCLS)
    target = model_lib.TargetNetwork(model, steps, center=model_lib.DinoCenter(FLAGS.dino_out_dim), steps_per_epoch=SPE)
    opt = model_lib.build_optimizer(lr)
    return model, target, opt, make_single_step(model, opt, strategy, target=target)


def _reference(q, t, x, vs, wt, c, Ts=0.1, Tt=0.04, grad_scale=1.0):
    """The float64 reference on captured RAW projections q / t [2b, D], x [L b, D], the raw online prototype variable vs and the
    NORMALISED target prototypes wt: the u / m form, the gradients carried through the three row normalisations."""
    qh, ssq = l2_normalize(q)
    kh, _ = l2_normalize(t)
    xh, ssx = l2_normalize(x)
    ws, ssw = l2_normalize(vs)
    r = mr.multicrop_loss_normalized(qh, kh, xh, ws, wt, c, Ts, Tt, grad_scale)
    r.update(kh=kh, wt=np.asarray(wt, np.float64), grad_q_raw=l2_normalize_bwd(qh, ssq, r['grad_q']),
             grad_x_raw=l2_normalize_bwd(xh, ssx, r['grad_x']), grad_v=l2_normalize_bwd(ws, ssw, r['grad_w']),
             grad_v_local=l2_normalize_bwd(ws, ssw, r['grad_w_local']), grad_v_global=l2_normalize_bwd(ws, ssw, r['grad_w_global']))
    return r


def test_add_dino_local_loss_vs_float64_through_the_prototype_head():
    """b = 33, L = 2, K = 200, D = 64, the global loss on the device: the handle carries what the local loss reads; the local value, the
    gradient of the raw local projections and the gradient of the RAW prototype variable (student and teacher term together)."""
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
    q = np.concatenate([a + 0.4 * g.standard_normal((b, D)), a + 0.4 * g.standard_normal((b, D))]).astype(np.float32)
    t = (q + 0.5 * g.standard_normal((2 * b, D))).astype(np.float32)
    x = (np.tile(a, (L, 1)) + 0.7 * g.standard_normal((L * b, D))).astype(np.float32) * 3.0
    wt = l2_normalize(vs + 0.1 * g.standard_normal((K, D)))[0].astype(np.float32)
    c = (0.05 * g.standard_normal(K)).astype(np.float32)
    res = []
    for scale in (1.0, 0.5):
        ref = _reference(q, t, x, vs, wt, c, 0.1, 0.07, grad_scale=scale)
        gl = obj_lib.add_dino_loss(_dev(q), _dev(t), head, _dev(wt), _dev(c), 0.1, 0.07)
        gl.backward(scale / (L + 1))
        assert tuple(gl.z.shape) == tuple(gl.u.shape) == tuple(gl.keys.shape) == (2 * b, D) and tuple(gl.row_stats.shape) == (2 * b, 2)
        assert (gl.student_temp, gl.teacher_temp) == (0.1, 0.07) and torch.equal(gl.center, _dev(c))
        loc = obj_lib.add_dino_local_loss(_dev(x), gl, head)
        dx = loc.backward(scale)
        assert head.saved is None and tuple(dx.shape) == (L * b, D)
        res += [_res('layer grad_x scale=%g' % scale, dx, ref['grad_x_raw'], GATE_GRAD),
                _res('layer grad_v (local share) scale=%g' % scale, head.kernel.grad, ref['grad_v_local'], GATE_GRAD)]
    res += [_res('layer local loss', loc.value, ref['local_loss'], GATE_LOSS), _res('layer u (by row)', gl.u, ref['u'], GATE_GRAD)]
    # frozen: neither key-side launch, the gradient slot keeps what it held
    before = head.kernel.grad.clone()
    loc = obj_lib.add_dino_local_loss(_dev(x), gl, head, update_prototypes=False)
    dx2 = loc.backward(0.5)
    torch.cuda.synchronize()
    assert torch.equal(dx2, dx) and torch.equal(head.kernel.grad, before) and head.saved is None
    with pytest.raises(ValueError, match='L views of the 33 images'):
        obj_lib.add_dino_local_loss(_dev(x[:40]), gl, head)
    _assert(res)


# ---------------------------------------------------------------------------------------------------------------- the step
def _capture(setattr_fn, model, target, opt):
    """Records the projections both loss calls are handed (with the centre and the target prototypes as the loss saw them), what they
    hand the model's backward, the centre and the target prototypes at each backward, and the gradients the optimizer is handed."""
    from simclr_amd import objective as obj_lib
    box = {'d_proj': [], 'center_at_backward': [], 'target_at_backward': []}
    orig_g, orig_l, orig_backward, orig_apply = obj_lib.add_dino_loss, obj_lib.add_dino_local_loss, model.backward, opt.apply_gradients
    tproto = lambda: [v for v in target.variables if v.name == 'model/prototype_head/kernel:0'][0]

    def global_fn(online, tgt, prototypes, wt, center, *a, **kw):
        box.update(q=online.detach().clone(), t=tgt.detach().clone(), wt=wt.detach().clone(), center=center.detach().clone(),
                   Ts=kw.get('student_temp'), Tt=kw.get('teacher_temp'), update=kw.get('update_prototypes'))
        box['global'] = orig_g(online, tgt, prototypes, wt, center, *a, **kw)
        box['vs'] = prototypes.kernel.value.detach().clone()
        return box['global']

    def local_fn(local_online, global_loss, prototypes, *a, **kw):
        assert global_loss is box['global']
        box.update(x=local_online.detach().clone(), local_update=kw.get('update_prototypes'),
                   center_at_local=target.center.value.detach().clone())
        box['vs_b'] = prototypes.kernel.value.detach().clone()
        box['local'] = orig_l(local_online, global_loss, prototypes, *a, **kw)
        return box['local']

    def backward(d_proj, *a, **kw):
        box['d_proj'].append(d_proj.detach().clone())
        box['center_at_backward'].append(target.center.value.detach().clone())
        box['target_at_backward'].append(tproto().value.detach().clone())
        return orig_backward(d_proj, *a, **kw)

    def apply(pairs, *a, **kw):
        pairs = list(pairs)
        box['applied'] = [v.name for _, v in pairs]
        g = model.prototype_head.kernel.grad
        box['proto_grad'] = None if g is None else g.detach().clone()
        box['flat'] = model._flat_grads.detach().clone()
        return orig_apply(pairs, *a, **kw)
    setattr_fn(obj_lib, 'add_dino_loss', global_fn)
    setattr_fn(obj_lib, 'add_dino_local_loss', local_fn)
    setattr_fn(model, 'backward', backward)
    setattr_fn(opt, 'apply_gradients', apply)
    return box


# image_size, local size, L, batch: 32 / 16; 32 / 24 with six views -- pass B has MORE convolution rows than pass A (6 * 24^2 > 2 * 32^2)
STEP_SHAPES = [(32, 16, 2, 16), (32, 24, 6, 8)]


@pytest.mark.parametrize('size,local,L,batch', STEP_SHAPES)
def test_two_pass_step_vs_float64_on_its_own_projections(monkeypatch, size, local, L, batch):
    """The prototype gradient the optimizer is handed is dW_A / (V - 1) + dW_B of the float64 reference on the projections the step
    itself produced, taken with the centre and the target prototypes as they stood BEFORE the step; the total loss, both row gradients;
    the centre and the target move ONCE, after pass B, from the pre-step values."""
    from simclr_amd import model as model_lib
    _flags(image_size=size, batch=batch, dino_local_crops=L, dino_local_crop_size=local, dino_center_momentum=0.5)
    _fresh_runtime()
    model, target, opt, step = _build()
    assert sorted(step.metrics) == ['train/contrast_loss', 'train/dino_teacher_entropy', 'train/supervised_acc', 'train/supervised_loss',
                                    'train/total_loss', 'train/weight_decay']
    # a non-zero centre, and target prototypes that differ from the online ones: the pre-step state both passes must read
    g = np.random.default_rng(3)
    c0 = (0.05 * g.standard_normal(K_STEP)).astype(np.float32)
    target.center.value.copy_(_dev(c0))
    name = 'model/prototype_head/kernel:0'
    tproto = [v for v in target.variables if v.name == name][0]
    tproto.value.add_(_dev(0.003 * g.standard_normal((K_STEP, 64))))
    vt0 = _np(tproto.value).copy()
    box = _capture(monkeypatch.setattr, model, target, opt)
    images, locs, ids = _batch(batch, size, local, L)
    labels = {'labels': torch.nn.functional.one_hot(ids, NCLS).float().to(DEV)}
    out = step((images.to(DEV), locs.to(DEV)), labels)
    torch.cuda.synchronize()
    assert tuple(box['q'].shape) == tuple(box['t'].shape) == (2 * batch, 64) and tuple(box['x'].shape) == (L * batch, 64)
    assert box['update'] is True and box['local_update'] is True and torch.equal(box['vs'], box['vs_b'])
    assert box['Ts'] == 0.1 and box['Tt'] == float(np.float32(0.04))
    # both passes read the pre-step centre and target
    assert len(box['d_proj']) == 2 and _np(box['center']).tobytes() == c0.tobytes() and _np(box['center_at_local']).tobytes() == c0.tobytes()
    assert all(_np(c).tobytes() == c0.tobytes() for c in box['center_at_backward'])
    assert all(_np(v).tobytes() == vt0.tobytes() for v in box['target_at_backward'])
    ref = _reference(_np(box['q']), _np(box['t']), _np(box['x']), _np(box['vs']), _np(box['wt']), c0)
    con = out['con_loss']
    res = [_res('step total loss', con.value, ref['loss'], GATE_LOSS),
           _res('step global value', box['global'].value, ref['global_loss'] * (L + 1), GATE_LOSS),
           _res('step local value', box['local'].value, ref['local_loss'], GATE_LOSS),
           _res('step teacher entropy (pass A)', con.entropy, ref['entropy'], GATE_LOSS),
           _res('step wt', box['wt'], l2_normalize(vt0)[0], 0, 1e-6),
           _res('step d_proj pass A', box['d_proj'][0], ref['grad_q_raw'], GATE_GRAD),
           _res('step d_proj pass B', box['d_proj'][1], ref['grad_x_raw'], GATE_GRAD),
           _res('step prototype grad = dW_A / (V-1) + dW_B', box['proto_grad'], ref['grad_v'], GATE_GRAD)]
    for part in ('grad_v_local', 'grad_v_global'):
        miss = _res('step prototype grad vs %s alone' % part, box['proto_grad'], ref[part], GATE_GRAD)
        assert not miss['ok'], miss
    assert step.metrics['train/contrast_loss'].result() == float(con.value)
    assert step.metrics['train/dino_teacher_entropy'].result() == float(con.entropy) == float(box['global'].entropy)
    assert name in box['applied'] and bool(torch.isfinite(box['flat']).all())
    # the centre moved ONCE, from the pre-step target prototypes and the mean GLOBAL key (applied twice it would sit elsewhere)
    want = center_update(c0, ref['wt'], ref['kh'], 0.5)
    twice = center_update(want, ref['wt'], ref['kh'], 0.5)
    bound = 64 * 2.0 ** -24 * np.abs(ref['kh'] @ ref['wt'].T).max() + 2.0 ** -23 * np.abs(want).max()
    res.append(_res('step centre', target.center.value, want, 0, bound))
    assert np.abs(twice - want).max() > 100 * bound
    # the target prototypes moved ONCE by 1 - tau_0 towards the stepped online ones
    omt = np.float32(1.0 - model_lib.byol_tau(0, 10, 0.9))
    assert _np(tproto.value).tobytes() == ema_f32(vt0, _np(model.prototype_head.kernel.value), omt).tobytes()
    assert not np.array_equal(_np(tproto.value), vt0)
    _assert(res)
    assert all(bool(torch.isfinite(v.value).all()) for v in model.variables + target.variables + target.center.variables)
    # a second step on the same buffers (the larger pass-B shape has been seen now)
    out2 = step((images.to(DEV), locs.to(DEV)), labels)
    torch.cuda.synchronize()
    assert math.isfinite(float(out2['con_loss'].value)) and float(out2['con_loss'].value) != float(con.value)


def test_supervised_head_gradient_is_pass_a_alone(monkeypatch):
    """With the same global views, the supervised head's gradient of a multi-crop step is bitwise the plain dino step's: the head is
    trained in pass A only and the saved buffer is added onto zeros."""
    grads = []
    for L in (0, 2):
        _flags(dino_local_crops=L, dino_local_crop_size=16)
        _fresh_runtime()
        model, target, opt, step = _build()
        box = _capture(monkeypatch.setattr, model, target, opt)
        images, locs, ids = _batch(16, 32, 16, 2)
        labels = {'labels': torch.nn.functional.one_hot(ids, NCLS).float().to(DEV)}
        step((images.to(DEV), locs.to(DEV)) if L else images.to(DEV), labels)
        torch.cuda.synchronize()
        assert ('local' in box) == bool(L)
        k = model.supervised_head.linear_layer.kernel
        off = model._flat_offsets[[id(v) for v in model._flat_order].index(id(k))]
        grads.append(box['flat'][off:off + k.numel()].clone())
    assert torch.equal(grads[0], grads[1]) and bool((grads[0] != 0).any())


def test_frozen_prototypes_stay_bitwise_unchanged(monkeypatch):
    """freeze = 1 epoch of 2 steps: neither pass writes a prototype gradient, the prototypes are bitwise unchanged on the online AND
    the target side while the centre moves; step 2 changes them on both sides."""
    _flags(dino_local_crops=2, dino_local_crop_size=16, dino_freeze_last_layer_epochs=1)
    _fresh_runtime()
    model, target, opt, step = _build()
    name = 'model/prototype_head/kernel:0'
    proto = model.prototype_head.kernel
    tproto = [v for v in target.variables if v.name == name][0]
    p0 = proto.value.clone()
    assert torch.equal(tproto.value, p0)
    box = _capture(monkeypatch.setattr, model, target, opt)
    images, locs, ids = _batch(16, 32, 16, 2)
    labels = {'labels': torch.nn.functional.one_hot(ids, NCLS).float().to(DEV)}
    for s in (0, 1):
        centre_before = target.center.value.clone()
        step((images.to(DEV), locs.to(DEV)), labels)
        torch.cuda.synchronize()
        assert box['update'] is False and box['local_update'] is False and name not in box['applied'], s
        assert torch.equal(proto.value, p0) and torch.equal(tproto.value, p0) and id(proto) not in opt._slots, s
        assert not torch.equal(target.center.value, centre_before)
    step((images.to(DEV), locs.to(DEV)), labels)
    torch.cuda.synchronize()
    assert box['update'] is True and box['local_update'] is True and name in box['applied']
    assert not torch.equal(proto.value, p0) and not torch.equal(tproto.value, p0) and bool(torch.isfinite(proto.value).all())


# ---------------------------------------------------------------------------------------------------------------- run.main
ARGS = ['--dataset=synthetic', '--resnet_depth=18', '--image_size=32', '--train_batch_size=8', '--use_blur=False', '--compute_dtype=f32',
        '--checkpoint_steps=2', '--train_steps=3', '--mode=train', '--proj_out_dim=64', '--dino_out_dim=200', '--dino_momentum=0.9',
        '--dino_freeze_last_layer_epochs=0', '--contrastive_loss=dino']


def _same(a, b):
    assert sorted(a['model']) == sorted(b['model'])
    assert all(torch.equal(a['model'][n], b['model'][n]) for n in a['model'])
    assert all(torch.equal(a['optimizer']['slots'][n], b['optimizer']['slots'][n]) for n in a['optimizer']['slots'])
    assert a['optimizer']['iterations'] == b['optimizer']['iterations']


def test_run_main_resumes_bitwise_and_other_modes_read_the_file(tmp_path, capsys):
    from simclr_amd import run
    from simclr_amd.checkpoint import INDEX_NAME
    from simclr_amd.flags import FLAGS
    args = ARGS + ['--dino_local_crops=2', '--dino_local_crop_size=16']
    full_dir, again_dir, ft_dir = str(tmp_path / 'full'), str(tmp_path / 'again'), str(tmp_path / 'ft')
    FLAGS.reset()
    run.main(args + ['--model_dir=' + full_dir])
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith('{') and 'train/dino_teacher_entropy' in l]
    assert lines and lines[0]['step'] == 2
    for k in ('train/contrast_loss', 'train/dino_teacher_entropy', 'train/total_loss'):
        assert math.isfinite(lines[0][k]), (k, lines[0])
    full = torch.load(os.path.join(full_dir, 'ckpt-3.pt'), map_location='cpu')
    name = 'model/prototype_head/kernel:0'
    assert 'dino/center' in full['model'] and 'target/' + name in full['model']           # the resume below compares them too
    two = torch.load(os.path.join(full_dir, 'ckpt-2.pt'), map_location='cpu')['model']
    assert not torch.equal(two['dino/center'], full['model']['dino/center'])
    assert not torch.equal(two['target/' + name], full['model']['target/' + name])
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
                       '--compute_dtype=f32', '--mode=eval', '--contrastive_loss=dino', '--proj_out_dim=64', '--knn_eval=True',
                       '--knn_k=5', '--dino_local_crops=2', '--dino_local_crop_size=16', '--model_dir=' + full_dir])
    assert result['global_step'] == 3
    for k in ('eval/label_top_1_accuracy', 'eval/knn_top_1_accuracy'):
        assert 0.0 <= result[k] <= 1.0, (k, result)
    FLAGS.reset()
    run.main(['--dataset=synthetic', '--resnet_depth=18', '--image_size=32', '--train_batch_size=8', '--compute_dtype=f32', '--mode=train',
              '--train_mode=finetune', '--contrastive_loss=dino', '--proj_out_dim=64', '--train_steps=1', '--checkpoint_steps=1',
              '--dino_local_crops=2', '--dino_local_crop_size=16', '--checkpoint=' + os.path.join(full_dir, 'ckpt-3.pt'),
              '--model_dir=' + ft_dir])
    written = torch.load(os.path.join(ft_dir, 'ckpt-1.pt'), map_location='cpu')['model']
    assert not any(n.startswith('target/') or n.startswith('dino/') or 'prototype_head' in n for n in written)


def test_run_main_without_local_crops_is_the_run_without_the_flag(tmp_path):
    from simclr_amd import run
    from simclr_amd.flags import FLAGS
    a_dir, b_dir, c_dir = str(tmp_path / 'a'), str(tmp_path / 'b'), str(tmp_path / 'c')
    short = [x for x in ARGS if not x.startswith('--train_steps')] + ['--train_steps=2']
    FLAGS.reset()
    run.main(short + ['--model_dir=' + a_dir])
    FLAGS.reset()
    run.main(short + ['--dino_local_crops=0', '--dino_local_crop_size=16', '--dino_local_crop_min_scale=0.2',
                      '--dino_local_crop_max_scale=0.3', '--model_dir=' + b_dir])
    a = torch.load(os.path.join(a_dir, 'ckpt-2.pt'), map_location='cpu')
    _same(a, torch.load(os.path.join(b_dir, 'ckpt-2.pt'), map_location='cpu'))
    FLAGS.reset()
    run.main(short + ['--dino_local_crops=2', '--dino_local_crop_size=16', '--model_dir=' + c_dir])
    c = torch.load(os.path.join(c_dir, 'ckpt-2.pt'), map_location='cpu')
    name = 'model/prototype_head/kernel:0'
    assert not torch.equal(a['model'][name], c['model'][name])
    with pytest.raises(ValueError, match='dino_local_crops belongs to'):
        FLAGS.reset()
        run.main([x for x in short if not x.startswith('--contrastive_loss')] + ['--contrastive_loss=swav', '--dino_local_crops=2'])


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
        _flags(batch=world * B2, dino_local_crops=L2, dino_local_crop_size=LOCAL2)
        RT = _fresh_runtime()
        strategy = comm.Strategy()
        RT.strategy = strategy
        model, target, opt, step = _build(strategy=strategy)
        attrs = {}
        box = _capture(lambda o, name, v: (attrs.setdefault((id(o), name), (o, name, getattr(o, name))), setattr(o, name, v)),
                       model, target, opt)
        images, locs, ids = _batch(world * B2, 32, LOCAL2, L2, seed=51)
        sl = slice(rank * B2, (rank + 1) * B2)
        out = step((images[sl].to(DEV), locs[sl].to(DEV)), {'labels': torch.nn.functional.one_hot(ids[sl], NCLS).float().to(DEV)})
        torch.cuda.synchronize()
        res = dict(q=_np(box['q']), t=_np(box['t']), x=_np(box['x']), vs=_np(box['vs']), wt=_np(box['wt']),
                   proto_grad=_np(box['proto_grad']), local=float(box['local'].value), total=float(out['con_loss'].value),
                   center=_np(target.center.value).copy())
        for o, name, v in attrs.values():
            setattr(o, name, v)
        dist.destroy_process_group()
        q.put((rank, 'ok', res))
    except Exception:  # noqa
        import traceback
        q.put((rank, 'FAIL', traceback.format_exc()))


def test_two_replica_step_vs_the_gathered_batch():
    """Two gloo ranks sharing one GPU.  Each rank's local value is the restatement's on its own rows -- its share of the one-replica
    loss on the gathered batch, whose value is the mean of the two; the prototype gradient after the ONE all-reduce is the gathered
    batch's on both ranks; both centres are bitwise equal and are the gathered GLOBAL keys' (the local views add nothing to it)."""
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
    vs, wt = boxes[0]['vs'], boxes[0]['wt']
    c0 = np.zeros(K_STEP, np.float32)
    cat = lambda name: np.concatenate([boxes[0][name][:B2], boxes[1][name][:B2], boxes[0][name][B2:], boxes[1][name][B2:]])
    x_all = np.concatenate([boxes[r]['x'][v * B2:(v + 1) * B2] for v in range(L2) for r in range(2)])
    whole = _reference(cat('q'), cat('t'), x_all, vs, wt, c0)
    want_c = center_update(c0, whole['wt'], whole['kh'], 0.9)
    bound = 64 * 2.0 ** -24 * np.abs(whole['kh'] @ whole['wt'].T).max() + 2.0 ** -23 * np.abs(want_c).max()
    out = [_res('two_replica local mean vs the gathered batch', 0.5 * (boxes[0]['local'] + boxes[1]['local']), whole['local_loss'], GATE_LOSS),
           _res('two_replica total mean vs the gathered batch', 0.5 * (boxes[0]['total'] + boxes[1]['total']), whole['loss'], GATE_LOSS),
           _res('two_replica centre vs the gathered global keys', boxes[0]['center'], want_c, 0, bound)]
    for r, bx in enumerate(boxes):
        ref = _reference(bx['q'], bx['t'], bx['x'], vs, wt, c0)
        out += [_res('two_replica local value rank %d' % r, bx['local'], ref['local_loss'], GATE_LOSS),
                _res('two_replica total value rank %d' % r, bx['total'], ref['loss'], GATE_LOSS),
                _res('two_replica prototype grad rank %d vs the gathered batch' % r, bx['proto_grad'], whole['grad_v'], GATE_GRAD)]
    _assert(out)
