"""MoCo v2 on the device (pytest -m gpu): the kernels of csrc/moco.hip through the C ABI and simclr_amd.ops against the float64
restatement tests/moco_reference.py, then the queue, the step, run.main end to end (metrics, resume, what other modes read from its
checkpoint) and two replicas over gloo.

Gates: those of tests/test_gpu_supcon.py / tests/test_gpu_byol.py for the same arithmetic -- loss 1e-5 relative, gradients 2e-4 of the
reference tensor's maximum.  Copies and repeated calls are compared bitwise."""
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
from tests.gpu_checks import DEV, _res, structured_images
from tests.moco_reference import l2_normalize, moco_logits, moco_loss, moco_loss_normalized, queue_init, queue_ptr
from tests.test_moco_reference import NEAR_T, near_converged

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


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)


# ---------------------------------------------------------------------------------------------------------------- loss kernels
def _unit_rows(g, rows, D):
    return l2_normalize(g.standard_normal((rows, D)))[0].astype(np.float32)


def _run_kernels(qh, th, queue, T, scales=(1.0, 0.5), tag=''):
    """Forward, backward at every scale and a second call (bitwise) against the float64 restatement on the same float32 rows."""
    from simclr_amd import ops
    qd, td, kd = _dev(qh), _dev(th), _dev(queue)
    out, stats, ws = ops.moco_fwd(qd, td, kd, T)
    out = out.clone()
    res = []
    for scale in scales:
        ref = moco_loss_normalized(qh, th, queue, T, grad_scale=scale)
        dq = ops.moco_bwd(qd, td, kd, T, stats, scale, ws)
        res.append(_res('moco_grad %s scale=%g' % (tag, scale), dq, ref['grad'], GATE_GRAD))
    res += [_res('moco_loss %s' % tag, out[0], ref['loss'], GATE_LOSS), _res('moco_acc %s' % tag, out[1], ref['acc'], 0, 1e-7),
            _res('moco_neg_mass %s' % tag, stats[:, 1], ref['neg_mass'], GATE_GRAD)]
    out2, stats2, ws2 = ops.moco_fwd(qd, td, kd, T)
    dq2 = ops.moco_bwd(qd, td, kd, T, stats2, scales[-1], ws2)
    torch.cuda.synchronize()
    assert torch.equal(out2, out) and torch.equal(stats2, stats) and torch.equal(dq2, dq), 'a second call is not bitwise the first'
    assert bool(torch.isfinite(dq).all()) and bool(torch.isfinite(out).all())
    return res, ref, out, dq


# b: rows 2 .. 140 -- below, across and past one 64-row block, the partner row in another workgroup; K: one row, a ragged single tile,
# one row past a tile, several tiles with a ragged last one, 65 tiles with one row in the last (more than one key split)
CASES = [(1, 1, 64, 1.0), (1, 63, 128, 0.07), (1, 4097, 256, 1.0), (3, 65, 256, 0.07), (3, 200, 64, 1.0), (3, 4097, 128, 0.07),
         (33, 1, 128, 0.07), (33, 63, 256, 1.0), (33, 200, 64, 0.07), (33, 4097, 64, 1.0), (70, 65, 64, 0.07), (70, 200, 128, 1.0),
         (70, 63, 64, 1.0), (70, 4097, 256, 0.07)]


@pytest.mark.parametrize('b,K,D,T', CASES)
def test_kernels_vs_float64(b, K, D, T):
    from simclr_amd import ops
    g = np.random.default_rng(1000 * b + K + D)
    qh, queue = _unit_rows(g, 2 * b, D), _unit_rows(g, K, D)
    # keys correlated with their queries (row r of q pairs with row (r + b) mod 2b of t), as in training
    th = l2_normalize(np.roll(qh, b, axis=0) + 0.5 * g.standard_normal((2 * b, D)))[0].astype(np.float32)
    if K == 4097:
        assert ops.moco_key_splits(2 * b, K) > 1 and K % 64 != 0          # several key splits, the last tile ragged
    res, ref, _, _ = _run_kernels(qh, th, queue, T, tag='b=%d K=%d D=%d T=%g' % (b, K, D, T))
    assert 0.0 < ref['loss'] and np.abs(ref['grad']).max() > 0.0
    _assert(res)


def test_key_splits_follow_the_shape():
    from simclr_amd import ops
    assert ops.moco_key_splits(2, 1) == 1 and ops.moco_key_splits(2, 64) == 1 and ops.moco_key_splits(2, 65) == 2
    assert ops.moco_key_splits(1024, 65536) > 1
    for two_n, K in ((0, 64), (3, 64), (2, 0)):
        with pytest.raises(ValueError, match='even two_n'):
            ops.moco_key_splits(two_n, K)


def test_near_converged_loss_and_gradient_keep_their_digits():
    """t = q + 1e-3 randn, T = 0.05, K = 64: the loss is 4.6e-6 and 1 - P+ ~ 1e-6.  logsumexp - s+ in fp32 misses this gate by three
    orders of magnitude and one minus P+ loses whole rows (tests/test_moco_reference.py)."""
    qh, th, queue = near_converged()
    res, ref, out, _ = _run_kernels(qh, th, queue, NEAR_T, tag='near-converged')
    assert 1e-6 < ref['loss'] < 1e-5 and ref['neg_mass'].max() < 1e-5
    _assert(res)


def _lattice_case():
    """Entries that are multiples of 1/8 in [-1/2, 1/2], D = 64: every dot product is a multiple of 1/64 below 16, exact in fp32 in any
    order.  Row 0's key is dense (norm 2, the largest in the set), its query is parallel to it and queue row 5 is a copy of that key:
    the positive TIES the best negative.  Row 1's positive is beaten by queue row 77, twice its key."""
    b, D, K = 20, 64, 130
    g = np.random.default_rng(12)
    lat = lambda rows: (g.integers(-2, 3, (rows, D)) * (g.random((rows, D)) < 0.5)).astype(np.float32) / 8.0
    q, t, queue = lat(2 * b), lat(2 * b), lat(K)
    for r in range(2, 2 * b, 2):         # every other query is its own key: mostly hits; the rest is unrelated to its key: mostly misses
        q[r] = t[(r + b) % (2 * b)]
    t[b] = np.where(g.random(D) < 0.5, 0.25, -0.25).astype(np.float32)      # row 0 pairs with t row b
    q[0] = 2.0 * t[b]
    queue[5] = t[b]
    q[1] = t[b + 1]
    queue[77] = 2.0 * t[b + 1]
    return b, q, t, queue


def test_exact_lattice_accuracy_and_ties():
    """T a power of two on the exact lattice: the accuracy equals the restatement's exactly, a tie is a hit."""
    T = 2.0
    b, q, t, queue = _lattice_case()
    sp, S, _ = moco_logits(q, t, queue, T)
    hits = sp >= S.max(-1)
    assert sp[0] == S[0].max() == S[0, 5] and sp[0] > 0 and (S[0] == sp[0]).sum() == 1     # the tie, with the copy alone
    assert sp[1] > 0 and S[1, 77] == 2.0 * sp[1] and not hits[1]
    assert hits[0] and 2 < hits.sum() < 2 * b - 2
    res, ref, out, _ = _run_kernels(q, t, queue, T, tag='lattice')
    assert ref['acc'] == hits.mean()
    assert float(out[1]) == float(np.float32(hits.sum() / (2.0 * b)))
    _assert(res)


def test_unnormalised_large_norm_queue_stays_finite():
    """The kernels take any rows: a queue of norm-80 rows, some parallel and some antiparallel to the queries, gives logits from -80 to
    80 in no particular order -- the running-maximum path of the online log-sum-exp.  Finite, and at the gates."""
    b, D, K, T = 33, 64, 200, 1.0
    g = np.random.default_rng(4)
    qh = _unit_rows(g, 2 * b, D)
    th = l2_normalize(np.roll(qh, b, axis=0) + 0.5 * g.standard_normal((2 * b, D)))[0].astype(np.float32)
    queue = 40.0 * g.standard_normal((K, D)).astype(np.float32) / np.sqrt(D)
    sign = np.where(np.arange(2 * b) % 2 == 0, 1.0, -1.0)[:, None]
    queue[100:100 + 2 * b] = (80.0 * sign * qh + 0.1 * g.standard_normal((2 * b, D))).astype(np.float32)
    sp, S, _ = moco_logits(qh, th, queue, T)
    assert S.max() > 79.0 and S.min() < -79.0
    res, ref, out, dq = _run_kernels(qh, th, queue, T, tag='large-norm queue')
    assert ref['loss'] > 50.0
    _assert(res)


def test_refusals_return_the_error_code_and_launch_nothing():
    from simclr_amd import ops
    from simclr_amd._lib import SimclrHipError, lib
    q, t, queue = torch.zeros(8, 64, device=DEV), torch.ones(8, 64, device=DEV), torch.ones(16, 64, device=DEV)
    out = torch.full((2,), 7.0, device=DEV)
    stats, dq = torch.full((8, 2), 7.0, device=DEV), torch.full((8, 64), 7.0, device=DEV)
    ws = torch.full((lib().moco_workspace_bytes(8, 16, 64) // 4,), 7.0, device=DEV)
    P = lambda x, off=0: ctypes.c_void_p(x.data_ptr() + off)
    raw = lib()._dll
    nan = float('nan')
    # (q, t, queue, two_n, K, D, T, workspace)
    cases = [(P(q), P(t), P(queue), 8, 16, 100, 1.0, P(ws)), (P(q), P(t), P(queue), 8, 16, 32, 1.0, P(ws)),
             (P(q), P(t), P(queue), 8, 16, 512, 1.0, P(ws)), (P(q), P(t), P(queue), 0, 16, 64, 1.0, P(ws)),
             (P(q), P(t), P(queue), 1, 16, 64, 1.0, P(ws)), (P(q), P(t), P(queue), 7, 16, 64, 1.0, P(ws)),
             (P(q), P(t), P(queue), -2, 16, 64, 1.0, P(ws)), (P(q), P(t), P(queue), 8, 0, 64, 1.0, P(ws)),
             (P(q), P(t), P(queue), 8, -1, 64, 1.0, P(ws)), (P(q), P(t), P(queue), 8, 16, 64, 0.0, P(ws)),
             (P(q), P(t), P(queue), 8, 16, 64, -0.5, P(ws)), (P(q), P(t), P(queue), 8, 16, 64, nan, P(ws)),
             (None, P(t), P(queue), 8, 16, 64, 1.0, P(ws)), (P(q), None, P(queue), 8, 16, 64, 1.0, P(ws)),
             (P(q), P(t), None, 8, 16, 64, 1.0, P(ws)), (P(q), P(t), P(queue), 8, 16, 64, 1.0, None),
             (P(q, 4), P(t), P(queue), 6, 16, 64, 1.0, P(ws)), (P(q), P(t, 8), P(queue), 6, 16, 64, 1.0, P(ws)),
             (P(q), P(t), P(queue, 4), 8, 15, 64, 1.0, P(ws)), (P(q), P(t), P(queue), 8, 16, 64, 1.0, P(ws, 4))]
    for a, c, k, two_n, K, D, T, w in cases:
        assert raw.simclr_moco_fwd(a, c, k, two_n, K, D, T, P(out), P(stats), w, None) == 1, (two_n, K, D, T)
        assert 'moco_fwd' in lib().last_error()
        assert raw.simclr_moco_bwd(a, c, k, two_n, K, D, T, P(stats), 1.0, P(dq), w, None) == 1, (two_n, K, D, T)
        assert 'moco_bwd' in lib().last_error()
    assert raw.simclr_moco_fwd(P(q), P(t), P(queue), 8, 16, 64, 1.0, None, P(stats), P(ws), None) == 1
    assert raw.simclr_moco_fwd(P(q), P(t), P(queue), 8, 16, 64, 1.0, P(out), None, P(ws), None) == 1
    assert raw.simclr_moco_bwd(P(q), P(t), P(queue), 8, 16, 64, 1.0, None, 1.0, P(dq), P(ws), None) == 1
    assert raw.simclr_moco_bwd(P(q), P(t), P(queue), 8, 16, 64, 1.0, P(stats), 1.0, None, P(ws), None) == 1
    assert raw.simclr_moco_bwd(P(q), P(t), P(queue), 6, 16, 64, 1.0, P(stats), 1.0, P(dq, 4), P(ws), None) == 1
    for two_n, K, D in ((8, 16, 100), (0, 16, 64), (7, 16, 64), (8, 0, 64)):
        assert lib().moco_workspace_bytes(two_n, K, D) == 0
    assert lib().moco_key_splits(7, 16) == 0 and lib().moco_key_splits(8, 0) == 0
    with pytest.raises(SimclrHipError, match='moco_fwd'):
        lib().moco_fwd(P(q), P(t), P(queue), 7, 16, 64, 1.0, P(out), P(stats), P(ws), None)
    with pytest.raises(ValueError, match='widths 64/128/256'):
        ops.moco_fwd(torch.zeros(8, 100, device=DEV), torch.zeros(8, 100, device=DEV), torch.zeros(4, 100, device=DEV), 1.0)
    with pytest.raises(ValueError, match='workspace is smaller'):
        ops.moco_bwd(q, t, queue, 1.0, stats, 1.0, torch.zeros(4, device=DEV))
    with pytest.raises(ValueError, match='row_stats'):
        ops.moco_bwd(q, t, queue, 1.0, torch.zeros(8, 4, device=DEV), 1.0, ws)
    torch.cuda.synchronize()
    for x in (out, stats, dq, ws):
        assert bool((x == 7.0).all())                     # nothing was written


# ---------------------------------------------------------------------------------------------------------------- queue
def _fresh_runtime():
    from simclr_amd.resnet import RT
    RT.reset()
    RT.device = torch.device(DEV)
    return RT


def test_enqueue_writes_its_slot_and_nothing_else():
    from simclr_amd import model as model_lib
    _fresh_runtime()
    K, D, rows = 96, 64, 32
    queue = model_lib.MocoQueue(K, D, seed=7)
    want = queue_init(K, D, 7)
    assert _np(queue.value).tobytes() == want.tobytes()                   # the seeded unit rows, bit for bit
    g = np.random.default_rng(1)
    for step in (0, 1, 2, 3, 7):                                          # steps 3 and 7 have wrapped: rows 0.. and 32..
        keys = _unit_rows(g, rows, D)
        ptr = queue.enqueue(_dev(keys), step)
        assert ptr == queue_ptr(step, rows, K) == (step * rows) % K
        want[ptr:ptr + rows] = keys
        torch.cuda.synchronize()
        assert _np(queue.value).tobytes() == want.tobytes(), step          # the slot bitwise, every other row untouched
    assert queue_ptr(3, rows, K) == 0
    queue.reset()
    assert _np(queue.value).tobytes() == queue_init(K, D, 7).tobytes()


# ---------------------------------------------------------------------------------------------------------------- step
def _flags(**kw):
    from simclr_amd.flags import FLAGS
    FLAGS.reset()
    kw.setdefault('proj_out_dim', 64)
    kw.setdefault('contrastive_loss', 'mocov2')
    kw.setdefault('use_blur', False)
    kw.setdefault('temperature', 0.2)
    kw.setdefault('moco_momentum', 0.9)
    kw.setdefault('moco_queue_size', 4 * B)
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
    queue = model_lib.MocoQueue(FLAGS.moco_queue_size, FLAGS.proj_out_dim, FLAGS.moco_queue_seed)
    target = model_lib.TargetNetwork(model, steps, queue=queue)
    opt = model_lib.build_optimizer(lr)
    return model, target, opt, make_single_step(model, opt, strategy, target=target)


def _values(variables):
    return {v.name: v.value.detach().clone() for v in variables}


def _capture(setattr_fn, model, target):
    """Records what the step hands the loss (with the queue as the loss saw it), what the loss hands the projection head's backward,
    and the queue at the moment of the backward."""
    from simclr_amd import objective as obj_lib
    box = {}
    orig_loss, orig_backward = obj_lib.add_moco_loss, model.backward

    def loss_fn(online, tgt, queue, *a, **kw):
        box['q'], box['t'], box['queue'] = online.detach().clone(), tgt.detach().clone(), queue.detach().clone()
        box['temperature'] = kw.get('temperature')
        box['loss'] = orig_loss(online, tgt, queue, *a, **kw)
        return box['loss']

    def backward(d_proj, *a, **kw):
        box['d_proj'] = d_proj.detach().clone()
        box['queue_at_backward'] = target.queue.value.detach().clone()
        return orig_backward(d_proj, *a, **kw)
    setattr_fn(obj_lib, 'add_moco_loss', loss_fn)
    setattr_fn(model, 'backward', backward)
    return box


@pytest.mark.parametrize('K', [2 * B, 4 * B])
def test_step_matches_the_restatement_on_the_pre_step_queue(monkeypatch, K):
    """K = 2N: the enqueue overwrites the whole queue, so a step that enqueued before its backward would differentiate a loss whose
    negatives are its own keys.  Loss and the gradient handed to the projection head are the restatement's on the captured projections
    and the queue as it stood BEFORE the step; afterwards the slot holds the step's keys and the target has moved by 1 - m."""
    FLAGS = _flags(moco_queue_size=K)
    _fresh_runtime()
    model, target, opt, step = _build()
    assert model.prediction_head is None
    assert sorted(step.metrics) == ['train/contrast_acc', 'train/contrast_loss', 'train/supervised_acc', 'train/supervised_loss',
                                    'train/total_loss', 'train/weight_decay']
    online0 = _values(model.variables)
    tv = _values(target.variables)
    assert len(tv) > 60 and all(torch.equal(tv[n], online0[n]) for n in tv)                # step 0: the target is the online copy
    queue0 = _np(target.queue.value).copy()
    assert queue0.tobytes() == queue_init(K, 64, 0).tobytes()
    box = _capture(monkeypatch.setattr, model, target)
    images, ids = _batch()
    labels = {'labels': torch.nn.functional.one_hot(ids, NCLS).float().to(DEV)}
    out = step(images.to(DEV), labels)
    torch.cuda.synchronize()
    assert tuple(box['q'].shape) == tuple(box['t'].shape) == (2 * B, 64) and box['temperature'] == 0.2
    assert _np(box['queue']).tobytes() == queue0.tobytes() and _np(box['queue_at_backward']).tobytes() == queue0.tobytes()
    ref = moco_loss(_np(box['q']), _np(box['t']), queue0, 0.2)
    con = out['con_loss']
    res = [_res('step_loss K=%d' % K, con.value, ref['loss'], GATE_LOSS), _res('step_acc K=%d' % K, con.acc, ref['acc'], 0, 1e-7),
           _res('step_d_proj K=%d' % K, box['d_proj'], ref['grad'], GATE_GRAD),
           _res('step_keys K=%d' % K, con.keys, ref['keys'], GATE_GRAD),
           # equal weights, the same pixels: the two networks agree, every positive logit is ~ 1 / T
           _res('step0_target_output K=%d' % K, box['t'], _np(box['q']), GATE_GRAD)]
    assert step.metrics['train/contrast_acc'].result() == float(con.acc) and step.metrics['train/contrast_loss'].result() == float(con.value)
    assert out['logits_con'] is None
    # the enqueue: rows [0, 2N) are the step's keys bitwise, the rest is untouched
    after = _np(target.queue.value)
    assert after[:2 * B].tobytes() == _np(con.keys).tobytes()
    assert after[2 * B:].tobytes() == queue0[2 * B:].tobytes()
    # the target moved by 1 - m towards the stepped online weights, in the float32 arithmetic of the kernel
    omt = np.float32(1.0 - 0.9)
    after_o = _values(model.variables)
    trained = {v.name for v in model.trainable_variables}
    moved = 0
    for v in target.variables:
        if v.name in trained:
            assert _np(v.value).tobytes() == ema_f32(_np(tv[v.name]), _np(after_o[v.name]), omt).tobytes(), v.name
            moved += int(not torch.equal(v.value, tv[v.name]))
    assert moved >= 20
    assert all(v.grad is None for v in target.variables + target.queue.variables)
    assert all(id(v) not in opt._slots for v in target.variables + target.queue.variables)
    # a second step reads the queue the first one left and writes the next slot (K = 2N: row 0 again)
    box2 = _capture(monkeypatch.setattr, model, target)
    out2 = step(images.to(DEV), labels)
    torch.cuda.synchronize()
    assert _np(box2['queue']).tobytes() == after.tobytes()
    ref2 = moco_loss(_np(box2['q']), _np(box2['t']), after, 0.2)
    ptr = queue_ptr(1, 2 * B, K)
    assert ptr == (0 if K == 2 * B else 2 * B)
    assert _np(target.queue.value)[ptr:ptr + 2 * B].tobytes() == _np(out2['con_loss'].keys).tobytes()
    res += [_res('step2_loss K=%d' % K, out2['con_loss'].value, ref2['loss'], GATE_LOSS),
            _res('step2_d_proj K=%d' % K, box2['d_proj'], ref2['grad'], GATE_GRAD)]
    _assert(res)
    assert all(bool(torch.isfinite(v.value).all()) for v in model.variables + target.variables)


# ---------------------------------------------------------------------------------------------------------------- run.main
ARGS = ['--dataset=synthetic', '--resnet_depth=18', '--image_size=32', '--train_batch_size=8', '--use_blur=False', '--compute_dtype=f32',
        '--checkpoint_steps=2', '--train_steps=3', '--mode=train', '--proj_out_dim=64', '--moco_queue_size=32', '--temperature=0.2',
        '--moco_momentum=0.9']


def test_run_main_trains_logs_resumes_bitwise_and_other_modes_read_the_file(tmp_path, capsys):
    """Three steps with a checkpoint after two: the run resumed from ckpt-2 writes a ckpt-3 bitwise equal to the uninterrupted one, the
    queue (whose third enqueue wrapped to row 0) included.  Then --mode=eval --knn_eval and a one-step fine-tune read the file as a
    plain pretraining checkpoint."""
    from simclr_amd import run
    from simclr_amd.checkpoint import INDEX_NAME
    from simclr_amd.flags import FLAGS
    args = ARGS + ['--contrastive_loss=mocov2']
    full_dir, again_dir, ft_dir = str(tmp_path / 'full'), str(tmp_path / 'again'), str(tmp_path / 'ft')
    FLAGS.reset()
    run.main(args + ['--model_dir=' + full_dir])
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith('{') and 'train/contrast_acc' in l]
    assert lines and lines[0]['step'] == 2
    for k in ('train/contrast_loss', 'train/contrast_acc', 'train/total_loss'):
        assert math.isfinite(lines[0][k]), (k, lines[0])
    assert 0.0 <= lines[0]['train/contrast_acc'] <= 1.0 and lines[0]['train/contrast_loss'] > 0.0
    assert not any(k in lines[0] for k in ('train/contrast_entropy', 'train/byol_cosine', 'train/align_loss', 'train/bt_on_diag',
                                           'train/contrast_positives'))
    full = torch.load(os.path.join(full_dir, 'ckpt-3.pt'), map_location='cpu')
    target_names = [n for n in full['model'] if n.startswith('target/')]
    assert len(target_names) > 60 and all(n[len('target/'):] in full['model'] for n in target_names)
    assert not any('prediction_head' in n for n in full['model'])
    assert tuple(full['model']['moco/queue'].shape) == (32, 64)
    assert not any(n.startswith('target/') or n.startswith('moco/') for n in full['optimizer']['slots'])
    two = torch.load(os.path.join(full_dir, 'ckpt-2.pt'), map_location='cpu')['model']['moco/queue']
    init = torch.from_numpy(queue_init(32, 64, 0))
    assert not torch.equal(two[:16], init[:16]) and not torch.equal(two[16:], init[16:])      # two steps filled both slots
    three = full['model']['moco/queue']
    assert torch.equal(three[16:], two[16:]) and not torch.equal(three[:16], two[:16])        # the third wrapped to row 0
    assert float((three.double().pow(2).sum(-1).sqrt() - 1.0).abs().max()) <= 1e-6            # unit rows
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
                       '--compute_dtype=f32', '--mode=eval', '--contrastive_loss=mocov2', '--proj_out_dim=64', '--knn_eval=True',
                       '--knn_k=5', '--model_dir=' + full_dir])
    assert result['global_step'] == 3
    for k in ('eval/label_top_1_accuracy', 'eval/knn_top_1_accuracy'):
        assert 0.0 <= result[k] <= 1.0, (k, result)
    # one fine-tuning step from the file: the online encoder, no target, no queue in what it writes
    FLAGS.reset()
    path = os.path.join(full_dir, 'ckpt-3.pt')
    run.main(['--dataset=synthetic', '--resnet_depth=18', '--image_size=32', '--train_batch_size=8', '--compute_dtype=f32', '--mode=train',
              '--train_mode=finetune', '--contrastive_loss=mocov2', '--proj_out_dim=64', '--train_steps=1', '--checkpoint_steps=1',
              '--checkpoint=' + path, '--model_dir=' + ft_dir])
    written = torch.load(os.path.join(ft_dir, 'ckpt-1.pt'), map_location='cpu')['model']
    assert not any(n.startswith('target/') or n.startswith('moco/') for n in written)
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
        _flags(train_batch_size=world * B, moco_queue_size=2 * world * 2 * B)
        RT = _fresh_runtime()
        strategy = comm.Strategy()
        RT.strategy = strategy
        model, target, opt, step = _build(strategy=strategy)
        attrs = {}
        box = _capture(lambda o, name, v: (attrs.setdefault((id(o), name), (o, name, getattr(o, name))), setattr(o, name, v)), model, target)
        images, ids = _batch(world * B, seed=51)
        out = step(images[rank * B:(rank + 1) * B].to(DEV), {'labels': ids[rank * B:(rank + 1) * B].to(DEV)})
        torch.cuda.synchronize()
        res = dict(q=_np(box['q']), t=_np(box['t']), d_proj=_np(box['d_proj']), queue_before=_np(box['queue']),
                   loss=float(out['con_loss'].value), acc=float(out['con_loss'].acc), keys=_np(out['con_loss'].keys),
                   queue=_np(target.queue.value).copy())
        for o, name, v in attrs.values():
            setattr(o, name, v)
        dist.destroy_process_group()
        q.put((rank, 'ok', res))
    except Exception:  # noqa
        import traceback
        q.put((rank, 'FAIL', traceback.format_exc()))


def test_two_replica_step_vs_the_restatement_on_the_gathered_batch():
    """Two gloo ranks sharing one GPU.  Both queues are bitwise equal after the step and hold the gathered keys in the NT-Xent layout
    (every replica's view-a rows, then every replica's view-b rows); each rank's loss is the restatement's on its own rows, the mean of
    the two is the restatement's on the gathered batch, and the gradient a rank hands its projection head is its slice of the gathered
    batch's gradient (grad_scale 1 / 2, no collective in the loss)."""
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
    K = 8 * B
    queue0 = queue_init(K, 64, 0)
    assert all(b['queue_before'].tobytes() == queue0.tobytes() for b in boxes)
    assert boxes[0]['queue'].tobytes() == boxes[1]['queue'].tobytes()
    want = queue0.copy()
    want[:4 * B] = np.concatenate([boxes[0]['keys'][:B], boxes[1]['keys'][:B], boxes[0]['keys'][B:], boxes[1]['keys'][B:]])
    assert boxes[0]['queue'].tobytes() == want.tobytes()
    q_all = np.concatenate([boxes[0]['q'][:B], boxes[1]['q'][:B], boxes[0]['q'][B:], boxes[1]['q'][B:]])
    t_all = np.concatenate([boxes[0]['t'][:B], boxes[1]['t'][:B], boxes[0]['t'][B:], boxes[1]['t'][B:]])
    whole = moco_loss(q_all, t_all, queue0, 0.2)
    out = [_res('two_replica_loss_mean vs the gathered batch', 0.5 * (boxes[0]['loss'] + boxes[1]['loss']), whole['loss'], GATE_LOSS)]
    for r, b in enumerate(boxes):
        ref = moco_loss(b['q'], b['t'], queue0, 0.2, grad_scale=0.5)
        idx = np.concatenate([np.arange(r * B, (r + 1) * B), 2 * B + np.arange(r * B, (r + 1) * B)])
        out += [_res('two_replica_loss rank %d' % r, b['loss'], ref['loss'], GATE_LOSS),
                _res('two_replica_acc rank %d' % r, b['acc'], ref['acc'], 0, 1e-7),
                _res('two_replica_d_proj rank %d' % r, b['d_proj'], ref['grad'], GATE_GRAD),
                _res('two_replica_d_proj rank %d vs the gathered batch' % r, b['d_proj'], whole['grad'][idx], GATE_GRAD)]
    _assert(out)
