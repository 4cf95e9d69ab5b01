"""NNCLR on the device (pytest -m gpu): the kernels of csrc/nnclr.hip and the search of csrc/knn.hip against the float64 restatement of
tests/nnclr_reference.py at the shapes the view boundary, the tile edges and the second of several ranks are met at; the step
(run.make_single_step with a model.SupportQueue) against the restatement on the queue as it stood BEFORE the step; run.main (resume,
--nn_queue_size=0, evaluation, k-NN evaluation and fine-tuning from the checkpoint); two replicas over gloo.

The gates of the loss and of the column gradient are 4 x the error of the float32 emulation against float64 on the case's own inputs
(nnclr_reference.EMULATION_ERROR, re-measured by tests/test_nnclr_reference.py).  The search must return the float64 index exactly:
every case asserts a float64 top-1 / top-2 gap above 4 D 2^-24 in every row it searches."""
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
import torch.nn.functional as F

from tests import nnclr_reference as ref_lib
from tests.gpu_checks import DEV, structured_images
from tests.nnclr_reference import FAMILIES, SHAPES, TEMPERATURES, TOL, f32, nnclr_emulated, nnclr_reference, relative_errors

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


def _check(name, err, tol, bad):
    print('%-4s %-84s err=%.3e tol=%.3e' % ('ok' if err <= tol else 'FAIL', name, err, tol))
    if not err <= tol:
        bad.append('%s err=%.3e tol=%.3e' % (name, err, tol))


def _np(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


# ---------------------------------------------------------------------------------------------------------------- search and sweeps
def _device(zs, S, n, rank, T, grad_scale=1.0):
    """The device path of replica `rank`: the search, the row gather, forward, backward.  -> dict of host values."""
    from simclr_amd import ops
    zd = [torch.from_numpy(z).to(DEV) for z in zs]
    z_all = torch.cat([z[:n] for z in zd] + [z[n:] for z in zd], 0).contiguous()
    Sd = torch.from_numpy(S).to(DEV)
    _, idx = ops.knn_topk(zd[rank], Sd, 1)
    nn = Sd.index_select(0, idx.reshape(-1).long())
    runs = []
    for _ in range(2):
        out, rs, ws = ops.nnclr_fwd(nn, zd[rank], z_all, rank, T)
        dz_all = ops.nnclr_bwd(nn, z_all, rank, T, rs, grad_scale, ws)
        torch.cuda.synchronize()
        runs.append((out[:3].clone(), rs.clone(), dz_all.clone()))
    return dict(idx=_np(idx.reshape(-1)), out=runs[0][0].cpu().double().numpy(), partial=runs[0][2].cpu().double().numpy(),
                repeat=all(torch.equal(a, b) for a, b in zip(*runs)), finite=bool(torch.isfinite(runs[0][2]).all()))


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'n%d-N%d-K%d-D%d-rank%d' % s)
def test_search_and_kernels_vs_float64(shape, family):
    n, N, K, D, rank = shape
    tol, bad = TOL[(shape, family)], []
    for T in TEMPERATURES:
        zs, S, ref = ref_lib.case_reference(shape, family, T)
        gap = float(ref['gap'][rank].min())
        assert gap > ref_lib.search_gap_needed(D), 'a row with a top-1 / top-2 gap of %.3g: choose another seed for this case' % gap
        got = _device(zs, S, n, rank, T)
        tag = 'n=%d N=%d K=%d D=%d rank=%d %s T=%g' % (shape + (family, T))
        assert np.array_equal(got['idx'], ref['nn_index'][rank]), tag                # the search: exact
        err = relative_errors(got['out'][0], got['partial'], ref, rank)
        _check('nnclr_loss ' + tag, err['loss'], tol['loss'], bad)
        _check('nnclr_grad ' + tag, err['grad'], tol['grad'], bad)
        assert got['out'][1] == float(np.float32(ref['acc'][rank])), tag             # a count: exact
        # z_r . nn_r is summed in double from float32 inputs: the float32 result is the rounded float64 one, give or take an ulp
        assert abs(got['out'][2] - ref['nn_sim'][rank]) <= 2.0 ** -23 * abs(ref['nn_sim'][rank]) + 1e-12, tag
        assert got['repeat'] and got['finite'], tag                                   # a second call is bitwise the first
        # the view mask: candidates taken from the row's OWN view are another loss, far outside the gate
        wrong = nnclr_reference(zs, S, f32(T), swapped=True)
        werr = relative_errors(got['out'][0], got['partial'], wrong, rank)
        assert werr['loss'] > tol['loss'] and werr['grad'] > tol['grad'], (tag, werr)
    assert not bad, '\n'.join(bad)


def test_grad_scale_is_folded_into_the_column_gradient():
    shape, family, T = (33, 33, 66, 64, 0), 'independent', 0.5
    zs, S, ref = ref_lib.case_reference(shape, family, T)
    got = _device(zs, S, shape[0], shape[4], T, grad_scale=0.25)
    err = relative_errors(got['out'][0], got['partial'], ref, shape[4], grad_scale=0.25)
    assert err['grad'] <= TOL[(shape, family)]['grad'], err


def test_duplicated_queue_rows_go_to_the_lowest_index():
    """Exact ties: every queue row occurs three times (bitwise copies), so every similarity occurs three times; the search returns the
    lowest index of the best triple."""
    from simclr_amd import ops
    g = np.random.default_rng(7)
    base = ref_lib.l2_normalize(g.standard_normal((50, 64)))[0].astype(np.float32)
    order = g.permutation(150)
    S = np.tile(base, (3, 1))[order]                                      # row k is base[order[k] % 50]
    z = ref_lib.l2_normalize(g.standard_normal((40, 64)))[0].astype(np.float32)
    idx, gap = ref_lib.search(z, base)
    assert gap.min() > ref_lib.search_gap_needed(64)
    want = np.array([min(k for k in range(150) if order[k] % 50 == j) for j in idx])
    assert np.array_equal(ref_lib.search(z, S)[0], want)                  # the reference's own tie rule
    _, got = ops.knn_topk(torch.from_numpy(z).to(DEV), torch.from_numpy(S).to(DEV), 1)
    torch.cuda.synchronize()
    assert np.array_equal(_np(got.reshape(-1)), want)


def test_kernels_refuse_bad_arguments():
    from simclr_amd import ops
    from simclr_amd._lib import SimclrHipError, lib
    L = lib()
    f = ctypes.c_float
    z = F.normalize(torch.randn(8, 64, generator=torch.Generator().manual_seed(3))).to(DEV)
    out, rs, ws = ops.nnclr_fwd(z, z, z, 0, 0.1)
    dz = ops.nnclr_bwd(z, z, 0, 0.1, rs, 1.0, ws)
    torch.cuda.synchronize()
    out0, rs0, dz0 = out[:3].clone(), rs.clone(), dz.clone()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    good = dict(nn=p(z), zl=p(z), za=p(z), n=4, N=4, D=64, rank=0, T=0.1, out=p(out), rs=p(rs), ws=p(ws), dz=p(dz))

    def fwd(**kw):
        a = dict(good, **kw)
        return L.nnclr_fwd(a['nn'], a['zl'], a['za'], a['n'], a['N'], a['D'], a['rank'], f(a['T']), a['out'], a['rs'], a['ws'], None)

    def bwd(**kw):
        a = dict(good, **kw)
        return L.nnclr_bwd(a['nn'], a['za'], a['n'], a['N'], a['D'], a['rank'], f(a['T']), a['rs'], f(1.0), a['dz'], a['ws'], None)
    odd = ctypes.c_void_p(z.data_ptr() + 4)
    nan, inf = float('nan'), float('inf')
    for call in (fwd, bwd):
        for kw, match in ((dict(D=100), 'D must be 64/128/256'), (dict(D=512), 'D must be 64/128/256'), (dict(n=0), 'n >= 1'),
                          (dict(n=1, N=1), 'N >= 2'), (dict(n=4, N=6), 'N = R\\*n'), (dict(rank=1), 'rank 1 out of range'),
                          (dict(rank=-1), 'rank -1 out of range'), (dict(T=0.0), 'temperature'), (dict(T=-1.0), 'temperature'),
                          (dict(T=nan), 'temperature'), (dict(T=inf), 'temperature'), (dict(nn=None), 'null or misaligned'),
                          (dict(za=odd), 'null or misaligned'), (dict(rs=None), 'null or misaligned'), (dict(ws=odd), 'null or misaligned')):
            with pytest.raises(SimclrHipError, match=match):
                call(**kw)
    for call, kw in ((fwd, dict(out=None)), (fwd, dict(zl=odd)), (bwd, dict(dz=None)), (bwd, dict(dz=odd))):
        with pytest.raises(SimclrHipError, match='null or misaligned'):
            call(**kw)
    assert L.nnclr_workspace_bytes(4, 4, 100) == 0 and L.nnclr_workspace_bytes(0, 4, 64) == 0 and L.nnclr_workspace_bytes(1, 1, 64) == 0
    assert L.nnclr_workspace_bytes(4, 6, 64) == 0 and L.nnclr_workspace_bytes(4, 8, 64) > 0 and L.nnclr_workspace_bytes(1, 2, 256) > 0
    torch.cuda.synchronize()
    # nothing was launched by a refused call: the outputs of the good calls are untouched
    assert torch.equal(out[:3], out0) and torch.equal(rs, rs0) and torch.equal(dz, dz0)
    wide = torch.zeros(8, 96, device=DEV)
    with pytest.raises(ValueError, match='64/128/256'):
        ops.nnclr_fwd(wide, wide, wide, 0, 0.1)
    with pytest.raises(ValueError, match='N = R\\*n >= 2'):
        ops.nnclr_fwd(z[:2], z[:2], z[:2], 0, 0.1)
    with pytest.raises(ValueError, match='one width'):
        ops.nnclr_fwd(z, z, wide, 0, 0.1)
    with pytest.raises(ValueError, match='z_local must be'):
        ops.nnclr_fwd(z, z[:4], z, 0, 0.1)
    with pytest.raises(ValueError, match='temperature'):
        ops.nnclr_fwd(z, z, z, 0, float('nan'))
    with pytest.raises(ValueError, match='rank 1 outside'):
        ops.nnclr_fwd(z, z, z, 1, 0.1)
    with pytest.raises(ValueError, match='row_stats must be'):
        ops.nnclr_bwd(z, z, 0, 0.1, rs[:4], 1.0, ws)
    with pytest.raises(ValueError, match='workspace is smaller'):
        ops.nnclr_bwd(z, z, 0, 0.1, rs, 1.0, ws[:8])
    with pytest.raises(ValueError, match='bad shape'):
        ops.nnclr_workspace(4, 6, 64, DEV)


# ---------------------------------------------------------------------------------------------------------------- handle and step
def _flags(**kw):
    from simclr_amd.flags import FLAGS
    FLAGS.reset()
    FLAGS.update(resnet_depth=18, image_size=SIZE, compute_dtype='f32', f32_matmul='exact', use_blur=False, train_batch_size=B,
                 train_mode='pretrain', contrastive_loss='ntxent', **kw)
    return FLAGS


def _fresh_runtime():
    from simclr_amd.resnet import RT
    RT.reset()
    RT.device = torch.device(DEV)
    return RT


def _capture(setattr_fn, model):
    """Records what the step hands the loss (the projection outputs and the queue AS IT STANDS at the search) and what it hands the
    projection head; the last step's captures stay."""
    from simclr_amd import objective as obj_lib
    box = {}
    orig_loss, orig_backward = obj_lib.add_nn_contrastive_loss, model.backward

    def loss_fn(hidden, support, *a, **kw):
        box['hidden'] = hidden.detach().clone()
        box['queue'] = support.detach().clone()
        box['kw'] = dict(kw)
        res = orig_loss(hidden, support, *a, **kw)
        box['loss'] = res
        return res

    def backward(d_proj, *a, **kw):
        box['d_proj'] = d_proj.detach().clone()
        return orig_backward(d_proj, *a, **kw)
    setattr_fn(obj_lib, 'add_nn_contrastive_loss', loss_fn)
    setattr_fn(model, 'backward', backward)
    return box


def _l2norm_bwd(h, dz, dtype):
    """d/dh of z = h / |h| from h and dz, in `dtype` arithmetic."""
    h, dz = np.asarray(h, dtype), np.asarray(dz, dtype)
    inv = (1.0 / np.sqrt((h.astype(np.float64) ** 2).sum(1, keepdims=True))).astype(dtype)
    z = (h * inv).astype(dtype)
    dot = (z * dz).sum(1, keepdims=True, dtype=dtype)
    return ((dz - z * dot).astype(dtype) * inv).astype(dtype)


def step_reference(hiddens, queue, nn_index, rank, T):
    """The restatement of a step on the captured projection outputs of every replica and the captured pre-step queue, with the
    neighbour indices the device found (asserted equal to the float64 search wherever its gap suffices): (loss of `rank`, d objective /
    d hidden of `rank`, the gates = 4 x the emulation's error on these inputs, chained through the normalisation in float32)."""
    T = f32(T)
    R, n = len(hiddens), hiddens[0].shape[0] // 2
    N, D = R * n, hiddens[0].shape[1]
    zs64 = [ref_lib.l2_normalize(np.asarray(h, np.float64))[0] for h in hiddens]
    ref = nnclr_reference(zs64, queue, T, nn_index=nn_index)
    for q in range(R):
        sure = ref['gap'][q] > ref_lib.search_gap_needed(D)
        assert np.array_equal(ref_lib.search(zs64[q], queue)[0][sure], np.asarray(nn_index[q])[sure])
    want = _l2norm_bwd(hiddens[rank], ref['grads'][rank], np.float64)
    zs32 = [z.astype(np.float32) for z in zs64]
    total = np.zeros((2 * n, D), np.float32)
    for q in range(R):
        emu = nnclr_emulated(zs32, queue, nn_index[q], q, T, grad_scale=1.0 / R)
        total += emu['partial'][ref_lib.replica_rows(rank, n, N)]
        if q == rank:
            emu_loss = emu['loss']
    got = _l2norm_bwd(hiddens[rank], total, np.float32)
    tol = dict(loss=4.0 * abs(float(emu_loss) - ref['loss'][rank]) / abs(ref['loss'][rank]),
               grad=4.0 * float(np.abs(got.astype(np.float64) - want).max() / np.abs(want).max()))
    return ref, want, tol


@pytest.mark.parametrize('queue_steps', [1, 4], ids=lambda k: 'K=%dN' % k)
def test_step_trains_the_restatement_on_the_pre_step_queue(monkeypatch, queue_steps):
    from simclr_amd import model as model_lib
    from simclr_amd.run import make_single_step
    K = queue_steps * B
    FLAGS = _flags(nn_queue_size=K, nn_queue_seed=3, temperature=0.2)
    _fresh_runtime()
    model = model_lib.Model(NCLS)
    box = _capture(monkeypatch.setattr, model)
    support = model_lib.SupportQueue(K, FLAGS.proj_out_dim, FLAGS.nn_queue_seed)
    assert np.array_equal(_np(support.value), model_lib.moco_queue_init(K, FLAGS.proj_out_dim, 3))
    assert [v.name for v in support.variables] == ['nnclr/queue'] and not support.variables[0].trainable
    optimizer = model_lib.build_optimizer(0.1)
    with pytest.raises(ValueError, match='needs a support queue'):
        make_single_step(model, optimizer, None)
    step = make_single_step(model, optimizer, None, support=support)
    assert sorted(step.metrics) == sorted(['train/contrast_acc', 'train/contrast_loss', 'train/nn_similarity', 'train/supervised_acc',
                                           'train/supervised_loss', 'train/total_loss', 'train/weight_decay'])
    g = torch.Generator().manual_seed(31)
    bad = []
    for s in range(2):                         # the second step searches a queue that holds the first step's rows
        images = structured_images(B, SIZE, 2, g).to(DEV)
        ids = torch.randint(0, NCLS, (B,), generator=g)
        out = step(images, {'labels': F.one_hot(ids, NCLS).float().to(DEV)})
        torch.cuda.synchronize()
        con = out['con_loss']
        assert tuple(box['hidden'].shape) == (2 * B, FLAGS.proj_out_dim) and box['kw']['temperature'] == FLAGS.temperature
        pre = _np(box['queue'])
        nn_index = _np(con.nn_index)
        assert nn_index.dtype == np.int32 and nn_index.shape == (2 * B,)
        assert np.array_equal(_np(con.neighbours), pre[nn_index])
        ref, want, tol = step_reference([_np(box['hidden'])], pre, [nn_index], 0, FLAGS.temperature)
        _check('step %d loss K=%d' % (s, K), abs(float(con.value) - ref['loss'][0]) / abs(ref['loss'][0]), tol['loss'], bad)
        _check('step %d d_proj K=%d' % (s, K),
               float(np.abs(_np(box['d_proj']).astype(np.float64) - want).max() / np.abs(want).max()), tol['grad'], bad)
        assert float(con.acc) == float(np.float32(ref['acc'][0]))
        assert abs(float(con.nn_sim) - ref['nn_sim'][0]) <= 1e-6
        # the queue afterwards: this step's view-a rows at ptr, every other row as it stood
        ptr = ref_lib.queue_ptr(s, B, K)
        assert ptr == model_lib.moco_queue_ptr(s, B, K) == (s * B) % K
        after = pre.copy()
        after[ptr:ptr + B] = _np(con.normalized)[:B]
        assert np.array_equal(_np(support.value), after)
    assert not bad, '\n'.join(bad)
    m = step.metrics
    assert 0.0 <= m['train/contrast_acc'].result() <= 1.0 and -1.0 <= m['train/nn_similarity'].result() <= 1.0
    assert out['logits_con'] is None
    assert all(bool(torch.isfinite(v.value).all()) for v in model.variables)


def test_a_support_queue_is_refused_without_the_flag():
    from simclr_amd import model as model_lib
    from simclr_amd.run import make_single_step
    FLAGS = _flags()
    _fresh_runtime()
    model = model_lib.Model(NCLS)
    with pytest.raises(ValueError, match='a support queue belongs to'):
        make_single_step(model, model_lib.build_optimizer(0.1), None, support=model_lib.SupportQueue(B, FLAGS.proj_out_dim, 0))


_RUN_COMMON = ['--dataset=synthetic', '--resnet_depth=18', '--image_size=32', '--train_batch_size=8', '--use_blur=False', '--compute_dtype=f32']
_RUN_ARGS = _RUN_COMMON + ['--checkpoint_steps=2', '--train_steps=3', '--mode=train']


def test_run_main_trains_logs_resumes_bitwise_and_feeds_eval_knn_and_finetune(tmp_path, capsys):
    from simclr_amd import model as model_lib
    from simclr_amd import run
    from simclr_amd.checkpoint import INDEX_NAME
    from simclr_amd.flags import FLAGS
    args = _RUN_ARGS + ['--nn_queue_size=16', '--nn_queue_seed=5']
    full_dir, again_dir = str(tmp_path / 'full'), str(tmp_path / 'again')
    FLAGS.reset()
    run.main(args + ['--model_dir=' + full_dir])
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith('{') and 'train/nn_similarity' in l]
    assert lines and lines[0]['step'] == 2
    for k in ('train/contrast_loss', 'train/contrast_acc', 'train/nn_similarity', 'train/total_loss'):
        assert math.isfinite(lines[0][k]), (k, lines[0])
    assert 'train/contrast_entropy' not in lines[0] and 0.0 <= lines[0]['train/contrast_acc'] <= 1.0
    full = torch.load(os.path.join(full_dir, 'ckpt-3.pt'), map_location='cpu')
    # the queue is the last entry, has no optimizer slot, and three steps of 8 rows left its second half as step 1 wrote it and its
    # first half as step 2 wrote it: nothing of the seeded rows is left
    assert list(full['model'])[-1] == 'nnclr/queue' and 'nnclr/queue' not in full['optimizer']['slots']
    queue = full['model']['nnclr/queue'].numpy()
    seeded = model_lib.moco_queue_init(16, queue.shape[1], 5)
    assert queue.shape == seeded.shape and not (queue == seeded).all(axis=1).any()
    two = torch.load(os.path.join(full_dir, 'ckpt-2.pt'), map_location='cpu')['model']['nnclr/queue'].numpy()
    assert np.array_equal(two[8:], queue[8:]) and not np.array_equal(two[:8], queue[:8])
    os.makedirs(again_dir)
    shutil.copy(os.path.join(full_dir, 'ckpt-2.pt'), os.path.join(again_dir, 'ckpt-2.pt'))
    with open(os.path.join(again_dir, INDEX_NAME), 'w') as f:
        json.dump({'model_checkpoint_path': 'ckpt-2.pt', 'all_model_checkpoint_paths': ['ckpt-2.pt']}, f)
    FLAGS.reset()
    run.main(args + ['--model_dir=' + again_dir])
    again = torch.load(os.path.join(again_dir, 'ckpt-3.pt'), map_location='cpu')
    assert list(again['model']) == list(full['model'])
    assert all(torch.equal(again['model'][n], full['model'][n]) for n in full['model'])          # the queue included
    assert all(torch.equal(again['optimizer']['slots'][n], full['optimizer']['slots'][n]) for n in full['optimizer']['slots'])
    assert again['optimizer']['iterations'] == full['optimizer']['iterations'] == 3
    assert len(glob.glob(os.path.join(again_dir, 'ckpt-*.pt'))) == 2
    capsys.readouterr()
    # evaluation, k-NN evaluation and fine-tuning read the checkpoint as a plain pretraining checkpoint; the flag is ignored there
    eval_args = ['--dataset=synthetic', '--resnet_depth=18', '--image_size=32', '--eval_batch_size=8', '--eval_steps=1', '--compute_dtype=f32',
                 '--mode=eval', '--nn_queue_size=16', '--model_dir=' + full_dir]
    FLAGS.reset()
    result = run.main(eval_args)
    assert result['global_step'] == 3 and 0.0 <= result['eval/label_top_1_accuracy'] <= 1.0, result
    FLAGS.reset()
    result = run.main(eval_args + ['--knn_eval=True', '--knn_k=5'])
    assert result['global_step'] == 3
    for k in ('eval/label_top_1_accuracy', 'eval/knn_top_1_accuracy'):
        assert 0.0 <= result[k] <= 1.0, (k, result)
    ft_dir = str(tmp_path / 'ft')
    FLAGS.reset()
    run.main(['--dataset=synthetic', '--resnet_depth=18', '--image_size=32', '--train_batch_size=8', '--compute_dtype=f32', '--mode=train',
              '--train_mode=finetune', '--nn_queue_size=16', '--train_steps=1', '--checkpoint_steps=1',
              '--checkpoint=' + os.path.join(full_dir, 'ckpt-3.pt'), '--model_dir=' + ft_dir])
    written = torch.load(os.path.join(ft_dir, 'ckpt-1.pt'), map_location='cpu')['model']
    enc = [n for n in written if n.startswith('model/resnet/')]
    assert len(enc) > 60 and all(n in full['model'] for n in enc) and 'nnclr/queue' not in written


def test_a_zero_queue_size_trains_what_no_flag_trains(tmp_path, capsys):
    """--nn_queue_size=0 is the run without the flag: bitwise in the logged loss and in every weight, and no queue in the checkpoint."""
    from simclr_amd import run
    from simclr_amd.flags import FLAGS
    results = []
    for name, extra in (('plain', []), ('zero', ['--nn_queue_size=0', '--nn_queue_seed=9'])):
        FLAGS.reset()
        d = str(tmp_path / name)
        run.main(_RUN_ARGS + extra + ['--model_dir=' + d])
        lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith('{') and 'train/contrast_loss' in l]
        assert lines and all('train/nn_similarity' not in l and 'train/contrast_entropy' in l for l in lines)
        results.append((lines, torch.load(os.path.join(d, 'ckpt-3.pt'), map_location='cpu')))
    (la, ca), (lb, cb) = results
    assert [(l['step'], l['train/contrast_loss'], l['train/total_loss']) for l in la] == \
           [(l['step'], l['train/contrast_loss'], l['train/total_loss']) for l in lb]
    assert list(ca['model']) == list(cb['model']) and all(torch.equal(ca['model'][n], cb['model'][n]) for n in ca['model'])
    assert 'nnclr/queue' not in ca['model']


# ---------------------------------------------------------------------------------------------------------------- two replicas
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


GLOO_T, GLOO_K = 0.2, 2 * 2 * B


def _worker(rank, world, port, q):
    try:
        import torch.distributed as dist
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        torch.cuda.set_device(0)
        dist.init_process_group('gloo', rank=rank, world_size=world)
        from simclr_amd import comm, ops
        from simclr_amd import model as model_lib
        from simclr_amd.run import make_single_step
        ops.set_f32_matmul('exact')
        FLAGS = _flags(nn_queue_size=GLOO_K, temperature=GLOO_T)
        FLAGS.update(train_batch_size=world * B)
        RT = _fresh_runtime()
        strategy = comm.Strategy()
        RT.strategy = strategy
        model = model_lib.Model(NCLS)
        attrs = {}
        box = _capture(lambda o, name, v: (attrs.setdefault((id(o), name), (o, name, getattr(o, name))), setattr(o, name, v)), model)
        support = model_lib.SupportQueue(GLOO_K, FLAGS.proj_out_dim, 0)
        step = make_single_step(model, model_lib.build_optimizer(0.1), strategy, support=support)
        g = torch.Generator().manual_seed(51)
        for _ in range(2):                     # the second step searches a queue that holds the first step's gathered rows
            images = structured_images(world * B, SIZE, 2, g)
            ids = torch.randint(0, NCLS, (world * B,), generator=g)
            out = step(images[rank * B:(rank + 1) * B].to(DEV), {'labels': ids[rank * B:(rank + 1) * B].to(DEV)})
            torch.cuda.synchronize()
        con = out['con_loss']
        res = dict(hidden=_np(box['hidden']), d_proj=_np(box['d_proj']), pre=_np(box['queue']), loss=float(con.value), acc=float(con.acc),
                   nn_index=_np(con.nn_index), normalized=_np(con.normalized), queue=_np(support.value))
        for o, name, v in attrs.values():
            setattr(o, name, v)
        dist.destroy_process_group()
        q.put((rank, 'ok', res))
    except Exception:  # noqa
        import traceback
        q.put((rank, 'FAIL', traceback.format_exc()))


def test_two_replica_step_vs_the_global_batch_restatement():
    """Two gloo ranks sharing one GPU, two steps: the queues stay bitwise equal across the ranks; each rank's loss share and the
    gradient its step hands its projection head are those of the objective (1 / R) sum_r loss_r on the global batch; the mean of the
    shares is the one-replica loss on the gathered batch."""
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
    assert np.array_equal(boxes[0]['pre'], boxes[1]['pre']) and np.array_equal(boxes[0]['queue'], boxes[1]['queue'])
    # the second step wrote the global view-a rows, rank 0's then rank 1's, at ptr = 2B; the first step's sit at 0
    after = boxes[0]['pre'].copy()
    after[2 * B:4 * B] = np.concatenate([b['normalized'][:B] for b in boxes])
    assert np.array_equal(boxes[0]['queue'], after)
    bad, hiddens, nn_index, refs, gates = [], [b['hidden'] for b in boxes], [b['nn_index'] for b in boxes], [], []
    for r, b in enumerate(boxes):
        ref, want, tol = step_reference(hiddens, b['pre'], nn_index, r, GLOO_T)
        _check('two_replica_loss rank %d' % r, abs(b['loss'] - ref['loss'][r]) / abs(ref['loss'][r]), tol['loss'], bad)
        _check('two_replica_d_proj rank %d' % r,
               float(np.abs(b['d_proj'].astype(np.float64) - want).max() / np.abs(want).max()), tol['grad'], bad)
        assert b['acc'] == float(np.float32(ref['acc'][r]))
        refs.append(ref['loss'][r])
        gates.append(tol['loss'])
    # the one-replica loss on the gathered batch: the same rows, the same neighbours, one replica of 2B images
    zs = [ref_lib.l2_normalize(np.asarray(h, np.float64))[0] for h in hiddens]
    one = nnclr_reference([ref_lib.z_all_of(zs, B)], boxes[0]['pre'], f32(GLOO_T),
                          nn_index=[np.concatenate([nn_index[0][:B], nn_index[1][:B], nn_index[0][B:], nn_index[1][B:]])])
    assert abs(one['loss'][0] - 0.5 * (refs[0] + refs[1])) <= 1e-12 * abs(one['loss'][0])      # the restatements agree among themselves
    mean = 0.5 * (boxes[0]['loss'] + boxes[1]['loss'])
    # each share lies within its gate of its restatement, so their mean lies within the larger gate, at most the sum, of the mean
    _check('two_replica_mean_vs_one_replica', abs(mean - one['loss'][0]) / abs(one['loss'][0]), gates[0] + gates[1], bad)
    assert not bad, '\n'.join(bad)
