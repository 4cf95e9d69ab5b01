"""The Barlow Twins loss on the device (pytest -m gpu): the Gram-form kernels of csrc/barlow.hip through the C ABI and simclr_amd.ops against
the float64 restatement tests/barlow_reference.py, then the handle inside the step, run.main end to end (metrics, resume) and two replicas
over gloo.

Gates: the project's own for the same arithmetic (GATE_LOSS, GATE_GRAD of tests/test_gpu_supcon.py) -- loss, on_diag and off_diag 1e-5
relative, gradients 2e-4 of the reference tensor's maximum; zhat 1e-5 absolute; the stored Gram blocks bitwise on integer data."""
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

from tests.barlow_reference import barlow_direct, barlow_gram, h_all_of, standardize
from tests.gpu_checks import DEV, _res, structured_images

pytestmark = pytest.mark.gpu
GATE_LOSS, GATE_GRAD = 1e-5, 2e-4
GATE_ZHAT = 1e-5
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


# ---------------------------------------------------------------------------------------------------------------- standardise
@pytest.mark.parametrize('N,D', [(5, 64), (70, 128), (256, 320)])
def test_standardize_vs_float64(N, D):
    """Rows randn + 10: raw fp32 moments (E[x^2] - E[x]^2) miss this gate by 5x or more, the two-pass form has 7x headroom."""
    from simclr_amd import ops
    g = np.random.default_rng(N + D)
    h = (g.standard_normal((2 * N, D)) + 10.0).astype(np.float32)
    zhat, rstd = ops.bt_standardize(torch.from_numpy(h).to(DEV))
    torch.cuda.synchronize()
    z1, r1 = standardize(h[:N])
    z2, r2 = standardize(h[N:])
    _assert([_res('bt_zhat N=%d D=%d' % (N, D), zhat, np.concatenate([z1, z2]), 0, GATE_ZHAT),
             _res('bt_rstd N=%d D=%d' % (N, D), rstd, np.stack([r1, r2]), GATE_LOSS)])


def test_standardize_of_one_row_is_zero():
    from simclr_amd import ops
    h = torch.randn(2, 128, generator=torch.Generator().manual_seed(1)) + 10.0
    zhat, rstd = ops.bt_standardize(h.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(zhat.cpu(), torch.zeros(2, 128))
    assert np.abs(rstd.cpu().numpy() - 1.0 / math.sqrt(1e-5)).max() <= 1e-5 / math.sqrt(1e-5)


# ---------------------------------------------------------------------------------------------------------------- loss and gradient
def _device(hs, n, lam, ls, rank, eps=1e-5):
    """The device path of replica `rank` on one device: the gathered block is standardised once, every replica q runs its forward and
    its backward with grad_scale = 1 / R, the column sums are added over the replicas (what strategy.all_reduce_sum does) and rank's rows
    go through the standardisation backward.  Returns (out [3] of every replica, dh [2n, D] = dL/dh_rank, zhat_all)."""
    from simclr_amd import ops
    R = len(hs)
    h_all = torch.from_numpy(h_all_of(hs, n)).to(DEV)
    zhat_all, rstd = ops.bt_standardize(h_all, eps)
    outs, g_rank, colsums = [], None, None
    for q in range(R):
        o_q, ws_q = ops.bt_fwd(zhat_all, n, q, lam, ls)
        g_q, cs_q = ops.bt_bwd(zhat_all, n, q, lam, ls, 1.0 / R, ws_q)
        outs.append(o_q[:3].clone())
        colsums = cs_q if colsums is None else colsums + cs_q
        if q == rank:
            g_rank = g_q
    dh = ops.bt_apply(g_rank, zhat_all, rstd, colsums, rank)
    torch.cuda.synchronize()
    return [o.cpu().double() for o in outs], dh, zhat_all


def _views(n, R, D, seed):
    g = np.random.default_rng(seed)
    return [g.standard_normal((2 * n, D)).astype(np.float32) for _ in range(R)]


SHAPES = [(5, 5, 64, 0), (70, 70, 128, 0), (64, 128, 64, 1), (33, 99, 320, 2), (16, 16, 2048, 0)]


@pytest.mark.parametrize('ls', [1.0, 0.024])
@pytest.mark.parametrize('lam', [0.0051, 1.0])
@pytest.mark.parametrize('n,N,D,rank', SHAPES)
def test_kernel_vs_float64(n, N, D, rank, lam, ls):
    R = N // n
    hs = _views(n, R, D, 3 + n + D)
    ref = barlow_gram(hs, lam, ls)
    outs, dh, _ = _device(hs, n, lam, ls, rank)
    o = outs[rank]
    tag = 'n=%d N=%d D=%d rank=%d lambda=%g scaling=%g' % (n, N, D, rank, lam, ls)
    _assert([_res('bt_loss ' + tag, o[0], ref['loss'][rank], GATE_LOSS), _res('bt_on_diag ' + tag, o[1], ref['on_diag'][rank], GATE_LOSS),
             _res('bt_off_diag ' + tag, o[2], ref['off_diag'][rank], GATE_LOSS), _res('bt_grad ' + tag, dh, ref['grads'][rank], GATE_GRAD)])


def test_near_converged_views():
    """h2 = h1 + 0.1 randn: C is close to the identity and off_diag is the difference of two larger sums, sum_ij C_ij^2 - sum_i c_i^2.
    The kernel accumulates the first, so off_diag is gated at 1e-5 of it, and on_diag (a sum of D small squares of 1 - c_i) at 1e-5 of D."""
    n = N = 256
    D = 64
    g = np.random.default_rng(8)
    h1 = g.standard_normal((n, D))
    hs = [np.concatenate([h1, h1 + 0.1 * g.standard_normal((n, D))]).astype(np.float32)]
    lam, ls = 0.0051, 1.0
    ref, direct = barlow_gram(hs, lam, ls), barlow_direct(hs, lam, ls)
    assert direct['frob'] > 3.0 * direct['off_diag'] and direct['on_diag'] < 1.0
    outs, dh, _ = _device(hs, n, lam, ls, 0)
    o = outs[0]
    _assert([_res('bt_near_on_diag', o[1], ref['on_diag'][0], 0, GATE_LOSS * D), _res('bt_near_off_diag', o[2], ref['off_diag'][0], 0, GATE_LOSS * direct['frob']),
             _res('bt_near_loss', o[0], ref['loss'][0], 0, GATE_LOSS * ls * (D + lam * direct['frob'])),
             _res('bt_near_grad', dh, ref['grads'][0], GATE_GRAD)])


@pytest.mark.parametrize('D', [64, 256])
def test_exact_lattice_gram_blocks(D):
    """zhat entries in {-2, ..., 2} fed to the Gram launch directly: every dot product is an integer of magnitude <= 4 D <= 1024, exact in
    fp32 in any summation order, so the stored blocks are bitwise the integer products -- at every tile edge (n = 70 and N = 140 fill no
    64-tile) and for both rank offsets."""
    from simclr_amd import ops
    n, N = 70, 140
    g = np.random.default_rng(D)
    z = g.integers(-2, 3, size=(2 * N, D)).astype(np.float32)
    zd = torch.from_numpy(z).to(DEV)
    zi = z.astype(np.int64)
    for rank in (0, 1):
        out, ws = ops.bt_fwd(zd, n, rank, 0.0051)
        gram = ops.bt_gram_blocks(ws, n, N, D)
        torch.cuda.synchronize()
        a = slice(rank * n, (rank + 1) * n)
        want = np.stack([zi[:N][a] @ zi[:N].T, zi[N:][a] @ zi[N:].T])
        assert tuple(gram.shape) == (2, n, N)
        assert np.array_equal(gram.cpu().numpy(), want.astype(np.float32)), 'rank %d' % rank
        # the sums the launch forms from those blocks, in float64 on the integers
        c = (zi[:N] * zi[N:]).sum(0) / N
        off = (want[0] * want[1]).sum() / (n * N) - (c ** 2).sum()
        _assert([_res('bt_lattice_on_diag D=%d rank=%d' % (D, rank), out[1], ((1.0 - c) ** 2).sum(), GATE_LOSS),
                 _res('bt_lattice_off_diag D=%d rank=%d' % (D, rank), out[2], off, GATE_LOSS)])


def test_kernel_is_bitwise_repeatable():
    from simclr_amd import ops
    n, N, D = 48, 96, 192
    h = (torch.randn(2 * N, D, generator=torch.Generator().manual_seed(5)) * 3.0 + 1.0).to(DEV)
    runs = []
    for _ in range(2):
        zhat, rstd = ops.bt_standardize(h)
        out, ws = ops.bt_fwd(zhat, n, 1, 0.0051, 0.5)
        gram = ops.bt_gram_blocks(ws, n, N, D).clone()
        gl, cs = ops.bt_bwd(zhat, n, 1, 0.0051, 0.5, 0.5, ws)
        dh = ops.bt_apply(gl, zhat, rstd, cs, 1)
        torch.cuda.synchronize()
        runs.append((zhat, rstd, out[:3].clone(), gram, gl, cs, dh))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_kernel_refuses_bad_arguments():
    from simclr_amd import ops
    from simclr_amd._lib import SimclrHipError, lib
    L = lib()
    f = ctypes.c_float
    for D in (100, 8256):
        assert L.bt_workspace_bytes(4, 4, D) == 0 and L.bt_gram_pitch(4, 4, D) == 0
        with pytest.raises(SimclrHipError, match='multiple of 64 in \\[64, 8192\\]'):
            L.bt_standardize(None, 4, D, f(1e-5), None, None, None)
        with pytest.raises(SimclrHipError, match='multiple of 64 in \\[64, 8192\\]'):
            L.bt_fwd(None, 4, 4, D, 0, f(0.0051), f(1.0), None, None, None)
        with pytest.raises(SimclrHipError, match='multiple of 64 in \\[64, 8192\\]'):
            L.bt_bwd(None, 4, 4, D, 0, f(0.0051), f(1.0), f(1.0), None, None, None, None)
        with pytest.raises(SimclrHipError, match='multiple of 64 in \\[64, 8192\\]'):
            L.bt_apply(None, None, None, None, 4, 4, D, 0, None, None)
    assert L.bt_workspace_bytes(4, 6, 64) == 0 and L.bt_workspace_bytes(0, 4, 64) == 0 and L.bt_workspace_bytes(4, 8, 64) > 0
    with pytest.raises(SimclrHipError, match='N = R\\*n'):
        L.bt_fwd(None, 4, 6, 128, 0, f(0.0051), f(1.0), None, None, None)
    with pytest.raises(SimclrHipError, match='N = R\\*n'):
        L.bt_bwd(None, 0, 4, 128, 0, f(0.0051), f(1.0), f(1.0), None, None, None, None)
    with pytest.raises(SimclrHipError, match='rank 2 out of range'):
        L.bt_fwd(None, 4, 8, 128, 2, f(0.0051), f(1.0), None, None, None)
    with pytest.raises(SimclrHipError, match='null argument'):
        L.bt_fwd(None, 4, 4, 128, 0, f(0.0051), f(1.0), None, None, None)
    with pytest.raises(SimclrHipError, match='null argument'):
        L.bt_apply(None, None, None, None, 4, 4, 128, 0, None, None)
    with pytest.raises(ValueError, match='multiples of 64'):
        ops.bt_standardize(torch.zeros(8, 100, device=DEV))
    with pytest.raises(ValueError, match='N = R\\*n'):
        ops.bt_fwd(torch.zeros(12, 64, device=DEV), 4, 0, 0.0051)


def test_two_replicas_on_one_device_equal_one_replica_on_the_whole_block():
    """rank 0 and rank 1 on the two halves of one gathered block: their loss values average to the one-replica loss on the whole block,
    and their gradients (column sums added) are its rows."""
    n, R, D, lam, ls = 40, 2, 128, 0.0051, 1.0
    hs = _views(n, R, D, 77)
    N = n * R
    whole = [h_all_of(hs, n)]
    outs1, dh1, z1 = _device(whole, N, lam, ls, 0)
    res = []
    for rank in range(R):
        outs2, dh2, z2 = _device(hs, n, lam, ls, rank)
        assert torch.equal(z1, z2)
        rows = np.concatenate([np.arange(rank * n, (rank + 1) * n), N + np.arange(rank * n, (rank + 1) * n)])
        res.append(_res('bt_replica_grad rank %d' % rank, dh2, dh1.cpu()[rows], GATE_GRAD))
    mean = [sum(float(o[k]) for o in outs2) / R for k in range(3)]
    res += [_res('bt_replica_loss_mean', mean[0], outs1[0][0], GATE_LOSS), _res('bt_replica_on_diag', mean[1], outs1[0][1], GATE_LOSS),
            _res('bt_replica_off_diag_mean', mean[2], outs1[0][2], GATE_LOSS)]
    ref = barlow_direct(whole, lam, ls)
    res += [_res('bt_whole_loss', outs1[0][0], ref['loss'], GATE_LOSS), _res('bt_whole_grad', dh1, ref['grad_all'], GATE_GRAD)]
    _assert(res)


def test_objective_handle_matches_the_restatement():
    from simclr_amd import objective
    n, D = 24, 192
    hs = _views(n, 1, D, 9)
    loss = objective.add_barlow_twins_loss(torch.from_numpy(hs[0]).to(DEV), lambda_weight=0.02, loss_scaling=0.5)
    dh = loss.backward(1.0)
    torch.cuda.synchronize()
    ref = barlow_gram(hs, 0.02, 0.5)
    assert not hasattr(loss, 'temperature')
    _assert([_res('handle_loss', loss.value, ref['loss'][0], GATE_LOSS), _res('handle_on_diag', loss.on_diag, ref['on_diag'][0], GATE_LOSS),
             _res('handle_off_diag', loss.off_diag, ref['off_diag'][0], GATE_LOSS), _res('handle_grad', dh, ref['grads'][0], GATE_GRAD),
             _res('handle_normalized', loss.normalized, ref['zhat_all'], 0, GATE_ZHAT)])


# ---------------------------------------------------------------------------------------------------------------- handle and step
def _flags(**kw):
    from simclr_amd.flags import FLAGS
    FLAGS.reset()
    kw.setdefault('proj_out_dim', 64)
    FLAGS.update(resnet_depth=18, image_size=SIZE, compute_dtype='f32', f32_matmul='exact', use_blur=False, train_batch_size=B,
                 train_mode='pretrain', contrastive_loss='barlow', **kw)
    return FLAGS


def _fresh_runtime():
    from simclr_amd.resnet import RT
    RT.reset()
    RT.device = torch.device(DEV)
    return RT


def _capture(setattr_fn, model):
    """Records what the step hands the loss (the block it reads) and what it hands the layer below it."""
    from simclr_amd import objective as obj_lib
    box = {}
    orig_loss, orig_backward = obj_lib.add_barlow_twins_loss, model.backward

    def loss_fn(hidden, *a, **kw):
        box['hidden'] = hidden.detach().clone()
        box['kw'] = {k: v for k, v in kw.items() if k in ('lambda_weight', 'loss_scaling')}
        box['loss'] = orig_loss(hidden, *a, **kw)
        return box['loss']

    def backward(d_proj, *a, **kw):
        box['d_proj'] = d_proj.detach().clone()
        return orig_backward(d_proj, *a, **kw)
    setattr_fn(obj_lib, 'add_barlow_twins_loss', loss_fn)
    setattr_fn(model, 'backward', backward)
    return box


def _np(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


@pytest.mark.parametrize('head_mode,width', [('nonlinear', 64), ('none', 512)])
def test_step_hands_the_layer_below_the_reference_gradient(monkeypatch, head_mode, width):
    """One step with a projection head of width 64 and one with proj_head_mode=none (the loss reads ResNet-18's 512-wide output)."""
    from simclr_amd import model as model_lib
    from simclr_amd.run import make_single_step
    FLAGS = _flags(proj_head_mode=head_mode, bt_lambda=0.01, bt_loss_scaling=0.5)
    _fresh_runtime()
    model = model_lib.Model(NCLS)
    box = _capture(monkeypatch.setattr, model)
    step = make_single_step(model, model_lib.build_optimizer(0.1), None)
    assert sorted(step.metrics) == ['train/bt_off_diag', 'train/bt_on_diag', 'train/contrast_loss', 'train/supervised_acc',
                                    'train/supervised_loss', 'train/total_loss', 'train/weight_decay']
    g = torch.Generator().manual_seed(31)
    images = structured_images(B, SIZE, 2, g).to(DEV)
    ids = torch.randint(0, NCLS, (B,), generator=g)
    out = step(images, {'labels': torch.nn.functional.one_hot(ids, NCLS).float().to(DEV)})
    torch.cuda.synchronize()
    assert tuple(box['hidden'].shape) == (2 * B, width) and out['logits_con'] is None
    assert box['kw'] == dict(lambda_weight=0.01, loss_scaling=0.5)
    ref = barlow_gram([_np(box['hidden'])], 0.01, 0.5)
    con = out['con_loss']
    _assert([_res('step_loss', con.value, ref['loss'][0], GATE_LOSS), _res('step_on_diag', con.on_diag, ref['on_diag'][0], GATE_LOSS),
             _res('step_off_diag', con.off_diag, ref['off_diag'][0], GATE_LOSS), _res('step_d_proj', box['d_proj'], ref['grads'][0], GATE_GRAD)])
    m = step.metrics
    assert m['train/bt_on_diag'].result() == float(con.on_diag) and m['train/bt_off_diag'].result() == float(con.off_diag)
    assert all(bool(torch.isfinite(v.value).all()) for v in model.variables)


def test_run_main_trains_logs_and_resumes_bitwise(tmp_path, capsys):
    from simclr_amd import run
    from simclr_amd.checkpoint import INDEX_NAME
    from simclr_amd.flags import FLAGS
    args = ['--dataset=synthetic', '--resnet_depth=18', '--image_size=32', '--train_batch_size=8', '--use_blur=False', '--compute_dtype=f32',
            '--checkpoint_steps=2', '--train_steps=3', '--mode=train', '--contrastive_loss=barlow', '--proj_out_dim=64']
    full_dir, again_dir = str(tmp_path / 'full'), str(tmp_path / 'again')
    FLAGS.reset()
    run.main(args + ['--model_dir=' + full_dir])
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith('{') and 'train/bt_on_diag' in l]
    assert lines and lines[0]['step'] == 2
    for k in ('train/contrast_loss', 'train/bt_on_diag', 'train/bt_off_diag', 'train/total_loss'):
        assert math.isfinite(lines[0][k]), (k, lines[0])
    assert 'train/contrast_entropy' not in lines[0] and 'train/contrast_acc' not in lines[0] and 'train/align_loss' not in lines[0]
    assert 0.0 <= lines[0]['train/bt_on_diag'] <= 4.0 * 64 and lines[0]['train/bt_off_diag'] >= 0.0
    full = torch.load(os.path.join(full_dir, 'ckpt-3.pt'), map_location='cpu')
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


# ---------------------------------------------------------------------------------------------------------------- two replicas
KEEP = 4096        # leading elements of every variable the replicas report


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _batch(world):
    g = torch.Generator().manual_seed(51)
    images = structured_images(world * B, SIZE, 2, g)
    ids = torch.randint(0, NCLS, (world * B,), generator=g)
    return images, ids


def _weights(model):
    return {v.name: _np(v.value.reshape(-1)[:KEEP]).copy() for v in model.variables}


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
        FLAGS = _flags()
        FLAGS.update(train_batch_size=world * B)
        RT = _fresh_runtime()
        strategy = comm.Strategy()
        RT.strategy = strategy
        model = model_lib.Model(NCLS)
        attrs = {}
        box = _capture(lambda o, name, v: (attrs.setdefault((id(o), name), (o, name, getattr(o, name))), setattr(o, name, v)), model)
        step = make_single_step(model, model_lib.build_optimizer(0.1), strategy)
        images, ids = _batch(world)
        out = step(images[rank * B:(rank + 1) * B].to(DEV), {'labels': ids[rank * B:(rank + 1) * B].to(DEV)})
        torch.cuda.synchronize()
        res = dict(hidden=_np(box['hidden']), d_proj=_np(box['d_proj']), loss=float(out['con_loss'].value),
                   on_diag=float(out['con_loss'].on_diag), off_diag=float(out['con_loss'].off_diag), weights=_weights(model))
        for o, name, v in attrs.values():
            setattr(o, name, v)
        dist.destroy_process_group()
        q.put((rank, 'ok', res))
    except Exception:  # noqa
        import traceback
        q.put((rank, 'FAIL', traceback.format_exc()))


def test_two_replica_step_vs_the_one_replica_step_on_the_gathered_batch():
    """Two gloo ranks sharing one GPU.  The gradient each rank's step hands its projection head equals the restatement's on the global
    batch of both ranks' projection outputs; the mean of the two loss values and the weights after the step agree with ONE replica's step
    on the gathered batch within the gradient gate."""
    import torch.multiprocessing as mp
    from simclr_amd import model as model_lib
    from simclr_amd.flags import FLAGS
    from simclr_amd.run import make_single_step
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
    FLAGS = _flags()
    ref = barlow_gram([b['hidden'] for b in boxes], FLAGS.bt_lambda, FLAGS.bt_loss_scaling)
    out = []
    for r, b in enumerate(boxes):
        out += [_res('two_replica_loss rank %d' % r, b['loss'], ref['loss'][r], GATE_LOSS),
                _res('two_replica_on_diag rank %d' % r, b['on_diag'], ref['on_diag'][r], GATE_LOSS),
                _res('two_replica_off_diag rank %d' % r, b['off_diag'], ref['off_diag'][r], GATE_LOSS),
                _res('two_replica_d_proj rank %d' % r, b['d_proj'], ref['grads'][r], GATE_GRAD)]
    # one replica, the gathered batch, the same initial weights (the initialisation is a function of the seed alone)
    FLAGS.update(train_batch_size=2 * B)
    _fresh_runtime()
    model = model_lib.Model(NCLS)
    step = make_single_step(model, model_lib.build_optimizer(0.1), None)
    images, ids = _batch(2)
    one = step(images.to(DEV), {'labels': ids.to(DEV)})
    torch.cuda.synchronize()
    after = _weights(model)
    out.append(_res('two_replica_loss_mean vs one replica', 0.5 * (boxes[0]['loss'] + boxes[1]['loss']), float(one['con_loss'].value), GATE_GRAD))
    for name in sorted(after):
        for r, b in enumerate(boxes):
            out.append(_res('two_replica_weights rank %d %s' % (r, name), b['weights'][name], after[name], GATE_GRAD))
    _assert(out)
