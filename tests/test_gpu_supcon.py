"""The supervised contrastive loss on the device (pytest -m gpu): the fused sweeps of csrc/supcon.hip through the C ABI and simclr_amd.ops
against the float64 restatement tests/supcon_reference.py, then the handle inside the step, run.main end to end (metrics, resume) and two
replicas over gloo.

Gates: the project's own for the same arithmetic (tests/test_gpu_gcl.py, tests/gpu_checks.py::check_ntxent) -- the loss 1e-5 relative,
gradients 2e-4 of the reference tensor's maximum; contrast_acc and contrast_positives are counts and must be exact wherever the dot
products are (the lattice test), the positive count everywhere."""
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

from tests.gpu_checks import DEV, _res, structured_images
from tests.supcon_reference import l2_normalize, supcon_reference

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


# ---------------------------------------------------------------------------------------------------------------- the sweeps
def _device(hs, ys, n, T, hidden_norm, rank):
    """The device path of one replica, assembled over replicas as tests/test_gpu_gcl.py::_device_lse does it: total gradient wrt rank's
    hidden = its query-side part + the sum over replicas q of dz_all_q[rank's rows].  Returns (out [3] of rank, dh [2n, D])."""
    from simclr_amd import ops
    R, D = len(hs), hs[0].shape[1]
    N = n * R
    zs, invs = [], []
    for h in hs:
        x = torch.from_numpy(h).to(DEV)
        z, inv = ops.l2norm_fwd(x) if hidden_norm else (x, None)
        zs.append(z); invs.append(inv)
    z_all = torch.cat([z[:n] for z in zs] + [z[n:] for z in zs], 0).contiguous()
    y_all = torch.from_numpy(np.concatenate(ys).astype(np.int32)).to(DEV)
    dz_slot = torch.zeros(2 * n, D, device=DEV)
    out = dz_local = None
    for q in range(R):
        o_q, rs_q, ws_q = ops.supcon_fwd(zs[q], z_all, y_all, q, T)
        dl, da = ops.supcon_bwd(zs[q], z_all, y_all, q, T, rs_q, 1.0 / R, ws_q)
        if q == rank:
            out, dz_local = o_q[:3].clone(), dl
        dz_slot[:n] += da[rank * n:(rank + 1) * n]
        dz_slot[n:] += da[N + rank * n:N + (rank + 1) * n]
    dz = dz_local + dz_slot
    dh = ops.l2norm_bwd(zs[rank], invs[rank], dz) if hidden_norm else dz
    torch.cuda.synchronize()
    return out.cpu().double(), dh


def _label_patterns(N):
    """arange(N) % C for C in {1, 3, N}, and a single singleton class among large ones."""
    single = np.arange(N) % 2
    single[N // 2] = 99
    return [('C=1', np.arange(N) % 1), ('C=3', np.arange(N) % 3), ('C=N', np.arange(N) % N), ('singleton', single)]


def check_supcon(n, R, D, T, hidden_norm, rank, labels_all, tag, seed=3, row_scale=None):
    g = np.random.default_rng(seed + n)
    hs = [g.standard_normal((2 * n, D)).astype(np.float32) for _ in range(R)]
    if row_scale is not None:       # rows of length row_scale
        hs = [(l2_normalize(h.astype(np.float64))[0] * row_scale).astype(np.float32) for h in hs]
    ys = [labels_all[r * n:(r + 1) * n] for r in range(R)]
    ref = supcon_reference(hs, ys, hidden_norm, T)
    o, dh = _device(hs, ys, n, T, hidden_norm, rank)
    tag = 'n=%d R=%d D=%d T=%g norm=%d rank=%d %s%s' % (n, R, D, T, hidden_norm, rank, tag, '' if row_scale is None else ' |row|=%g' % row_scale)
    return [_res('supcon_loss ' + tag, o[0], ref['loss'][rank], GATE_LOSS),
            _res('supcon_positives ' + tag, o[2], np.float32(ref['positives'][rank]), 0, 0),     # a count: exact
            _res('supcon_grad ' + tag, dh, ref['grads'][rank], GATE_GRAD)]


SHAPES = [(1, 1, 64, 0), (8, 1, 64, 0), (24, 1, 128, 0), (64, 2, 128, 1), (96, 2, 256, 0), (100, 1, 128, 0)]


@pytest.mark.parametrize('hidden_norm', [True, False])
@pytest.mark.parametrize('T', [0.1, 1.0])
@pytest.mark.parametrize('n,R,D,rank', SHAPES)
def test_kernel_vs_float64(n, R, D, rank, T, hidden_norm):
    res = []
    for tag, labels_all in _label_patterns(n * R):
        res += check_supcon(n, R, D, T, hidden_norm, rank, labels_all, tag)
    _assert(res)


def _lattice_case():
    """n = 24, D = 64, entries in {-1, -1/2, 0, 1/2, 1}: every dot product is a multiple of 1/4 below 2^7, exact in fp32.  Three planted
    rows give view 1 of image 0 (class 0) the same logit, 16, on its other view (a positive) and on view 1 of image 1 (class 1): a tie
    between the best positive and the best non-positive, which counts as a hit."""
    n, D = 24, 64
    g = np.random.default_rng(17)
    h = g.integers(-2, 3, size=(2 * n, D)).astype(np.float32) / 2.0
    q = np.zeros(D, np.float32); q[:32] = 1.0
    t = np.zeros(D, np.float32); t[:16] = 1.0; t[32:48] = 1.0
    u = np.zeros(D, np.float32); u[:16] = 1.0; u[48:] = 1.0
    h[0], h[n], h[1] = q, t, u
    y = np.arange(n) % 3
    return n, D, h, y


def test_exact_lattice_counts_and_ties():
    n, D, h, y = _lattice_case()
    S = h.astype(np.float64) @ h.astype(np.float64).T
    off = S - np.diag(np.full(2 * n, np.inf))
    assert (np.diag(S) > off.max(axis=1)).all(), 'the self logit must lie strictly above every other: a missed mask then flips the result'
    ycol = np.concatenate([y, y])
    pos = (ycol[:, None] == ycol[None, :]) & ~np.eye(2 * n, dtype=bool)
    pmax = np.where(pos, S, -np.inf).max(axis=1)
    omax = np.where(~pos & ~np.eye(2 * n, dtype=bool), S, -np.inf).max(axis=1)
    assert (pmax == omax).any() and (pmax < omax).any() and (pmax > omax).any(), 'the case must hold a tie, a miss and a clear hit'
    ref = supcon_reference([h], [y], False, 1.0)
    assert 0.0 < ref['acc'][0] < 1.0
    o, dh = _device([h], [y], n, 1.0, False, 0)
    print('lattice: acc %r (ref %r) positives %r (ref %r)' % (float(o[1]), ref['acc'][0], float(o[2]), ref['positives'][0]))
    assert float(o[1]) == float(np.float32(ref['acc'][0]))
    assert float(o[2]) == float(np.float32(ref['positives'][0]))
    _assert([_res('supcon_lattice_loss', o[0], ref['loss'][0], GATE_LOSS), _res('supcon_lattice_grad', dh, ref['grads'][0], GATE_GRAD)])
    # one class only: no non-positive column anywhere, every row a hit
    o1, _ = _device([h], [np.zeros(n, np.int64)], n, 1.0, False, 0)
    assert float(o1[1]) == 1.0 and float(o1[2]) == 2.0 * n - 1


@pytest.mark.parametrize('hidden_norm,T', [(True, 0.1), (False, 1.0)])
@pytest.mark.parametrize('n,D', [(24, 128), (100, 64)])
def test_distinct_labels_equal_ntxent(n, D, hidden_norm, T):
    from simclr_amd import objective
    g = torch.Generator().manual_seed(n + D)
    h = torch.randn(2 * n, D, generator=g).to(DEV)
    y = torch.randperm(n, generator=g).to(DEV)
    sup = objective.add_supcon_loss(h, y, hidden_norm, T)
    d_sup = sup.backward(1.0)
    nt, logits, _ = objective.add_contrastive_loss(h, hidden_norm, T)
    d_nt = nt.backward(1.0)
    torch.cuda.synchronize()
    assert float(sup.positives) == 1.0
    _assert([_res('supcon_vs_ntxent_loss n=%d D=%d' % (n, D), sup.value, nt.value, GATE_LOSS),
             _res('supcon_vs_ntxent_grad n=%d D=%d' % (n, D), d_sup, d_nt, GATE_GRAD)])


@pytest.mark.parametrize('n,R,D', [(24, 1, 128), (64, 2, 64)])
def test_kernel_unbounded_logits(n, R, D):
    """hidden_norm=False with rows of length 30 at T = 0.1: S / T reaches 9000 -- exp() of it overflows fp32 unless the running row
    maximum is subtracted."""
    res = check_supcon(n, R, D, 0.1, False, R - 1, np.arange(n * R) % 3, 'C=3', row_scale=30.0)
    assert all(math.isfinite(r['err']) for r in res)
    _assert(res)


def test_kernel_is_bitwise_deterministic_and_blind_to_class_names():
    from simclr_amd import ops
    g = torch.Generator().manual_seed(5)
    n, N, D = 96, 192, 128
    z = F.normalize(torch.randn(2 * n, D, generator=g)).to(DEV)
    z_all = torch.cat([z[:n], F.normalize(torch.randn(n, D, generator=g)).to(DEV), z[n:],
                       F.normalize(torch.randn(n, D, generator=g)).to(DEV)], 0).contiguous()
    y = torch.randint(0, 7, (N,), generator=g).to(torch.int32)
    rename = torch.tensor([40, -3, 2 ** 31 - 1, 0, 6, 1, -2 ** 31], dtype=torch.int64)      # a permutation of names, extremes included
    runs = []
    for labels in (y, y, rename[y.long()].to(torch.int32)):
        lab = labels.to(DEV)
        out, rs, ws = ops.supcon_fwd(z, z_all, lab, 0, 0.1)
        dl, da = ops.supcon_bwd(z, z_all, lab, 0, 0.1, rs, 0.5, ws)
        torch.cuda.synchronize()
        runs.append((out[:3].clone(), rs.clone(), dl, da))
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)


def test_kernel_refuses_bad_arguments():
    from simclr_amd import ops
    from simclr_amd._lib import SimclrHipError, lib
    L = lib()
    f = ctypes.c_float
    with pytest.raises(SimclrHipError, match='D must be 64/128/256'):
        L.supcon_fwd(None, None, None, 4, 4, 100, 0, f(0.1), None, None, None, None)
    with pytest.raises(SimclrHipError, match='D must be 64/128/256'):
        L.supcon_bwd(None, None, None, 4, 4, 512, 0, f(0.1), None, f(1.0), None, None, None, None)
    with pytest.raises(SimclrHipError, match='n >= 1'):
        L.supcon_fwd(None, None, None, 0, 4, 128, 0, f(0.1), None, None, None, None)
    with pytest.raises(SimclrHipError, match='N = R\\*n'):
        L.supcon_bwd(None, None, None, 4, 6, 128, 0, f(0.1), None, f(1.0), None, None, None, None)
    with pytest.raises(SimclrHipError, match='rank 2 out of range'):
        L.supcon_fwd(None, None, None, 4, 8, 128, 2, f(0.1), None, None, None, None)
    with pytest.raises(SimclrHipError, match='null argument'):
        L.supcon_fwd(None, None, None, 4, 4, 128, 0, f(0.1), None, None, None, None)
    with pytest.raises(SimclrHipError, match='null argument'):
        L.supcon_bwd(None, None, None, 4, 4, 128, 0, f(0.1), None, f(1.0), None, None, None, None)
    assert L.supcon_workspace_bytes(4, 4, 100) == 0 and L.supcon_workspace_bytes(0, 4, 64) == 0 and L.supcon_workspace_bytes(4, 8, 64) > 0
    z = torch.zeros(8, 64, device=DEV)
    with pytest.raises(ValueError, match='labels_all must hold the N = 4'):
        ops.supcon_fwd(z, z, torch.zeros(5, dtype=torch.int32, device=DEV), 0, 0.1)
    with pytest.raises(ValueError, match='labels_all must hold the N = 4'):
        ops.supcon_fwd(z, z, torch.zeros(4, dtype=torch.int64, device=DEV), 0, 0.1)
    with pytest.raises(ValueError, match='64/128/256'):
        ops.supcon_fwd(torch.zeros(8, 96, device=DEV), torch.zeros(8, 96, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV), 0, 0.1)


# ---------------------------------------------------------------------------------------------------------------- handle and step
def _flags(**kw):
    from simclr_amd.flags import FLAGS
    FLAGS.reset()
    FLAGS.update(resnet_depth=18, image_size=SIZE, compute_dtype='f32', f32_matmul='exact', use_blur=False, train_batch_size=B,
                 train_mode='pretrain', contrastive_loss='supcon', **kw)
    return FLAGS


def _fresh_runtime():
    from simclr_amd.resnet import RT
    RT.reset()
    RT.device = torch.device(DEV)
    return RT


def _capture(setattr_fn, model):
    """Records what the step hands the loss (projection outputs, labels) and what it hands the projection head."""
    from simclr_amd import objective as obj_lib
    box = {}
    orig_loss, orig_backward = obj_lib.add_supcon_loss, model.backward

    def loss_fn(hidden, labels, *a, **kw):
        box['hidden'] = hidden.detach().clone()
        box['labels'] = obj_lib._class_ids(labels).detach().clone()
        box['loss'] = orig_loss(hidden, labels, *a, **kw)
        return box['loss']

    def backward(d_proj, *a, **kw):
        box['d_proj'] = d_proj.detach().clone()
        return orig_backward(d_proj, *a, **kw)
    setattr_fn(obj_lib, 'add_supcon_loss', loss_fn)
    setattr_fn(model, 'backward', backward)
    return box


def _np(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


@pytest.mark.parametrize('lineareval', [True, False])
def test_step_hands_the_projection_head_the_reference_gradient(monkeypatch, lineareval):
    from simclr_amd import model as model_lib
    from simclr_amd.run import make_single_step
    FLAGS = _flags(lineareval_while_pretraining=lineareval)
    _fresh_runtime()
    model = model_lib.Model(NCLS)
    box = _capture(monkeypatch.setattr, model)
    step = make_single_step(model, model_lib.build_optimizer(0.1), None)
    sup = ['train/supervised_acc', 'train/supervised_loss'] if lineareval else []
    assert sorted(step.metrics) == sorted(['train/contrast_acc', 'train/contrast_loss', 'train/contrast_positives', 'train/total_loss',
                                           'train/weight_decay'] + sup)
    g = torch.Generator().manual_seed(31)
    images = structured_images(B, SIZE, 2, g).to(DEV)
    ids = torch.randint(0, NCLS, (B,), generator=g)
    out = step(images, {'labels': F.one_hot(ids, NCLS).float().to(DEV)})
    torch.cuda.synchronize()
    assert tuple(box['hidden'].shape) == (2 * B, FLAGS.proj_out_dim) and out['logits_con'] is None
    assert np.array_equal(_np(box['labels']), ids.numpy())
    ref = supcon_reference([_np(box['hidden'])], [ids.numpy()], FLAGS.hidden_norm, FLAGS.temperature)
    con = out['con_loss']
    _assert([_res('step_loss', con.value, ref['loss'][0], GATE_LOSS), _res('step_positives', con.positives, np.float32(ref['positives'][0]), 0, 0),
             _res('step_d_proj', box['d_proj'], ref['grads'][0], GATE_GRAD)])
    m = step.metrics
    assert m['train/contrast_positives'].result() == float(np.float32(ref['positives'][0]))
    assert 0.0 <= m['train/contrast_acc'].result() <= 1.0
    assert all(bool(torch.isfinite(v.value).all()) for v in model.variables)


def test_run_main_trains_logs_and_resumes_bitwise(tmp_path, capsys):
    from simclr_amd import run
    from simclr_amd.checkpoint import INDEX_NAME
    from simclr_amd.flags import FLAGS
    args = ['--dataset=synthetic', '--resnet_depth=18', '--image_size=32', '--train_batch_size=8', '--use_blur=False', '--compute_dtype=f32',
            '--checkpoint_steps=2', '--train_steps=3', '--mode=train', '--contrastive_loss=supcon']
    full_dir, again_dir = str(tmp_path / 'full'), str(tmp_path / 'again')
    FLAGS.reset()
    run.main(args + ['--model_dir=' + full_dir])
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith('{') and 'train/contrast_positives' in l]
    assert lines and lines[0]['step'] == 2
    for k in ('train/contrast_loss', 'train/contrast_acc', 'train/contrast_positives', 'train/total_loss'):
        assert math.isfinite(lines[0][k]), (k, lines[0])
    assert 'train/contrast_entropy' not in lines[0] and 'train/align_loss' not in lines[0]
    assert 1.0 <= lines[0]['train/contrast_positives'] <= 15.0 and 0.0 <= lines[0]['train/contrast_acc'] <= 1.0
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
        g = torch.Generator().manual_seed(51)
        images = structured_images(world * B, SIZE, 2, g)
        ids = torch.randint(0, NCLS, (world * B,), generator=g)
        out = step(images[rank * B:(rank + 1) * B].to(DEV), {'labels': ids[rank * B:(rank + 1) * B].to(DEV)})      # integer ids this time
        torch.cuda.synchronize()
        res = dict(hidden=_np(box['hidden']), labels=_np(box['labels']), d_proj=_np(box['d_proj']), loss=float(out['con_loss'].value),
                   acc=float(out['con_loss'].acc), positives=float(out['con_loss'].positives), want_labels=ids[rank * B:(rank + 1) * B].numpy())
        for o, name, v in attrs.values():
            setattr(o, name, v)
        dist.destroy_process_group()
        q.put((rank, 'ok', res))
    except Exception:  # noqa
        import traceback
        q.put((rank, 'FAIL', traceback.format_exc()))


def test_two_replica_step_vs_the_global_batch_restatement():
    """Two gloo ranks sharing one GPU: the gradient each rank's step hands its projection head equals the gradient of the single-process
    objective (1 / R) sum_r loss_r on the global batch of both ranks' projection outputs and labels."""
    import torch.multiprocessing as mp
    from simclr_amd.flags import FLAGS
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
    FLAGS.reset()
    assert all(np.array_equal(b['labels'], b['want_labels']) for b in boxes)
    ref = supcon_reference([b['hidden'] for b in boxes], [b['labels'] for b in boxes], FLAGS.hidden_norm, FLAGS.temperature)
    out = []
    for r, b in enumerate(boxes):
        out += [_res('two_replica_loss rank %d' % r, b['loss'], ref['loss'][r], GATE_LOSS),
                _res('two_replica_positives rank %d' % r, b['positives'], np.float32(ref['positives'][r]), 0, 0),
                _res('two_replica_d_proj rank %d' % r, b['d_proj'], ref['grads'][r], GATE_GRAD)]
    _assert(out)
