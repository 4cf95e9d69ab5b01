"""The representation diagnostics on the device (pytest -m gpu): the kernels of csrc/repr.hip through simclr_amd.ops and the C ABI against
the float64 restatement tests/repr_reference.py, then the handle of metrics.representation_stats, the measured step under three losses,
run.main end to end (keys per logging window, resume, the flag at 0) and two replicas over gloo.

Gates: per output 4 x the error of the float32 emulation of that case against float64, never below one float32 ulp of the float64
value (repr_reference.gates; the figures measured on the device are recorded in tests/golden/REPR_HAND_DERIVED.md)."""
import ctypes
import json
import os
import shutil
import socket

import numpy as np
import pytest
import torch

from tests import repr_reference as rr
from tests.gpu_checks import DEV, structured_images

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


def _np(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def _device(z32, t=2.0, ws=None):
    from simclr_amd import ops
    out = ops.repr_stats(torch.from_numpy(np.array(z32, np.float32)).to(DEV), t, ws)
    torch.cuda.synchronize()
    return _np(out).astype(np.float64)


def _check(tag, got, ref, gate):
    """Prints every figure, then asserts."""
    err, ok = rr.compare(got, ref, gate)
    for k, name in enumerate(rr.NAMES):
        print('%-4s %-8s %-44s got=%+.9e ref=%+.9e err=%.3e gate=%.3e ulps=%.2f' % (
            'ok' if ok[k] else 'FAIL', name, tag, got[k], ref[k], err[k], gate[k], err[k] / max(rr.ulp32(ref[k]), 1e-300)))
    assert ok.all(), '%s: %s' % (tag, [(n, e, g) for n, e, g, o in zip(rr.NAMES, err, gate, ok) if not o])


# ---------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize('N,D', rr.SHAPES, ids=lambda v: str(v))
def test_kernels_vs_float64(N, D):
    from simclr_amd import ops
    assert ops.repr_tile_edge(N, D) == rr.EDGES[(N, D)]
    for t in rr.TS:
        for fam in rr.FAMILIES:
            z, ref, emu, gate = rr.case(N, D, t, fam)
            assert min(rr.trace_cov(z)) > 1e-9          # the collapse branch cannot flip
            _check('N=%d D=%d t=%g %s' % (N, D, t, fam), _device(z, t), ref, gate)


def test_hand_cases_on_the_device():
    """Every product and sum of the first two cases is exact in float32, so the device value is the float32 neighbour of the float64
    one; identical rows give four zeros bitwise."""
    for tag, z, want in (('signed basis rows', rr.hand_basis(64), np.array([0.0, -4.0, 1.0, 63.0])),
                         ('antipodal rows', rr.hand_antipodal(64, 64), rr.hand_antipodal_values(64, 64, 2.0))):
        _check(tag, _device(z, 2.0), want, np.array([rr.ulp32(w) if w else 0.0 for w in want]))
    from simclr_amd import ops
    out = ops.repr_stats(torch.from_numpy(rr.hand_collapsed()).to(DEV), 2.0)
    assert out.cpu().view(torch.int32).tolist() == [0, 0, 0, 0]
    two = _device(rr.case_views(2, 64, 'gauss'), 2.0)
    assert abs(two[3] - 1.0) <= rr.ulp32(1.0)


def test_kernels_are_bitwise_repeatable():
    from simclr_amd import ops
    for N, D in ((129, 192), (70, 2048), (1409, 64)):            # the last on the 128-wide tile
        z = torch.from_numpy(np.array(rr.case_views(N, D, 'clusters'))).to(DEV)
        keep = z.clone()
        ws = ops.repr_workspace(N, D, DEV)
        a = ops.repr_stats(z, 2.0, ws).clone()
        ws.fill_(float('nan'))                       # nothing of an earlier call is read
        b = ops.repr_stats(z, 2.0, ws)
        c = ops.repr_stats(z, 2.0)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), c.view(torch.int32))
        assert torch.equal(z, keep)                  # the input is read only


@pytest.mark.parametrize('N,D', [(2, 64), (65, 128), (129, 192), (1409, 64), (1536, 64)], ids=lambda v: str(v))
def test_workspace_and_output_stay_between_guard_bands(N, D):
    from simclr_amd import _lib, ops
    L = _lib.lib()
    assert L.repr_tile_edge(N, D) == rr.EDGES[(N, D)]
    nbytes = L.repr_workspace_bytes(N, D)
    assert nbytes > 0 and nbytes % 8 == 0
    G = 512
    buf = torch.full((nbytes // 8 + 2 * G,), -7.25, device=DEV, dtype=torch.float64)
    outbuf = torch.full((4 + 2 * G,), -7.25, device=DEV, dtype=torch.float32)
    z = torch.from_numpy(np.array(rr.case_views(N, D, 'gauss'))).to(DEV)
    ws, out = buf[G:G + nbytes // 8], outbuf[G:G + 4]
    L.repr_stats(ctypes.c_void_p(z.data_ptr()), N, D, ctypes.c_float(2.0), ctypes.c_void_p(ws.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    for band in (buf[:G], buf[G + nbytes // 8:], outbuf[:G], outbuf[G + 4:]):
        assert bool((band == -7.25).all())
    assert torch.equal(out.clone(), ops.repr_stats(z, 2.0))


def test_refusals_through_ops_and_the_c_abi():
    from simclr_amd import _lib, ops
    good = torch.zeros(16, 64, device=DEV)
    for bad, msg in ((torch.zeros(16, 100, device=DEV), 'multiples of 64'), (torch.zeros(16, 32, device=DEV), 'multiples of 64'),
                     (torch.zeros(2, 64, device=DEV), 'rows per view'), (torch.zeros(15, 64, device=DEV), r'\[2N, D\]'),
                     (torch.zeros(16, 64, device=DEV, dtype=torch.float64), r'\[2N, D\]')):
        with pytest.raises(ValueError, match=msg):
            ops.repr_stats(bad)
    for t in (0.0, -1.0, 16.5, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='t must lie'):
            ops.repr_stats(good, t)
    with pytest.raises(ValueError, match='workspace holds'):
        ops.repr_stats(good, 2.0, torch.zeros(8, device=DEV, dtype=torch.float64))
    L = _lib.lib()
    ws, out = ops.repr_workspace(8, 64, DEV), torch.full((4,), -7.25, device=DEV)
    p = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None else None
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for z, N, D, t, w, o, msg in ((good, 8, 96, 2.0, ws, out, 'multiple of 64'), (good, 8, 8256, 2.0, ws, out, 'multiple of 64'),
                                  (good, 1, 64, 2.0, ws, out, '2 <= N'), (good, 65537, 64, 2.0, ws, out, '2 <= N'),
                                  (good, 8, 64, 0.0, ws, out, 't must lie'), (good, 8, 64, float('nan'), ws, out, 't must lie'),
                                  (good, 8, 64, 17.0, ws, out, 't must lie'), (None, 8, 64, 2.0, ws, out, 'null argument'),
                                  (good, 8, 64, 2.0, None, out, 'null argument'), (good, 8, 64, 2.0, ws, None, 'null argument')):
        with pytest.raises(_lib.SimclrHipError, match=msg):
            L.repr_stats(p(z), N, D, ctypes.c_float(t), p(w), p(o), s)
    torch.cuda.synchronize()
    assert bool((out == -7.25).all())                 # a refused call launches nothing


# ---------------------------------------------------------------------------------------------------------------- handle
def test_handle_matches_the_restatement():
    from simclr_amd import metrics
    n, D, t = 40, 128, 3.0
    h = torch.from_numpy((3.0 * np.random.RandomState(11).randn(2 * n, D)).astype(np.float32)).to(DEV)
    keep = h.clone()
    s = metrics.representation_stats(h, None, t)
    torch.cuda.synchronize()
    assert torch.equal(h, keep) and s.gathered is s.normalized and tuple(s.values.shape) == (4,) and s.values.dtype == torch.float32
    for k, name in enumerate(rr.NAMES):
        assert getattr(s, name).data_ptr() == s.values[k:k + 1].data_ptr() and tuple(getattr(s, name).shape) == (1,)
    z = _np(s.normalized)
    assert np.abs(z.astype(np.float64) - rr.normalize(_np(h))).max() < 4e-7
    ref, emu = rr.direct(z, t), rr.emulate(z, t)
    _check('handle', _np(s.values).astype(np.float64), ref, rr.gates(emu, ref))
    # the scale of the input changes nothing beyond the rounding of the normalisation
    s3 = metrics.representation_stats(h / 3.0, None, t)
    assert float((s3.values - s.values).abs().max()) < 1e-4


# ---------------------------------------------------------------------------------------------------------------- step
def _fresh_runtime():
    from simclr_amd.resnet import RT
    RT.reset()
    RT.device = torch.device(DEV)
    return RT


def _flags(loss, K, **kw):
    from simclr_amd.flags import FLAGS
    FLAGS.reset()
    kw.setdefault('proj_out_dim', 64)
    if loss == 'byol':
        kw.setdefault('byol_pred_hidden_dim', 128)
    if loss == 'dino':
        kw.update(dino_out_dim=200, dino_momentum=0.9, dino_freeze_last_layer_epochs=0, dino_local_crops=2, dino_local_crop_size=16)
    FLAGS.update(resnet_depth=18, image_size=SIZE, compute_dtype='f32', f32_matmul='exact', use_blur=False, train_batch_size=B,
                 train_mode='pretrain', train_steps=10, contrastive_loss=loss, repr_metrics_steps=K, repr_uniform_t=3.0, **kw)
    return FLAGS


def _build(loss):
    from simclr_amd import model as model_lib
    from simclr_amd.flags import FLAGS
    from simclr_amd.run import make_single_step
    model = model_lib.Model(NCLS)
    target = None
    if loss == 'byol':
        target = model_lib.TargetNetwork(model, 10)
    elif loss == 'dino':
        target = model_lib.TargetNetwork(model, 10, center=model_lib.DinoCenter(FLAGS.dino_out_dim), steps_per_epoch=2)
    return model, make_single_step(model, model_lib.build_optimizer(0.1), None, target=target)


def _three_steps(loss, K, monkeypatch=None):
    from simclr_amd import metrics
    _flags(loss, K)
    _fresh_runtime()
    model, step = _build(loss)
    seen = []
    if monkeypatch is not None:
        orig = metrics.start_representation_stats

        def start(hidden, *a, **kw):
            seen.append(hidden.detach().clone())
            return orig(hidden, *a, **kw)
        monkeypatch.setattr(metrics, 'start_representation_stats', start)
    g = torch.Generator().manual_seed(31)
    outs = []
    for _ in range(3):
        images = structured_images(B, SIZE, 2, g).to(DEV)
        labels = {'labels': torch.nn.functional.one_hot(torch.randint(0, NCLS, (B,), generator=g), NCLS).float().to(DEV)}
        feats = (images, structured_images(B, 16, 2, g).to(DEV)) if loss == 'dino' else images
        outs.append(step(feats, labels))
    torch.cuda.synchronize()
    if monkeypatch is not None:
        monkeypatch.undo()
    return {v.name: v.value.detach().clone() for v in model.variables}, outs, seen, step


@pytest.mark.parametrize('loss', ['ntxent', 'byol', 'dino'])
def test_measured_steps_leave_the_weights_bitwise_alone(loss, monkeypatch):
    """Three steps with K = 1 (dino: two local crops) against K = 0: the weights are bitwise equal, and what every step returns under
    `repr_stats` is representation_stats of the online projection that step produced."""
    from simclr_amd import metrics
    off, outs0, _, step0 = _three_steps(loss, 0)
    assert all('repr_stats' not in o for o in outs0) and not any('repr' in n for n in step0.metrics)
    on, outs, seen, step = _three_steps(loss, 1, monkeypatch)
    assert sorted(on) == sorted(off) and all(torch.equal(on[n], off[n]) for n in off)
    assert len(seen) == 3 and all(tuple(h.shape) == (2 * B, 64) for h in seen)
    for o, hidden in zip(outs, seen):
        again = metrics.representation_stats(hidden, None, 3.0)
        assert torch.equal(o['repr_stats'].values.view(torch.int32), again.values.view(torch.int32))
        z = _np(again.normalized)
        ref = rr.direct(z, 3.0)
        _check('step %s' % loss, _np(again.values).astype(np.float64), ref, rr.gates(rr.emulate(z, 3.0), ref))
    last = outs[-1]['repr_stats']
    for nm, attr in metrics.REPR_METRICS:
        m = step.metrics[nm]
        assert m._count == 3
        want = sum(float(getattr(o['repr_stats'], attr)) for o in outs) / 3.0
        assert abs(m.result() - want) <= 1e-6 * max(abs(want), 1.0), (nm, m.result(), want)
    assert 0.0 <= float(last.align) <= 4.0 and -12.0 <= float(last.uniform) <= 0.0 and float(last.std) >= 0.0 and float(last.rank) <= 15.0


def test_only_every_kth_step_is_measured():
    _flags('ntxent', 2)
    _fresh_runtime()
    model, step = _build('ntxent')
    g = torch.Generator().manual_seed(31)
    got = []
    for _ in range(4):
        images = structured_images(B, SIZE, 2, g).to(DEV)
        labels = {'labels': torch.nn.functional.one_hot(torch.randint(0, NCLS, (B,), generator=g), NCLS).float().to(DEV)}
        got.append(step(images, labels)['repr_stats'])
    assert [h is not None for h in got] == [False, True, False, True]
    assert step.metrics['train/repr_rank']._count == 2 and step.metrics['train/total_loss']._count == 4


# ---------------------------------------------------------------------------------------------------------------- run.main
COMMON = ['--dataset=synthetic', '--resnet_depth=18', '--image_size=32', '--train_batch_size=8', '--use_blur=False', '--compute_dtype=f32',
          '--contrastive_loss=ntxent', '--proj_out_dim=64', '--checkpoint_steps=1', '--train_steps=4', '--mode=train']
FOUR = ['train/repr_align', 'train/repr_rank', 'train/repr_std', 'train/repr_uniform']


def _main(args, model_dir, capsys):
    from simclr_amd import run
    from simclr_amd.flags import FLAGS
    FLAGS.reset()
    capsys.readouterr()
    run.main(COMMON + args + ['--model_dir=' + model_dir])
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith('{') and 'train/total_loss' in l]
    with open(os.path.join(model_dir, 'summaries.jsonl')) as f:
        tags = [json.loads(l) for l in f]
    return lines, tags, torch.load(os.path.join(model_dir, 'ckpt-4.pt'), map_location='cpu')


def _same(a, b):
    assert sorted(a['model']) == sorted(b['model']) and all(torch.equal(a['model'][n], b['model'][n]) for n in a['model'])
    assert all(torch.equal(a['optimizer']['slots'][n], b['optimizer']['slots'][n]) for n in a['optimizer']['slots'])
    assert a['optimizer']['iterations'] == b['optimizer']['iterations']


def test_run_main_logs_measured_windows_only_resumes_bitwise_and_is_inert_at_zero(tmp_path, capsys):
    """run.main with K = 3 over four steps, a logging window per step, then a resume from step 2.  K = 3 and not 2 on purpose: the
    synthetic stream resumes bitwise from an even step only, and with K = 2 a measurement count kept by the process (wrong) and one read
    from optimizer.iterations (right) would both measure the second step after a resume from step 2; with K = 3 only the right one
    measures step 3.  K = 2 is covered at the step level by test_only_every_kth_step_is_measured."""
    from simclr_amd.checkpoint import INDEX_NAME
    dirs = {k: str(tmp_path / k) for k in ('plain', 'zero', 'two', 'again')}
    plain_lines, plain_tags, plain = _main([], dirs['plain'], capsys)
    zero_lines, zero_tags, zero = _main(['--repr_metrics_steps=0', '--repr_uniform_t=7'], dirs['zero'], capsys)
    _same(plain, zero)
    # the logged names per window (several logged scalars -- the weight decay, the supervised loss -- are summed with atomics and differ
    # in the last digit between two runs of the same weights; the checkpoints above are the bitwise statement)
    strip = lambda ls: [(l['step'], sorted(l)) for l in ls]
    names = lambda ts: [(r['tag'], r['step']) for r in ts]
    assert strip(plain_lines) == strip(zero_lines) and names(plain_tags) == names(zero_tags)
    assert not any('repr' in k for l in plain_lines for k in l)
    # K = 3, a logging window per step: step 3 alone is measured
    lines, tags, two = _main(['--repr_metrics_steps=3'], dirs['two'], capsys)
    _same(plain, two)                                                    # read-only: the weights of K = 0
    assert [l['step'] for l in lines] == [1, 2, 3, 4]
    assert [sorted(k for k in l if 'repr' in k) for l in lines] == [[], [], FOUR, []]
    assert sorted((r['tag'], r['step']) for r in tags if 'repr' in r['tag']) == sorted((k, 3) for k in FOUR)
    assert strip([{k: v for k, v in l.items() if 'repr' not in k} for l in lines]) == strip(plain_lines)
    l2 = lines[2]
    assert 0.0 <= l2['train/repr_align'] <= 4.0 and -8.0 <= l2['train/repr_uniform'] <= 0.0 and l2['train/repr_std'] >= 0.0
    assert 0.0 <= l2['train/repr_rank'] <= 7.0
    # resume from step 2 (the synthetic stream restarts, and its pool of two batches is back in phase at an even step): step 3, the
    # first step of the resumed run, is measured again -- the count is the optimizer's, not the process's -- and the final checkpoint
    # is bitwise the full run's
    os.makedirs(dirs['again'])
    shutil.copy(os.path.join(dirs['two'], 'ckpt-2.pt'), os.path.join(dirs['again'], 'ckpt-2.pt'))
    with open(os.path.join(dirs['again'], INDEX_NAME), 'w') as f:
        json.dump({'model_checkpoint_path': 'ckpt-2.pt', 'all_model_checkpoint_paths': ['ckpt-2.pt']}, f)
    again_lines, _, again = _main(['--repr_metrics_steps=3'], dirs['again'], capsys)
    _same(two, again)
    assert [l['step'] for l in again_lines] == [3, 4] and [sorted(k for k in l if 'repr' in k) for l in again_lines] == [FOUR, []]
    assert all(again_lines[0][k] == lines[2][k] for k in FOUR)
    assert not any('repr' in n for n in two['model'])                   # checkpoints gain nothing


# ---------------------------------------------------------------------------------------------------------------- two replicas
N_LOCAL, D_REP = 24, 128


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _local_hidden(rank):
    return (2.0 * np.random.RandomState(70 + rank).randn(2 * N_LOCAL, D_REP)).astype(np.float32)


def _worker(rank, world, port, q):
    try:
        import torch.distributed as dist
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        torch.cuda.set_device(0)
        dist.init_process_group('gloo', rank=rank, world_size=world)
        from simclr_amd import comm, metrics
        strategy = comm.Strategy()
        s = metrics.representation_stats(torch.from_numpy(_local_hidden(rank)).to(DEV), strategy, 2.0)
        torch.cuda.synchronize()
        res = dict(values=_np(s.values).copy(), gathered=_np(s.gathered).copy())
        dist.destroy_process_group()
        q.put((rank, 'ok', res))
    except Exception:  # noqa
        import traceback
        q.put((rank, 'FAIL', traceback.format_exc()))


def test_two_replicas_report_the_same_bits_as_one_process_on_the_whole_batch():
    import torch.multiprocessing as mp
    from simclr_amd import metrics
    os.environ['SIMCLR_PEER_STATS'] = '0'
    os.environ['SIMCLR_SHARE_GPU'] = '1'
    try:
        ctx = mp.get_context('spawn')
        q = ctx.Queue()
        port = _free_port()
        procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
        for p in procs:
            p.start()
        res = [q.get(timeout=300) for _ in procs]
        for p in procs:
            p.join(timeout=60)
    finally:
        os.environ.pop('SIMCLR_PEER_STATS', None)
        os.environ.pop('SIMCLR_SHARE_GPU', None)
    assert all(r[1] == 'ok' for r in res), res
    a, b = [r[2] for r in sorted(res, key=lambda r: r[0])]
    assert a['values'].tobytes() == b['values'].tobytes() and a['gathered'].tobytes() == b['gathered'].tobytes()
    h = [_local_hidden(r) for r in range(2)]
    whole = np.concatenate([h[0][:N_LOCAL], h[1][:N_LOCAL], h[0][N_LOCAL:], h[1][N_LOCAL:]])       # view-major
    one = metrics.representation_stats(torch.from_numpy(whole).to(DEV), None, 2.0)
    torch.cuda.synchronize()
    assert _np(one.gathered).tobytes() == a['gathered'].tobytes() and _np(one.values).tobytes() == a['values'].tobytes()
    z = _np(one.gathered)
    ref = rr.direct(z, 2.0)
    _check('two replicas', a['values'].astype(np.float64), ref, rr.gates(rr.emulate(z, 2.0), ref))
