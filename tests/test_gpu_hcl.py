"""The hard-negative / debiased NT-Xent on the device (pytest -m gpu): the fused sweeps of csrc/hcl.hip through the C ABI and simclr_amd.ops
against the float64 restatement tests/hcl_reference.py, then the handle inside the step, run.main end to end (metrics, resume, the
default flags) and two replicas over gloo.

Gates: 4 x the error of the float32 emulation of the kernels' arithmetic against float64 on the case's own inputs
(tests/hcl_reference.py: EMULATION_ERROR for the kernel cases, measured in the test for the step cases) -- the loss relative to itself,
the gradient relative to its largest entry.  The share of rows on the floor is a count and must be exact.  The gradient jumps at the
floor, so every case asserts first that no row lies within KINK_MARGIN of it: no row is ever left out of a comparison."""
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

from tests import hcl_reference as ref_lib
from tests.gpu_checks import DEV, structured_images
from tests.hcl_reference import FAMILIES, KINK_MARGIN, PARAMS, SHAPES, TOL, f32, hcl_emulated, hcl_reference, relative_errors

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


# ---------------------------------------------------------------------------------------------------------------- the sweeps
def _device(zs, n, T, beta, tau_plus, rank):
    """The device path of one replica on normalised float32 blocks, assembled over replicas as tests/test_gpu_supcon.py::_device does
    it: total gradient wrt rank's block = its query-side part + the sum over replicas q of dz_all_q[rank's rows], grad_scale = 1 / R.
    Returns (out [2] of rank, dz [2n, D])."""
    from simclr_amd import ops
    R, D = len(zs), zs[0].shape[1]
    N = n * R
    zd = [torch.from_numpy(z).to(DEV) for z in zs]
    z_all = torch.cat([z[:n] for z in zd] + [z[n:] for z in zd], 0).contiguous()
    dz_slot = torch.zeros(2 * n, D, device=DEV)
    out = dz_local = None
    for q in range(R):
        o_q, rs_q, ws_q = ops.hcl_fwd(zd[q], z_all, q, T, beta, tau_plus)
        dl, da = ops.hcl_bwd(zd[q], z_all, q, T, beta, tau_plus, rs_q, 1.0 / R, ws_q)
        if q == rank:
            out, dz_local = o_q[:2].clone(), dl
        dz_slot[:n] += da[rank * n:(rank + 1) * n]
        dz_slot[n:] += da[N + rank * n:N + (rank + 1) * n]
    dz = dz_local + dz_slot
    torch.cuda.synchronize()
    return out.cpu().double(), dz.cpu().double().numpy()


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'n%d-R%d-D%d-rank%d' % s)
def test_kernel_vs_float64(shape, family):
    n, R, D, rank = shape
    tol, bad, shares = TOL[(shape, family)], [], set()
    for params in PARAMS:
        zs, ref = ref_lib.case_reference(shape, family, params)
        near = ref_lib.kink_distance(ref)
        assert near >= KINK_MARGIN, 'a row %.3g from the floor at %r: choose another seed for this case' % (near, params)
        out, dz = _device(zs, n, *params, rank)
        err = relative_errors(out[0], dz, ref, rank)
        tag = 'n=%d R=%d D=%d rank=%d %s T=%g beta=%g tau_plus=%g floor=%.3f' % (shape + (family,) + params + (ref['floor_share'][rank],))
        _check('hcl_loss ' + tag, err['loss'], tol['loss'], bad)
        _check('hcl_grad ' + tag, err['grad'], tol['grad'], bad)
        assert float(out[1]) == float(np.float32(ref['floor_share'][rank])), tag          # a count: exact
        shares.add(ref['floor_share'][rank])
    assert not bad, '\n'.join(bad)
    if family == 'correlated':
        assert 0.0 in shares and 1.0 in shares, 'the correlated family must hold all-floor and no-floor cases'


def test_a_mixed_case_has_rows_on_both_sides_of_the_floor():
    """n = 65 (a last tile of two rows, the view boundary inside the second tile), independent views, T = 0.1, beta = 0,
    tau_plus = 0.1: a few rows on the floor, most above -- the per-row decision, not a per-launch one."""
    shape, params = (65, 1, 64, 0), (0.1, 0.0, 0.1)
    zs, ref = ref_lib.case_reference(shape, 'independent', params)
    assert 0.0 < ref['floor_share'][0] < 0.5
    from simclr_amd import ops
    z = torch.from_numpy(zs[0]).to(DEV)
    out, rs, _ = ops.hcl_fwd(z, z, 0, *params)
    torch.cuda.synchronize()
    on_floor = (rs[:, 2] == 0).cpu().numpy()
    assert np.array_equal(on_floor, ref['on_floor']) and float(out[1]) == float(np.float32(ref['floor_share'][0]))


def test_kernel_is_bitwise_deterministic():
    from simclr_amd import ops
    g = torch.Generator().manual_seed(5)
    n, N, D = 96, 192, 128
    z = F.normalize(torch.randn(2 * n, D, generator=g)).to(DEV)
    z_all = torch.cat([z[:n], F.normalize(torch.randn(n, D, generator=g)).to(DEV), z[n:],
                       F.normalize(torch.randn(n, D, generator=g)).to(DEV)], 0).contiguous()
    for beta, tau_plus in ((0.5, 0.1), (0.0, 0.0)):
        runs = []
        for _ in range(2):
            out, rs, ws = ops.hcl_fwd(z, z_all, 0, 0.1, beta, tau_plus)
            dl, da = ops.hcl_bwd(z, z_all, 0, 0.1, beta, tau_plus, rs, 0.5, ws)
            torch.cuda.synchronize()
            runs.append((out[:2].clone(), rs.clone(), dl, da))
        for a, b in zip(*runs):
            assert torch.equal(a, b)
        assert bool(torch.isfinite(runs[0][2]).all()) and bool(torch.isfinite(runs[0][3]).all())


@pytest.mark.parametrize('shape', [(24, 1, 128, 0), (64, 2, 128, 1), (100, 1, 128, 0)], ids=lambda s: 'n%d-R%d-D%d-rank%d' % s)
def test_zero_flags_equal_the_ntxent_kernels(shape):
    """beta = 0, tau_plus = 0 against ops.ntxent_fwd / _bwd on the same blocks: the two launches agree within the case's gate."""
    from simclr_amd import ops
    n, R, D, rank = shape
    zs = ref_lib.case_views(n, R, D, 'independent', ref_lib.CASE_SEED[(shape, 'independent')])
    zd = [torch.from_numpy(z).to(DEV) for z in zs]
    z_all = torch.cat([z[:n] for z in zd] + [z[n:] for z in zd], 0).contiguous()
    tol, bad = TOL[(shape, 'independent')], []
    for T in ref_lib.TEMPERATURES:
        out, rs, ws = ops.hcl_fwd(zd[rank], z_all, rank, T, 0.0, 0.0)
        dl, da = ops.hcl_bwd(zd[rank], z_all, rank, T, 0.0, 0.0, rs, 1.0, ws)
        o2, rs2, ws2 = ops.ntxent_fwd(zd[rank], z_all, rank, T)
        dl2, da2 = ops.ntxent_bwd(zd[rank], z_all, rank, T, rs2, 1.0, o2, ws2)
        torch.cuda.synchronize()
        assert float(out[1]) == 0.0
        _check('hcl_vs_ntxent_loss T=%g' % T, abs(float(out[0]) - float(o2[0])) / abs(float(o2[0])), tol['loss'], bad)
        for nm, a, b in (('dz_local', dl, dl2), ('dz_all', da, da2)):
            _check('hcl_vs_ntxent_%s T=%g' % (nm, T), float((a - b).abs().max() / b.abs().max()), tol['grad'], bad)
    assert not bad, '\n'.join(bad)


def test_kernel_refuses_bad_arguments():
    from simclr_amd import ops
    from simclr_amd._lib import SimclrHipError, lib
    L = lib()
    f = ctypes.c_float
    z = torch.zeros(8, 64, device=DEV)
    out, rs, ws = ops.hcl_fwd(z, z, 0, 0.1, 0.5, 0.1)
    torch.cuda.synchronize()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    good = dict(zl=p(z), za=p(z), n=4, N=4, D=64, rank=0, T=0.1, beta=0.5, tau=0.1, out=p(out), rs=p(rs), ws=p(ws))

    def fwd(**kw):
        a = dict(good, **kw)
        return L.hcl_fwd(a['zl'], a['za'], a['n'], a['N'], a['D'], a['rank'], f(a['T']), f(a['beta']), f(a['tau']), a['out'], a['rs'], a['ws'], None)

    def bwd(**kw):
        a = dict(good, dl=p(z), da=p(z))
        a.update(kw)
        return L.hcl_bwd(a['zl'], a['za'], a['n'], a['N'], a['D'], a['rank'], f(a['T']), f(a['beta']), f(a['tau']), a['rs'], f(1.0), a['dl'],
                         a['da'], a['ws'], None)
    odd = ctypes.c_void_p(z.data_ptr() + 4)
    nan, inf = float('nan'), float('inf')
    for call in (fwd, bwd):
        for kw, match in ((dict(D=100), 'D must be 64/128/256'), (dict(D=512), 'D must be 64/128/256'), (dict(n=0), 'n >= 1'),
                          (dict(n=1, N=1), 'N >= 2'), (dict(n=4, N=6), 'N = R\\*n'), (dict(rank=1), 'rank 1 out of range'),
                          (dict(rank=-1), 'rank -1 out of range'), (dict(T=0.0), 'temperature'), (dict(T=-1.0), 'temperature'),
                          (dict(T=nan), 'temperature'), (dict(T=inf), 'temperature'), (dict(beta=-0.5), 'beta'), (dict(beta=nan), 'beta'),
                          (dict(beta=inf), 'beta'), (dict(tau=-0.1), 'tau_plus'), (dict(tau=1.0), 'tau_plus'), (dict(tau=nan), 'tau_plus'),
                          (dict(zl=None), 'null or misaligned'), (dict(za=odd), 'null or misaligned'), (dict(rs=None), 'null or misaligned'),
                          (dict(ws=odd), 'null or misaligned')):
            with pytest.raises(SimclrHipError, match=match):
                call(**kw)
    with pytest.raises(SimclrHipError, match='null or misaligned'):
        fwd(out=None)
    with pytest.raises(SimclrHipError, match='null or misaligned'):
        bwd(dl=None)
    with pytest.raises(SimclrHipError, match='null or misaligned'):
        bwd(da=odd)
    assert L.hcl_workspace_bytes(4, 4, 100) == 0 and L.hcl_workspace_bytes(0, 4, 64) == 0 and L.hcl_workspace_bytes(1, 1, 64) == 0
    assert L.hcl_workspace_bytes(4, 6, 64) == 0 and L.hcl_workspace_bytes(4, 8, 64) > 0 and L.hcl_workspace_bytes(1, 2, 256) > 0
    # nothing was launched by a refused call: the outputs of the good call are untouched
    o2, rs2, _ = ops.hcl_fwd(z, z, 0, 0.1, 0.5, 0.1)
    torch.cuda.synchronize()
    assert torch.equal(out[:2], o2[:2]) and torch.equal(rs, rs2)
    with pytest.raises(ValueError, match='64/128/256'):
        ops.hcl_fwd(torch.zeros(8, 96, device=DEV), torch.zeros(8, 96, device=DEV), 0, 0.1, 0.5, 0.1)
    with pytest.raises(ValueError, match='N = R\\*n >= 2'):
        ops.hcl_fwd(torch.zeros(2, 64, device=DEV), torch.zeros(2, 64, device=DEV), 0, 0.1, 0.5, 0.1)
    with pytest.raises(ValueError, match='beta must be'):
        ops.hcl_fwd(z, z, 0, 0.1, -1.0, 0.1)
    with pytest.raises(ValueError, match='tau_plus must lie'):
        ops.hcl_fwd(z, z, 0, 0.1, 0.5, 1.0)


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
    """Records what the step hands the loss (the projection outputs) and what it hands the projection head."""
    from simclr_amd import objective as obj_lib
    box = {}
    orig_loss, orig_backward = obj_lib.add_hard_negative_contrastive_loss, model.backward

    def loss_fn(hidden, *a, **kw):
        box['hidden'] = hidden.detach().clone()
        box['kw'] = dict(kw)
        res = orig_loss(hidden, *a, **kw)
        box['loss'] = res[0]
        return res

    def backward(d_proj, *a, **kw):
        box['d_proj'] = d_proj.detach().clone()
        return orig_backward(d_proj, *a, **kw)
    setattr_fn(obj_lib, 'add_hard_negative_contrastive_loss', loss_fn)
    setattr_fn(model, 'backward', backward)
    return box


def _np(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def _l2norm_bwd_f32(h, dz):
    """d/dh of z = h / |h| in float32 arithmetic, from float32 h and dz."""
    one = np.float32
    h, dz = np.asarray(h, one), np.asarray(dz, one)
    inv = (1.0 / np.sqrt((h.astype(np.float64) ** 2).sum(1, keepdims=True))).astype(one)
    z = (h * inv).astype(one)
    dot = (z * dz).sum(1, keepdims=True, dtype=one)
    return ((dz - z * dot).astype(one) * inv).astype(one)


def step_gate(hiddens, rank, T, beta, tau_plus):
    """The reference of a step on the captured projection outputs (hidden_norm: the handle normalises) and 4 x the emulation's error on
    them: the emulated kernels on the float32 normalised rows, chained through the normalisation in float32.  Asserts the kink margin."""
    T, beta, tau_plus = f32(T), f32(beta), f32(tau_plus)
    ref = hcl_reference(hiddens, T, beta, tau_plus, hidden_norm=True)
    near = ref_lib.kink_distance(ref)
    assert near >= KINK_MARGIN, 'a row %.3g from the floor: choose another seed for this case' % near
    zs = [ref_lib.l2_normalize(np.asarray(h, np.float64))[0].astype(np.float32) for h in hiddens]
    emu = hcl_emulated(zs, rank, T, beta, tau_plus)
    err = relative_errors(emu['loss'], _l2norm_bwd_f32(hiddens[rank], emu['grad']), ref, rank)
    return ref, {k: 4.0 * v for k, v in err.items()}


STEP_PARAMS = [(1.0, 0.0), (0.5, 0.1)]


@pytest.mark.parametrize('beta,tau_plus', STEP_PARAMS)
def test_step_hands_the_projection_head_the_reference_gradient(monkeypatch, beta, tau_plus):
    from simclr_amd import model as model_lib
    from simclr_amd.run import make_single_step
    FLAGS = _flags(hard_negative_beta=beta, debiased_tau_plus=tau_plus)
    _fresh_runtime()
    model = model_lib.Model(NCLS)
    box = _capture(monkeypatch.setattr, model)
    step = make_single_step(model, model_lib.build_optimizer(0.1), None)
    assert sorted(step.metrics) == sorted(['train/contrast_acc', 'train/contrast_entropy', 'train/contrast_floor_share', 'train/contrast_loss',
                                           'train/supervised_acc', 'train/supervised_loss', 'train/total_loss', 'train/weight_decay'])
    g = torch.Generator().manual_seed(31)
    images = structured_images(B, SIZE, 2, g).to(DEV)
    ids = torch.randint(0, NCLS, (B,), generator=g)
    out = step(images, {'labels': F.one_hot(ids, NCLS).float().to(DEV)})
    torch.cuda.synchronize()
    assert tuple(box['hidden'].shape) == (2 * B, FLAGS.proj_out_dim)
    assert (box['kw']['beta'], box['kw']['tau_plus'], box['kw']['temperature']) == (beta, tau_plus, FLAGS.temperature)
    ref, tol = step_gate([_np(box['hidden'])], 0, FLAGS.temperature, beta, tau_plus)
    con, bad = out['con_loss'], []
    err = relative_errors(float(con.value), _np(box['d_proj']), ref, 0)
    print('step: floor share %r (ref %r), kink distance %.3g' % (float(con.floor_share), ref['floor_share'][0], ref_lib.kink_distance(ref)))
    _check('step_loss beta=%g tau_plus=%g' % (beta, tau_plus), err['loss'], tol['loss'], bad)
    _check('step_d_proj beta=%g tau_plus=%g' % (beta, tau_plus), err['grad'], tol['grad'], bad)
    assert not bad, '\n'.join(bad)
    assert float(con.floor_share) == float(np.float32(ref['floor_share'][0]))
    m = step.metrics
    assert m['train/contrast_floor_share'].result() == float(np.float32(ref['floor_share'][0]))
    # the logits are NT-Xent's: the two metrics of the handle are those of add_contrastive_loss on the same projection outputs
    from simclr_amd import objective as obj_lib
    _, logits, _ = obj_lib.add_contrastive_loss(box['hidden'], True, FLAGS.temperature)
    assert m['train/contrast_acc'].result() == float(logits.contrast_acc) and 0.0 <= m['train/contrast_acc'].result() <= 1.0
    assert m['train/contrast_entropy'].result() == float(logits.contrast_entropy)
    assert float(out['logits_con'].contrast_acc) == float(logits.contrast_acc)
    assert tuple(out['logits_con'].shape) == (B, B)
    assert all(bool(torch.isfinite(v.value).all()) for v in model.variables)


_RUN_ARGS = ['--dataset=synthetic', '--resnet_depth=18', '--image_size=32', '--train_batch_size=8', '--use_blur=False', '--compute_dtype=f32',
             '--checkpoint_steps=2', '--train_steps=3', '--mode=train']


def test_run_main_trains_logs_and_resumes_bitwise(tmp_path, capsys):
    from simclr_amd import run
    from simclr_amd.checkpoint import INDEX_NAME
    from simclr_amd.flags import FLAGS
    args = _RUN_ARGS + ['--hard_negative_beta=0.5', '--debiased_tau_plus=0.1']
    full_dir, again_dir = str(tmp_path / 'full'), str(tmp_path / 'again')
    FLAGS.reset()
    run.main(args + ['--model_dir=' + full_dir])
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith('{') and 'train/contrast_floor_share' in l]
    assert lines and lines[0]['step'] == 2
    for k in ('train/contrast_loss', 'train/contrast_acc', 'train/contrast_entropy', 'train/contrast_floor_share', 'train/total_loss'):
        assert math.isfinite(lines[0][k]), (k, lines[0])
    assert 0.0 <= lines[0]['train/contrast_floor_share'] <= 1.0 and 0.0 <= lines[0]['train/contrast_acc'] <= 1.0
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


def test_zero_flags_train_what_no_flags_train(tmp_path, capsys):
    """--hard_negative_beta=0 --debiased_tau_plus=0 is the run without the two flags: bitwise in the logged loss and in every weight."""
    from simclr_amd import run
    from simclr_amd.flags import FLAGS
    results = []
    for name, extra in (('plain', []), ('zeros', ['--hard_negative_beta=0', '--debiased_tau_plus=0.0'])):
        FLAGS.reset()
        d = str(tmp_path / name)
        run.main(_RUN_ARGS + extra + ['--model_dir=' + d])
        lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith('{') and 'train/contrast_loss' in l]
        assert lines and all('train/contrast_floor_share' not in l for l in lines)
        results.append((lines, torch.load(os.path.join(d, 'ckpt-3.pt'), map_location='cpu')))
    (la, ca), (lb, cb) = results
    assert [(l['step'], l['train/contrast_loss'], l['train/total_loss']) for l in la] == \
           [(l['step'], l['train/contrast_loss'], l['train/total_loss']) for l in lb]
    assert sorted(ca['model']) == sorted(cb['model']) and all(torch.equal(ca['model'][n], cb['model'][n]) for n in ca['model'])


# ---------------------------------------------------------------------------------------------------------------- two replicas
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


GLOO_PARAMS = (0.5, 0.1)


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
        FLAGS = _flags(hard_negative_beta=GLOO_PARAMS[0], debiased_tau_plus=GLOO_PARAMS[1])
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
        out = step(images[rank * B:(rank + 1) * B].to(DEV), {'labels': ids[rank * B:(rank + 1) * B].to(DEV)})
        torch.cuda.synchronize()
        res = dict(hidden=_np(box['hidden']), d_proj=_np(box['d_proj']), loss=float(out['con_loss'].value),
                   floor_share=float(out['con_loss'].floor_share))
        for o, name, v in attrs.values():
            setattr(o, name, v)
        dist.destroy_process_group()
        q.put((rank, 'ok', res))
    except Exception:  # noqa
        import traceback
        q.put((rank, 'FAIL', traceback.format_exc()))


def test_two_replica_step_vs_the_global_batch_restatement():
    """Two gloo ranks sharing one GPU: the gradient each rank's step hands its projection head equals the gradient of the single-process
    objective (1 / R) sum_r loss_r on the global batch of both ranks' projection outputs."""
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
    bad = []
    for r, b in enumerate(boxes):
        ref, tol = step_gate([x['hidden'] for x in boxes], r, FLAGS.temperature, *GLOO_PARAMS)
        err = relative_errors(b['loss'], b['d_proj'], ref, r)
        _check('two_replica_loss rank %d' % r, err['loss'], tol['loss'], bad)
        _check('two_replica_d_proj rank %d' % r, err['grad'], tol['grad'], bad)
        assert b['floor_share'] == float(np.float32(ref['floor_share'][r]))
    assert not bad, '\n'.join(bad)
