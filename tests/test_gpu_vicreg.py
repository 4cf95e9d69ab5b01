"""The VICReg loss on the device (pytest -m gpu): the split-k Gram kernels of csrc/vicreg.hip through the C ABI and simclr_amd.ops against
the float64 restatement tests/vicreg_reference.py, then the handle inside the step, run.main end to end (metrics, resume, eval, k-NN,
fine-tune) and two replicas over gloo.

Gates: 4 x the error of the float32 emulation of each quantity against float64 (tests/vicreg_reference.py: TOL per case, CENTER_TOL,
WHITENED_TOL; recorded in tests/golden/VICREG_HAND_DERIVED.md and re-measured by tests/test_vicreg_reference.py), cov relative to its
minuend and the gradient relative to the case's largest entry; the stored Gram blocks bitwise on integer data.  Where a check runs at a
shape outside that table (the handle, the step, the replicas) it takes the widest row of the table."""
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

from tests import vicreg_reference as vr
from tests.gpu_checks import DEV, structured_images
from tests.vicreg_reference import h_all_of, vicreg_gram

pytestmark = pytest.mark.gpu
B, SIZE, NCLS = 16, 32, 4
# the widest recorded budget of every quantity: for shapes between the rows of the table
WIDEST = {k: max(e[k] for e in vr.TOL.values()) for k in ('loss', 'inv', 'var', 'cov', 'grad')}


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


def _check(tag, errors, tols):
    """errors, tols: dicts name -> figure.  Prints every figure, then asserts."""
    bad = []
    for k in tols:
        ok = errors[k] <= tols[k] and math.isfinite(errors[k])
        print('%-4s %-70s err=%.3e tol=%.3e' % ('ok' if ok else 'FAIL', '%s %s' % (k, tag), errors[k], tols[k]))
        if not ok:
            bad.append('%s %s err=%.3e tol=%.3e' % (k, tag, errors[k], tols[k]))
    assert not bad, '\n'.join(bad)


# ---------------------------------------------------------------------------------------------------------------- centre
@pytest.mark.parametrize('N,D', vr.CENTER_SHAPES)
def test_center_vs_float64(N, D):
    from simclr_amd import ops
    h = vr.center_case(N, D, 0)
    xc, stats = ops.vicreg_center(torch.from_numpy(h).to(DEV))
    torch.cuda.synchronize()
    assert tuple(stats.shape) == (2, 2, D) and stats.dtype == torch.float64
    _check('N=%d D=%d' % (N, D), vr.center_errors(_np(xc), _np(stats), h), vr.CENTER_TOL[(N, D)])


# ---------------------------------------------------------------------------------------------------------------- loss and gradient
def _device(hs, n, coeffs, rank, eps=1e-4, gamma=1.0):
    """The device path of replica `rank` on one device: the gathered block is centred once, the replica runs its forward and its
    backward with grad_scale = 1 / R.  Returns dict(loss, inv, var, cov, grad = dL/dh_rank [2n, D], xc_all, stats, ws)."""
    from simclr_amd import ops
    R = len(hs)
    h_all = torch.from_numpy(h_all_of(hs, n)).to(DEV)
    xc_all, stats = ops.vicreg_center(h_all, eps)
    out, ws = ops.vicreg_fwd(h_all, xc_all, stats, n, rank, *coeffs, gamma=gamma)
    dh = ops.vicreg_bwd(h_all, xc_all, stats, n, rank, *coeffs, gamma, 1.0 / R, ws)
    torch.cuda.synchronize()
    o = out[:4].cpu().double()
    return dict(loss=float(o[0]), inv=float(o[1]), var=float(o[2]), cov=float(o[3]), grad=_np(dh), xc_all=xc_all, stats=stats, ws=ws)


@pytest.mark.parametrize('coeffs', vr.COEFF_SETS)
@pytest.mark.parametrize('n,N,D,rank', vr.MAIN_SHAPES)
def test_kernel_vs_float64(n, N, D, rank, coeffs):
    hs = vr.case_views(n, N // n, D, 0)
    ref = vicreg_gram(hs, *coeffs)
    std = ref['stats'][:, 1]
    assert (std < 1.0).any() and (std >= 1.0).any()                  # columns on each side of the hinge
    got = _device(hs, n, coeffs, rank)
    _check('n=%d N=%d D=%d rank=%d coeffs=%s' % (n, N, D, rank, coeffs), vr.relative_errors(got, ref, rank, coeffs), vr.TOL[(n, N, D, rank)])


def test_shapes_cover_every_split_path():
    from simclr_amd import ops
    splits = {s[:3]: ops.vicreg_k_splits(*s[:3]) for s in vr.MAIN_SHAPES}
    assert 1 in splits.values() and 2 in splits.values() and any(S >= 4 for S in splits.values())
    for (n, N, D), S in splits.items():
        assert S == vr.k_splits(n, N, D)[0]
    # a case whose last part is shorter than the others
    assert any(S > 1 and D % vr.k_splits(n, N, D)[1] != 0 for (n, N, D), S in splits.items())


@pytest.mark.parametrize('D', [64, 2048])
def test_exact_lattice_gram_blocks(D):
    """Integer rows in [-3, 3] in +/- pairs: every column mean is 0, xc is the input itself, every dot product is an integer of magnitude
    <= 9 D < 2^24, exact in fp32 in any summation order and under any split, so the stored (merged) blocks are bitwise the integer
    products -- at every tile edge (n = 70 and N = 140 fill no 64-tile) and for both rank offsets -- and cov is the float64 value to
    double rounding."""
    from simclr_amd import ops
    n, N = 70, 140
    g = np.random.default_rng(D)
    half = g.integers(-3, 4, size=(2, N // 2, D))
    z = np.concatenate([half[0], -half[0], half[1], -half[1]]).astype(np.float32)            # [2N, D]
    zi = z.astype(np.int64)
    if D == 2048:
        assert ops.vicreg_k_splits(n, N, D) > 1
    zd = torch.from_numpy(z).to(DEV)
    xc, stats = ops.vicreg_center(zd)
    assert torch.equal(xc, zd)
    var = [(zi[v * N:(v + 1) * N] ** 2).sum(0) / (N - 1.0) for v in range(2)]
    for rank in (0, 1):
        out, ws = ops.vicreg_fwd(zd, xc, stats, n, rank)
        gram = ops.vicreg_gram_blocks(ws, n, N, D)
        torch.cuda.synchronize()
        a = slice(rank * n, (rank + 1) * n)
        want = np.stack([zi[:N][a] @ zi[:N].T, zi[N:][a] @ zi[N:].T])
        assert tuple(gram.shape) == (2, n, N)
        assert np.array_equal(gram.cpu().numpy(), want.astype(np.float32)), 'rank %d' % rank
        minuend = sum(2.0 / (N - 1.0) ** 2 * float((want[v] ** 2).sum()) / D for v in range(2))
        cov = minuend - sum(float((var[v] ** 2).sum()) / D for v in range(2))
        got = float(out[3])
        # the kernel's double equals this one to a few ulps of the minuend; the output is then rounded to fp32
        assert abs(got - np.float32(cov)) <= abs(np.spacing(np.float32(cov))) and abs(got - cov) <= 2.0 ** -23 * abs(cov) + 1e-12 * minuend


def test_whitened_near_decorrelated_case():
    hs = vr.whitened_views()
    coeffs = vr.COEFF_SETS[0]
    ref = vicreg_gram(hs, *coeffs)
    assert ref['minuend'][0] >= 1000.0 * abs(ref['cov'][0])
    got = _device(hs, 256, coeffs, 0)
    print('cov: device %.3e float64 %.3e minuend %.3f' % (got['cov'], ref['cov'][0], ref['minuend'][0]))
    _check('whitened N=256 D=64', vr.relative_errors(got, ref, 0, coeffs), vr.WHITENED_TOL)


def test_kernel_is_bitwise_repeatable():
    from simclr_amd import ops
    for n, N, D in [(48, 96, 192), (33, 99, 320), (16, 16, 2048)]:           # S = 1, 2, 16
        h = (torch.randn(2 * N, D, generator=torch.Generator().manual_seed(5)) * 3.0 + 1.0).to(DEV)
        runs = []
        for _ in range(2):
            xc, stats = ops.vicreg_center(h)
            out, ws = ops.vicreg_fwd(h, xc, stats, n, 1 if N > n else 0, 25.0, 25.0, 1.0)
            gram = ops.vicreg_gram_blocks(ws, n, N, D).clone()
            dh = ops.vicreg_bwd(h, xc, stats, n, 1 if N > n else 0, 25.0, 25.0, 1.0, 1.0, 0.5, ws)
            torch.cuda.synchronize()
            runs.append((xc, stats, out[:4].clone(), gram, dh))
        for a, b in zip(*runs):
            assert torch.equal(a, b)


def test_kernel_refuses_bad_arguments():
    """Every refusal returns an error code before anything is launched (the pointers of these calls are null or misaligned: a launch
    would fault)."""
    from simclr_amd import ops
    from simclr_amd._lib import SimclrHipError, lib
    L = lib()
    f = ctypes.c_float
    ok = torch.zeros(8, 64, device=DEV)
    st = torch.zeros(2, 2, 64, device=DEV, dtype=torch.float64)
    ws = ops.vicreg_workspace(4, 4, 64, DEV)
    out = torch.zeros(4, device=DEV)
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)

    def fwd(h=P(ok), xc=P(ok), stats=P(st), n=4, N=4, D=64, rank=0, c=(25.0, 25.0, 1.0), o=P(out), w=P(ws)):
        return L.vicreg_fwd(h, xc, stats, n, N, D, rank, f(c[0]), f(c[1]), f(c[2]), f(1.0), o, w, None)

    def bwd(h=P(ok), xc=P(ok), stats=P(st), n=4, N=4, D=64, rank=0, c=(25.0, 25.0, 1.0), w=P(ws), dh=P(ok)):
        return L.vicreg_bwd(h, xc, stats, n, N, D, rank, f(c[0]), f(c[1]), f(c[2]), f(1.0), f(1.0), w, dh, None)

    for D in (100, 8256, 32):
        assert L.vicreg_workspace_bytes(4, 4, D) == 0 and L.vicreg_gram_pitch(4, 4, D) == 0 and L.vicreg_k_splits(4, 4, D) == 0
        with pytest.raises(SimclrHipError, match='multiple of 64 in \\[64, 8192\\]'):
            L.vicreg_center(P(ok), 4, D, f(1e-4), P(ok), P(st), None)
        with pytest.raises(SimclrHipError, match='multiple of 64 in \\[64, 8192\\]'):
            fwd(D=D)
        with pytest.raises(SimclrHipError, match='multiple of 64 in \\[64, 8192\\]'):
            bwd(D=D)
    assert L.vicreg_workspace_bytes(4, 6, 64) == 0 and L.vicreg_workspace_bytes(0, 4, 64) == 0 and L.vicreg_workspace_bytes(1, 1, 64) == 0
    assert L.vicreg_workspace_bytes(4, 8, 64) > 0 and L.vicreg_workspace_bytes(1, 2, 64) > 0
    with pytest.raises(SimclrHipError, match='N >= 2'):
        L.vicreg_center(P(ok), 1, 64, f(1e-4), P(ok), P(st), None)
    with pytest.raises(SimclrHipError, match='eps must be >= 0'):
        L.vicreg_center(P(ok), 4, 64, f(-1e-4), P(ok), P(st), None)
    for call in (fwd, bwd):
        for kw in (dict(n=4, N=6), dict(n=0, N=4), dict(n=1, N=1), dict(n=8, N=4)):
            with pytest.raises(SimclrHipError, match='N = R\\*n'):
                call(**kw)
        with pytest.raises(SimclrHipError, match='rank 2 out of range'):
            call(n=4, N=8, rank=2)
        with pytest.raises(SimclrHipError, match='rank -1 out of range'):
            call(rank=-1)
        for c in ((-1.0, 25.0, 1.0), (25.0, float('inf'), 1.0), (25.0, 25.0, float('nan'))):
            with pytest.raises(SimclrHipError, match='finite and >= 0'):
                call(c=c)
        for kw in (dict(h=None), dict(xc=None), dict(stats=None), dict(w=None)):
            with pytest.raises(SimclrHipError, match='null argument'):
                call(**kw)
        for kw in (dict(h=P(ok, 4)), dict(xc=P(ok, 4)), dict(stats=P(st, 8)), dict(w=P(ws, 8))):
            with pytest.raises(SimclrHipError, match='16-byte aligned'):
                call(**kw)
    with pytest.raises(SimclrHipError, match='null argument'):
        fwd(o=None)
    with pytest.raises(SimclrHipError, match='null argument'):
        bwd(dh=None)
    with pytest.raises(SimclrHipError, match='16-byte aligned'):
        bwd(dh=P(ok, 4))
    with pytest.raises(SimclrHipError, match='null argument'):
        L.vicreg_center(None, 4, 64, f(1e-4), P(ok), P(st), None)
    with pytest.raises(SimclrHipError, match='16-byte aligned'):
        L.vicreg_center(P(ok, 4), 4, 64, f(1e-4), P(ok), P(st), None)
    torch.cuda.synchronize()
    # nothing was launched: the buffers a launch would have written are untouched
    assert float(out.abs().sum()) == 0.0 and float(ok.abs().sum()) == 0.0 and float(st.abs().sum()) == 0.0
    with pytest.raises(ValueError, match='multiples of 64'):
        ops.vicreg_center(torch.zeros(8, 100, device=DEV))
    with pytest.raises(ValueError, match='N = R\\*n'):
        ops.vicreg_fwd(torch.zeros(12, 64, device=DEV), torch.zeros(12, 64, device=DEV), st, 4, 0)


def test_two_replicas_on_one_device_equal_one_replica_on_the_whole_block():
    """rank 0 and rank 1 on the two halves of one gathered block: their loss values average to the one-replica loss on the whole block,
    and their gradients are its rows."""
    n, R, D, coeffs = 40, 2, 128, vr.COEFF_SETS[0]
    hs = vr.case_views(n, R, D, 7)
    N = n * R
    whole = [h_all_of(hs, n)]
    one = _device(whole, N, coeffs, 0)
    ref = vicreg_gram(whole, *coeffs)
    _check('whole block', vr.relative_errors(one, ref, 0, coeffs), WIDEST)
    parts = [_device(hs, n, coeffs, rank) for rank in range(R)]
    sc = vr.error_scales(ref, 0, *coeffs)
    errs = {}
    for k in ('loss', 'inv', 'cov'):
        errs[k] = abs(sum(p[k] for p in parts) / R - one[k]) / sc[k]
    errs['var'] = max(abs(p['var'] - one['var']) for p in parts) / sc['var']
    errs['grad'] = 0.0
    for rank, p in enumerate(parts):
        assert torch.equal(p['xc_all'], one['xc_all']) and torch.equal(p['stats'], one['stats'])
        rows = vr.replica_rows(rank, n, N)
        errs['grad'] = max(errs['grad'], float(np.abs(p['grad'].astype(np.float64) - one['grad'][rows]).max()) / sc['grad'])
    # two device results against each other: each within its gate of the float64 value
    _check('mean of two replicas vs the whole block', errs, {k: 2.0 * v for k, v in WIDEST.items()})


def test_objective_handle_matches_the_restatement():
    from simclr_amd import objective
    n, D, coeffs = 24, 192, (2.0, 4.0, 0.5)
    hs = vr.case_views(n, 1, D, 9)
    loss = objective.add_vicreg_loss(torch.from_numpy(hs[0]).to(DEV), *coeffs, eps=1e-3, gamma=1.25)
    loss.backward_start(1.0)
    dh = loss.backward_finish()
    torch.cuda.synchronize()
    ref = vicreg_gram(hs, *coeffs, eps=1e-3, gamma=1.25)
    assert not hasattr(loss, 'temperature') and tuple(dh.shape) == (2 * n, D)
    got = dict(loss=float(loss.value), inv=float(loss.invariance), var=float(loss.variance), cov=float(loss.covariance), grad=_np(dh))
    _check('handle', vr.relative_errors(got, ref, 0, coeffs, gamma=1.25), WIDEST)
    xc_err = float(np.abs(_np(loss.centered).astype(np.float64) - ref['xc_all']).max() / np.abs(ref['xc_all']).max())
    _check('handle', dict(centered=xc_err), dict(centered=max(t['xc'] for t in vr.CENTER_TOL.values())))
    again = loss.backward(1.0)
    torch.cuda.synchronize()
    assert torch.equal(again, dh)


# ---------------------------------------------------------------------------------------------------------------- handle and step
def _flags(**kw):
    from simclr_amd.flags import FLAGS
    FLAGS.reset()
    kw.setdefault('proj_out_dim', 64)
    FLAGS.update(resnet_depth=18, image_size=SIZE, compute_dtype='f32', f32_matmul='exact', use_blur=False, train_batch_size=B,
                 train_mode='pretrain', contrastive_loss='vicreg', **kw)
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
    orig_loss, orig_backward = obj_lib.add_vicreg_loss, model.backward

    def loss_fn(hidden, *a, **kw):
        box['hidden'] = hidden.detach().clone()
        box['kw'] = {k: v for k, v in kw.items() if k in ('sim_coeff', 'std_coeff', 'cov_coeff')}
        box['loss'] = orig_loss(hidden, *a, **kw)
        return box['loss']

    def backward(d_proj, *a, **kw):
        box['d_proj'] = d_proj.detach().clone()
        return orig_backward(d_proj, *a, **kw)
    setattr_fn(obj_lib, 'add_vicreg_loss', loss_fn)
    setattr_fn(model, 'backward', backward)
    return box


def _handle(con):
    return dict(loss=float(con.value), inv=float(con.invariance), var=float(con.variance), cov=float(con.covariance))


@pytest.mark.parametrize('head_mode,width', [('nonlinear', 64), ('none', 512)])
def test_step_hands_the_layer_below_the_reference_gradient(monkeypatch, head_mode, width):
    """One step with a projection head of width 64 and one with proj_head_mode=none (the loss reads ResNet-18's 512-wide output)."""
    from simclr_amd import model as model_lib
    from simclr_amd.run import make_single_step
    coeffs = (10.0, 5.0, 2.0)
    _flags(proj_head_mode=head_mode, vicreg_sim_coeff=coeffs[0], vicreg_std_coeff=coeffs[1], vicreg_cov_coeff=coeffs[2])
    _fresh_runtime()
    model = model_lib.Model(NCLS)
    box = _capture(monkeypatch.setattr, model)
    step = make_single_step(model, model_lib.build_optimizer(0.1), None)
    assert sorted(step.metrics) == ['train/contrast_loss', 'train/supervised_acc', 'train/supervised_loss', 'train/total_loss',
                                    'train/vicreg_cov', 'train/vicreg_inv', 'train/vicreg_var', 'train/weight_decay']
    g = torch.Generator().manual_seed(31)
    images = structured_images(B, SIZE, 2, g).to(DEV)
    ids = torch.randint(0, NCLS, (B,), generator=g)
    out = step(images, {'labels': torch.nn.functional.one_hot(ids, NCLS).float().to(DEV)})
    torch.cuda.synchronize()
    assert tuple(box['hidden'].shape) == (2 * B, width) and out['logits_con'] is None
    assert box['kw'] == dict(sim_coeff=coeffs[0], std_coeff=coeffs[1], cov_coeff=coeffs[2])
    ref = vicreg_gram([_np(box['hidden'])], *coeffs)
    con = out['con_loss']
    got = dict(_handle(con), grad=_np(box['d_proj']))
    _check('step %s' % head_mode, vr.relative_errors(got, ref, 0, coeffs), WIDEST)
    m = step.metrics
    assert m['train/vicreg_inv'].result() == float(con.invariance) and m['train/vicreg_var'].result() == float(con.variance)
    assert m['train/vicreg_cov'].result() == float(con.covariance) and m['train/contrast_loss'].result() == float(con.value)
    assert all(bool(torch.isfinite(v.value).all()) for v in model.variables)


def test_run_main_trains_logs_resumes_bitwise_and_feeds_eval_knn_and_finetune(tmp_path, capsys):
    from simclr_amd import run
    from simclr_amd.checkpoint import INDEX_NAME
    from simclr_amd.flags import FLAGS
    common = ['--dataset=synthetic', '--resnet_depth=18', '--image_size=32', '--train_batch_size=8', '--use_blur=False', '--compute_dtype=f32',
              '--contrastive_loss=vicreg', '--proj_out_dim=64']
    args = common + ['--checkpoint_steps=2', '--train_steps=3', '--mode=train']
    full_dir, again_dir = str(tmp_path / 'full'), str(tmp_path / 'again')
    FLAGS.reset()
    run.main(args + ['--model_dir=' + full_dir])
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith('{') and 'train/vicreg_inv' in l]
    assert lines and lines[0]['step'] == 2
    for k in ('train/contrast_loss', 'train/vicreg_inv', 'train/vicreg_var', 'train/vicreg_cov', 'train/total_loss'):
        assert math.isfinite(lines[0][k]), (k, lines[0])
    assert 'train/contrast_entropy' not in lines[0] and 'train/contrast_acc' not in lines[0] and 'train/bt_on_diag' not in lines[0]
    assert lines[0]['train/vicreg_inv'] >= 0.0 and 0.0 <= lines[0]['train/vicreg_var'] <= 1.0
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
    # the checkpoint carries no extra state: the same variables as a plain NT-Xent run of the same model
    assert not any('vicreg' in n for n in full['model'])
    capsys.readouterr()
    # evaluation, k-NN evaluation and fine-tuning read the checkpoint; the loss flags are ignored there
    FLAGS.reset()
    result = run.main(['--dataset=synthetic', '--resnet_depth=18', '--image_size=32', '--eval_batch_size=8', '--eval_steps=1',
                       '--compute_dtype=f32', '--mode=eval', '--contrastive_loss=vicreg', '--proj_out_dim=64', '--model_dir=' + full_dir])
    assert result['global_step'] == 3 and 0.0 <= result['eval/label_top_1_accuracy'] <= 1.0, result
    FLAGS.reset()
    result = run.main(['--dataset=synthetic', '--resnet_depth=18', '--image_size=32', '--eval_batch_size=8', '--eval_steps=1',
                       '--compute_dtype=f32', '--mode=eval', '--contrastive_loss=vicreg', '--proj_out_dim=64', '--knn_eval=True',
                       '--knn_k=5', '--model_dir=' + full_dir])
    assert result['global_step'] == 3
    for k in ('eval/label_top_1_accuracy', 'eval/knn_top_1_accuracy'):
        assert 0.0 <= result[k] <= 1.0, (k, result)
    # one fine-tuning step from the file
    ft_dir = str(tmp_path / 'ft')
    FLAGS.reset()
    run.main(['--dataset=synthetic', '--resnet_depth=18', '--image_size=32', '--train_batch_size=8', '--compute_dtype=f32', '--mode=train',
              '--train_mode=finetune', '--contrastive_loss=vicreg', '--proj_out_dim=64', '--train_steps=1', '--checkpoint_steps=1',
              '--checkpoint=' + os.path.join(full_dir, 'ckpt-3.pt'), '--model_dir=' + ft_dir])
    written = torch.load(os.path.join(ft_dir, 'ckpt-1.pt'), map_location='cpu')['model']
    enc = [n for n in written if n.startswith('model/resnet/')]
    assert len(enc) > 60 and all(n in full['model'] for n in enc)


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
        res = dict(_handle(out['con_loss']), hidden=_np(box['hidden']), d_proj=_np(box['d_proj']), weights=_weights(model))
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
    on the gathered batch within the project's gradient gate for two steps of different arithmetic order (2e-4, tests/test_gpu_barlow.py)."""
    import torch.multiprocessing as mp
    from simclr_amd import model as model_lib
    from simclr_amd.flags import FLAGS
    from simclr_amd.run import make_single_step
    from tests.gpu_checks import _res
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
    coeffs = (FLAGS.vicreg_sim_coeff, FLAGS.vicreg_std_coeff, FLAGS.vicreg_cov_coeff)
    ref = vicreg_gram([b['hidden'] for b in boxes], *coeffs)
    for r, b in enumerate(boxes):
        _check('two replicas, rank %d' % r, vr.relative_errors(dict(b, grad=b['d_proj']), ref, r, coeffs), WIDEST)
    # one replica, the gathered batch, the same initial weights (the initialisation is a function of the seed alone)
    FLAGS.update(train_batch_size=2 * B)
    _fresh_runtime()
    model = model_lib.Model(NCLS)
    step = make_single_step(model, model_lib.build_optimizer(0.1), None)
    images, ids = _batch(2)
    one = step(images.to(DEV), {'labels': ids.to(DEV)})
    torch.cuda.synchronize()
    after = _weights(model)
    GATE_GRAD = 2e-4
    out = [_res('two_replica_loss_mean vs one replica', 0.5 * (boxes[0]['loss'] + boxes[1]['loss']), float(one['con_loss'].value), GATE_GRAD)]
    for name in sorted(after):
        for r, b in enumerate(boxes):
            out.append(_res('two_replica_weights rank %d %s' % (r, name), b['weights'][name], after[name], GATE_GRAD))
    bad = [r for r in out if not r['ok']]
    assert not bad, '\n'.join('%s err=%.3e tol=%.3e' % (r['name'], r['err'], r['tol']) for r in bad)
