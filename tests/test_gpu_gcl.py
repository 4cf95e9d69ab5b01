"""The generalized contrastive loss on the device (pytest -m gpu): the decoupled NT-Xent sweeps and the sliced-Wasserstein sort-and-match
kernel of csrc/gcl.hip through the C ABI and simclr_amd.ops against the float64 reference tests/gcl_reference.py, the composed SWD loss,
then the handle inside the step, run.main end to end (metrics, resume) and two replicas over gloo
(colabs/intriguing_properties/generalized_contrastive_loss.ipynb).

Gates: the project's NT-Xent gates (tests/gpu_checks.py::check_ntxent) -- the loss and its two terms 1e-5 relative, gradients 2e-4 of the
reference tensor's maximum; the arithmetic is the same exact fp32-input MFMA."""
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

from tests.gcl_reference import gcl_reference, l2_normalize
from tests.gpu_checks import DEV, _res, structured_images

pytestmark = pytest.mark.gpu
GATE_LOSS, GATE_GRAD = 1e-5, 2e-4
B, SIZE, NCLS = 16, 32, 10
LAM, LS = 0.75, 1.5               # lambda_weight / loss_scaling of the kernel-level checks: neither is 1, so a dropped factor shows


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


# ---------------------------------------------------------------------------------------------------------------- decoupled sweep
def _device_lse(hs, n, T, hidden_norm, rank, lam=LAM, ls=LS):
    """The device path of one replica, assembled over replicas the way gpu_checks.check_ntxent does it: total gradient wrt rank's
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
    dz_slot = torch.zeros(2 * n, D, device=DEV)
    out = dz_local = None
    for q in range(R):
        o_q, rs_q, ws_q = ops.gcl_lse_fwd(zs[q], z_all, T, lam, ls)
        dl, da = ops.gcl_lse_bwd(zs[q], z_all, T, rs_q, 1.0 / R, ws_q, lam, ls, rank=q, skip_self=hidden_norm)    # as the loss handle calls it
        if q == rank:
            out, dz_local = o_q[:3].clone(), dl
        dz_slot[:n] += da[rank * n:(rank + 1) * n]
        dz_slot[n:] += da[N + rank * n:N + (rank + 1) * n]
    dz = dz_local + dz_slot
    dh = ops.l2norm_bwd(zs[rank], invs[rank], dz) if hidden_norm else dz
    torch.cuda.synchronize()
    return out.cpu().double(), dh


def check_lse(n, R, D, T, hidden_norm, rank, seed=3, row_scale=None):
    g = np.random.default_rng(seed + n)
    hs = [g.standard_normal((2 * n, D)).astype(np.float32) for _ in range(R)]
    if row_scale is not None:       # rows of length row_scale
        hs = [(l2_normalize(h.astype(np.float64))[0] * row_scale).astype(np.float32) for h in hs]
    ref = gcl_reference(hs, LAM, T, 'logsumexp', hidden_norm, LS)
    o, dh = _device_lse(hs, n, T, hidden_norm, rank)
    tag = 'n=%d R=%d D=%d T=%g norm=%d rank=%d%s' % (n, R, D, T, hidden_norm, rank, '' if row_scale is None else ' |row|=%g' % row_scale)
    return [_res('gcl_lse_loss ' + tag, o[0], ref['loss'][rank], GATE_LOSS),
            _res('gcl_lse_align ' + tag, o[1], ref['align'][rank], GATE_LOSS),
            _res('gcl_lse_dist ' + tag, o[2], ref['dist'][rank], GATE_LOSS),
            _res('gcl_lse_grad ' + tag, dh, ref['grads'][rank], GATE_GRAD)]


LSE_SHAPES = [(8, 1, 64, 0), (24, 1, 128, 0), (64, 2, 128, 0), (64, 2, 128, 1), (96, 2, 256, 0), (256, 1, 128, 0)]


@pytest.mark.parametrize('hidden_norm', [True, False])
@pytest.mark.parametrize('T', [0.1, 1.0])
@pytest.mark.parametrize('n,R,D,rank', LSE_SHAPES)
def test_decoupled_kernel_vs_float64(n, R, D, rank, T, hidden_norm):
    _assert(check_lse(n, R, D, T, hidden_norm, rank))


def test_decoupled_kernel_closed_forms():
    """n = 8, D = 64, T = 0.1.  All rows identical: align 0, dist = 1/T + log(2N/D).  hidden1 = hidden2 = eye(n, D): align 0,
    dist = log(2 e^(1/T) + 2N - 2) - log D.  Both pin the unmasked self column and the log of the hidden width."""
    n, D, T = 8, 64, 0.1
    res = []
    for name, h, closed in (('identical', np.ones((2 * n, D), np.float32), 1 / T + math.log(2 * n / D)),
                            ('eye', np.concatenate([np.eye(n, D), np.eye(n, D)]).astype(np.float32),
                             math.log(2 * math.exp(1 / T) + 2 * n - 2) - math.log(D))):
        o, _ = _device_lse([h], n, T, True, 0, lam=1.0, ls=1.0)
        res += [_res('gcl_closed_%s_align' % name, o[1], 0.0, 0, 0), _res('gcl_closed_%s_dist' % name, o[2], closed, GATE_LOSS),
                _res('gcl_closed_%s_loss' % name, o[0], closed, GATE_LOSS)]
    assert abs((1 / T + math.log(2 * n / D)) - 8.6137056) < 1e-6
    _assert(res)


@pytest.mark.parametrize('n,R,D', [(24, 1, 128), (64, 2, 64)])
def test_decoupled_kernel_unbounded_logits(n, R, D):
    """hidden_norm=False with rows of length 30 at T = 0.1: S / T reaches 9000 -- exp() of it overflows fp32 unless the running row
    maximum is subtracted."""
    res = check_lse(n, R, D, 0.1, False, R - 1, row_scale=30.0)
    assert all(math.isfinite(r['err']) for r in res)
    _assert(res)


def test_decoupled_kernel_is_bitwise_deterministic():
    from simclr_amd import ops
    g = torch.Generator().manual_seed(5)
    n, N, D = 96, 192, 128
    z = F.normalize(torch.randn(2 * n, D, generator=g)).to(DEV)
    z_all = torch.cat([z[:n], F.normalize(torch.randn(n, D, generator=g)).to(DEV), z[n:],
                       F.normalize(torch.randn(n, D, generator=g)).to(DEV)], 0).contiguous()
    runs = []
    for _ in range(2):
        out, rs, ws = ops.gcl_lse_fwd(z, z_all, 0.1, LAM, LS)
        dl, da = ops.gcl_lse_bwd(z, z_all, 0.1, rs, 0.5, ws, LAM, LS, rank=0, skip_self=True)
        torch.cuda.synchronize()
        runs.append((out.clone(), rs.clone(), dl, da))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_decoupled_kernel_refuses_bad_arguments():
    from simclr_amd import ops
    from simclr_amd._lib import SimclrHipError, lib
    L = lib()
    f = ctypes.c_float
    with pytest.raises(SimclrHipError, match='D must be 64/128/256'):
        L.gcl_lse_fwd(None, None, 4, 4, 100, f(0.1), f(1.0), f(1.0), None, None, None, None)
    with pytest.raises(SimclrHipError, match='D must be 64/128/256'):
        L.gcl_lse_bwd(None, None, 4, 4, 512, f(0.1), f(1.0), f(1.0), 0, 0, None, f(1.0), None, None, None, None)
    with pytest.raises(SimclrHipError, match='null argument'):
        L.gcl_lse_fwd(None, None, 4, 4, 128, f(0.1), f(1.0), f(1.0), None, None, None, None)
    with pytest.raises(SimclrHipError, match='null argument'):
        L.gcl_lse_bwd(None, None, 4, 4, 128, f(0.1), f(1.0), f(1.0), 0, 0, None, f(1.0), None, None, None, None)
    with pytest.raises(SimclrHipError, match='N = R\\*n'):
        L.gcl_lse_fwd(None, None, 4, 6, 128, f(0.1), f(1.0), f(1.0), None, None, None, None)
    assert L.gcl_lse_workspace_bytes(4, 4, 100) == 0 and L.gcl_lse_workspace_bytes(4, 8, 64) > 0
    z = torch.zeros(8, 96, device=DEV)
    with pytest.raises(ValueError, match='64/128/256'):
        ops.gcl_lse_fwd(z, z, 0.1)


# ---------------------------------------------------------------------------------------------------------------- sort kernel
SORT_KINDS = ['normal', 'sorted', 'descending', 'all_equal', 'lattice', 'signed_zero']


def _sort_keys(kind, D, M, g):
    x = g.standard_normal((D, M)).astype(np.float32)
    if kind == 'sorted':
        x = np.sort(x, axis=1)
    elif kind == 'descending':
        x = -np.sort(-x, axis=1)
    elif kind == 'all_equal':
        x[:] = g.standard_normal((D, 1)).astype(np.float32)
    elif kind == 'lattice':
        x = g.integers(-3, 4, size=(D, M)).astype(np.float32)
    elif kind == 'signed_zero':
        x = np.where(g.random((D, M)) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
        x[:, ::5] = g.integers(-1, 2, size=x[:, ::5].shape).astype(np.float32)
    return np.ascontiguousarray(x)


@pytest.mark.parametrize('kind', SORT_KINDS)
@pytest.mark.parametrize('D', [3, 128])
@pytest.mark.parametrize('M', [2, 16, 200, 1000, 2048, 8192])
def test_sort_kernel_vs_stable_argsort(M, D, kind):
    from simclr_amd import ops
    g = np.random.default_rng(M * 7 + D)
    Pt = _sort_keys(kind, D, M, g)
    Qt = _sort_keys('lattice' if kind == 'lattice' else 'normal', D, M, g)
    coeff = 2.0 / (D * M)
    dP, col_loss, perm = ops.swd_sort_match(torch.from_numpy(Pt).to(DEV), torch.from_numpy(Qt).to(DEV), coeff, want_perm=True)
    torch.cuda.synchronize()
    perm = perm.cpu().numpy()
    want = np.argsort(Pt, axis=1, kind='stable')
    assert perm.dtype == np.int32 and np.array_equal(perm, want), 'perm differs from numpy.argsort(kind="stable") in %d places' % int((perm != want).sum())
    assert np.array_equal(np.sort(perm, axis=1), np.broadcast_to(np.arange(M), (D, M)))          # every row index once per column
    Ps = np.take_along_axis(Pt.astype(np.float64), want, axis=1)
    Qs = np.sort(Qt.astype(np.float64), axis=1)
    dP_ref = np.zeros((M, D))
    np.put_along_axis(dP_ref, want.T, (coeff * (Ps - Qs)).T, axis=0)
    tag = 'M=%d D=%d %s' % (M, D, kind)
    _assert([_res('swd_dP ' + tag, dP, dP_ref, GATE_GRAD),
             _res('swd_col_loss ' + tag, col_loss, ((Qs - Ps) ** 2).sum(axis=1), GATE_LOSS),
             _res('swd_total ' + tag, col_loss.double().sum(), ((Qs - Ps) ** 2).sum(), GATE_LOSS)])


def test_sort_kernel_without_perm_and_refusals():
    from simclr_amd import ops
    from simclr_amd._lib import SimclrHipError, lib
    g = np.random.default_rng(0)
    Pt, Qt = (torch.from_numpy(_sort_keys('normal', 5, 300, g)).to(DEV) for _ in range(2))
    a = ops.swd_sort_match(Pt, Qt, 0.5, want_perm=True)
    b = ops.swd_sort_match(Pt, Qt, 0.5, want_perm=False)
    torch.cuda.synchronize()
    assert b[2] is None and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(SimclrHipError, match='M must be 1..8192'):
        lib().swd_sort_match(None, None, 8193, 4, ctypes.c_float(1.0), None, None, None, None)
    with pytest.raises(SimclrHipError, match='null argument'):
        lib().swd_sort_match(None, None, 64, 4, ctypes.c_float(1.0), None, None, None, None)
    big = torch.zeros(2, 8193, device=DEV)
    with pytest.raises(ValueError, match='8192'):
        ops.swd_sort_match(big, big, 1.0)


@pytest.mark.parametrize('M,N,K', [(128, 200, 128), (200, 64, 64), (64, 8192, 128), (30, 50, 256)])
def test_projection_gemm_vs_float64(M, N, K):
    from simclr_amd import ops
    g = torch.Generator().manual_seed(M + N + K)
    A, Bm = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    C = ops.gcl_gemm_nt(A.to(DEV), Bm.to(DEV))
    torch.cuda.synchronize()
    # K exact fp32 products accumulated in fp32: K * 2^-24 relative to sum |a||b| <= sqrt(K) * K-term norms; 2e-5 of the maximum holds it
    _assert([_res('gcl_gemm_nt %dx%dx%d' % (M, N, K), C, A.double() @ Bm.double().T, 2e-5)])


# ---------------------------------------------------------------------------------------------------------------- composed SWD loss
def _orthogonal(D, g):
    q, r = torch.linalg.qr(torch.randn(D, D, generator=g, dtype=torch.float64))
    return (q * torch.sign(torch.diagonal(r))).float()


def _perm_sorts(P64, perm):
    """The device's permutation orders the float64 projections up to 1e-6 max|P| (keys a few ulps apart may swap on the device's fp32
    GEMM) and is a permutation of every column: a condition on the sort, not a tolerance on the result."""
    M = P64.shape[0]
    assert np.array_equal(np.sort(perm, axis=0), np.broadcast_to(np.arange(M)[:, None], perm.shape))
    Ps = np.take_along_axis(P64, perm, axis=0)
    return float(np.diff(Ps, axis=0).min()) >= -1e-6 * float(np.abs(P64).max()) if M > 1 else True


@pytest.mark.parametrize('hidden_norm', [True, False])
@pytest.mark.parametrize('dist', ['normal', 'uniform'])
@pytest.mark.parametrize('D', [64, 128])
@pytest.mark.parametrize('n', [8, 100, 256])
def test_composed_swd_loss_vs_float64(n, D, dist, hidden_norm):
    from simclr_amd import objective
    g = torch.Generator().manual_seed(n + D)
    h = torch.randn(2 * n, D, generator=g)
    W = _orthogonal(D, g)
    prior = torch.randn(2 * n, D, generator=g) if dist == 'normal' else torch.rand(2 * n, D, generator=g) * 2 - 1
    loss = objective.generalized_contrastive_loss(h[:n].to(DEV), h[n:].to(DEV), LAM, 1.0, dist, hidden_norm, LS,
                                                  rand_w=W.to(DEV), prior=prior.to(DEV))
    dh = loss.backward(1.0)
    torch.cuda.synchronize()
    perm = loss.perm.cpu().numpy().T.astype(np.int64)                  # [M, D]
    free = gcl_reference([h.numpy()], LAM, 1.0, dist, hidden_norm, LS, W.numpy(), prior.numpy())
    assert _perm_sorts(free['P'], perm), 'the device permutation does not sort the float64 projections'
    ref = gcl_reference([h.numpy()], LAM, 1.0, dist, hidden_norm, LS, W.numpy(), prior.numpy(), perm=perm)
    tag = 'n=%d D=%d %s norm=%d' % (n, D, dist, hidden_norm)
    _assert([_res('gcl_swd_loss ' + tag, loss.value, ref['loss'][0], GATE_LOSS),
             _res('gcl_swd_align ' + tag, loss.align, ref['align'][0], GATE_LOSS),
             _res('gcl_swd_dist ' + tag, loss.dist_match, ref['dist'][0], GATE_LOSS),
             _res('gcl_swd_grad ' + tag, dh, ref['grads'][0], GATE_GRAD)])


def test_handle_unknown_prior_and_given_draws():
    from simclr_amd import objective
    h = torch.randn(16, 64, generator=torch.Generator().manual_seed(0)).to(DEV)
    with pytest.raises(ValueError, match='Unknown prior cauchy'):
        objective.generalized_contrastive_loss(h[:8], h[8:], dist='cauchy')
    a = objective.generalized_contrastive_loss(h[:8], h[8:])                       # the notebook's defaults: dist='normal'
    objective.set_gcl_step(1)
    b = objective.generalized_contrastive_loss(h[:8], h[8:])
    objective.set_gcl_step(0)
    c = objective.generalized_contrastive_loss(h[:8], h[8:])
    assert float(a.value) == float(c.value) != float(b.value) and torch.equal(a.backward(), c.backward())
    assert float(a.align) == float(b.align)


# ---------------------------------------------------------------------------------------------------------------- handle and step
def _flags(dist, **kw):
    from simclr_amd.flags import FLAGS
    FLAGS.reset()
    FLAGS.update(resnet_depth=18, image_size=SIZE, compute_dtype='f32', f32_matmul='exact', use_blur=False, train_batch_size=B,
                 train_mode='pretrain', contrastive_loss='generalized', gcl_dist=dist, gcl_lambda=LAM, gcl_loss_scaling=LS, gcl_seed=11, **kw)
    return FLAGS


def _fresh_runtime():
    from simclr_amd.resnet import RT
    RT.reset()
    RT.device = torch.device(DEV)
    return RT


def _capture(monkeypatch_setattr, model):
    """Records what the step hands the loss (projection outputs), what the loss drew, and what the step hands the projection head."""
    from simclr_amd import objective as obj_lib
    box = {}
    orig_loss, orig_draws, orig_backward = obj_lib.generalized_loss_of_block, obj_lib.gcl_draws, model.backward

    def loss_fn(hidden, *a, **kw):
        box['hidden'] = hidden.detach().clone()
        box['loss'] = orig_loss(hidden, *a, **kw)
        return box['loss']

    def draws(*a, **kw):
        box['rand_w'], box['prior'] = orig_draws(*a, **kw)
        return box['rand_w'], box['prior']

    def backward(d_proj, *a, **kw):
        box['d_proj'] = d_proj.detach().clone()
        return orig_backward(d_proj, *a, **kw)
    monkeypatch_setattr(obj_lib, 'generalized_loss_of_block', loss_fn)
    monkeypatch_setattr(obj_lib, 'gcl_draws', draws)
    monkeypatch_setattr(model, 'backward', backward)
    return box


def _np(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def _reference_of_box(boxes, dist, T, hidden_norm):
    """Float64 oracle of the captured projection outputs of every replica (under the device's permutation for the SWD priors)."""
    hs = [_np(b['hidden']) for b in boxes]
    if dist == 'logsumexp':
        return gcl_reference(hs, LAM, T, dist, hidden_norm, LS)
    W, prior = _np(boxes[0]['rand_w']), _np(boxes[0]['prior'])
    perm = boxes[0]['perm'].T.astype(np.int64)
    free = gcl_reference(hs, LAM, T, dist, hidden_norm, LS, W, prior)
    assert _perm_sorts(free['P'], perm), 'the device permutation does not sort the float64 projections'
    return gcl_reference(hs, LAM, T, dist, hidden_norm, LS, W, prior, perm=perm)


@pytest.mark.parametrize('dist', ['logsumexp', 'normal', 'uniform'])
def test_step_hands_the_projection_head_the_reference_gradient(monkeypatch, dist):
    from simclr_amd import model as model_lib
    from simclr_amd.run import make_single_step
    FLAGS = _flags(dist)
    _fresh_runtime()
    model = model_lib.Model(NCLS)
    box = _capture(monkeypatch.setattr, model)
    step = make_single_step(model, model_lib.build_optimizer(0.1), None)
    assert sorted(step.metrics) == ['train/align_loss', 'train/contrast_loss', 'train/dist_loss', 'train/supervised_acc',
                                    'train/supervised_loss', 'train/total_loss', 'train/weight_decay']
    g = torch.Generator().manual_seed(31)
    images = structured_images(B, SIZE, 2, g).to(DEV)
    labels = F.one_hot(torch.randint(0, NCLS, (B,), generator=g), NCLS).float().to(DEV)
    out = step(images, {'labels': labels})
    torch.cuda.synchronize()
    assert tuple(box['hidden'].shape) == (2 * B, FLAGS.proj_out_dim) and out['logits_con'] is None
    if dist != 'logsumexp':
        box['perm'] = box['loss'].perm.cpu().numpy()
    ref = _reference_of_box([box], dist, FLAGS.temperature, FLAGS.hidden_norm)
    con = out['con_loss']
    _assert([_res('step_loss ' + dist, con.value, ref['loss'][0], GATE_LOSS), _res('step_align ' + dist, con.align, ref['align'][0], GATE_LOSS),
             _res('step_dist ' + dist, con.dist_match, ref['dist'][0], GATE_LOSS),
             _res('step_d_proj ' + dist, box['d_proj'], ref['grads'][0], GATE_GRAD)])
    m = step.metrics
    assert abs(m['train/contrast_loss'].result() - LS * (m['train/align_loss'].result() + LAM * m['train/dist_loss'].result())) \
        <= 1e-5 * abs(m['train/contrast_loss'].result())
    assert all(bool(torch.isfinite(v.value).all()) for v in model.variables)


@pytest.mark.parametrize('dist', ['logsumexp', 'normal', 'uniform'])
def test_run_main_trains_logs_and_resumes_bitwise(tmp_path, capsys, dist):
    from simclr_amd import run
    from simclr_amd.checkpoint import INDEX_NAME
    from simclr_amd.flags import FLAGS
    args = ['--dataset=synthetic', '--resnet_depth=18', '--image_size=32', '--train_batch_size=8', '--use_blur=False', '--compute_dtype=f32',
            '--checkpoint_steps=2', '--train_steps=3', '--mode=train', '--contrastive_loss=generalized', '--gcl_dist=' + dist,
            '--gcl_lambda=0.5', '--gcl_seed=3']
    full_dir, again_dir = str(tmp_path / 'full'), str(tmp_path / 'again')
    FLAGS.reset()
    run.main(args + ['--model_dir=' + full_dir])
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith('{') and 'train/dist_loss' in l]
    assert lines and lines[0]['step'] == 2
    for k in ('train/contrast_loss', 'train/align_loss', 'train/dist_loss', 'train/total_loss'):
        assert math.isfinite(lines[0][k]), (k, lines[0])
    assert 'train/contrast_acc' not in lines[0] and 'train/contrast_entropy' not in lines[0]
    assert abs(lines[0]['train/contrast_loss'] - (lines[0]['train/align_loss'] + 0.5 * lines[0]['train/dist_loss'])) \
        <= 1e-5 * abs(lines[0]['train/contrast_loss'])
    full = torch.load(os.path.join(full_dir, 'ckpt-3.pt'), map_location='cpu')
    # a run stopped after step 2 and started again: step 3 draws what the uninterrupted run drew (a function of the step alone)
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


def _worker(rank, world, port, dist_name, q):
    try:
        import torch.distributed as dist
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        torch.cuda.set_device(0)
        dist.init_process_group('gloo', rank=rank, world_size=world)
        from simclr_amd import comm, ops
        from simclr_amd import model as model_lib
        from simclr_amd.run import make_single_step
        ops.set_f32_matmul('exact')
        FLAGS = _flags(dist_name)
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
        labels = F.one_hot(torch.randint(0, NCLS, (world * B,), generator=g), NCLS).float()
        out = step(images[rank * B:(rank + 1) * B].to(DEV), {'labels': labels[rank * B:(rank + 1) * B].to(DEV)})
        torch.cuda.synchronize()
        res = dict(hidden=_np(box['hidden']), d_proj=_np(box['d_proj']), loss=float(out['con_loss'].value),
                   align=float(out['con_loss'].align), dist=float(out['con_loss'].dist_match))
        if dist_name != 'logsumexp':
            res.update(rand_w=_np(box['rand_w']), prior=_np(box['prior']), perm=_np(box['loss'].perm))
        for o, name, v in attrs.values():
            setattr(o, name, v)
        dist.destroy_process_group()
        q.put((rank, 'ok', res))
    except Exception:  # noqa
        import traceback
        q.put((rank, 'FAIL', traceback.format_exc()))


@pytest.mark.parametrize('dist_name', ['logsumexp', 'normal'])
def test_two_replica_step_vs_the_global_batch_oracle(dist_name):
    """Two gloo ranks sharing one GPU: the gradient each rank's step hands its projection head equals the gradient of the single-process
    objective (1 / R) sum_r loss_r on the global batch of both ranks' projection outputs."""
    import torch.multiprocessing as mp
    from simclr_amd.flags import FLAGS
    os.environ['SIMCLR_PEER_STATS'] = '0'          # the statistics travel over gloo (the peer-mapped exchange has its own tests)
    try:
        ctx = mp.get_context('spawn')
        q = ctx.Queue()
        port = _free_port()
        procs = [ctx.Process(target=_worker, args=(r, 2, port, dist_name, q)) for r in range(2)]
        for p in procs:
            p.start()
        res = [q.get(timeout=600) for _ in procs]
        for p in procs:
            p.join(timeout=60)
    finally:
        os.environ.pop('SIMCLR_PEER_STATS', None)
    assert all(r[1] == 'ok' for r in res), res
    boxes = [r[2] for r in sorted(res, key=lambda r: r[0])]
    if dist_name != 'logsumexp':
        assert np.array_equal(boxes[0]['rand_w'], boxes[1]['rand_w']) and np.array_equal(boxes[0]['prior'], boxes[1]['prior'])
        assert np.array_equal(boxes[0]['perm'], boxes[1]['perm'])
        assert boxes[0]['dist'] == boxes[1]['dist']                  # the identical global term on both ranks
    FLAGS.reset()
    ref = _reference_of_box(boxes, dist_name, FLAGS.temperature, FLAGS.hidden_norm)
    out = []
    for r, b in enumerate(boxes):
        out += [_res('two_replica_loss %s rank %d' % (dist_name, r), b['loss'], ref['loss'][r], GATE_LOSS),
                _res('two_replica_align %s rank %d' % (dist_name, r), b['align'], ref['align'][r], GATE_LOSS),
                _res('two_replica_dist %s rank %d' % (dist_name, r), b['dist'], ref['dist'][r], GATE_LOSS),
                _res('two_replica_d_proj %s rank %d' % (dist_name, r), b['d_proj'], ref['grads'][r], GATE_GRAD)]
    _assert(out)
