"""The cached-feature linear probe on the device (pytest -m gpu): simclr_logreg_fwd / simclr_logreg_bwd against the float64 reference
and the float32 emulation of tests/logreg_reference.py, the L-BFGS fit on toy problems, run.main end to end and two replicas over gloo.

Gate of every device value: 4 x the emulation's error on the same inputs, never below one float32 ulp (logreg_reference.gates).
Measured on the MI355X: see README "cached-feature linear probe"."""
import json
import multiprocessing as mp
import os
import socket

import numpy as np
import pytest
import torch

from tests import logreg_reference as lr
from tests.data_fixtures import make_dataset

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _t(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _device_eval(inp, l2, slabs=None):
    """dict(f, lse, hits, S, G, dW, db) of the kernels through ops, the l2 terms added in float64 as logreg.value_and_grad does."""
    from simclr_amd import ops
    x, labels, weights, W, b = (_t(a) for a in inp)
    n, C = x.shape[0], W.shape[0]
    S = float(inp[2].astype(np.float64).sum())
    inv_S = 1.0 / S
    out3 = torch.zeros(3, device=DEV, dtype=torch.float64)
    lse, G = torch.empty(n, device=DEV, dtype=torch.float64), torch.empty(n, C, device=DEV)
    dW = db = None
    for i, (o, e) in enumerate(slabs or [(0, n)]):
        out, l, g = ops.logreg_fwd(x[o:e], W, b, labels[o:e], weights[o:e], inv_S, 1)
        out3 += out
        lse[o:e], G[o:e] = l, g[:, :C]
        dW, db = ops.logreg_bwd(g, x[o:e], C, dW, db, accumulate=i > 0)
    W64, b64 = inp[3].astype(np.float64), inp[4].astype(np.float64)
    out3 = out3.cpu().numpy()
    assert out3[2] == S
    return dict(f=out3[0] * inv_S + 0.5 * l2 * ((W64 * W64).sum() + (b64 * b64).sum()), lse=lse.cpu().numpy(), hits=out3[1], S=S,
                G=G.cpu().numpy().astype(np.float64), dW=dW.cpu().numpy().astype(np.float64) + l2 * W64,
                db=db.cpu().numpy().astype(np.float64) + l2 * b64)


@pytest.mark.parametrize('case', lr.CASES, ids=str)
def test_kernels_meet_the_emulation_gates(case):
    from simclr_amd import logreg, ops
    n, D, C, fam = case
    inp, ref, emu, gate = lr.case(*case)
    assert np.all(lr.gap_ok(inp[0], inp[3], inp[4]))
    assert ops.logreg_tile_edge(n, D, C) == lr.fwd_edge(n, C) and ops.logreg_tile_edge(n, D, C, backward=True) == lr.bwd_edge(D, C)
    assert ops.logreg_row_splits(n, D, C) == lr.row_parts(n, D, C)[0]
    if (n, D, C) == lr.SPLIT_SHAPE:
        P, rows = lr.row_parts(n, D, C)
        assert ops.logreg_row_splits(n, D, C) == P > 1 and n % rows != 0
    l2 = lr.L2[(n, D, C)]
    got = _device_eval(inp, l2)
    res = lr.compare(got, ref, gate)
    for k, (err, ok) in res.items():
        print('RATIO %s %s err=%.3e gate=%.3e ratio=%.3f' % (case, k, err, gate.get(k, 0.0), err / gate[k] if k in gate else err))
    assert all(ok for _, ok in res.values()), res
    # the product path returns the same numbers
    x, labels, weights, W, b = (_t(a) for a in inp)
    f, grad, hits, wsum = logreg.value_and_grad(x, labels, weights, W, b, l2, 1.0 / ref['S'])
    assert abs(f - got['f']) <= 1e-14 * max(1.0, abs(f)) and hits == got['hits'] and wsum == ref['S']
    assert np.array_equal(grad.cpu().numpy(), np.concatenate([got['dW'].ravel(), got['db']]))


def test_zero_parameters_hand_case():
    """W = 0, b = 0: every logit is 0 exactly, lse = log C, out[0] = S log C within 1e-15 relative, and class 0 -- the lowest index of
    the all-way tie -- is the maximum: the hits are the weight of the label-0 rows."""
    from simclr_amd import ops
    for n, D, C in [(65, 64, 3), (130, 128, 65), (300, 64, 4096)]:
        x, labels, weights, W, b = lr.case_inputs(n, D, C, 'gauss')
        S = float(weights.astype(np.float64).sum())
        out, lse, G = ops.logreg_fwd(_t(x), _t(0 * W), _t(0 * b), _t(labels), _t(weights), 1.0 / S, 1)
        out = out.cpu().numpy()
        assert abs(out[0] - S * np.log(C)) <= 1e-15 * S * np.log(C), (out[0], S * np.log(C))
        assert out[1] == float(weights[labels == 0].astype(np.float64).sum()) and out[2] == S
        assert np.abs(lse.cpu().numpy() - np.log(C)).max() <= 1e-15 * np.log(C)
        want = (weights.astype(np.float64) / S)[:, None] * (1.0 / C - np.eye(C)[labels])
        assert np.abs(G[:, :C].cpu().numpy() - want).max() <= lr.ulp32(np.abs(want).max())


def _guarded(shape, dtype, fill):
    """A tensor of `shape` in the middle of a larger one filled with `fill`: (view, whole, check) -- check() asserts the bands hold."""
    numel = int(np.prod(shape))
    band = 1024
    whole = torch.full((numel + 2 * band,), fill, device=DEV, dtype=dtype)
    view = whole[band:band + numel].view(*shape)

    def check():
        assert bool((whole[:band] == fill).all()) and bool((whole[band + numel:] == fill).all())
    return view, whole, check


@pytest.mark.parametrize('shape', [(65, 64, 3), (130, 128, 65), (1100, 64, 5)], ids=str)
def test_bitwise_repeats_guard_bands_and_modes(shape):
    """Every mode repeats bitwise; mode 0 and mode 1 return the same three doubles; nothing is written outside store, lse, dw, db and
    the workspace's reported size, nor into the store columns >= C."""
    from simclr_amd import _lib, ops
    n, D, C = shape
    x, labels, weights, W, b = (_t(a) for a in lr.case_inputs(n, D, C, 'gauss'))
    pitch = ops.logreg_store_pitch(C)
    nbytes = _lib.lib().logreg_workspace_bytes(n, D, C)
    assert nbytes % 8 == 0
    outs = {}
    for mode in (0, 1, 2):
        runs = []
        for _ in range(2):
            store, _, chk_store = _guarded((n, pitch), torch.float32, -7.0)
            lse, _, chk_lse = _guarded((n,), torch.float64, -7.0)
            ws, _, chk_ws = _guarded((nbytes // 8,), torch.float64, -7.0)
            out, lse, st = ops.logreg_fwd(x, W, b, labels, weights, 0.01, mode, store if mode else None, lse, ws)
            torch.cuda.synchronize()
            chk_store(); chk_lse(); chk_ws()
            if mode:
                assert st.data_ptr() == store.data_ptr() and bool((store[:, C:] == -7.0).all()) and bool((store[:, :C] != -7.0).all())
            else:
                assert st is None and bool((store == -7.0).all())
            runs.append((out.clone(), lse.clone(), store.clone()))
        assert all(torch.equal(a, c) for a, c in zip(*runs)), mode
        outs[mode] = runs[0]
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][0], outs[2][0])
    assert torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][1], outs[2][1])
    g = outs[1][2]
    runs = []
    for _ in range(2):
        dw, _, chk_dw = _guarded((C, D), torch.float32, -7.0)
        db, _, chk_db = _guarded((C,), torch.float32, -7.0)
        ws, _, chk_ws = _guarded((nbytes // 8,), torch.float64, -7.0)
        ops.logreg_bwd(g, x, C, dw, db, ws=ws)
        torch.cuda.synchronize()
        chk_dw(); chk_db(); chk_ws()
        assert bool((dw != -7.0).all()) and bool((db != -7.0).all())
        runs.append((dw.clone(), db.clone()))
    assert all(torch.equal(a, c) for a, c in zip(*runs))


def test_two_slabs_accumulate_like_their_emulation():
    n, D, C = 130, 128, 65
    inp = lr.case_inputs(n, D, C, 'gauss')
    slabs = [(0, 96), (96, n)]
    ref = lr.direct(*inp, 1e-3)
    emu = lr.emulate(*inp, 1e-3, slabs=slabs)
    gate = lr.gates(emu, ref)
    res = lr.compare(_device_eval(inp, 1e-3, slabs), ref, gate)
    assert all(ok for _, ok in res.values()), res


def test_value_and_grad_walks_slabs_with_one_workspace(monkeypatch):
    """logreg.value_and_grad with slabs of 96 rows on 130: the ragged last slab runs in the buffers of the first, and the sums are those
    of the two kernel calls made by hand."""
    from simclr_amd import logreg
    n, D, C = 130, 128, 65
    inp = lr.case_inputs(n, D, C, 'gauss')
    want = _device_eval(inp, 1e-3, [(0, 96), (96, n)])
    monkeypatch.setattr(logreg, 'SLAB_ROWS', 96)
    logreg._BUFFERS.clear()
    x, labels, weights, W, b = (_t(a) for a in inp)
    for _ in range(2):
        f, grad, hits, wsum = logreg.value_and_grad(x, labels, weights, W, b, 1e-3, 1.0 / want['S'])
        assert abs(f - want['f']) <= 1e-14 * max(1.0, abs(f)) and hits == want['hits'] and wsum == want['S']
        assert np.array_equal(grad.cpu().numpy(), np.concatenate([want['dW'].ravel(), want['db']]))
        f0 = logreg.value_and_grad(x, labels, weights, W, b, 1e-3, 1.0 / want['S'], want_grad=False)[0]
        assert f0 == f
    assert len(logreg._BUFFERS) == 1 and next(iter(logreg._BUFFERS))[:2] == (96, 34)
    logreg._BUFFERS.clear()


def test_refusals_on_device_tensors():
    from simclr_amd import _lib, ops
    x, labels, weights, W, b = (_t(a) for a in lr.case_inputs(65, 64, 3, 'gauss'))
    with pytest.raises(ValueError, match=r'labels must lie in \[0, 3\)'):
        ops.logreg_fwd(x, W, b, torch.full_like(labels, 3), weights, 1.0)
    with pytest.raises(ValueError, match=r'labels must lie in \[0, 3\)'):
        ops.logreg_fwd(x, W, b, labels - 1, weights, 1.0)
    with pytest.raises(ValueError, match='multiples of 64'):
        ops.logreg_fwd(x[:, :32].contiguous(), W[:, :32].contiguous(), b, labels, weights, 1.0)
    with pytest.raises(ValueError, match='w must be a float32'):
        ops.logreg_fwd(x, W.double(), b, labels, weights, 1.0)
    with pytest.raises(ValueError, match='16-byte aligned'):
        ops.logreg_fwd(x, W, torch.zeros(4, device=DEV)[1:], labels, weights, 1.0)
    with pytest.raises(ValueError, match='workspace must hold'):
        ops.logreg_fwd(x, W, b, labels, weights, 1.0, ws=torch.zeros(8, device=DEV, dtype=torch.float64))
    with pytest.raises(ValueError, match='store must be'):
        ops.logreg_fwd(x, W, b, labels, weights, 1.0, 2, store=torch.zeros(65, 3, device=DEV))
    with pytest.raises(ValueError, match='g must be'):
        ops.logreg_bwd(torch.zeros(65, 3, device=DEV), x, 3)
    # the library itself refuses through its return code
    L = _lib.lib()
    p = lambda t: t.data_ptr()
    with pytest.raises(_lib.SimclrHipError, match='mode must be'):
        L.logreg_fwd(p(x), p(W), p(b), p(labels), p(weights), 65, 64, 3, 1.0, 5, None, None, None, None, None)
    with pytest.raises(_lib.SimclrHipError, match='16-byte aligned'):
        L.logreg_bwd(p(x) + 4, p(x), 65, 64, 3, p(W), p(b), 0, p(x), None)
    out, _, _ = ops.logreg_fwd(x, W, b, labels, weights, 1.0)        # and still works afterwards
    assert bool(torch.isfinite(out).all())


# ------------------------------------------------------------------ the fit
@pytest.mark.parametrize('problem', lr.TOY_PROBLEMS, ids=str)
def test_fit_reaches_the_unique_minimiser(problem):
    from simclr_amd import logreg
    N, D, C, l2, sep = problem
    tol = 1e-5
    xn, labels, weights = lr.toy_problem(N, D, C, sep)
    x, y, w = _t(xn), _t(labels), _t(weights)
    fit = logreg.fit(x, y, w, C, l2)
    print('FIT %s iterations=%d evaluations=%d f=%.9g |g|inf=%.3e' % (problem, fit.iterations, fit.evaluations, fit.loss, fit.grad_norm))
    assert fit.converged and fit.iterations < 200 and len(fit.losses) == fit.iterations
    assert all(b <= a for a, b in zip(fit.losses, fit.losses[1:]))
    W32, b32 = fit.W.cpu().numpy(), fit.b.cpu().numpy()
    ref = lr.direct(xn, labels, weights, W32, b32, l2)
    emu = lr.emulate(xn, labels, weights, W32, b32, l2)
    g64 = np.concatenate([ref['dW'].ravel(), ref['db']])
    gemu = np.concatenate([emu['dW'].ravel(), emu['db']])
    gerr = np.abs(gemu - g64).max()
    print('FIT %s |g64|inf=%.3e bound=%.3e emulation gradient error=%.3e' % (problem, np.abs(g64).max(), tol * max(1.0, abs(ref['f'])), gerr))
    assert np.abs(g64).max() <= tol * max(1.0, abs(ref['f'])) + 4.0 * gerr
    assert abs(fit.loss - ref['f']) <= max(4.0 * abs(emu['f'] - ref['f']), lr.ulp32(ref['f']))
    if np.all(lr.gap_ok(xn, W32, b32)):
        assert fit.train_top_1 == ref['hits'] / ref['S']
    # strict convexity (modulus l2): a point with gradient g lies within |g|_2 / l2 of the minimiser.  The float64 solver's point, solved
    # to 1e-10, stands for the minimiser: its own distance |g_best|_2 / l2 is asserted to be below 1e-3 of the bound it is measured with
    # (|g_best|_2 <= sqrt(dim) 1e-10 max(1, f) is at most 2.3e-4 of the |g64|_2 of these fits)
    best = lr.solve(xn, labels, weights, C, l2, max_iterations=2000, tolerance=1e-10)
    assert best.converged
    rb = lr.direct(xn, labels, weights, best.W, best.b, l2)
    gb = np.concatenate([rb['dW'].ravel(), rb['db']])
    dist = np.sqrt(((W32 - best.W) ** 2).sum() + ((b32 - best.b) ** 2).sum())
    print('FIT %s distance=%.3e bound=%.3e float64 solver\'s own=%.3e' % (problem, dist, np.linalg.norm(g64) / l2, np.linalg.norm(gb) / l2))
    assert np.linalg.norm(gb) <= 1e-3 * np.linalg.norm(g64)
    assert dist <= np.linalg.norm(g64) / l2
    again = logreg.fit(x, y, w, C, l2)
    assert torch.equal(again.W, fit.W) and torch.equal(again.b, fit.b) and again.losses == fit.losses
    assert (again.iterations, again.evaluations, again.grad_norm, again.loss) == (fit.iterations, fit.evaluations, fit.grad_norm, fit.loss)


def test_fit_stops_at_the_cap_and_warm_starts():
    from simclr_amd import logreg
    N, D, C, l2, sep = lr.TOY_PROBLEMS[0]
    x, y, w = (_t(a) for a in lr.toy_problem(N, D, C, sep))
    short = logreg.fit(x, y, w, C, l2, max_iterations=3)
    assert not short.converged and short.iterations == 3 and len(short.losses) == 3
    full = logreg.fit(x, y, w, C, l2)
    warm = logreg.fit(x, y, w, C, l2, init=(full.W, full.b))
    assert warm.converged and warm.iterations == 0 and warm.evaluations == 1 and torch.equal(warm.W, full.W)
    mu, var = logreg.standardize_stats(x * 3.0 + 1.0, w)
    keep = w > 0
    h = (x * 3.0 + 1.0).double()[keep]
    assert torch.allclose(mu, h.mean(0), rtol=1e-13, atol=1e-13) and torch.allclose(var, h.var(0, unbiased=False), rtol=1e-12, atol=1e-13)


# ------------------------------------------------------------------ end to end
_MAIN = ['--resnet_depth=18', '--image_size=32', '--train_batch_size=16', '--eval_batch_size=16', '--use_blur=False',
         '--compute_dtype=f32', '--f32_matmul=exact', '--mode=train_then_eval', '--train_steps=2', '--checkpoint_steps=2',
         '--lineareval_while_pretraining=False']
_LOGREG_KEYS = {'eval/logreg_top_1_accuracy', 'eval/logreg_top_5_accuracy', 'eval/logreg_loss', 'logreg/train_loss',
                'logreg/train_top_1_accuracy', 'logreg/iterations', 'logreg/evaluations', 'logreg/grad_norm', 'logreg/converged',
                'logreg/l2', 'global_step'}


def _fresh_model(num_classes=10):
    """A model under the flags run.main left, its variables built (inference: nothing moves)."""
    from simclr_amd import model as model_lib
    from simclr_amd.resnet import RT
    RT.reset()
    RT.device = torch.device(DEV, torch.cuda.current_device())
    model = model_lib.Model(num_classes)
    model(torch.zeros(2, 32, 32, 3, device=DEV), training=False)
    model.release()
    return model


def _check_files(model_dir, result, l2s):
    for name in ('logreg_result.json', 'logreg_result_2.json'):
        saved = json.load(open(os.path.join(model_dir, name)))
        fits = saved.pop('fits')
        assert set(saved) == _LOGREG_KEYS and saved == {k: result[k] for k in _LOGREG_KEYS}
        assert [f['logreg/l2'] for f in fits] == l2s and all(set(f) == _LOGREG_KEYS for f in fits) and fits[-1] == saved
    assert result['global_step'] == 2 and result['logreg/l2'] == l2s[-1]
    assert 0.0 <= result['eval/logreg_top_1_accuracy'] <= result['eval/logreg_top_5_accuracy'] <= 1.0
    assert np.isfinite(result['eval/logreg_loss']) and np.isfinite(result['logreg/train_loss']) and result['logreg/iterations'] >= 1
    return fits


def test_run_main_on_synthetic_data(tmp_path):
    from simclr_amd import run
    from simclr_amd.flags import FLAGS
    model_dir = str(tmp_path / 'm')
    try:
        FLAGS.reset()
        result = run.main(_MAIN + ['--dataset=synthetic', '--eval_steps=2', '--model_dir=' + model_dir, '--logreg_eval=True',
                                   '--logreg_l2=1e-2,1e-3', '--knn_eval=True', '--knn_k=5'])
        assert set(result) == _LOGREG_KEYS | {'eval/knn_top_1_accuracy', 'eval/knn_top_5_accuracy'}      # the union
        assert os.path.exists(os.path.join(model_dir, 'knn_result.json'))
        fits = _check_files(model_dir, result, [1e-2, 1e-3])
        assert len(fits) == 2
        # --mode=eval on the checkpoint just written: the second wiring path gives the same probe
        eval_args = [a for a in _MAIN if not a.startswith(('--mode', '--train_steps', '--checkpoint_steps'))] + [
            '--mode=eval', '--dataset=synthetic', '--eval_steps=2', '--model_dir=' + model_dir]
        FLAGS.reset()
        again = run.main(eval_args + ['--logreg_eval=True', '--logreg_l2=1e-2,1e-3'])
        assert again == {k: result[k] for k in _LOGREG_KEYS}
        assert _check_files(model_dir, again, [1e-2, 1e-3]) == fits
        # a cold fit of the second value needs more evaluations than the warm-started one
        FLAGS.reset()
        cold = run.main(eval_args + ['--logreg_eval=True', '--logreg_l2=1e-3'])
        print('SYNTHETIC evaluations: warm %d, cold %d' % (fits[1]['logreg/evaluations'], cold['logreg/evaluations']))
        assert fits[1]['logreg/evaluations'] < cold['logreg/evaluations']
        # both stand within |g|_2^2 / (2 l2) of the one minimum (strong convexity), |g|_2 <= sqrt(dim) |g|_inf, dim = 10 * 512 + 10
        slack = 5130 * (cold['logreg/grad_norm'] ** 2 + fits[1]['logreg/grad_norm'] ** 2) / (2 * 1e-3)
        assert abs(cold['logreg/train_loss'] - fits[1]['logreg/train_loss']) <= slack + 1e-6 * abs(cold['logreg/train_loss'])
        # the flag off: no logreg key, and the files are not touched
        for name in ('logreg_result.json', 'logreg_result_2.json'):
            os.remove(os.path.join(model_dir, name))
        FLAGS.reset()
        plain = run.main(eval_args)
        assert not plain or not any('logreg' in k for k in plain)
        assert not os.path.exists(os.path.join(model_dir, 'logreg_result.json'))
        assert not os.path.exists(os.path.join(model_dir, 'logreg_result_2.json'))
    finally:
        FLAGS.reset()


def test_run_main_on_a_dataset_with_a_padded_last_batch(tmp_path):
    from simclr_amd import data as data_lib
    from simclr_amd import knn, logreg, run
    from simclr_amd.checkpoint import Checkpoint
    from simclr_amd.flags import FLAGS
    data_dir, model_dir, plain_dir = str(tmp_path / 'data'), str(tmp_path / 'm'), str(tmp_path / 'plain')
    make_dataset(data_dir)                                        # 103 train / 37 validation images, 10 classes
    try:
        FLAGS.reset()
        result = run.main(_MAIN + ['--dataset=waves', '--data_dir=' + data_dir, '--model_dir=' + model_dir, '--logreg_eval=True',
                                   '--logreg_l2=1e-2,1e-3'])
        assert set(result) == _LOGREG_KEYS
        fits = _check_files(model_dir, result, [1e-2, 1e-3])
        assert not os.path.exists(os.path.join(model_dir, 'knn_result.json'))
        # the same probe by hand from the restored model: the padded rows of both splits carry weight 0
        model = _fresh_model()
        Checkpoint(model=model).restore(os.path.join(model_dir, 'ckpt-2.pt'), model_only=False).expect_partial()
        builder = data_lib.ArrayDatasetBuilder('waves', data_dir)
        dev = torch.device(DEV, torch.cuda.current_device())
        h, lab, w = knn.extract_features(model, data_lib.DatasetIterator(builder.split('train'), 10, 16, False, device=dev), normalize=False)
        assert h.shape[0] == 112 and float(w.sum()) == 103
        mu, var = logreg.standardize_stats(h, w)
        x = logreg.standardize(h, mu, var)
        first = logreg.fit(x, lab, w, 10, 1e-2, FLAGS.logreg_max_iterations, FLAGS.logreg_tolerance, FLAGS.logreg_history)
        warm = logreg.fit(x, lab, w, 10, 1e-3, FLAGS.logreg_max_iterations, FLAGS.logreg_tolerance, FLAGS.logreg_history,
                          init=(first.W, first.b))
        cold = logreg.fit(x, lab, w, 10, 1e-3, FLAGS.logreg_max_iterations, FLAGS.logreg_tolerance, FLAGS.logreg_history)
        print('E2E evaluations: first %d, warm %d, cold %d; run.main %s' % (first.evaluations, warm.evaluations, cold.evaluations,
                                                                            [f['logreg/evaluations'] for f in fits]))
        assert (fits[0]['logreg/evaluations'], fits[0]['logreg/train_loss']) == (first.evaluations, first.loss)
        assert (fits[1]['logreg/evaluations'], fits[1]['logreg/train_loss']) == (warm.evaluations, warm.loss)
        assert fits[1]['logreg/evaluations'] < cold.evaluations
        hq, qlab, qw = knn.extract_features(model, data_lib.DatasetIterator(builder.split('validation'), 10, 16, False, device=dev),
                                            normalize=False)
        counts = logreg.score(logreg.standardize(hq, mu, var), qlab, qw, warm.W, warm.b).cpu().numpy()
        assert counts[3] == 37
        assert result['eval/logreg_top_1_accuracy'] == counts[1] / 37 and result['eval/logreg_top_5_accuracy'] == counts[2] / 37
        assert result['eval/logreg_loss'] == counts[0] / 37
        # the flag off: no file, the result of before
        FLAGS.reset()
        plain = run.main(_MAIN + ['--dataset=waves', '--data_dir=' + data_dir, '--model_dir=' + plain_dir])
        assert plain is None and not os.path.exists(os.path.join(plain_dir, 'logreg_result.json'))
        assert os.path.exists(os.path.join(plain_dir, 'ckpt-2.pt'))
    finally:
        FLAGS.reset()


# ------------------------------------------------------------------ two replicas over gloo on one GPU
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _shard(n, rank, world=2, B=32):
    """Eval-style shards: global batch B, B / world rows per replica and step, positions past the end are row 0 with weight 0."""
    b = B // world
    steps = -(-n // B)
    pos = (np.arange(steps)[:, None] * B + rank * b + np.arange(b)[None, :]).reshape(-1)
    return np.where(pos < n, pos, 0), (pos < n).astype(np.float32)


_GLOO_CASE = (130, 128, 65, 'gauss')


def _logreg_worker(rank, world, port, q):
    try:
        import torch.distributed as dist
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          SIMCLR_DIST_BACKEND='gloo', SIMCLR_SHARE_GPU='1')
        torch.cuda.set_device(0)
        dist.init_process_group('gloo', rank=rank, world_size=world)
        from simclr_amd import comm, logreg
        from simclr_amd.resnet import RT
        RT.reset()
        RT.device = torch.device('cuda', 0)
        strategy = comm.Strategy()
        t = lambda a: torch.from_numpy(np.array(a)).to(RT.device)
        x, labels, weights, W, b = lr.case_inputs(*_GLOO_CASE)
        S = float(weights.astype(np.float64).sum())
        pos, keep = _shard(len(x), rank)
        f2, g2, hits2, w2 = logreg.value_and_grad(t(x[pos]), t(labels[pos]), t(weights[pos] * keep), t(W), t(b), 1e-3, 1.0 / S,
                                                  True, strategy)
        f1, g1, hits1, w1 = logreg.value_and_grad(t(x), t(labels), t(weights), t(W), t(b), 1e-3, 1.0 / S, True, None)
        N, D, C, l2, sep = lr.TOY_PROBLEMS[0]
        xn, yn, wn = lr.toy_problem(N, D, C, sep)
        pos, keep = _shard(N, rank)
        mu, var = logreg.standardize_stats(t(xn[pos]), t(wn[pos] * keep), strategy)
        mu1, var1 = logreg.standardize_stats(t(xn), t(wn), None)
        fit = logreg.fit(t(xn[pos]), t(yn[pos]), t(wn[pos] * keep), C, l2, strategy=strategy)
        torch.cuda.synchronize()
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, 'ok', dict(f2=f2, f1=f1, hits2=hits2, hits1=hits1, w2=w2, w1=w1, g2=g2.cpu().numpy(), g1=g1.cpu().numpy(),
                                stats=float(max((mu - mu1).abs().max(), (var - var1).abs().max())),
                                fit=(fit.converged, fit.iterations, fit.loss, fit.W.cpu().numpy(), fit.b.cpu().numpy()))))
    except Exception:  # noqa
        import traceback
        q.put((rank, 'FAIL', traceback.format_exc()))


def test_two_ranks_over_gloo_fit_the_probe_of_one_process():
    """Disjoint shards of the bank on two ranks, one all-reduce per evaluation: the hit counts and the weight total are exactly one
    process's, f and the gradient meet the gates of the case against float64, both ranks hold the same bits, and the sharded fit
    converges to the float64 minimiser."""
    os.environ['SIMCLR_PEER_STATS'] = '0'
    try:
        ctx = mp.get_context('spawn')
        q = ctx.Queue()
        port = _free_port()
        procs = [ctx.Process(target=_logreg_worker, args=(r, 2, port, q)) for r in range(2)]
        for p in procs:
            p.start()
        res = [q.get(timeout=300) for _ in procs]
        for p in procs:
            p.join(timeout=60)
    finally:
        os.environ.pop('SIMCLR_PEER_STATS', None)
    assert all(r[1] == 'ok' for r in res), res
    inp, ref, emu, gate = lr.case(*_GLOO_CASE)
    g64 = np.concatenate([ref['dW'].ravel(), ref['db']])
    ggate = max(gate['dW'], gate['db'])
    a, c = res[0][2], res[1][2]
    assert a['f2'] == c['f2'] and np.array_equal(a['g2'], c['g2']) and np.array_equal(a['fit'][3], c['fit'][3])
    for m in (a, c):
        assert m['hits2'] == m['hits1'] == ref['hits'] and m['w2'] == m['w1'] == ref['S']
        print('GLOO f two ranks %.17g one %.17g float64 %.17g gate %.3e' % (m['f2'], m['f1'], ref['f'], gate['f']))
        assert abs(m['f2'] - ref['f']) <= gate['f'] and abs(m['f1'] - ref['f']) <= gate['f']
        assert np.abs(m['g2'] - g64).max() <= ggate and np.abs(m['g1'] - g64).max() <= ggate
        assert m['stats'] <= 1e-13
        converged, iterations, loss, W, b = m['fit']
        assert converged and iterations < 200
    N, D, C, l2, sep = lr.TOY_PROBLEMS[0]
    xn, yn, wn = lr.toy_problem(N, D, C, sep)
    r = lr.direct(xn, yn, wn, a['fit'][3], a['fit'][4], l2)
    e = lr.emulate(xn, yn, wn, a['fit'][3], a['fit'][4], l2)
    gerr = max(np.abs(e['dW'] - r['dW']).max(), np.abs(e['db'] - r['db']).max())
    assert max(np.abs(r['dW']).max(), np.abs(r['db']).max()) <= 1e-5 * max(1.0, abs(r['f'])) + 4.0 * gerr
