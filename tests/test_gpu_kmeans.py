"""The k-means clustering evaluation on the device (pytest -m gpu): simclr_kmeans_assign / _update / _finish against the float64
reference and the float32 emulation of tests/kmeans_reference.py, the fit on planted toys, run.main end to end and two replicas over
gloo.  Every test here fails without the feature.

Gates (kmeans_reference.gates): `best` and J at 4 x the emulation's error on the same inputs, never below one float32 ulp of 1; c_new at
one float32 ulp of 1; assignments, counts, sums and wsum exact.  Measured on the MI355X: see README "k-means clustering evaluation"."""
import json
import multiprocessing as mp
import os
import socket

import numpy as np
import pytest
import torch

from tests import kmeans_reference as km
from tests.data_fixtures import make_dataset

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _t(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _device(inp, slabs=None):
    """The three launches through ops on one case: the dict of kmeans_reference.NAMES."""
    from simclr_amd import ops
    x, w, c, prev = (_t(a) for a in inp)
    n, K = x.shape[0], c.shape[0]
    assign, best = prev.clone(), torch.empty(n, device=DEV)
    out3 = torch.zeros(3, device=DEV, dtype=torch.float64)
    sums = wsum = None
    for i, (o, e) in enumerate(slabs or [(0, n)]):
        _, _, out = ops.kmeans_assign(x[o:e], c, w[o:e], assign[o:e], best[o:e])
        out3 += out
        sums, wsum = ops.kmeans_update(x[o:e], w[o:e], assign[o:e], K, sums, wsum, accumulate=i > 0)
    c_new, out2 = ops.kmeans_finish(sums, wsum, c)
    out3, out2 = out3.cpu().numpy(), out2.cpu().numpy()
    return dict(assign=assign.cpu().numpy(), best=best.cpu().numpy().astype(np.float64), J=out3[0] / out3[1], S=out3[1], changed=out3[2],
                sums=sums.cpu().numpy(), wsum=wsum.cpu().numpy(), c_new=c_new.cpu().numpy().astype(np.float64), kept=out2[0], shift=out2[1],
                c_new32=c_new)


@pytest.mark.parametrize('case', km.CASES, ids=str)
def test_kernels_meet_the_emulation_gates(case):
    from simclr_amd import ops
    n, D, K, fam = case
    inp, ref, emu, gate, _ = km.case(*case)
    assert np.all(km.gap_ok(inp[0], inp[2], inp[1]))                 # a condition on the inputs: then the exact index is demanded
    assert ops.kmeans_tile_edge(n, D, K) == km.tile_edge(n, K) == (128 if (n, D, K) == km.WIDE_SHAPE else 64)
    got = _device(inp)
    res = km.compare(got, ref, gate, inp[1])
    for k, (err, ok) in res.items():
        print('RATIO %s %s err=%.3e gate=%.3e ratio=%.3f' % (case, k, err, gate.get(k, 0.0), err / gate[k] if k in gate else err))
    assert all(ok for _, ok in res.values()), res
    # max_k (1 - c_new_k . c_prev_k) is the double dot product of the centroids the launch wrote
    c64 = got['c_new']
    want = float((1.0 - (c64 * inp[2].astype(np.float64)).sum(1)).max())
    assert abs(got['shift'] - want) <= 1e-13


def test_ties_go_to_the_lowest_index():
    """Every centroid a copy of one row, and every row that row: all K scores of a row are bitwise equal."""
    from simclr_amd import ops
    for n, D, K in [(65, 64, 63), (130, 128, 200), (2049, 64, 2049)]:
        row = km.unit(np.random.RandomState(n).randn(1, D))
        x, c = _t(np.repeat(row, n, 0)), _t(np.repeat(row, K, 0))
        a, best, out = ops.kmeans_assign(x, c, torch.ones(n, device=DEV))
        assert bool((a == 0).all()) and bool((best == best[0]).all()) and float(out[2]) == n
        # a centroid equal to a row's own, placed twice: the lower of the two indices
        c2 = km.unit(np.random.RandomState(n + 1).randn(K, D))
        c2[K - 1] = c2[3] = row[0]
        a, _, _ = ops.kmeans_assign(x, _t(c2), torch.ones(n, device=DEV))
        assert bool((a == 3).all())


def test_nan_scores_order_below_every_number():
    from simclr_amd import ops
    x, w, c, _ = (np.array(a) for a in km.case_inputs(65, 64, 63, 'gauss'))
    want = km.assign64(x, c[1:])[0] + 1
    c[0] = np.nan
    a, best, _ = ops.kmeans_assign(_t(x), _t(c), _t(w))
    assert np.array_equal(a.cpu().numpy(), want) and bool(torch.isfinite(best).all())


def _guarded(shape, dtype, fill):
    """A tensor of `shape` in the middle of a larger one filled with `fill`: (view, check) -- check() asserts the bands hold."""
    numel = int(np.prod(shape))
    band = 1024
    whole = torch.full((numel + 2 * band,), fill, device=DEV, dtype=dtype)
    view = whole[band:band + numel].view(*shape)

    def check():
        assert bool((whole[:band] == fill).all()) and bool((whole[band + numel:] == fill).all())
    return view, check


@pytest.mark.parametrize('shape', [(65, 64, 63), (130, 64, 65), (2049, 64, 2049)], ids=str)
def test_bitwise_repeats_and_guard_bands(shape):
    from simclr_amd import _lib, ops
    n, D, K = shape
    x, w, c, prev = (_t(a) for a in km.case_inputs(n, D, K, 'gauss'))
    nbytes = _lib.lib().kmeans_workspace_bytes(n, D, K)
    assert nbytes % 8 == 0
    runs = []
    for _ in range(2):
        assign, chk_a = _guarded((n,), torch.int32, -7)
        best, chk_b = _guarded((n,), torch.float32, -7.0)
        ws, chk_ws = _guarded((nbytes // 8,), torch.float64, -7.0)
        sums, chk_s = _guarded((K, D), torch.float64, -7.0)
        wsum, chk_w = _guarded((K,), torch.float64, -7.0)
        c_new, chk_c = _guarded((K, D), torch.float32, -7.0)
        assign.copy_(prev)
        _, _, out3 = ops.kmeans_assign(x, c, w, assign, best, ws)
        ops.kmeans_update(x, w, assign, K, sums, wsum)
        _, out2 = ops.kmeans_finish(sums, wsum, c, c_new, ws)
        torch.cuda.synchronize()
        for chk in (chk_a, chk_b, chk_ws, chk_s, chk_w, chk_c):
            chk()
        assert bool((best != -7.0).all()) and bool((assign >= 0).all()) and bool((c_new != -7.0).all())
        runs.append([t.clone() for t in (assign, best, out3, sums, wsum, c_new, out2)])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_two_slabs_accumulate_to_the_one_call_sums():
    """Two slabs add (slab 0) + (slab 1) per cluster, one call adds the rows one by one: the sums agree in double up to the order of
    the additions, so they are gated at 4 eps64 x the largest sum; everything else is exact."""
    inp = km.case_inputs(130, 64, 65, 'tight')
    one, two = _device(inp), _device(inp, [(0, 96), (96, 130)])
    assert np.array_equal(one['assign'], two['assign']) and np.array_equal(one['best'], two['best'])
    assert np.array_equal(one['wsum'], two['wsum']) and (one['S'], one['changed'], one['kept']) == (two['S'], two['changed'], two['kept'])
    assert np.abs(one['sums'] - two['sums']).max() <= 4 * np.finfo(np.float64).eps * np.abs(one['sums']).max()
    assert abs(one['J'] - two['J']) <= 4 * np.finfo(np.float64).eps
    assert np.abs(one['c_new'] - two['c_new']).max() <= km.ULP1


def test_bad_order_and_offsets_are_skipped_and_clamped():
    """The C entry given an order entry outside [0, n) and offsets outside [0, n]: the entries are skipped / clamped, the sums are those
    of the valid rows, nothing outside the buffers is written.  A refusal-and-clamp test: nothing faults."""
    from simclr_amd import _lib
    n, D, K = 130, 64, 65
    xn, wn, cn, _ = km.case_inputs(n, D, K, 'gauss')
    a = km.assign64(xn, cn)[0]
    order = np.argsort(a, kind='stable').astype(np.int32)
    offsets = np.searchsorted(a[order], np.arange(K + 1)).astype(np.int32)
    bad_order, bad_offsets = order.copy(), offsets.copy()
    dropped = [int(order[5]), int(order[77])]
    bad_order[5], bad_order[77] = n, -3                       # one past the end, and negative
    bad_offsets[0], bad_offsets[K] = -9, n + 1000             # clamped to 0 and n: the same segments
    keep = np.ones(n, bool)
    keep[dropped] = False
    want_s, want_w = km.update64(xn, np.where(keep, wn, 0).astype(np.float32), a, K)
    x, w = _t(xn), _t(wn)
    sums, chk_s = _guarded((K, D), torch.float64, -7.0)
    wsum, chk_w = _guarded((K,), torch.float64, -7.0)
    p = lambda t: t.data_ptr()
    o, f = _t(bad_order), _t(bad_offsets)
    _lib.lib().kmeans_update(p(x), p(w), p(o), p(f), n, D, K, p(sums), p(wsum), 0, None)
    torch.cuda.synchronize()
    chk_s(); chk_w()
    assert np.array_equal(sums.cpu().numpy(), want_s) and np.array_equal(wsum.cpu().numpy(), want_w)
    # a decreasing pair of offsets is an empty segment
    f2 = offsets.copy()
    f2[3] = n
    _lib.lib().kmeans_update(p(x), p(w), p(_t(order)), p(_t(f2)), n, D, K, p(sums), p(wsum), 0, None)
    torch.cuda.synchronize()
    chk_s(); chk_w()
    assert bool(torch.isfinite(sums).all())


def test_refusals_on_device_tensors():
    from simclr_amd import _lib, ops
    x, w, c, prev = (_t(a) for a in km.case_inputs(65, 64, 63, 'gauss'))
    with pytest.raises(ValueError, match='multiples of 64'):
        ops.kmeans_assign(x[:, :32].contiguous(), c[:, :32].contiguous(), w)
    with pytest.raises(ValueError, match='c must be a float32'):
        ops.kmeans_assign(x, c.double(), w)
    with pytest.raises(ValueError, match='16-byte aligned'):
        ops.kmeans_assign(x, c, torch.zeros(66, device=DEV)[1:])
    with pytest.raises(ValueError, match='workspace must hold'):
        ops.kmeans_assign(x, c, w, ws=torch.zeros(8, device=DEV, dtype=torch.float64))
    with pytest.raises(ValueError, match='assign must be'):
        ops.kmeans_update(x, w, prev.long(), 63)
    with pytest.raises(ValueError, match='may not alias'):
        ops.kmeans_finish(torch.zeros(63, 64, device=DEV, dtype=torch.float64), torch.zeros(63, device=DEV, dtype=torch.float64), c, c)
    L = _lib.lib()
    p = lambda t: t.data_ptr()
    with pytest.raises(_lib.SimclrHipError, match='16-byte aligned'):
        L.kmeans_assign(p(x) + 4, p(c), p(w), 65, 64, 63, p(prev), p(w), p(x), p(x), None)
    with pytest.raises(_lib.SimclrHipError, match='2 <= K <= 16384'):
        L.kmeans_update(p(x), p(w), p(prev), p(prev), 65, 64, 1, p(x), p(x), 0, None)
    a, best, out = ops.kmeans_assign(x, c, w)                    # and still works afterwards
    assert bool(torch.isfinite(out).all()) and float(out[2]) == 65


# ------------------------------------------------------------------ the fit
def _check_fit_against_reference(x, w, K, seed, restarts):
    from simclr_amd import kmeans
    ref = km.fit64(x, w, K, seed=seed, restarts=restarts)
    assert all(km.lloyd_gaps_ok(x, w, run) for run in ref['runs'])            # a condition on the data, checked on the CPU
    fit = kmeans.fit(_t(x), _t(w), K, seed, restarts)
    assert fit.restart == ref['restart'] and fit.iterations == ref['iterations'] and fit.converged and ref['converged']
    assert [r['iterations'] for r in fit.restarts] == [r['iterations'] for r in ref['runs']]
    assert [r['empty_clusters'] for r in fit.restarts] == [r['empties'] for r in ref['runs']] and fit.empty_clusters == ref['empties']
    # the gate of J: 4 x the emulation's error at the reference's final centroids, never below one float32 ulp of 1
    prev = np.full(len(x), -1, np.int32)
    jgate = km.gates(km.emulate(x, w, ref['c'], prev), km.direct(x, w, ref['c'], prev))['J']
    print('FIT K=%d J device %.12g float64 %.12g gate %.3e iterations %d' % (K, fit.inertia, ref['J'], jgate, fit.iterations))
    assert abs(fit.inertia - ref['J']) <= jgate
    assert all(b <= a + jgate for a, b in zip(fit.inertias, fit.inertias[1:])) and len(fit.inertias) == fit.iterations
    a, _, _ = kmeans.assign(_t(x), _t(w), fit.centroids)
    assert np.array_equal(a.cpu().numpy()[w > 0], ref['assigns'][-1][w > 0])
    again = kmeans.fit(_t(x), _t(w), K, seed, restarts)
    assert torch.equal(again.centroids, fit.centroids) and again.inertias == fit.inertias and again.restarts == fit.restarts
    return fit, a


def test_fit_recovers_the_planted_directions():
    from simclr_amd import kmeans
    x, labels, w = km.planted()
    fit, a = _check_fit_against_reference(x, w, 8, 0, 2)
    T = kmeans.contingency(a, _t(labels), _t(w), 8, 8)
    assert int(T.sum()) == 509
    s = kmeans.scores(T, T)
    assert s['eval/kmeans_nmi'] == 1.0 and s['eval/kmeans_ari'] == 1.0 and s['eval/kmeans_top_1_accuracy'] == 1.0
    assert s.get(kmeans.MATCHED_KEY, 1.0) == 1.0
    short = kmeans.fit(_t(x), _t(w), 8, 0, 1, max_iterations=1)
    assert not short.converged and short.iterations == 1
    warm = kmeans.fit(_t(x), _t(w), 8, init=fit.centroids)
    assert warm.converged and warm.iterations <= 2 and abs(warm.inertia - fit.inertia) <= km.ULP1


def test_fit_with_more_clusters_than_directions_counts_the_empties():
    x, _, w = km.planted(seed=2)
    fit, _ = _check_fit_against_reference(x, w, 12, 3, 1)
    assert fit.empty_clusters == 1


def test_fit_walks_slabs(monkeypatch):
    from simclr_amd import kmeans
    x, _, w = km.planted()
    one = kmeans.fit(_t(x), _t(w), 8, 0, 1)
    monkeypatch.setattr(kmeans, 'SLAB_ROWS', 200)
    three = kmeans.fit(_t(x), _t(w), 8, 0, 1)
    assert three.iterations == one.iterations and abs(three.inertia - one.inertia) <= 1e-14
    assert float((three.centroids - one.centroids).abs().max()) <= km.ULP1


# ------------------------------------------------------------------ end to end
_MAIN = ['--resnet_depth=18', '--image_size=32', '--train_batch_size=16', '--eval_batch_size=16', '--use_blur=False',
         '--compute_dtype=f32', '--f32_matmul=exact', '--mode=train_then_eval', '--train_steps=2', '--checkpoint_steps=2',
         '--lineareval_while_pretraining=False']
_KEYS = {'eval/kmeans_nmi', 'eval/kmeans_ari', 'eval/kmeans_top_1_accuracy', 'kmeans/inertia', 'kmeans/iterations', 'kmeans/converged',
         'kmeans/empty_clusters', 'kmeans/restart', 'kmeans/k', 'global_step'}
_MATCHED = 'eval/kmeans_matched_accuracy'


def _check_files(model_dir, result, keys, restarts):
    for name in ('kmeans_result.json', 'kmeans_result_2.json'):
        saved = json.load(open(os.path.join(model_dir, name)))
        runs = saved.pop('restarts')
        assert set(saved) == keys and saved == {k: result[k] for k in keys}
        assert len(runs) == restarts and all(set(r) == {'inertia', 'iterations', 'converged', 'empty_clusters'} for r in runs)
        assert runs[result['kmeans/restart']]['inertia'] == result['kmeans/inertia'] == min(r['inertia'] for r in runs)
    assert result['global_step'] == 2 and 1 <= result['kmeans/iterations'] <= 50
    assert -1e-12 <= result['eval/kmeans_nmi'] <= 1.0 + 1e-12 and -1.0 <= result['eval/kmeans_ari'] <= 1.0
    assert 0.0 <= result['eval/kmeans_top_1_accuracy'] <= 1.0 and 0.0 <= result['kmeans/inertia'] <= 2.0


def test_run_main_on_synthetic_data(tmp_path):
    from simclr_amd import run
    from simclr_amd.flags import FLAGS
    model_dir = str(tmp_path / 'm')
    try:
        FLAGS.reset()
        result = run.main(_MAIN + ['--dataset=synthetic', '--eval_steps=2', '--model_dir=' + model_dir, '--kmeans_eval=True',
                                   '--kmeans_restarts=2', '--knn_eval=True', '--knn_k=5', '--logreg_eval=True', '--logreg_l2=1e-2'])
        kkeys = {k for k in result if 'kmeans' in k} | {'global_step'}
        assert kkeys == _KEYS | {_MATCHED} and result['kmeans/k'] == 10            # K = the class count: the matched key is there
        assert {'eval/knn_top_1_accuracy', 'eval/logreg_top_1_accuracy'} <= set(result)          # the union
        assert result[_MATCHED] >= result['eval/kmeans_top_1_accuracy'] - 1.0 and 0.0 <= result[_MATCHED] <= 1.0
        _check_files(model_dir, result, kkeys, 2)
        eval_args = [a for a in _MAIN if not a.startswith(('--mode', '--train_steps', '--checkpoint_steps'))] + [
            '--mode=eval', '--dataset=synthetic', '--eval_steps=2', '--model_dir=' + model_dir]
        FLAGS.reset()
        again = run.main(eval_args + ['--kmeans_eval=True', '--kmeans_restarts=2'])
        assert again == {k: result[k] for k in kkeys}                              # bitwise, on the second wiring path
        _check_files(model_dir, again, kkeys, 2)
        FLAGS.reset()
        seven = run.main(eval_args + ['--kmeans_eval=True', '--kmeans_k=7'])
        assert set(seven) == _KEYS and seven['kmeans/k'] == 7                      # K != num_classes: no matched key
        for name in ('kmeans_result.json', 'kmeans_result_2.json'):
            os.remove(os.path.join(model_dir, name))
        FLAGS.reset()
        plain = run.main(eval_args)
        assert not plain or not any('kmeans' in k for k in plain)
        assert not os.path.exists(os.path.join(model_dir, 'kmeans_result.json'))
        assert not os.path.exists(os.path.join(model_dir, 'kmeans_result_2.json'))
    finally:
        FLAGS.reset()


def test_run_main_on_a_dataset_with_padded_last_batches(tmp_path):
    from simclr_amd import data as data_lib
    from simclr_amd import kmeans, knn, run
    from simclr_amd.checkpoint import Checkpoint
    from simclr_amd.flags import FLAGS
    from simclr_amd.resnet import RT
    from simclr_amd import model as model_lib
    data_dir, model_dir, plain_dir = str(tmp_path / 'data'), str(tmp_path / 'm'), str(tmp_path / 'plain')
    make_dataset(data_dir)                                        # 103 train / 37 validation images, 10 classes
    try:
        FLAGS.reset()
        result = run.main(_MAIN + ['--dataset=waves', '--data_dir=' + data_dir, '--model_dir=' + model_dir, '--kmeans_eval=True',
                                   '--kmeans_k=7', '--kmeans_seed=3'])
        assert set(result) == _KEYS and result['kmeans/k'] == 7
        _check_files(model_dir, result, _KEYS, 1)
        assert not os.path.exists(os.path.join(model_dir, 'knn_result.json'))
        # the same clustering by hand from the restored model: the padded rows of both splits carry weight 0
        RT.reset()
        RT.device = torch.device(DEV, torch.cuda.current_device())
        model = model_lib.Model(10)
        model(torch.zeros(2, 32, 32, 3, device=DEV), training=False)
        model.release()
        Checkpoint(model=model).restore(os.path.join(model_dir, 'ckpt-2.pt'), model_only=False).expect_partial()
        builder = data_lib.ArrayDatasetBuilder('waves', data_dir)
        dev = torch.device(DEV, torch.cuda.current_device())
        x, lab, w = knn.extract_features(model, data_lib.DatasetIterator(builder.split('train'), 10, 16, False, device=dev))
        assert x.shape[0] == 112 and float(w.sum()) == 103
        fit = kmeans.fit(x, w, 7, 3, 1, FLAGS.kmeans_max_iterations, FLAGS.kmeans_tolerance)
        assert (fit.inertia, fit.iterations, fit.empty_clusters) == (result['kmeans/inertia'], result['kmeans/iterations'],
                                                                      result['kmeans/empty_clusters'])
        xq, qlab, qw = knn.extract_features(model, data_lib.DatasetIterator(builder.split('validation'), 10, 16, False, device=dev))
        bank = kmeans.contingency(kmeans.assign(x, w, fit.centroids)[0], lab, w, 7, 10)
        ev = kmeans.contingency(kmeans.assign(xq, qw, fit.centroids)[0], qlab, qw, 7, 10)
        assert int(bank.sum()) == 103 and int(ev.sum()) == 37
        s = kmeans.scores(bank, ev)
        assert all(result[k] == v for k, v in s.items()) and _MATCHED not in s
        # against the numpy restatement on the same features, where its gaps allow the comparison
        ref = km.fit64(x.cpu().numpy(), w.cpu().numpy(), 7, seed=3)
        if km.lloyd_gaps_ok(x.cpu().numpy(), w.cpu().numpy(), ref):
            assert ref['iterations'] == fit.iterations and abs(ref['J'] - fit.inertia) <= 512 * 2.0 ** -24
        FLAGS.reset()
        plain = run.main(_MAIN + ['--dataset=waves', '--data_dir=' + data_dir, '--model_dir=' + plain_dir])
        assert plain is None and not os.path.exists(os.path.join(plain_dir, 'kmeans_result.json'))
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
    return pos, np.where(pos < n, pos, 0), (pos < n).astype(np.float32)


def _kmeans_worker(rank, world, port, q):
    try:
        import torch.distributed as dist
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          SIMCLR_DIST_BACKEND='gloo', SIMCLR_SHARE_GPU='1')
        torch.cuda.set_device(0)
        dist.init_process_group('gloo', rank=rank, world_size=world)
        from simclr_amd import comm, kmeans
        from simclr_amd.resnet import RT
        RT.reset()
        RT.device = torch.device('cuda', 0)
        strategy = comm.Strategy()
        t = lambda a: torch.from_numpy(np.array(a)).to(RT.device)
        x, _, w = km.planted()
        pos, rows, keep = _shard(len(x), rank)
        assert np.array_equal(kmeans.shard_positions(len(pos), 16, strategy), pos)
        xs, ws = t(x[rows]), t(w[rows] * keep)
        c0 = t(x[km.start_rows(w, 8, 0, 0)])
        first = kmeans.lloyd(xs, ws, c0, 1, 1e-6, strategy)                       # one iteration: the first assignments
        two = kmeans.fit(xs, ws, 8, 0, 2, strategy=strategy, positions=pos)
        one = kmeans.fit(t(x), t(w), 8, 0, 2)
        torch.cuda.synchronize()
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, 'ok', dict(first=first[6].cpu().numpy(), rows=rows, keep=keep, J2=two.inertia, J1=one.inertia, it2=two.iterations,
                                it1=one.iterations, r2=two.restart, r1=one.restart, c2=two.centroids.cpu().numpy(),
                                c1=one.centroids.cpu().numpy(), Js2=two.inertias)))
    except Exception:  # noqa
        import traceback
        q.put((rank, 'FAIL', traceback.format_exc()))


def test_two_ranks_over_gloo_cluster_like_one_process():
    """Disjoint shards of the bank on two ranks, one all-reduce per iteration: both ranks hold the same bits, the start and the
    first-iteration assignments are exactly one process's, and the final J lies within the gate of one process's."""
    os.environ['SIMCLR_PEER_STATS'] = '0'
    try:
        ctx = mp.get_context('spawn')
        q = ctx.Queue()
        port = _free_port()
        procs = [ctx.Process(target=_kmeans_worker, args=(r, 2, port, q)) for r in range(2)]
        for p in procs:
            p.start()
        res = [q.get(timeout=300) for _ in procs]
        for p in procs:
            p.join(timeout=60)
    finally:
        os.environ.pop('SIMCLR_PEER_STATS', None)
    assert all(r[1] == 'ok' for r in res), res
    a, c = res[0][2], res[1][2]
    assert a['J2'] == c['J2'] and np.array_equal(a['c2'], c['c2']) and a['Js2'] == c['Js2'] and a['it2'] == c['it2']
    x, _, w = km.planted()
    want = km.assign64(x, x[km.start_rows(w, 8, 0, 0)])[0]
    prev = np.full(len(x), -1, np.int32)
    for m in (a, c):
        live = m['keep'] > 0
        assert np.array_equal(m['first'][live], want[m['rows']][live])
        jgate = km.gates(km.emulate(x, w, m['c1'], prev), km.direct(x, w, m['c1'], prev))['J']
        print('GLOO J two ranks %.17g one %.17g gate %.3e' % (m['J2'], m['J1'], jgate))
        assert abs(m['J2'] - m['J1']) <= jgate and m['it2'] == m['it1'] and m['r2'] == m['r1']
        assert np.abs(m['c2'] - m['c1']).max() <= km.ULP1
