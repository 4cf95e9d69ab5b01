"""The weighted k-NN evaluation on the device (pytest -m gpu): simclr_knn_topk / simclr_knn_vote against the float64 reference
tests/knn_reference.py, Model.features, run.main end to end and two replicas over gloo."""
import json
import multiprocessing as mp
import os
import socket

import numpy as np
import pytest
import torch

from tests import knn_reference as ref
from tests.data_fixtures import make_dataset

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _S():
    from simclr_amd import ops
    return ops.KNN_SLAB


def _topk(q, bank, k):
    from simclr_amd import ops
    v, i = ops.knn_topk(torch.from_numpy(np.ascontiguousarray(q, np.float32)).to(DEV),
                        torch.from_numpy(np.ascontiguousarray(bank, np.float32)).to(DEV), k)
    torch.cuda.synchronize()
    return v.cpu().numpy(), i.cpu().numpy()


def _lattice(rng, rows, D):
    return rng.integers(-2, 3, (rows, D)).astype(np.float32) / 4.0


def _unit_rows(rng, rows, D):
    x = rng.standard_normal((rows, D))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _check_exact(q, bank, k):
    val, idx = _topk(q, bank, k)
    want_val, want_idx = ref.topk(ref.similarities(q, bank), k)
    assert idx.dtype == np.int32 and val.dtype == np.float32
    assert np.array_equal(idx, want_idx), np.argwhere(idx != want_idx)[:4]
    assert np.array_equal(val.view(np.uint32), want_val.astype(np.float32).view(np.uint32))


# ------------------------------------------------------------------ 1. exact lattice, bitwise
# the whole grid of the kernel's edges: N as (multiples of S, offset) = k, S - 1 and the ragged three-slab 2 S + 77
LATTICE_CASES = [(Q, n, D, k) for Q in (1, 37, 130) for n in ((0, 0), (1, -1), (2, 77)) for D in (16, 128, 2048) for k in (1, 5, 200, 256)]


@pytest.mark.parametrize('Q,n_spec,D,k', LATTICE_CASES)
def test_topk_on_an_exact_lattice_is_bitwise_the_reference(Q, n_spec, D, k):
    """Entries in {-2 .. 2} / 4: every product and partial sum is exact in fp32 in any order and ties are plentiful, so indices and
    value bits must equal the float64 reference's."""
    N = n_spec[0] * _S() + n_spec[1] or k
    rng = np.random.default_rng([Q, N, D, k])
    _check_exact(_lattice(rng, Q, D), _lattice(rng, N, D), k)


def test_topk_repeated_bank_row_only_the_index_separates():
    rng = np.random.default_rng(5)
    S, D = _S(), 128
    bank = _lattice(rng, 2 * S + 77, D)
    bank[rng.choice(len(bank), 900, replace=False)] = np.sign(_lattice(rng, 1, D)) * 0.5     # one row, 900 copies across the three slabs
    q = _lattice(rng, 37, D)
    q[0] = bank[bank.shape[0] - 1]
    _check_exact(q, bank, 200)


@pytest.mark.parametrize('k', [200, 256])
def test_topk_bank_sorted_by_ascending_similarity(k):
    """The worst case of the streaming selection: every query is a positive multiple of one vector and the bank is sorted by ascending
    similarity to it, so every key of every tile beats the running k-th key and is appended -- 128 per tile to each of the lists, by
    all four waves -- and every list is cut as often as it can be.  No key may be lost."""
    rng = np.random.default_rng(k)
    S, D = _S(), 128
    u = rng.integers(-1, 2, (1, D)).astype(np.float32) / 2.0
    q = np.concatenate([u, u / 2.0] * 20)[:37]
    bank = _lattice(rng, 2 * S + 77, D)
    bank = bank[np.argsort(ref.similarities(u, bank)[0], kind='stable')]
    _check_exact(q, bank, k)


def test_topk_all_equal_similarities():
    S = _S()
    _check_exact(np.full((37, 16), 0.5, np.float32), np.full((2 * S + 77, 16), 0.25, np.float32), 256)
    _check_exact(np.zeros((3, 16), np.float32), _lattice(np.random.default_rng(1), S - 1, 16), 5)      # every similarity +0


# ------------------------------------------------------------------ 2. random unit rows
@pytest.mark.parametrize('Q,n_spec,D,k', [(64, (3, 5), 2048, 200), (64, (0, 1000), 128, 200)])
def test_topk_on_random_unit_rows(Q, n_spec, D, k):
    """eps = D * 2^-24: the first-order bound on an fp32 dot product of unit vectors (derived, not measured)."""
    N = n_spec[0] * _S() + n_spec[1]
    rng = np.random.default_rng([Q, N, D])
    q, bank = _unit_rows(rng, Q, D), _unit_rows(rng, N, D)
    eps = D * 2.0 ** -24
    val, idx = _topk(q, bank, k)
    sim = ref.similarities(q, bank)
    got = np.take_along_axis(sim, idx.astype(np.int64), 1)
    print('max |value - float64| = %.3e (eps %.3e)' % (np.abs(val - got).max(), eps))
    assert (idx >= 0).all() and (idx < N).all()
    assert np.abs(val - got).max() <= eps
    assert (np.diff(val, axis=1) <= 0).all()
    assert all(len(set(r.tolist())) == k for r in idx)
    left = sim.copy()
    np.put_along_axis(left, idx.astype(np.int64), -np.inf, 1)
    assert (left.max(1) <= val[:, -1].astype(np.float64) + 2 * eps).all()


# ------------------------------------------------------------------ 3 + 4. position independence, repeatability
def _host_merge(parts, k):
    """parts: [(val [Q, k'], global idx [Q, k'])] -> the first k of (value descending, index ascending) per row, on the fp32 values."""
    val = np.concatenate([p[0] for p in parts], 1)
    idx = np.concatenate([p[1] for p in parts], 1)
    o = np.stack([np.lexsort((idx[i], -val[i].astype(np.float64)))[:k] for i in range(len(val))])
    return np.take_along_axis(val, o, 1), np.take_along_axis(idx, o, 1)


def test_topk_does_not_depend_on_position_and_repeats_bitwise():
    S, D, k, Q = _S(), 128, 200, 70
    rng = np.random.default_rng(11)
    q, bank = _unit_rows(rng, Q, D), _unit_rows(rng, 2 * S + 77, D)
    bank[5000] = bank[17]                                     # equal similarities in different slabs
    val, idx = _topk(q, bank, k)
    val2, idx2 = _topk(q, bank, k)
    assert np.array_equal(idx, idx2) and np.array_equal(val.view(np.uint32), val2.view(np.uint32))          # repeatable
    h = S + 333                                               # the halves cut a slab and a tile at other places than the whole bank does
    a, b = _topk(q, bank[:h], k), _topk(q, bank[h:], k)
    mval, midx = _host_merge([a, (b[0], b[1] + h)], k)
    assert np.array_equal(midx, idx) and np.array_equal(mval.view(np.uint32), val.view(np.uint32))
    qa, qb = _topk(q[:33], bank, k), _topk(q[33:], bank, k)
    assert np.array_equal(np.concatenate([qa[1], qb[1]]), idx)
    assert np.array_equal(np.concatenate([qa[0], qb[0]]).view(np.uint32), val.view(np.uint32))


# ------------------------------------------------------------------ 5. the vote
def _vote(top_val, top_label, C, T):
    from simclr_amd import ops
    p, s = ops.knn_vote(torch.from_numpy(np.ascontiguousarray(top_val, np.float32)).to(DEV),
                        torch.from_numpy(np.ascontiguousarray(top_label, np.int32)).to(DEV), C, T)
    torch.cuda.synchronize()
    return p.cpu().numpy(), s.cpu().numpy()


@pytest.mark.parametrize('C', [3, 10, 1000])
def test_vote_on_equal_similarities_is_exact_and_ties_go_to_the_lower_class(C):
    """All similarities equal: every exponent argument is 0 ln 2, every weight exactly 1, the scores are neighbour counts -- exact in
    fp32 and full of ties, which the class id must break."""
    rng = np.random.default_rng(C)
    Q, k = 64, 200 if C > 3 else 7
    v = np.full((Q, k), 0.625, np.float32)
    lab = rng.integers(0, C, (Q, k))
    pred, score = _vote(v, lab, C, 0.0901)
    want_p, want_s = ref.vote(v, lab, C, 0.0901)
    assert np.array_equal(pred, want_p) and np.array_equal(score, want_s.astype(np.float32))
    ties = (want_s[:, :-1] == want_s[:, 1:]) & (want_p[:, 1:] >= 0)
    assert ties.sum() > Q // 4 and (want_p[:, :-1][ties] < want_p[:, 1:][ties]).all()
    if C == 3:
        assert (pred[:, 3:] == -1).all() and (score[:, 3:] == 0).all()


@pytest.mark.parametrize('C', [3, 10])
def test_vote_on_lattice_similarities_predicts_exactly(C):
    """Similarities on a 1/16 grid and T = fp32(1 / (16 ln 2)): every exponent argument is an integer multiple of ln 2 as far as fp32
    holds it, every weight 2^-n up to the rounding of expf.  The seed is chosen on the reference alone so that in EVERY row the float64
    scores of ranks 1 .. 6 are pairwise more than 1e-4 relative apart (asserted): all five predictions of all rows must then be exact."""
    rng = np.random.default_rng([C, 1, 0])
    Q, k = 64, 200
    T = float(np.float32(1.0 / (16.0 * np.log(2.0))))
    v = -np.sort(-rng.integers(0, 12, (Q, k)), axis=1).astype(np.float32) / 16.0
    lab = rng.integers(0, C, (Q, k))
    scores = ref.class_scores(v, lab, C, T)
    top = -np.sort(-scores, axis=1)[:, :6]
    assert ((top[:, :-1] - top[:, 1:]) > 1e-4 * np.abs(top[:, :-1])).all()
    want_p, want_s = ref.top5(scores)
    pred, score = _vote(v, lab, C, T)
    assert np.array_equal(pred, want_p)
    n = min(C, 5)
    assert (np.abs(score[:, :n] - want_s[:, :n]) <= 1e-5 * want_s[:, :n]).all()


@pytest.mark.parametrize('C,lattice', [(3, False), (10, False), (1000, False), (10, True)])
def test_vote_scores_and_predictions_match_float64(C, lattice):
    """Scores within 1e-5 relative of float64 (the 200 weights span at most exp(2 / 0.07): no cancellation); classes compared on the
    rows whose float64 margin (rank 1 over 2; rank 5 over 6 for the top-5 set) exceeds 1e-4 relative -- at most 5 % are left out,
    which the seeds below satisfy on the reference alone.  lattice: similarities on a 1/16 grid and T = 1 / (16 ln 2), so that every
    exponent argument is an integer multiple of ln 2 (as far as fp32 holds ln 2)."""
    rng = np.random.default_rng([C, int(lattice)])
    Q, k = 256, 200
    if lattice:
        T = float(np.float32(1.0 / (16.0 * np.log(2.0))))
        v = -np.sort(-rng.integers(0, 12, (Q, k)), axis=1).astype(np.float32) / 16.0
    else:
        T = 0.07
        v = -np.sort(-rng.uniform(0.2, 0.9, (Q, k)), axis=1).astype(np.float32)
    lab = rng.integers(0, C, (Q, k))
    scores = ref.class_scores(v, lab, C, T)
    want_p, want_s = ref.top5(scores)
    d1, d5 = ref.decided_rows(scores)
    assert d1.mean() >= 0.95 and d5.mean() >= 0.95
    pred, score = _vote(v, lab, C, T)
    n = min(C, 5)
    got_ref = np.take_along_axis(scores, pred[:, :n].astype(np.int64), 1)
    rel = np.abs(score[:, :n] - got_ref) / got_ref
    print('max relative score error %.3e' % rel.max())
    assert rel.max() <= 1e-5
    assert np.array_equal(pred[d1, 0], want_p[d1, 0])
    assert all(set(a.tolist()) == set(b.tolist()) for a, b in zip(pred[d5], want_p[d5]))
    assert (np.diff(score[:, :n], axis=1) <= 0).all()


# ------------------------------------------------------------------ 6. knn_predict
def test_knn_predict_of_the_bank_on_itself_finds_every_label():
    from simclr_amd import knn
    rng = np.random.default_rng(3)
    bank = torch.from_numpy(_unit_rows(rng, 512, 64)).to(DEV)
    labels = torch.from_numpy(rng.integers(0, 10, 512)).to(DEV)
    pred5, score5 = knn.knn_predict(bank, bank, labels, 10, k=1)
    assert torch.equal(pred5[:, 0].long(), labels)
    assert torch.equal(score5[:, 0], torch.ones(512, device=DEV)) and bool((score5[:, 1:] == 0).all())


# ------------------------------------------------------------------ 7. refusals
def test_refusals_on_device_tensors():
    import ctypes
    from simclr_amd import _lib, ops
    q, bank = torch.zeros(4, 32, device=DEV), torch.zeros(10, 32, device=DEV)
    L = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    out_v, out_i = torch.zeros(4, 8, device=DEV), torch.zeros(4, 8, device=DEV, dtype=torch.int32)
    ws = torch.zeros(1024, device=DEV)
    for k, N, D, match in ((0, 10, 32, 'k must be'), (257, 10, 32, 'k must be'), (8, 7, 32, 'fewer than k'), (8, 10, 24, 'multiple of 16')):
        with pytest.raises(_lib.SimclrHipError, match=match):
            L.knn_topk(p(q), p(bank), 4, N, D, k, p(out_v), p(out_i), p(ws), None)
    for args in ((None, p(bank), p(out_v), p(out_i), p(ws)), (p(q), None, p(out_v), p(out_i), p(ws)), (p(q), p(bank), None, p(out_i), p(ws)),
                 (p(q), p(bank), p(out_v), None, p(ws)), (p(q), p(bank), p(out_v), p(out_i), None)):
        with pytest.raises(_lib.SimclrHipError, match='null argument'):
            L.knn_topk(args[0], args[1], 4, 10, 32, 8, args[2], args[3], args[4], None)
    lab, pr, sc = torch.zeros(4, 8, device=DEV, dtype=torch.int32), torch.zeros(4, 5, device=DEV, dtype=torch.int32), torch.zeros(4, 5, device=DEV)
    for c in (0, 40000):
        with pytest.raises(_lib.SimclrHipError, match='num_classes must be'):
            L.knn_vote(p(out_v), p(lab), 4, 8, c, 0.07, p(pr), p(sc), None)
        with pytest.raises(ValueError, match='num_classes'):
            ops.knn_vote(out_v, lab, c, 0.07)
    with pytest.raises(_lib.SimclrHipError, match='null argument'):
        L.knn_vote(p(out_v), p(lab), 4, 8, 10, 0.07, None, p(sc), None)
    for k in (0, 257, 11):
        with pytest.raises(ValueError, match='knn_topk'):
            ops.knn_topk(q, bank, k)
    with pytest.raises(ValueError, match='multiple of 16'):
        ops.knn_topk(torch.zeros(4, 24, device=DEV), torch.zeros(10, 24, device=DEV), 2)
    pr2, _ = ops.knn_vote(out_v, lab, 32768, 0.07)               # the largest class count runs
    torch.cuda.synchronize()
    assert pr2.cpu().tolist() == [[0, 1, 2, 3, 4]] * 4


# ------------------------------------------------------------------ 8. Model.features
def _pretrain_flags(**kw):
    from simclr_amd.flags import FLAGS
    FLAGS.reset()
    FLAGS.update(resnet_depth=18, image_size=32, compute_dtype='f32', f32_matmul='exact', use_blur=False, train_batch_size=8,
                 train_mode='pretrain', lineareval_while_pretraining=True, **kw)
    return FLAGS


def _fresh_model(num_classes=10):
    from simclr_amd import model as model_lib
    from simclr_amd.resnet import RT
    RT.reset()
    RT.device = torch.device(DEV, torch.cuda.current_device())
    model = model_lib.Model(num_classes)
    model(torch.zeros(2, 32, 32, 3, device=DEV), training=False)          # builds the variables (inference: nothing moves)
    model.release()
    return model


def test_features_are_the_encoder_output_the_heads_read():
    FLAGS = _pretrain_flags()
    try:
        model = _fresh_model()
        x = torch.rand(8, 32, 32, 3, generator=torch.Generator().manual_seed(4)).to(DEV)
        model(x, training=False)
        want = model.resnet_model.endpoints['final_avg_pool'].float().clone()
        model.release()
        state = [v.value.clone() for v in model.variables]
        got = model.features(x)
        assert got.dtype == torch.float32 and tuple(got.shape) == (8, 512) and torch.equal(got, want)
        assert float(got.abs().sum()) > 0
        assert all(torch.equal(a, v.value) for a, v in zip(state, model.variables))       # no variable, no moving statistic moved
        assert model.resnet_model._final is None and not model.resnet_model.endpoints       # no activation is kept
        with pytest.raises(ValueError, match='single-view'):
            model.features(torch.zeros(8, 32, 32, 6, device=DEV))
    finally:
        FLAGS.reset()


def _two_steps(call_features):
    from simclr_amd import model as model_lib
    from simclr_amd.run import make_single_step, synthetic_batches
    model = _fresh_model()
    step = make_single_step(model, model_lib.build_optimizer(0.1), None)
    data = synthetic_batches(8, 32, 10, torch.device(DEV), seed=9)
    x, lab = next(data)
    step(x, lab)
    if call_features:
        model.features(torch.rand(8, 32, 32, 3, generator=torch.Generator().manual_seed(5)).to(DEV))
    x, lab = next(data)
    step(x, lab)
    torch.cuda.synchronize()
    return ([v.value.clone() for v in model.variables], model._flat_grads.clone(),
            {k: float(m.result()) for k, m in step.metrics.items()})


def test_features_between_two_training_steps_change_nothing():
    FLAGS = _pretrain_flags()
    try:
        v0, g0, m0 = _two_steps(False)
        v1, g1, m1 = _two_steps(True)
        assert torch.equal(g0, g1)
        # the reported scalars of the NT-Xent kernels (fixed-order reductions).  The supervised-loss, weight-decay and total-loss
        # SCALARS are sums of float atomics over workgroups (csrc/pool.hip) and differ in the last bit between any two runs; no
        # gradient or variable reads them.
        for name in ('train/contrast_loss', 'train/contrast_acc', 'train/contrast_entropy'):
            assert m0[name] == m1[name], name
        # those scalars: each is a sum of per-workgroup terms (at most 64 at this size) added atomically in any order, so two runs
        # differ by at most 64 * 2^-24 = 2^-18 relative, whatever happens between the steps
        assert set(m0) == set(m1)
        for name in m0:
            assert abs(m0[name] - m1[name]) <= 2.0 ** -18 * abs(m0[name]), (name, m0[name], m1[name])
        assert len(v0) == len(v1) and all(torch.equal(a, b) for a, b in zip(v0, v1))
    finally:
        FLAGS.reset()


# ------------------------------------------------------------------ 9. end to end
_MAIN = ['--dataset=waves', '--resnet_depth=18', '--image_size=32', '--train_batch_size=16', '--eval_batch_size=16', '--use_blur=False',
         '--compute_dtype=f32', '--f32_matmul=exact', '--mode=train_then_eval', '--train_steps=2', '--checkpoint_steps=2',
         '--lineareval_while_pretraining=False']


def test_run_main_writes_the_knn_result(tmp_path):
    from simclr_amd import data as data_lib
    from simclr_amd import knn, run
    from simclr_amd.checkpoint import Checkpoint
    from simclr_amd.flags import FLAGS
    data_dir, model_dir, plain_dir = str(tmp_path / 'data'), str(tmp_path / 'm'), str(tmp_path / 'plain')
    make_dataset(data_dir)                                        # 103 train / 37 validation images, 10 classes
    try:
        FLAGS.reset()
        result = run.main(_MAIN + ['--data_dir=' + data_dir, '--model_dir=' + model_dir, '--knn_eval=True', '--knn_k=5'])
        assert set(result) == {'eval/knn_top_1_accuracy', 'eval/knn_top_5_accuracy', 'global_step'} and result['global_step'] == 2
        for name in ('knn_result.json', 'knn_result_2.json'):
            assert json.load(open(os.path.join(model_dir, name))) == {k: float(v) for k, v in result.items()}
        # the same features through extract_features of the restored model
        model = _fresh_model()
        Checkpoint(model=model).restore(os.path.join(model_dir, 'ckpt-2.pt'), model_only=False).expect_partial()
        builder = data_lib.ArrayDatasetBuilder('waves', data_dir)
        dev = torch.device(DEV, torch.cuda.current_device())
        bank, bank_lab, bank_w = knn.extract_features(model, data_lib.DatasetIterator(builder.split('train'), 10, 16, False, device=dev))
        qf, q_lab, q_w = knn.extract_features(model, data_lib.DatasetIterator(builder.split('validation'), 10, 16, False, device=dev))
        assert bank.shape[0] == 112 and float(bank_w.sum()) == 103 and qf.shape[0] == 48 and float(q_w.sum()) == 37     # padded batches
        torch.testing.assert_close(bank.norm(dim=1), torch.ones(112, device=DEV), rtol=1e-5, atol=0)
        keep = bank_w > 0
        bank, bank_lab = bank[keep].contiguous(), bank_lab[keep]
        counts = knn.knn_hit_counts(qf, q_lab, q_w, bank, bank_lab, 10, 5, FLAGS.knn_temperature).cpu().numpy()
        assert counts[2] == 37                                    # the padded last eval batch counts each of the 37 examples once
        assert result['eval/knn_top_1_accuracy'] == counts[0] / 37 and result['eval/knn_top_5_accuracy'] == counts[1] / 37
        # the float64 reference on those features; a row inside the 1e-4 margin may fall either way
        w = q_w.cpu().numpy() > 0
        qn, bn = qf.cpu().numpy()[w], bank.cpu().numpy()
        val, idx = ref.topk(ref.similarities(qn, bn), 5)
        scores = ref.class_scores(val, bank_lab.cpu().numpy()[idx], 10, FLAGS.knn_temperature)
        want_p, _ = ref.top5(scores)
        d1, d5 = ref.decided_rows(scores)
        hit = want_p == q_lab.cpu().numpy()[w].reshape(-1, 1)
        lo1, lo5 = int((hit[:, 0] & d1).sum()), int((hit.any(1) & d5).sum())
        print('reference hits %d / %d of 37, undecided rows %d / %d' % (hit[:, 0].sum(), hit.any(1).sum(), (~d1).sum(), (~d5).sum()))
        assert lo1 <= counts[0] <= lo1 + int((~d1).sum()) and lo5 <= counts[1] <= lo5 + int((~d5).sum())
        # the flag off: no k-NN result
        FLAGS.reset()
        plain = run.main(_MAIN + ['--data_dir=' + data_dir, '--model_dir=' + plain_dir])
        assert plain is None and not os.path.exists(os.path.join(plain_dir, 'knn_result.json'))
        assert os.path.exists(os.path.join(plain_dir, 'ckpt-2.pt'))
    finally:
        FLAGS.reset()


# ------------------------------------------------------------------ 10. two replicas over gloo on one GPU
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _shard_case():
    """Bank of 300 and 90 queries (unit rows, D = 64, 10 classes) and their eval-style shards: global batch 32, 16 rows per replica
    and step, positions past the end are row 0 with weight 0."""
    rng = np.random.default_rng(21)
    bank, q = _unit_rows(rng, 300, 64), _unit_rows(rng, 90, 64)
    return bank, rng.integers(0, 10, 300), q, rng.integers(0, 10, 90)


def _shard(rows, labels, rank, world=2, B=32):
    n, b = len(rows), B // world
    steps = -(-n // B)
    pos = (np.arange(steps)[:, None] * B + rank * b + np.arange(b)[None, :]).reshape(-1)
    w = (pos < n).astype(np.float32)
    pos = np.where(pos < n, pos, 0)
    return rows[pos], labels[pos], w


def _knn_worker(rank, world, port, q):
    try:
        import torch.distributed as dist
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          SIMCLR_DIST_BACKEND='gloo', SIMCLR_SHARE_GPU='1')
        torch.cuda.set_device(0)
        dist.init_process_group('gloo', rank=rank, world_size=world)
        from simclr_amd import comm, knn
        from simclr_amd.resnet import RT
        RT.reset()
        RT.device = torch.device('cuda', 0)
        strategy = comm.Strategy()
        bank, bank_lab, qs, q_lab = _shard_case()
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(RT.device)
        f, l, w = _shard(bank, bank_lab, rank)
        g_bank, g_lab = knn.gather_bank(t(f), t(l), t(w), strategy, batch=16)
        same_bank = bool(torch.equal(g_bank, t(bank)) and torch.equal(g_lab, t(bank_lab)))
        f, l, w = _shard(qs, q_lab, rank)
        mine = knn.knn_hit_counts(t(f), t(l), t(w), g_bank, g_lab, 10, 20, 0.07)
        total = knn.reduce_hit_counts(mine.clone(), strategy)
        single = knn.knn_hit_counts(t(qs), t(q_lab), torch.ones(90, device=RT.device), t(bank), t(bank_lab), 10, 20, 0.07)
        torch.cuda.synchronize()
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, 'ok', dict(same_bank=same_bank, mine=mine.cpu().tolist(), total=total.cpu().tolist(), single=single.cpu().tolist())))
    except Exception:  # noqa
        import traceback
        q.put((rank, 'FAIL', traceback.format_exc()))


def test_two_ranks_over_gloo_count_the_hits_of_one_process():
    """Given features sharded as bank and queries over two ranks through gather_bank / knn_hit_counts / reduce_hit_counts: the gathered
    bank is the whole bank in split order without the padding, and the summed hit counts are exactly the single-process counts
    (position independence of the similarities)."""
    os.environ['SIMCLR_PEER_STATS'] = '0'
    try:
        ctx = mp.get_context('spawn')
        q = ctx.Queue()
        port = _free_port()
        procs = [ctx.Process(target=_knn_worker, args=(r, 2, port, q)) for r in range(2)]
        for p in procs:
            p.start()
        res = [q.get(timeout=300) for _ in procs]
        for p in procs:
            p.join(timeout=60)
    finally:
        os.environ.pop('SIMCLR_PEER_STATS', None)
    assert all(r[1] == 'ok' for r in res), res
    for _, _, m in res:
        assert m['same_bank'] and m['total'] == m['single'] and m['single'][2] == 90.0, m
        assert 0 < m['single'][0] <= m['single'][1] <= 90
    assert sorted(m['mine'][2] for _, _, m in res) == [42.0, 48.0]           # 16 + 16 + 10 and 16 + 16 + 16 of the 90
