"""The weighted k-NN evaluation without a device: hand cases of the float64 reference (tests/knn_reference.py), the flag checks of
run.check_knn_flags, the bank selection of --knn_bank_examples and the argument checks of the ops wrappers / the C ABI."""
import ctypes

import numpy as np
import pytest
import torch

from tests import knn_reference as ref


def test_all_tied_similarities_order_by_bank_index():
    q = np.ones((2, 4))
    bank = np.ones((7, 4))
    val, idx = ref.topk(ref.similarities(q, bank), 3)
    assert idx.tolist() == [[0, 1, 2], [0, 1, 2]] and (val == 4.0).all()


def test_k_equal_n_is_a_full_sort_and_nan_sorts_last():
    sim = np.array([[0.5, np.nan, 0.75, 0.5, -1.0]])
    val, idx = ref.topk(sim, 5)
    assert idx.tolist() == [[2, 0, 3, 4, 1]]
    assert val[0, :4].tolist() == [0.75, 0.5, 0.5, -1.0] and np.isnan(val[0, 4])


def test_vote_by_hand_absent_class_and_tie_rule():
    # three neighbours: similarities 1, 1 - T ln 2, 1 - T ln 2 -> weights 1, 1/2, 1/2; classes 4, 2, 2 -> score 1 each: class 2 first
    T = 0.5
    v = np.array([[1.0, 1.0 - T * np.log(2.0), 1.0 - T * np.log(2.0)]])
    scores = ref.class_scores(v, np.array([[4, 2, 2]]), 6, T)
    np.testing.assert_allclose(scores[0], [0, 0, 1, 0, 1, 0], atol=1e-15)
    scores[0, 2] = scores[0, 4] = 1.0                            # the exact tie
    pred, sc = ref.top5(scores)
    assert pred.tolist() == [[2, 4, 0, 1, 3]]                    # absent classes score 0 and follow in class order; class 5 is left out
    assert sc.tolist() == [[1.0, 1.0, 0.0, 0.0, 0.0]]


def test_fewer_than_five_classes_pad_with_minus_one():
    pred, sc = ref.vote(np.array([[0.9, 0.8]]), np.array([[1, 1]]), 3, 0.07)
    assert pred.tolist() == [[1, 0, 2, -1, -1]]
    assert sc[0, 1:].tolist() == [0.0, 0.0, 0.0, 0.0] and sc[0, 0] == pytest.approx(1.0 + np.exp(-0.1 / 0.07))


def test_scores_add_in_rank_order():
    """The accumulation order is part of the definition: in float64 the rank-order sum of the reference equals a left-to-right sum."""
    rng = np.random.default_rng(0)
    v = -np.sort(-rng.uniform(0.2, 0.9, (3, 50)), axis=1)
    lab = np.zeros((3, 50), np.int64)
    s = ref.class_scores(v, lab, 2, 0.07)
    for i in range(3):
        acc = 0.0
        for r in range(50):
            acc += np.exp((v[i, r] - v[i, 0]) / 0.07)
        assert s[i, 0] == acc and s[i, 1] == 0.0


def test_hit_counts_weigh_the_padding_out():
    pred5 = np.array([[1, 2, 3, 4, 5], [0, 9, 8, 7, 6], [3, 1, 0, 2, 4]])
    assert ref.hit_counts(pred5, [1, 6, 0], [1, 1, 0]).tolist() == [1.0, 2.0, 2.0]


@pytest.fixture
def flags():
    from simclr_amd.flags import FLAGS
    FLAGS.reset()
    yield FLAGS
    FLAGS.reset()


def test_knn_flags_default_off(flags):
    from simclr_amd import run
    assert flags.knn_eval is False and flags.knn_k == 200 and flags.knn_temperature == 0.07 and flags.knn_bank_examples == 0
    flags.update(knn_k=0)                      # the flag is off: nothing is checked, nothing runs
    assert run.check_knn_flags(100) is None


@pytest.mark.parametrize('update,n,match', [
    (dict(knn_k=0), 1000, 'knn_k'), (dict(knn_k=257), 1000, 'knn_k'), (dict(knn_temperature=0.0), 1000, 'knn_temperature'),
    (dict(knn_temperature=-1.0), 1000, 'knn_temperature'), (dict(knn_k=200), 150, 'fewer than'),
    (dict(knn_k=50, knn_bank_examples=40), 1000, 'fewer than'), (dict(knn_bank_examples=2000), 1000, 'exceeds'),
    (dict(knn_bank_examples=-1), 1000, 'knn_bank_examples')])
def test_knn_flag_checks_raise(flags, update, n, match):
    from simclr_amd import run
    flags.update(knn_eval=True, **update)
    with pytest.raises(ValueError, match=match):
        run.check_knn_flags(n)


def test_knn_flag_checks_pass_and_size_the_bank(flags):
    from simclr_amd import run
    flags.update(knn_eval=True)
    assert run.check_knn_flags(1281167) == 1281167
    flags.update(knn_bank_examples=5000)
    assert run.check_knn_flags(1281167) == 5000 and run.check_knn_flags() == 5000


def test_main_refuses_bad_knn_flags_before_device_work(flags, monkeypatch):
    from simclr_amd import run

    def no_device(*a, **k):
        raise AssertionError('device work before the flag check')
    monkeypatch.setattr(run, 'init_distributed', no_device)
    for bad in ('--knn_k=300', '--knn_temperature=0', '--knn_bank_examples=7'):
        with pytest.raises(ValueError, match='knn'):
            run.main(['--knn_eval=True', '--mode=eval', '--image_size=32', bad])
        flags.reset()


def test_bank_examples_select_a_prefix_of_the_epoch_permutation():
    from simclr_amd import knn
    from simclr_amd.data import epoch_permutation
    assert knn.knn_bank_indices(3, 50, 0).tolist() == list(range(50))
    sel = knn.knn_bank_indices(3, 50, 20)
    assert sel.tolist() == epoch_permutation(3, 0, 50)[:20].tolist() and len(set(sel.tolist())) == 20
    assert knn.knn_bank_indices(3, 50, 30)[:20].tolist() == sel.tolist()          # a larger bank extends a smaller one
    assert knn.knn_bank_indices(4, 50, 20).tolist() != sel.tolist()
    with pytest.raises(ValueError, match='exceeds'):
        knn.knn_bank_indices(3, 50, 51)


def test_ops_wrappers_refuse_before_the_call():
    from simclr_amd import ops
    q, bank = torch.zeros(4, 32), torch.zeros(10, 32)                              # host tensors: a refusal comes before any pointer is taken
    for k in (0, 257, 11):
        with pytest.raises(ValueError, match='knn_topk'):
            ops.knn_topk(q, bank, k)
    with pytest.raises(ValueError, match='multiple of 16'):
        ops.knn_topk(torch.zeros(4, 24), torch.zeros(10, 24), 2)
    with pytest.raises(ValueError, match='fp32'):
        ops.knn_topk(q.double(), bank.double(), 2)
    v, l = torch.zeros(4, 5), torch.zeros(4, 5, dtype=torch.int32)
    for c in (0, 40000):
        with pytest.raises(ValueError, match='num_classes'):
            ops.knn_vote(v, l, c, 0.07)
    with pytest.raises(ValueError, match='temperature'):
        ops.knn_vote(v, l, 10, 0.0)
    with pytest.raises(ValueError, match='int32'):
        ops.knn_vote(v, l.long(), 10, 0.07)


def test_c_abi_refuses_with_messages():
    from simclr_amd import _lib, ops
    L = _lib.lib()
    assert L.knn_slab_rows() == ops.KNN_SLAB
    fake = ctypes.c_void_p(1 << 20)                                                # never dereferenced: every call below is refused
    for k, N, D, match in ((0, 100, 32, 'k must be'), (257, 1000, 32, 'k must be'), (8, 7, 32, 'fewer than k'), (8, 100, 24, 'multiple of 16')):
        with pytest.raises(_lib.SimclrHipError, match=match):
            L.knn_topk(fake, fake, 4, N, D, k, fake, fake, fake, None)
        assert L.knn_workspace_bytes(4, N, D, k) == 0
    with pytest.raises(_lib.SimclrHipError, match='null argument'):
        L.knn_topk(None, fake, 4, 100, 32, 8, fake, fake, fake, None)
    with pytest.raises(_lib.SimclrHipError, match='null argument'):
        L.knn_topk(fake, fake, 4, 100, 32, 8, fake, fake, None, None)
    for c in (0, 40000):
        with pytest.raises(_lib.SimclrHipError, match='num_classes must be'):
            L.knn_vote(fake, fake, 4, 8, c, 0.07, fake, fake, None)
    with pytest.raises(_lib.SimclrHipError, match='null argument'):
        L.knn_vote(fake, None, 4, 8, 10, 0.07, fake, fake, None)
    # linear in Q * k * slabs
    assert L.knn_workspace_bytes(256, 1281167, 2048, 200) == 256 * 200 * 8 * -(-1281167 // ops.KNN_SLAB)
