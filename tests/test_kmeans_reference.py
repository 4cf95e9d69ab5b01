"""The k-means clustering evaluation without a device: the float64 restatement (tests/kmeans_reference.py) against sklearn and the
hand cases of tests/golden/KMEANS_HAND_DERIVED.md, the identities of the loop and of sharding, the emulation's error budget, the mutants,
and the host side of the feature (flags, refusals, the C boundary).

Without the feature the identity, hand-case, budget and mutant tests still pass (they check the restatement); the flag, refusal, score
and C-boundary tests fail."""
import itertools

import numpy as np
import pytest
import torch

from tests import kmeans_reference as km


# ---- scores ----------------------------------------------------------------------------------------------------------------------------
def _random_tables():
    rng = np.random.RandomState(3)
    for K, C in [(2, 2), (3, 5), (5, 3), (4, 4), (7, 2)]:
        yield rng.randint(0, 6, (K, C)) + np.eye(K, C, dtype=np.int64)


def _labels_of(T):
    a = [k for k in range(T.shape[0]) for c in range(T.shape[1]) for _ in range(T[k, c])]
    y = [c for k in range(T.shape[0]) for c in range(T.shape[1]) for _ in range(T[k, c])]
    return np.array(a), np.array(y)


def test_nmi_and_ari_match_sklearn():
    metrics = pytest.importorskip('sklearn.metrics')
    from simclr_amd import kmeans
    for T in _random_tables():
        a, y = _labels_of(T)
        want_nmi = metrics.normalized_mutual_info_score(y, a, average_method='arithmetic')
        want_ari = metrics.adjusted_rand_score(y, a)
        for mod in (km, kmeans):
            assert abs(mod.nmi(T) - want_nmi) <= 1e-12 and abs(mod.ari(T) - want_ari) <= 1e-12, (mod, T)


def test_hand_cases_of_the_golden_note():
    from simclr_amd import kmeans
    for mod in (km, kmeans):
        ident = np.diag([3, 2, 4])
        assert abs(mod.nmi(ident) - 1.0) <= 1e-15 and mod.ari(ident) == 1.0
        indep = np.array([[1, 1], [1, 1]])
        # independent 2 x 2 with m rows per cell: MI = 0 exactly; the ARI of a FINITE independent table is -1 / (2 (2 m - 1)), not 0 (its
        # expectation is taken over random tables with these margins): -1/2 at m = 1, -1/18 at m = 5, -> 0 as m grows
        assert abs(mod.nmi(indep)) <= 1e-14 and abs(mod.ari(indep) + 0.5) <= 1e-15
        for m in (5, 50, 50000):
            big = np.full((2, 2), m)
            assert abs(mod.nmi(big)) <= 1e-14 and abs(mod.ari(big) + 1.0 / (2 * (2 * m - 1))) <= 1e-15
        assert abs(mod.ari(np.full((2, 2), 50000))) <= 1e-5
        single = np.array([[4, 3, 2]])                                     # one cluster against three classes
        assert mod.nmi(single) == 0.0 and mod.ari(single) == 0.0
        assert mod.nmi(np.array([[9]])) == 1.0 and mod.ari(np.array([[9]])) == 1.0        # both partitions a single block
        T = np.array([[4, 1, 0], [0, 3, 2], [1, 0, 5]])
        for p in itertools.permutations(range(3)):
            assert abs(mod.nmi(T[list(p)]) - mod.nmi(T)) <= 1e-15 and abs(mod.ari(T[list(p)]) - mod.ari(T)) <= 1e-15


def test_many_to_one_accuracy_with_a_tie_and_an_absent_cluster():
    from simclr_amd import kmeans
    bank = np.array([[3, 3, 0], [0, 0, 0], [0, 1, 4]])       # cluster 0: a tie -> class 0; cluster 1: absent from the bank
    ev = np.array([[2, 5, 0], [1, 1, 1], [0, 0, 3]])         # hits: 2 (cluster 0 -> class 0) + 0 + 3 = 5 of 13
    assert km.many_to_one(bank, ev) == 5 / 13 and kmeans.many_to_one_accuracy(bank, ev) == 5 / 13
    out = kmeans.scores(bank, ev)
    assert out['eval/kmeans_top_1_accuracy'] == 5 / 13 and set(out) >= {'eval/kmeans_nmi', 'eval/kmeans_ari'}
    assert kmeans.MATCHED_KEY not in kmeans.scores(bank[:2], ev[:2])       # K != num_classes: the key is absent


def test_matched_accuracy_against_brute_force():
    pytest.importorskip('scipy.optimize')
    from simclr_amd import kmeans
    rng = np.random.RandomState(5)
    for K in (2, 3, 4, 5):
        for _ in range(4):
            E = rng.randint(0, 9, (K, K))
            E[0, 0] += 1
            assert kmeans.matched_accuracy(E) == km.matched_brute(E)
            assert kmeans.scores(E, E)[kmeans.MATCHED_KEY] == km.matched_brute(E)
    assert kmeans.matched_accuracy(np.ones((2, 3), np.int64)) is None


# ---- loop and sharding -----------------------------------------------------------------------------------------------------------------
def test_objective_never_rises_over_the_reference_iterations():
    x, _, w = km.planted()
    for K in (8, 12, 3):
        run = km.lloyd64(x, w, x[km.start_rows(w, K, 0, 0)], 50, 0.0)
        assert all(b <= a + 1e-15 for a, b in zip(run['Js'], run['Js'][1:])), run['Js']
        assert run['converged']


def test_cancelling_and_memberless_clusters_keep_their_centroid():
    e = np.eye(64, dtype=np.float32)
    x = np.stack([e[0], -e[0], e[1]])                    # rows 0 and 1 cancel in cluster 0
    w = np.ones(3, np.float32)
    c = np.stack([e[5], e[1], e[7]])
    sums, wsum = km.update64(x, w, np.array([0, 0, 1]), 3)
    c_new, kept, _ = km.finish64(sums, wsum, c)
    assert kept == 2 and np.array_equal(c_new[0], c[0]) and np.array_equal(c_new[2], c[2]) and np.array_equal(c_new[1], e[1])
    assert wsum[0] == 2.0 and np.all(sums[0] == 0.0) and wsum[2] == 0.0


def test_zero_weight_rows_and_row_permutations_change_nothing():
    x, w, c, prev = km.case_inputs(130, 64, 65, 'gauss')
    ref = km.direct(x, w, c, prev)
    x2 = np.concatenate([x, km.unit(np.random.RandomState(1).randn(7, 64))])
    w2 = np.concatenate([w, np.zeros(7, np.float32)])
    got = km.direct(x2, w2, c, np.concatenate([prev, np.full(7, -1, np.int32)]))
    for k in ('J', 'S', 'changed', 'kept'):
        assert got[k] == ref[k]
    assert np.array_equal(got['sums'], ref['sums']) and np.array_equal(got['c_new'], ref['c_new'])
    p = np.random.RandomState(2).permutation(len(x))
    assert np.array_equal(km.assign64(x[p], c)[0], km.assign64(x, c)[0][p])
    acc = km._accumulate(x, c)
    assert np.array_equal(km._accumulate(x[p], c), acc[p])                 # a score is a function of its two rows


@pytest.mark.parametrize('R', [1, 2, 3])
def test_shards_sum_to_the_one_process_sums(R):
    x, w, c, _ = km.case_inputs(130, 64, 65, 'tight')
    a, best, sums, wsum, J = km.iteration64(x, w, c, R)
    a1, best1, sums1, wsum1, J1 = km.iteration64(x, w, c, 1)
    assert np.array_equal(a, a1) and np.array_equal(wsum, wsum1) and J == J1
    assert np.abs(sums - sums1).max() <= 1e-14 * np.abs(sums1).max()


def test_the_start_rule_gives_the_same_rows_for_any_sharding():
    from simclr_amd import kmeans
    w = np.ones(103, np.float32)
    w[[5, 17]] = 0.0
    want = km.start_rows(w, 10, 4, 1)
    cand = np.nonzero(w > 0)[0]
    assert np.array_equal(kmeans.start_positions(cand, 10, 4, 1), want) and len(set(want)) == 10 and not set(want) & {5, 17}
    assert not np.array_equal(km.start_rows(w, 10, 4, 0), want)
    for R, b in ((1, 16), (2, 8), (4, 4)):                   # eval-style shards of global batches of 16: the candidates are the same set
        seen = []
        for rank in range(R):
            n_local = -(-103 // 16) * b
            i = np.arange(n_local)
            pos = (i // b) * b * R + rank * b + i % b
            seen.append(pos[pos < 103][w[pos[pos < 103]] > 0])
        assert np.array_equal(np.sort(np.concatenate(seen)), cand)
    with pytest.raises(ValueError, match='exceeds the 101 rows'):
        kmeans.start_positions(cand, 102, 0, 0)
    assert np.array_equal(kmeans.shard_positions(6, 2), np.arange(6))


# ---- the emulation's budget and the mutants ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', km.CASES, ids=str)
def test_emulation_error_budget_and_mutants(case):
    n, D, K, fam = case
    inp, ref, emu, gate, acc = km.case(*case)
    x, w, c, prev = inp
    assert np.all(km.gap_ok(x, c, w))
    # the float32 accumulators err by at most D 2^-24 sum_k |x_k c_k| <= D 2^-24 on unit rows (and by far less in practice)
    err = np.abs(emu['best'] - ref['best'])[w > 0].max()
    assert err <= D * 2.0 ** -24, (err, D * 2.0 ** -24)
    assert all(ok for _, ok in km.compare(emu, ref, gate, w).values())
    applied = []
    for mutant in km.MUTANTS:
        res = km.compare(km.emulate(*inp, mutant=mutant, acc=acc), ref, gate, w)
        if km.mutant_applies(mutant, *case):
            applied.append(mutant)
            assert not all(ok for _, ok in res.values()), (mutant, res)
        else:
            assert all(ok for _, ok in res.values()), (mutant, res)
    print('MUTANTS %s applied: %s' % (case, applied))


def test_every_mutant_has_cases_and_the_exemptions_are_the_stated_ones():
    """ties_to_highest needs an exact tie (K >= 3: the copied centroid); last_tile_dropped a second centroid tile whose centroids win a
    weighted row; empty_to_zero an empty cluster; weights_ignored a weight other than 1; unnormalised a cluster whose sum is no unit row."""
    applies = {m: [c for c in km.CASES if km.mutant_applies(m, *c)] for m in km.MUTANTS}
    for m, cases in applies.items():
        assert len(cases) >= 6, (m, cases)
    assert all(c in applies['ties_to_highest'] for c in km.CASES if c[2] >= 3 and c[3] != 'padlast')
    assert not any(c in applies['ties_to_highest'] for c in km.CASES if c[2] == 2)
    assert all(c in applies['last_tile_dropped'] for c in km.CASES if c[2] > km.tile_edge(c[0], c[2]) and c[3] == 'padlast')
    assert not any(c in applies['last_tile_dropped'] for c in km.CASES if c[2] <= 64)
    assert all(c in applies['empty_to_zero'] for c in km.CASES if c[2] >= 3)
    assert all(c in applies['weights_ignored'] for c in km.CASES if c[3] != 'padlast')
    assert {km.tile_edge(n, K) for n, D, K in km.SHAPES} == {64, 128} and km.tile_edge(*km.WIDE_SHAPE[::2]) == 128


def test_planted_toy_meets_its_gap_condition_and_is_recovered():
    x, labels, w = km.planted()
    fit = km.fit64(x, w, 8, seed=0, restarts=2)
    assert all(km.lloyd_gaps_ok(x, w, run) for run in fit['runs'])
    T = km.table(fit['assigns'][-1], labels, 8, 8, w)
    assert fit['converged'] and abs(km.nmi(T) - 1.0) <= 1e-12 and km.ari(T) == 1.0
    assert fit['restart'] == 0 and fit['runs'][0]['J'] < fit['runs'][1]['J']
    x2, _, w2 = km.planted(seed=2)
    more = km.fit64(x2, w2, 12, seed=3, restarts=1)
    assert km.lloyd_gaps_ok(x2, w2, more) and more['converged'] and more['empties'] == 1


# ---- the host side of the feature ------------------------------------------------------------------------------------------------
def test_flag_defaults_and_result_keys():
    from simclr_amd import kmeans
    from simclr_amd.flags import FLAGS
    FLAGS.reset()
    d = FLAGS.flag_values_dict()
    assert (d['kmeans_eval'], d['kmeans_k'], d['kmeans_restarts'], d['kmeans_max_iterations'], d['kmeans_tolerance'], d['kmeans_seed'],
            d['kmeans_bank_examples']) == (False, 0, 1, 50, 1e-6, 0, 0)
    assert kmeans.RESULT_KEYS == ('eval/kmeans_nmi', 'eval/kmeans_ari', 'eval/kmeans_top_1_accuracy', 'kmeans/inertia',
                                  'kmeans/iterations', 'kmeans/converged', 'kmeans/empty_clusters', 'kmeans/restart', 'kmeans/k',
                                  'global_step')
    assert kmeans.MATCHED_KEY == 'eval/kmeans_matched_accuracy'
    FLAGS.parse(['--kmeans_eval', '--kmeans_k=100', '--kmeans_restarts=3'])
    assert FLAGS.kmeans_eval is True and FLAGS.kmeans_k == 100 and FLAGS.kmeans_restarts == 3
    FLAGS.reset()


@pytest.mark.parametrize('update, flag', [
    (dict(kmeans_k=1), 'kmeans_k'), (dict(kmeans_k=-2), 'kmeans_k'), (dict(kmeans_k=16385), 'kmeans_k'),
    (dict(kmeans_restarts=0), 'kmeans_restarts'), (dict(kmeans_restarts=17), 'kmeans_restarts'),
    (dict(kmeans_max_iterations=0), 'kmeans_max_iterations'), (dict(kmeans_max_iterations=1001), 'kmeans_max_iterations'),
    (dict(kmeans_tolerance=-1e-9), 'kmeans_tolerance'), (dict(kmeans_tolerance=1.0), 'kmeans_tolerance'),
    (dict(kmeans_tolerance=float('nan')), 'kmeans_tolerance'),
    (dict(kmeans_seed=-1), 'kmeans_seed'),
    (dict(kmeans_bank_examples=-1), 'kmeans_bank_examples'),
    (dict(width_multiplier=5), 'kmeans_eval'),                     # 2048 x 5 = 10240 > 8192
])
def test_start_up_refusals_name_the_flag(update, flag):
    from simclr_amd import run
    from simclr_amd.flags import FLAGS
    FLAGS.reset()
    FLAGS.update(kmeans_eval=True, mode='eval', **update)
    try:
        with pytest.raises(ValueError, match=flag):
            run.check_kmeans_flags()
        FLAGS.update(mode='train')
        assert run.check_kmeans_flags() is None                   # --mode=train ignores the flags
    finally:
        FLAGS.reset()


def test_bank_and_cluster_count_refusals():
    from simclr_amd import run
    from simclr_amd.flags import FLAGS
    FLAGS.reset()
    FLAGS.update(kmeans_eval=True, mode='eval', kmeans_bank_examples=101)
    try:
        with pytest.raises(ValueError, match='kmeans_bank_examples=101 exceeds the 100 examples'):
            run.check_kmeans_flags(100, 10)
        FLAGS.update(kmeans_bank_examples=40)
        assert run.check_kmeans_flags(100, 10) == 40 and run.check_kmeans_flags() == 40
        FLAGS.update(kmeans_bank_examples=0, kmeans_tolerance=0.0)
        assert run.check_kmeans_flags(100, 10) == 100 and run.check_kmeans_flags() is None
        FLAGS.update(kmeans_k=101)
        with pytest.raises(ValueError, match='kmeans_k: 101 clusters exceed the 100 bank examples'):
            run.check_kmeans_flags(100, 10)
        FLAGS.update(kmeans_k=0)
        with pytest.raises(ValueError, match='kmeans_k'):
            run.check_kmeans_flags(100000, 20000)                 # K = the class count, above 16384
        with pytest.raises(ValueError, match='kmeans_k: 10 clusters exceed the 8 bank examples'):
            run.check_kmeans_flags(8, 10)
        FLAGS.update(kmeans_eval=False, kmeans_restarts=0)
        assert run.check_kmeans_flags(100, 10) is None            # the flag off: nothing is looked at
    finally:
        FLAGS.reset()


def _cpu_args(n=8, D=64, K=3):
    return (torch.zeros(n, D), torch.zeros(K, D), torch.ones(n))


@pytest.mark.parametrize('name, change, match', [
    ('width', lambda a: (torch.zeros(8, 96), torch.zeros(3, 96), a[2]), 'multiples of 64'),
    ('wide', lambda a: (torch.zeros(8, 8256), torch.zeros(3, 8256), a[2]), 'multiples of 64'),
    ('one centroid', lambda a: (a[0], torch.zeros(1, 64), a[2]), '2 <= K <= 16384'),
    ('centroids', lambda a: (a[0], torch.zeros(16385, 64), a[2]), '2 <= K <= 16384'),
    ('no rows', lambda a: (torch.zeros(0, 64), a[1], a[2][:0]), '1 <= n <= 65536'),
    ('rows', lambda a: (torch.zeros(65537, 64), a[1], torch.ones(65537)), '1 <= n <= 65536'),
    ('x dtype', lambda a: (a[0].double(),) + a[1:], 'x must be a float32'),
    ('c shape', lambda a: (a[0], torch.zeros(3, 128), a[2]), 'c must be a float32'),
    ('weights shape', lambda a: a[:2] + (torch.ones(7),), 'weights must be'),
    ('misaligned', lambda a: (torch.zeros(8 * 64 + 1)[1:].view(8, 64),) + a[1:], '16-byte aligned'),
    ('not contiguous', lambda a: (torch.zeros(8, 128)[:, :64],) + a[1:], 'contiguous'),
])
def test_ops_refuse_before_any_launch(name, change, match):
    from simclr_amd import ops
    with pytest.raises(ValueError, match=match):
        ops.kmeans_assign(*change(_cpu_args()))


def test_ops_refuse_the_other_arguments():
    from simclr_amd import ops
    x, c, w = _cpu_args()
    a = torch.zeros(8, dtype=torch.int32)
    with pytest.raises(ValueError, match='assign must be a int32'):
        ops.kmeans_assign(x, c, w, assign=a.long())
    with pytest.raises(ValueError, match='best must be'):
        ops.kmeans_assign(x, c, w, best=torch.zeros(7))
    with pytest.raises(ValueError, match='workspace must hold'):
        ops.kmeans_assign(x, c, w, ws=torch.zeros(2, dtype=torch.float64))
    with pytest.raises(ValueError, match='assign must be'):
        ops.kmeans_update(x, w, a.long(), 3)
    with pytest.raises(ValueError, match='accumulate=True needs'):
        ops.kmeans_update(x, w, a, 3, accumulate=True)
    with pytest.raises(ValueError, match='sums must be a float64'):
        ops.kmeans_update(x, w, a, 3, sums=torch.zeros(3, 64), wsum=torch.zeros(3, dtype=torch.float64))
    with pytest.raises(ValueError, match='2 <= K <= 16384'):
        ops.kmeans_update(x, w, a, 1)
    sums, wsum = torch.zeros(3, 64, dtype=torch.float64), torch.zeros(3, dtype=torch.float64)
    with pytest.raises(ValueError, match='c_prev must be'):
        ops.kmeans_finish(sums, wsum, torch.zeros(3, 32))
    with pytest.raises(ValueError, match='sums must be a float64'):
        ops.kmeans_finish(sums.float(), wsum, c)
    with pytest.raises(ValueError, match='may not alias'):
        ops.kmeans_finish(sums, wsum, c, c_new=c)
    with pytest.raises(ValueError, match='multiples of 64'):
        ops.kmeans_workspace(8, 100, 3, 'cpu')
    assert ops.kmeans_dim_ok(64) and ops.kmeans_dim_ok(8192) and not ops.kmeans_dim_ok(32) and not ops.kmeans_dim_ok(8256)
    assert (ops.KMEANS_MIN_K, ops.KMEANS_MAX_K) == (2, 16384)


def test_fit_refuses_bad_arguments():
    from simclr_amd import kmeans
    for kw, match in ((dict(k=1), 'k must be'), (dict(restarts=0), 'restarts'), (dict(max_iterations=0), 'max_iterations'),
                      (dict(tolerance=1.5), 'tolerance'), (dict(tolerance=float('nan')), 'tolerance'), (dict(seed=-1), 'seed')):
        args = dict(k=3, seed=0, restarts=1, max_iterations=10, tolerance=1e-6)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            kmeans.fit(torch.zeros(4, 64), torch.ones(4), **args)
    with pytest.raises(ValueError, match='multiples of 64'):
        kmeans.fit(torch.zeros(4, 100), torch.ones(4), 3)
    with pytest.raises(ValueError, match='k = 5 exceeds the 4 rows'):
        kmeans.fit(torch.zeros(4, 64), torch.ones(4), 5)


def test_contingency_counts_the_weighted_rows():
    from simclr_amd import kmeans
    a = torch.tensor([0, 1, 1, 2, 2, 2], dtype=torch.int32)
    y = torch.tensor([0, 1, 0, 2, 2, 1])
    w = torch.tensor([1.0, 1.0, 0.0, 1.0, 1.0, 1.0])
    T = kmeans.contingency(a, y, w, 4, 3)
    assert T.dtype == torch.int64 and T.tolist() == [[1, 0, 0], [0, 1, 0], [0, 1, 2], [0, 0, 0]]
    assert np.array_equal(T.numpy(), km.table(a.numpy(), y.numpy(), 4, 3, w.numpy()))
    with pytest.raises(ValueError, match='assignments must lie'):
        kmeans.contingency(a, y, w, 2, 3)


def test_c_boundary_declares_exports_and_refuses():
    from simclr_amd import _lib
    sig = _lib.parse_header()
    for name in ('simclr_kmeans_assign', 'simclr_kmeans_update', 'simclr_kmeans_finish', 'simclr_kmeans_workspace_bytes',
                 'simclr_kmeans_tile_edge'):
        assert name in sig, name
    L = _lib.lib()
    assert L.abi_version() == 8
    assert L.kmeans_workspace_bytes(257, 2048, 1000) > 0 and L.kmeans_workspace_bytes(257, 2000, 1000) == 0
    assert L.kmeans_workspace_bytes(0, 64, 2) == 0 and L.kmeans_workspace_bytes(4, 64, 1) == 0 and L.kmeans_workspace_bytes(4, 64, 16385) == 0
    assert L.kmeans_workspace_bytes(65537, 64, 2) == 0 and L.kmeans_workspace_bytes(4, 64, 16384) > 0
    for n, D, K in km.SHAPES:
        assert L.kmeans_tile_edge(n, D, K) == km.tile_edge(n, K), (n, D, K)
        assert L.kmeans_workspace_bytes(n, D, K) % 8 == 0
    assert L.kmeans_tile_edge(65536, 2048, 1000) == 128 and L.kmeans_tile_edge(4, 100, 3) == 0
    with pytest.raises(_lib.SimclrHipError, match='multiple of 64'):
        L.kmeans_assign(None, None, None, 4, 100, 3, None, None, None, None, None)
    with pytest.raises(_lib.SimclrHipError, match='2 <= K <= 16384'):
        L.kmeans_assign(None, None, None, 4, 64, 1, None, None, None, None, None)
    with pytest.raises(_lib.SimclrHipError, match='1 <= n <= 65536'):
        L.kmeans_update(None, None, None, None, 65537, 64, 3, None, None, 0, None)
    with pytest.raises(_lib.SimclrHipError, match='2 <= K <= 16384'):
        L.kmeans_finish(None, None, None, 16385, 64, None, None, None, None)
    for call in (lambda: L.kmeans_assign(None, None, None, 4, 64, 3, None, None, None, None, None),
                 lambda: L.kmeans_update(None, None, None, None, 4, 64, 3, None, None, 0, None),
                 lambda: L.kmeans_finish(None, None, None, 3, 64, None, None, None, None)):
        with pytest.raises(_lib.SimclrHipError, match='null argument'):
            call()
    import ctypes
    fake, odd = ctypes.c_void_p(1 << 20), ctypes.c_void_p((1 << 20) + 4)
    with pytest.raises(_lib.SimclrHipError, match='16-byte aligned'):
        L.kmeans_update(fake, odd, fake, fake, 4, 64, 3, fake, fake, 0, None)
    with pytest.raises(_lib.SimclrHipError, match='16-byte aligned'):
        L.kmeans_finish(fake, fake, fake, 3, 64, odd, fake, fake, None)
