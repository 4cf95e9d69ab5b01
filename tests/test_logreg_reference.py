"""CPU tests of the cached-feature linear probe: the restatements of tests/logreg_reference.py against autograd and the hand cases
(tests/golden/LOGREG_HAND_DERIVED.md), the solver's properties, the emulation's error budget and its mutants, and the host side of
the feature: flags, refusals, result keys, the C boundary."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import logreg_reference as lr


def _small(n=23, D=6, C=4, seed=0):
    rng = np.random.RandomState(seed)
    x = rng.randn(n, D)
    labels = rng.randint(0, C, n).astype(np.int32)
    weights = np.array([0.5, 2.0, 1.0, 0.0, 1.5])[np.arange(n) % 5]
    return x, labels, weights, 0.3 * rng.randn(C, D), 0.2 * rng.randn(C)


@pytest.mark.parametrize('R', [1, 2, 3])
def test_gradient_matches_autograd(R):
    x, labels, weights, W, b = _small()
    l2 = 3e-2
    ref = lr.direct(x, labels, weights, W, b, l2, R)
    Wt, bt = torch.tensor(W, requires_grad=True), torch.tensor(b, requires_grad=True)
    s = torch.tensor(x) @ Wt.T + bt
    w = torch.tensor(weights)
    nll = torch.nn.functional.cross_entropy(s, torch.tensor(labels).long(), reduction='none')
    f = (w * nll).sum() / w.sum() + 0.5 * l2 * ((Wt * Wt).sum() + (bt * bt).sum())
    f.backward()
    assert abs(ref['f'] - float(f.detach())) <= 1e-13 * abs(float(f.detach()))
    np.testing.assert_allclose(ref['dW'], Wt.grad.numpy(), rtol=0, atol=1e-14)
    np.testing.assert_allclose(ref['db'], bt.grad.numpy(), rtol=0, atol=1e-14)
    np.testing.assert_allclose(ref['lse'], torch.logsumexp(s, 1).detach().numpy(), rtol=1e-14)


def test_hand_case_zero_parameters():
    x, labels, weights, W, b = _small(C=5)
    ref = lr.direct(x, labels, weights, 0 * W, 0 * b, 1e-2)
    C, S = 5, weights.sum()
    assert abs(ref['f'] - math.log(C)) <= 1e-15
    onehot = np.eye(C)[labels]
    np.testing.assert_allclose(ref['G'], (weights / S)[:, None] * (1.0 / C - onehot), rtol=0, atol=1e-17)
    assert ref['hits'] == weights[labels == 0].sum()             # every logit ties: the lowest index, class 0, is the maximum


def test_hand_case_two_by_two():
    """tests/golden/LOGREG_HAND_DERIVED.md, case 2."""
    l2 = 0.5
    W = np.array([[math.log(3.0), 0.0], [0.0, 0.0]])
    ref = lr.direct(np.eye(2), np.array([0, 1]), np.ones(2), W, np.zeros(2), l2)
    assert abs(ref['f'] - (0.5 * math.log(8.0 / 3.0) + 0.25 * math.log(3.0) ** 2)) <= 1e-15
    np.testing.assert_allclose(ref['lse'], [math.log(4.0), math.log(2.0)], rtol=1e-15)
    np.testing.assert_allclose(ref['G'], [[-0.125, 0.125], [0.25, -0.25]], rtol=0, atol=1e-16)
    np.testing.assert_allclose(ref['dW'], [[-0.125 + l2 * math.log(3.0), 0.25], [0.125, -0.25]], rtol=0, atol=1e-16)
    np.testing.assert_allclose(ref['db'], [0.125, -0.125], rtol=0, atol=1e-16)
    assert ref['hits'] == 1.0                                    # row 1 ties: class 0 is the maximum, its label is 1


def test_row_permutation_and_zero_weight_rows_change_nothing():
    x, labels, weights, W, b = _small()
    ref = lr.direct(x, labels, weights, W, b, 1e-2)
    perm = np.random.RandomState(1).permutation(len(x))
    got = lr.direct(x[perm], labels[perm], weights[perm], W, b, 1e-2)
    assert abs(got['f'] - ref['f']) <= 1e-14 and np.abs(got['dW'] - ref['dW']).max() <= 1e-15 and got['hits'] == ref['hits']
    keep = weights > 0
    got = lr.direct(x[keep], labels[keep], weights[keep], W, b, 1e-2)
    assert abs(got['f'] - ref['f']) <= 1e-14 and np.abs(got['dW'] - ref['dW']).max() <= 1e-15
    assert np.abs(got['db'] - ref['db']).max() <= 1e-15 and got['hits'] == ref['hits'] and np.all(ref['G'][~keep] == 0)


def test_the_minimiser_is_unique_and_f_never_rises():
    x, labels, weights = lr.toy_problem(90, 8, 3, 0.5)
    a = lr.solve(x, labels, weights, 3, 1e-2, tolerance=1e-9)
    rng = np.random.RandomState(3)
    b = lr.solve(x, labels, weights, 3, 1e-2, tolerance=1e-9, init=(rng.randn(3, 8), rng.randn(3)))
    assert a.converged and b.converged
    # strict convexity with modulus l2: |theta - theta*| <= |g| / l2
    assert np.abs(a.W - b.W).max() <= 2 * 1e-9 * math.sqrt(27) / 1e-2 and np.abs(a.b - b.b).max() <= 2 * 1e-9 * math.sqrt(27) / 1e-2
    for fit in (a, b):
        assert all(n <= p for p, n in zip(fit.losses, fit.losses[1:])) and len(fit.losses) == fit.iterations
    two = lr.solve(x, labels, weights, 3, 1e-2, tolerance=1e-9, R=2)
    assert np.abs(two.W - a.W).max() <= 1e-6


@pytest.mark.parametrize('problem', lr.TOY_PROBLEMS, ids=str)
def test_toy_problems_converge_well_inside_the_cap(problem):
    """The fits of tests/test_gpu_logreg.py in float64: converged at tolerance 1e-5 far below the cap of 200, f monotone."""
    N, D, C, l2, sep = problem
    fit = lr.solve(*lr.toy_problem(N, D, C, sep), C, l2)
    print(problem, 'iterations', fit.iterations, 'evaluations', fit.evaluations)
    assert fit.converged and fit.iterations <= 100
    assert all(n <= p for p, n in zip(fit.losses, fit.losses[1:]))


@pytest.mark.parametrize('case', lr.CASES, ids=str)
def test_emulation_error_budget_and_mutants(case):
    """The emulation is a float32 restatement: its error against float64 stays within a budget worked out from the formats -- D
    roundings of 2^-24 of the row's scale per logit (the bound gap_threshold states, divided by 4), carried into lse (absolute), f, and,
    relative to its size, G; dW and db add n such terms -- and every mutant lands outside the gates on every case of the table it
    applies to (padded_columns_in_lse has no column to let in where C fills its tiles: there it must equal the definition)."""
    n, D, C, fam = case
    inp, ref, emu, gate = lr.case(*case)
    x, labels, weights, W, b = inp
    logit_err = float((lr.gap_threshold(x, W) / 4.0).max()) + 4 * lr.ulp32(float(np.abs(ref['lse']).max()))
    assert np.abs(emu['lse'] - ref['lse']).max() <= logit_err
    assert abs(emu['f'] - ref['f']) <= logit_err
    wmax = float(weights.max()) / ref['S']
    assert np.abs(emu['G'] - ref['G']).max() <= wmax * (2 * logit_err + 2.0 ** -22)
    xmax = float(np.abs(x).max())
    assert np.abs(emu['dW'] - ref['dW']).max() <= n * wmax * xmax * (2 * logit_err + 2.0 ** -21)
    assert np.abs(emu['db'] - ref['db']).max() <= n * wmax * (2 * logit_err + 2.0 ** -21)
    assert emu['hits'] == ref['hits']
    assert np.all(lr.gap_ok(x, W, b)) and not np.any(x[0]) and np.any(x[1:], axis=1).all()
    assert all(ok for _, ok in lr.compare(emu, ref, gate).values())
    results = lr.mutant_results(*case)
    assert set(results) == set(lr.MUTANTS)
    for mutant, res in results.items():
        if lr.mutant_applies(mutant, n, D, C):
            assert not all(ok for _, ok in res.values()), (mutant, res)
        else:
            assert all(ok for _, ok in res.values()), (mutant, res)


def test_search_direction_falls_back_to_steepest_descent():
    """A pair with negative curvature (never stored by the solver, hand-built here) makes the two-loop recursion return an ASCENT
    direction: both implementations drop the history and return -g.  With a proper pair they return the quasi-Newton step."""
    from simclr_amd import logreg
    g = np.array([1.0, 0.0])
    bad = [(np.array([1.0, 0.0]), np.array([-1.0, 0.0]), -1.0)]
    d, gd, pairs = lr.search_direction(g, bad)
    assert np.array_equal(d, -g) and gd == -1.0 and pairs == []
    tg = torch.tensor(g)
    td, tgd, tpairs = logreg.search_direction(tg, [tuple(torch.tensor(a) if isinstance(a, np.ndarray) else a for a in bad[0])])
    assert torch.equal(td, -tg) and tgd == -1.0 and tpairs == []
    good = [(np.array([1.0, 0.0]), np.array([2.0, 0.0]), 0.5)]               # curvature 2 along e_1: H = 1/2 there
    d, gd, pairs = lr.search_direction(g, good)
    assert np.allclose(d, [-0.5, 0.0]) and gd == -0.5 and len(pairs) == 1
    td, tgd, tpairs = logreg.search_direction(tg, [tuple(torch.tensor(a) if isinstance(a, np.ndarray) else a for a in good[0])])
    assert np.allclose(td.numpy(), d) and tgd == gd and len(tpairs) == 1


def test_every_table_shape_gives_padded_columns_a_case_or_says_why():
    assert len(lr.MUTANTS) >= 5
    ragged = [s for s in lr.SHAPES if lr.mutant_applies('padded_columns_in_lse', *s)]
    assert len(ragged) >= 6 and {(129, 192, 64), (300, 64, 4096), (40, 1024, 4096)}.isdisjoint(ragged)
    P, rows = lr.row_parts(*lr.SPLIT_SHAPE)
    assert P > 1 and lr.SPLIT_SHAPE[0] % rows != 0 and rows % 32 == 0


# ---- the host side of the feature ------------------------------------------------------------------------------------------------
def test_flag_defaults_and_result_keys():
    from simclr_amd import logreg
    from simclr_amd.flags import FLAGS
    FLAGS.reset()
    d = FLAGS.flag_values_dict()
    assert (d['logreg_eval'], d['logreg_l2'], d['logreg_max_iterations'], d['logreg_tolerance'], d['logreg_history'],
            d['logreg_bank_examples']) == (False, '1e-4', 200, 1e-5, 10, 0)
    assert logreg.RESULT_KEYS == ('eval/logreg_top_1_accuracy', 'eval/logreg_top_5_accuracy', 'eval/logreg_loss', 'logreg/train_loss',
                                  'logreg/train_top_1_accuracy', 'logreg/iterations', 'logreg/evaluations', 'logreg/grad_norm',
                                  'logreg/converged', 'logreg/l2', 'global_step')
    assert logreg.parse_l2_list('1e-2, 1e-3') == [1e-2, 1e-3] and logreg.parse_l2_list('1e-4') == [1e-4]
    FLAGS.parse(['--logreg_eval', '--logreg_l2=1e-2,1e-3', '--logreg_history=5'])
    assert FLAGS.logreg_eval is True and FLAGS.logreg_l2 == '1e-2,1e-3' and FLAGS.logreg_history == 5
    FLAGS.reset()


@pytest.mark.parametrize('update, flag', [
    (dict(logreg_l2='0'), 'logreg_l2'), (dict(logreg_l2='-1e-3'), 'logreg_l2'), (dict(logreg_l2='nan'), 'logreg_l2'),
    (dict(logreg_l2='inf'), 'logreg_l2'), (dict(logreg_l2=''), 'logreg_l2'), (dict(logreg_l2='1e-3,,1e-4'), 'logreg_l2'),
    (dict(logreg_l2='abc'), 'logreg_l2'),
    (dict(logreg_max_iterations=0), 'logreg_max_iterations'), (dict(logreg_max_iterations=10001), 'logreg_max_iterations'),
    (dict(logreg_tolerance=0.0), 'logreg_tolerance'), (dict(logreg_tolerance=1.0), 'logreg_tolerance'),
    (dict(logreg_tolerance=float('nan')), 'logreg_tolerance'),
    (dict(logreg_history=0), 'logreg_history'), (dict(logreg_history=65), 'logreg_history'),
    (dict(logreg_bank_examples=-1), 'logreg_bank_examples'),
    (dict(width_multiplier=5), 'logreg_eval'),                     # 2048 x 5 = 10240 > 8192
])
def test_start_up_refusals_name_the_flag(update, flag):
    from simclr_amd import run
    from simclr_amd.flags import FLAGS
    FLAGS.reset()
    FLAGS.update(logreg_eval=True, mode='eval', **update)
    try:
        with pytest.raises(ValueError, match=flag):
            run.check_logreg_flags()
        FLAGS.update(mode='train')
        assert run.check_logreg_flags() is None                   # --mode=train ignores the flags
    finally:
        FLAGS.reset()


def test_bank_and_class_refusals():
    from simclr_amd import run
    from simclr_amd.flags import FLAGS
    FLAGS.reset()
    FLAGS.update(logreg_eval=True, mode='eval', logreg_bank_examples=101)
    try:
        with pytest.raises(ValueError, match='logreg_bank_examples=101 exceeds the 100 examples'):
            run.check_logreg_flags(100)
        FLAGS.update(logreg_bank_examples=40)
        assert run.check_logreg_flags(100) == 40 and run.check_logreg_flags() == 40
        FLAGS.update(logreg_bank_examples=0)
        assert run.check_logreg_flags(100) == 100 and run.check_logreg_flags() is None
        with pytest.raises(ValueError, match='logreg_eval takes 2..4096 classes'):
            run.check_logreg_classes(4097)
        run.check_logreg_classes(4096)
        FLAGS.update(logreg_eval=False, logreg_history=0)
        assert run.check_logreg_flags(100) is None                # the flag off: nothing is looked at
    finally:
        FLAGS.reset()


def _cpu_args(n=8, D=64, C=3):
    return (torch.zeros(n, D), torch.zeros(C, D), torch.zeros(C), torch.zeros(n, dtype=torch.int32), torch.ones(n))


@pytest.mark.parametrize('name, change, match', [
    ('width', lambda a: (torch.zeros(8, 96), torch.zeros(3, 96)) + a[2:], 'multiples of 64'),
    ('wide', lambda a: (torch.zeros(8, 8256), torch.zeros(3, 8256)) + a[2:], 'multiples of 64'),
    ('one class', lambda a: (a[0], torch.zeros(1, 64), torch.zeros(1)) + a[3:], '2 <= C <= 4096'),
    ('classes', lambda a: (a[0], torch.zeros(4097, 64), torch.zeros(4097)) + a[3:], '2 <= C <= 4096'),
    ('no rows', lambda a: (torch.zeros(0, 64), a[1], a[2], a[3][:0], a[4][:0]), '1 <= n <= 65536'),
    ('rows', lambda a: (torch.zeros(65537, 64), a[1], a[2], torch.zeros(65537, dtype=torch.int32), torch.ones(65537)), '1 <= n <= 65536'),
    ('x dtype', lambda a: (a[0].double(),) + a[1:], 'x must be a float32'),
    ('b shape', lambda a: a[:2] + (torch.zeros(4),) + a[3:], 'b must be a float32'),
    ('labels dtype', lambda a: a[:3] + (a[3].long(), a[4]), 'labels must be'),
    ('weights shape', lambda a: a[:4] + (torch.ones(7),), 'weights must be'),
    ('misaligned', lambda a: (torch.zeros(8 * 64 + 1)[1:].view(8, 64),) + a[1:], '16-byte aligned'),
    ('label range', lambda a: a[:3] + (torch.full((8,), 3, dtype=torch.int32), a[4]), r'labels must lie in \[0, 3\)'),
    ('negative label', lambda a: a[:3] + (torch.full((8,), -1, dtype=torch.int32), a[4]), r'labels must lie in \[0, 3\)'),
])
def test_ops_refuse_before_any_launch(name, change, match):
    from simclr_amd import ops
    with pytest.raises(ValueError, match=match):
        ops.logreg_fwd(*change(_cpu_args()), 1.0)


def test_ops_refuse_scalars_and_backward_arguments():
    from simclr_amd import ops
    a = _cpu_args()
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='inv_S'):
            ops.logreg_fwd(*a, bad)
    with pytest.raises(ValueError, match='mode'):
        ops.logreg_fwd(*a, 1.0, mode=3)
    with pytest.raises(ValueError, match='store must be'):
        ops.logreg_fwd(*a, 1.0, mode=1, store=torch.zeros(8, 3))
    with pytest.raises(ValueError, match='lse must be'):
        ops.logreg_fwd(*a, 1.0, lse=torch.zeros(8))
    g = torch.zeros(8, 4)
    with pytest.raises(ValueError, match='g must be'):
        ops.logreg_bwd(torch.zeros(8, 3), a[0], 3)
    with pytest.raises(ValueError, match='accumulate=True needs'):
        ops.logreg_bwd(g, a[0], 3, accumulate=True)
    with pytest.raises(ValueError, match='dw must be'):
        ops.logreg_bwd(g, a[0], 3, dw=torch.zeros(3, 32), db=torch.zeros(3))
    with pytest.raises(ValueError, match='2 <= C <= 4096'):
        ops.logreg_bwd(g, a[0], 1)
    assert ops.logreg_store_pitch(3) == 4 and ops.logreg_store_pitch(1000) == 1000 and ops.logreg_store_pitch(65) == 68


def test_fit_refuses_bad_arguments():
    from simclr_amd import logreg
    for kw, match in ((dict(l2=0.0), 'l2'), (dict(l2=float('nan')), 'l2'), (dict(max_iterations=0), 'max_iterations'),
                      (dict(tolerance=1.5), 'tolerance'), (dict(history=65), 'history')):
        args = dict(l2=1e-3, max_iterations=10, tolerance=1e-5, history=10)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            logreg.fit(torch.zeros(4, 64), torch.zeros(4, dtype=torch.int32), torch.ones(4), 3, **args)
    with pytest.raises(ValueError, match='multiples of 64'):
        logreg.fit(torch.zeros(4, 100), torch.zeros(4, dtype=torch.int32), torch.ones(4), 3, 1e-3)
    with pytest.raises(ValueError, match=r'labels must lie in \[0, 3\)'):
        logreg.fit(torch.zeros(4, 64), torch.full((4,), 3, dtype=torch.int32), torch.ones(4), 3, 1e-3)


def test_c_boundary_declares_exports_and_refuses():
    from simclr_amd import _lib
    sig = _lib.parse_header()
    for name in ('simclr_logreg_fwd', 'simclr_logreg_bwd', 'simclr_logreg_workspace_bytes', 'simclr_logreg_row_splits',
                 'simclr_logreg_tile_edge', 'simclr_logreg_bwd_tile_edge', 'simclr_logreg_store_pitch'):
        assert name in sig, name
    L = _lib.lib()
    assert L.abi_version() == 8
    assert L.logreg_workspace_bytes(257, 2048, 1000) > 0 and L.logreg_workspace_bytes(257, 2000, 1000) == 0
    assert L.logreg_workspace_bytes(0, 64, 2) == 0 and L.logreg_workspace_bytes(4, 64, 1) == 0 and L.logreg_workspace_bytes(4, 64, 4097) == 0
    for n, D, C in lr.SHAPES:
        assert L.logreg_row_splits(n, D, C) == lr.row_parts(n, D, C)[0], (n, D, C)
        assert L.logreg_tile_edge(n, D, C) == lr.fwd_edge(n, C) and L.logreg_bwd_tile_edge(n, D, C) == lr.bwd_edge(D, C)
    assert L.logreg_row_splits(*lr.SPLIT_SHAPE) > 1 and L.logreg_row_splits(65536, 2048, 10) == 8
    assert {L.logreg_tile_edge(*s) for s in lr.SHAPES} == {64, 128} and {L.logreg_bwd_tile_edge(*s) for s in lr.SHAPES} == {64, 128}
    one = ctypes.c_double(1.0)
    with pytest.raises(_lib.SimclrHipError, match='multiple of 64'):
        L.logreg_fwd(None, None, None, None, None, 4, 100, 3, one, 0, None, None, None, None, None)
    with pytest.raises(_lib.SimclrHipError, match='2 <= C <= 4096'):
        L.logreg_fwd(None, None, None, None, None, 4, 64, 1, one, 0, None, None, None, None, None)
    with pytest.raises(_lib.SimclrHipError, match='1 <= n <= 65536'):
        L.logreg_bwd(None, None, 65537, 64, 3, None, None, 0, None, None)
    with pytest.raises(_lib.SimclrHipError, match='mode must be'):
        L.logreg_fwd(None, None, None, None, None, 4, 64, 3, one, 3, None, None, None, None, None)
    with pytest.raises(_lib.SimclrHipError, match='inv_S'):
        L.logreg_fwd(None, None, None, None, None, 4, 64, 3, ctypes.c_double(0.0), 0, None, None, None, None, None)
    with pytest.raises(_lib.SimclrHipError, match='null argument'):
        L.logreg_fwd(None, None, None, None, None, 4, 64, 3, one, 0, None, None, None, None, None)
    with pytest.raises(_lib.SimclrHipError, match='null argument'):
        L.logreg_bwd(None, None, 4, 64, 3, None, None, 0, None, None)
    fake, odd = ctypes.c_void_p(1 << 20), ctypes.c_void_p((1 << 20) + 4)
    with pytest.raises(_lib.SimclrHipError, match='16-byte aligned'):
        L.logreg_bwd(fake, odd, 4, 64, 3, fake, fake, 0, fake, None)
