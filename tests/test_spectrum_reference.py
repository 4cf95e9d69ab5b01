"""The eigen-spectrum evaluation without a device: the float64 definition and the float32 emulation of tests/spectrum_reference.py
against hand cases (tests/golden/SPECTRUM_HAND_DERIVED.md), identities, the mutants, and the host side of the feature (flags,
refusals, result keys, the C boundary).

The identity, hand-case, budget and mutant tests exercise the reference (and simclr_amd.spectrum.scores where they say so); the flag,
refusal, ABI-symbol and score tests fail without the feature: they import simclr_amd.spectrum, read the new flags or call the new
entry points."""
import numpy as np
import pytest
import torch

from tests import repr_reference as rp
from tests import spectrum_reference as sr

SCORE_KEYS = ('eval/spectrum_rankme', 'eval/spectrum_participation_ratio', 'eval/spectrum_numerical_rank', 'eval/spectrum_top1_share',
              'eval/spectrum_dims_90', 'eval/spectrum_dims_99')


def _both(lam, **kw):
    """scores of the product and of the restatement; they agree to rounding on every key."""
    from simclr_amd import spectrum
    a, b = spectrum.scores(lam, **kw), sr.scores64(lam, **kw)
    assert set(a) == set(b), (set(a) ^ set(b))
    for k in a:
        assert abs(a[k] - b[k]) <= 1e-12 * max(1.0, abs(b[k])), (k, a[k], b[k])
    return a


# ---- hand cases (tests/golden/SPECTRUM_HAND_DERIVED.md) ---------------------------------------------------------------------------
def test_identical_rows_score_zero():
    x = np.repeat(np.random.RandomState(0).randn(1, 64), 9, 0).astype(np.float32)
    C, S, _ = sr.cov64(x, np.ones(9))
    assert S == 9 and np.abs(C).max() == 0.0
    s = _both(sr.eig64(C))
    assert all(s[k] == 0 for k in SCORE_KEYS) and 'eval/spectrum_alpha' not in s and s['spectrum/trace'] == 0.0


def test_isotropic_spectrum():
    D = 64
    s = _both(np.full(D, 2.5))
    assert abs(s['eval/spectrum_participation_ratio'] - D) <= 1e-12 * D
    # p_i = 1 / D + 1e-7 for every i: H = -(1 + D e) log(1 / D + e), rankme = (1 / D + e)^-(1 + D e) = 64.00129389...
    want = (1.0 / D + 1e-7) ** -(1.0 + D * 1e-7)
    assert abs(want - 64.00129389027936) <= 1e-9 and abs(s['eval/spectrum_rankme'] - want) <= 1e-10
    assert abs(s['eval/spectrum_alpha']) <= 1e-12 and s['eval/spectrum_numerical_rank'] == D
    assert abs(s['eval/spectrum_top1_share'] - 1.0 / D) <= 1e-15 and s['eval/spectrum_dims_90'] == 58 and s['eval/spectrum_dims_99'] == 64


def test_harmonic_spectrum_has_alpha_one():
    s = _both(1.0 / np.arange(1.0, 65.0))
    assert abs(s['eval/spectrum_alpha'] - 1.0) <= 1e-12
    s = _both(1.0 / np.arange(1.0, 65.0) ** 2, alpha_first=3, alpha_last=20)
    assert abs(s['eval/spectrum_alpha'] - 2.0) <= 1e-12


def test_rank_five_spectrum():
    lam = np.r_[5.0, 4.0, 3.0, 2.0, 1.0, np.zeros(59)]
    s = _both(lam)
    assert s['eval/spectrum_numerical_rank'] == 5 and 'eval/spectrum_alpha' not in s
    assert abs(s['eval/spectrum_participation_ratio'] - 225.0 / 55.0) <= 1e-12 and abs(s['eval/spectrum_top1_share'] - 1.0 / 3.0) <= 1e-15
    assert (s['eval/spectrum_dims_90'], s['eval/spectrum_dims_99']) == (4, 5)            # 14 of 15 >= 13.5; 15 of 15 >= 14.85
    assert abs(s['eval/spectrum_rankme'] - 4.826862909364821) <= 1e-9
    # a negative eigenvalue is set to 0 and counted; the order of the input does not matter
    t = _both(np.r_[-1e-9, lam[::-1][1:]])
    assert t['spectrum/negative_eigenvalues'] == 1 and t['eval/spectrum_numerical_rank'] == 5
    # the fit needs 8 points: ranks 16 and 17 with first = 10
    assert 'eval/spectrum_alpha' not in _both(np.r_[1.0 / np.arange(1.0, 17.0), np.zeros(48)])
    assert abs(_both(np.r_[1.0 / np.arange(1.0, 18.0), np.zeros(47)])['eval/spectrum_alpha'] - 1.0) <= 1e-12


# ---- identities ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(65, 64), (64, 128), (130, 192)], ids=str)
def test_participation_ratio_from_the_eigenvalues_and_from_the_matrix(shape):
    x, w = sr.case_inputs(*shape, 'mean5')
    C, _, _ = sr.cov64(x, w)
    pr = _both(sr.eig64(C))['eval/spectrum_participation_ratio']
    want = np.trace(C) ** 2 / (C * C).sum()
    assert abs(pr - want) <= 1e-9 * want
    # tests/repr_reference.py's rank is the mean of the two views' participation ratios: the same rows as both views
    r = rp.direct(np.concatenate([x, x]))[3]
    assert abs(pr - r) <= 1e-9 * r


@pytest.mark.parametrize('case', [c for c in sr.CASES[:16] if c != (2, 64, 'nanpad')], ids=str)      # that one counts a single row
def test_the_delta_correction_is_exact(case):
    (x, w), ref, _, _ = sr.case(*case)
    C, S, mu = sr.cov64(x, w)
    assert S == ref['count'] and np.array_equal(mu.astype(np.float32), ref['mu32'])
    scale = np.abs(C).max()
    assert np.abs(ref['C'] - C).max() <= 64 * sr.EPS64 * max(scale, 1.0)
    # without the correction the fp32-rounded mean would show: S delta delta^T / (S - 1) is its size
    delta = ref['mu'] - ref['mu32'].astype(np.float64)
    assert np.abs(ref['raw'] / (S - 1) - C - S / (S - 1) * np.outer(delta, delta)).max() <= 64 * sr.EPS64 * max(scale, 1.0)


def test_row_permutations_and_weight_zero_rows_change_nothing():
    x, w = sr.case_inputs(130, 192, 'gauss')
    C, S, mu = sr.cov64(x, w)
    perm = np.random.RandomState(3).permutation(130)
    Cp, Sp, _ = sr.cov64(x[perm], w[perm])
    assert Sp == S and np.abs(Cp - C).max() <= 64 * sr.EPS64 * np.abs(C).max()
    junk = np.full((7, 192), np.nan, np.float32)
    junk[3] = np.inf
    order = np.random.RandomState(4).permutation(137)
    x2, w2 = np.concatenate([x, junk])[order], np.concatenate([w, np.zeros(7, np.float32)])[order]
    C2, S2, _ = sr.cov64(x2, w2)
    assert S2 == S and np.abs(C2 - C).max() <= 64 * sr.EPS64 * np.abs(C).max()
    emu, emu2 = sr.emulate(x, w), sr.emulate(np.concatenate([x, junk]), np.concatenate([w, np.zeros(7, np.float32)]))
    assert emu2['count'] == S and np.array_equal(emu2['sums'], emu['sums']) and np.isfinite(emu2['raw']).all()
    # a negative and a NaN weight do not count either
    w3 = np.concatenate([w, np.array([-1.0, np.nan, 0.0, -0.0, 0.0, 0.0, 0.0], np.float32)])
    assert sr.colsum64(np.concatenate([x, junk]), w3)[1] == S


@pytest.mark.parametrize('R', [1, 2, 3])
def test_shards_add_to_the_one_process_sums(R):
    x, w = sr.case_inputs(130, 192, 'nanpad')
    ref = sr.reference(x, w)
    parts = [np.arange(r, 130, R) for r in range(R)]
    sums = sum(sr.colsum64(x[p], w[p])[0] for p in parts)
    S = sum(sr.colsum64(x[p], w[p])[1] for p in parts)
    assert S == ref['count'] and np.abs(sums - ref['sums']).max() <= 4 * sr.EPS64 * np.abs(ref['sums']).max()
    raw = sum(sr.raw64(x[p], w[p], ref['mu32']) for p in parts)
    # float64 sums of S terms in another order: S eps64 sum |terms|, and the largest entry (a diagonal one) bounds every sum |terms|
    assert np.abs(raw - ref['raw']).max() <= S * sr.EPS64 * np.abs(ref['raw']).max()
    emu = sum(sr.emulate_raw(x[p], w[p], ref['mu32']) for p in parts)
    assert np.abs(emu - ref['raw']).max() <= sr.gates(sr.emulate(x, w), ref)['raw']


# ---- the emulation's budget and the mutants -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', sr.CASES, ids=str)
def test_emulation_error_budget_and_mutants(case):
    n, D, fam = case
    (x, w), ref, emu, gate = sr.case(*case)
    part_rows, parts = sr.row_plan(n, D)
    assert part_rows % 32 == 0 and part_rows <= 8192 and (parts - 1) * part_rows < n <= parts * part_rows
    err = np.abs(emu['raw'] - ref['raw'])
    assert np.all(err <= sr.error_budget(x, w, ref['mu32'], part_rows))
    assert emu['count'] == ref['count'] and np.array_equal(emu['sums'], ref['sums'])
    assert all(ok for _, ok in sr.compare(emu, ref, gate).values())
    assert np.array_equal(emu['raw'], emu['raw'].T)
    applied = []
    for mutant in sr.MUTANTS:
        if sr.mutant_applies(mutant, *case):
            res = sr.compare(sr.emulate(x, w, mutant, base=emu), ref, gate)
            applied.append(mutant)
            assert not all(ok for _, ok in res.values()), (mutant, res)
    print('MUTANTS %s applied: %s' % (case, applied))


def test_every_mutant_has_cases():
    applies = {m: [c for c in sr.CASES if sr.mutant_applies(m, *c)] for m in sr.MUTANTS}
    assert all(len(v) >= 6 for v in applies.values()), applies
    assert len(applies['lower_unwritten']) == len(applies['divisor_s']) == len(sr.CASES) - 1
    assert {sr.tile_edge(n, D) for n, D in sr.SHAPES} == {64, 128}
    assert sr.smallest_three_part_ragged_n(64) == 65 and (65, 64) in sr.SHAPES
    # the rule never puts a D that is no multiple of 128 on the 128-wide tile
    assert all(sr.tile_edge(n, D) == 64 for n in (1, 300, 65536) for D in range(64, 8193, 128))


def test_uncentred_fp32_accumulation_misses_the_covariance_of_shifted_features():
    """The probe of the issue: on column mean 5, deviation 0.9 the uncentred float32 form misses the gate of every case, the centred
    one passes; figures in DESIGN.md section 32."""
    for n, D in sr.SHAPES:
        (x, w), ref, emu, gate = sr.case(n, D, 'mean5')
        bad = sr.emulate(x, w, 'uncentred')
        e_bad, e_ok = np.abs(bad['raw'] - ref['raw']).max(), np.abs(emu['raw'] - ref['raw']).max()
        print('UNCENTRED (%d, %d) centred %.3e uncentred %.3e gate %.3e' % (n, D, e_ok, e_bad, gate['raw']))
        assert e_bad > gate['raw'] >= e_ok


def test_rankme_on_lambda_is_rejected_on_the_planted_spectrum():
    x, w = sr.planted_harmonic()
    ref, emu = sr.reference(x, w), sr.emulate(x, w)
    lam = sr.eig64(ref['C'])
    assert np.abs(lam - 1.0 / np.arange(1, 129)).max() <= 1e-7            # the planting survives the rounding to float32
    g = sr.gates(emu, ref)['C_fro'] + sr.LAPACK_REL * lam[0]
    assert g <= 1e-3 * lam[-1]
    sg = sr.score_gates(lam, g)
    good, bad = sr.scores64(lam), sr.scores64(lam, rankme_on_lambda=True)
    lam_emu = sr.eig64(emu['C'])
    assert np.abs(lam_emu - lam).max() <= g
    assert abs(sr.scores64(lam_emu)['eval/spectrum_rankme'] - good['eval/spectrum_rankme']) <= sg['rankme']
    assert abs(bad['eval/spectrum_rankme'] - good['eval/spectrum_rankme']) > sg['rankme']
    assert abs(good['eval/spectrum_alpha'] - 1.0) <= sg['alpha'] + 1e-7 and good['eval/spectrum_numerical_rank'] == 128


def test_lapack_allowance_covers_a_symmetric_permutation():
    worst = 0.0
    for c in sr.CASES:
        ref = sr.case(*c)[1]
        if ref['C'] is None:
            continue
        lam = sr.eig64(ref['C'])
        P = np.random.RandomState(0).permutation(c[1])
        worst = max(worst, np.abs(lam - sr.eig64(ref['C'][np.ix_(P, P)])).max() / lam[0])
    print('LAPACK largest relative difference %.3e, allowance %.3e' % (worst, sr.LAPACK_REL))
    assert worst <= sr.LAPACK_REL


# ---- the host side of the feature ------------------------------------------------------------------------------------------------
def test_flag_defaults_and_result_keys():
    from simclr_amd import spectrum
    from simclr_amd.flags import FLAGS
    FLAGS.reset()
    d = FLAGS.flag_values_dict()
    assert (d['spectrum_eval'], d['spectrum_bank_examples'], d['spectrum_rank_threshold'], d['spectrum_alpha_first'],
            d['spectrum_alpha_last']) == (False, 0, 1e-6, 10, 0)
    assert spectrum.RESULT_KEYS == SCORE_KEYS + ('spectrum/trace', 'spectrum/rows', 'spectrum/dim', 'spectrum/negative_eigenvalues',
                                                 'global_step')
    assert spectrum.ALPHA_KEY == 'eval/spectrum_alpha'
    s = spectrum.scores(1.0 / np.arange(1.0, 65.0))
    assert set(s) | {'spectrum/rows', 'global_step'} == set(spectrum.RESULT_KEYS) | {spectrum.ALPHA_KEY}
    FLAGS.parse(['--spectrum_eval', '--spectrum_bank_examples=100', '--spectrum_alpha_last=40'])
    assert FLAGS.spectrum_eval is True and FLAGS.spectrum_bank_examples == 100 and FLAGS.spectrum_alpha_last == 40
    FLAGS.reset()


@pytest.mark.parametrize('update, flag', [
    (dict(spectrum_rank_threshold=0.0), 'spectrum_rank_threshold'), (dict(spectrum_rank_threshold=1.0), 'spectrum_rank_threshold'),
    (dict(spectrum_rank_threshold=float('nan')), 'spectrum_rank_threshold'),
    (dict(spectrum_alpha_first=0), 'spectrum_alpha_first'),
    (dict(spectrum_alpha_last=16), 'spectrum_alpha_last'), (dict(spectrum_alpha_last=-1), 'spectrum_alpha_last'),
    (dict(spectrum_bank_examples=-1), 'spectrum_bank_examples'),
    (dict(spectrum_bank_examples=1), 'spectrum_bank_examples'),
    (dict(width_multiplier=5), 'spectrum_eval'),                     # 2048 x 5 = 10240 > 8192
])
def test_start_up_refusals_name_the_flag(update, flag):
    from simclr_amd import run
    from simclr_amd.flags import FLAGS
    FLAGS.reset()
    FLAGS.update(spectrum_eval=True, mode='eval', **update)
    try:
        with pytest.raises(ValueError, match=flag):
            run.check_spectrum_flags()
        FLAGS.update(mode='train')
        assert run.check_spectrum_flags() is None                 # --mode=train ignores the flags
    finally:
        FLAGS.reset()


def test_bank_refusals():
    from simclr_amd import run
    from simclr_amd.flags import FLAGS
    FLAGS.reset()
    FLAGS.update(spectrum_eval=True, mode='eval', spectrum_bank_examples=101)
    try:
        with pytest.raises(ValueError, match='spectrum_bank_examples=101 exceeds the 100 examples'):
            run.check_spectrum_flags(100)
        FLAGS.update(spectrum_bank_examples=40, spectrum_alpha_last=17)
        assert run.check_spectrum_flags(100) == 40 and run.check_spectrum_flags() == 40
        FLAGS.update(spectrum_bank_examples=0)
        assert run.check_spectrum_flags(100) == 100 and run.check_spectrum_flags() is None
        with pytest.raises(ValueError, match='spectrum_bank_examples: a covariance needs at least 2 bank examples'):
            run.check_spectrum_flags(1)
        FLAGS.update(spectrum_eval=False, spectrum_alpha_first=0)
        assert run.check_spectrum_flags(100) is None              # the flag off: nothing is looked at
    finally:
        FLAGS.reset()


def _cpu_args(n=8, D=64):
    return (torch.zeros(n, D), torch.ones(n))


@pytest.mark.parametrize('name, change, match', [
    ('width', lambda a: (torch.zeros(8, 96), a[1]), 'multiples of 64'),
    ('wide', lambda a: (torch.zeros(8, 8256), a[1]), 'multiples of 64'),
    ('no rows', lambda a: (torch.zeros(0, 64), a[1][:0]), '1 <= n <= 65536'),
    ('rows', lambda a: (torch.zeros(65537, 64), torch.ones(65537)), '1 <= n <= 65536'),
    ('x dtype', lambda a: (a[0].double(), a[1]), 'x must be a float32'),
    ('x rank', lambda a: (torch.zeros(8, 8, 8), a[1]), r'need x \[n, D\]'),
    ('weights shape', lambda a: (a[0], torch.ones(7)), 'weights must be'),
    ('weights dtype', lambda a: (a[0], torch.ones(8, dtype=torch.float64)), 'weights must be'),
    ('misaligned', lambda a: (torch.zeros(8 * 64 + 1)[1:].view(8, 64), a[1]), '16-byte aligned'),
    ('not contiguous', lambda a: (torch.zeros(8, 128)[:, :64], a[1]), 'contiguous'),
])
def test_ops_refuse_before_any_launch(name, change, match):
    from simclr_amd import ops
    x, w = change(_cpu_args())
    with pytest.raises(ValueError, match=match):
        ops.spectrum_colsum(x, w)
    with pytest.raises(ValueError, match=match):
        ops.spectrum_cov(x, w, torch.zeros(x.shape[-1]))


def test_ops_refuse_the_other_arguments():
    from simclr_amd import ops, spectrum
    x, w = _cpu_args()
    with pytest.raises(ValueError, match='sums must be a float64'):
        ops.spectrum_colsum(x, w, sums=torch.zeros(65))
    with pytest.raises(ValueError, match='sums must be'):
        ops.spectrum_colsum(x, w, sums=torch.zeros(64, dtype=torch.float64))
    with pytest.raises(ValueError, match='accumulate=True needs sums'):
        ops.spectrum_colsum(x, w, accumulate=True)
    with pytest.raises(ValueError, match='workspace must hold'):
        ops.spectrum_colsum(x, w, ws=torch.zeros(2, dtype=torch.float64))
    with pytest.raises(ValueError, match='mu32 must be a float32'):
        ops.spectrum_cov(x, w, torch.zeros(64, dtype=torch.float64))
    with pytest.raises(ValueError, match='mu32 must be'):
        ops.spectrum_cov(x, w, torch.zeros(128))
    with pytest.raises(ValueError, match='cov must be a float64'):
        ops.spectrum_cov(x, w, torch.zeros(64), cov=torch.zeros(64, 64))
    with pytest.raises(ValueError, match='accumulate=True needs cov'):
        ops.spectrum_cov(x, w, torch.zeros(64), accumulate=True)
    with pytest.raises(ValueError, match='workspace must hold'):
        ops.spectrum_cov(x, w, torch.zeros(64), ws=torch.zeros(2, dtype=torch.float64))
    with pytest.raises(ValueError, match='multiples of 64'):
        ops.spectrum_workspace(8, 100, 'cpu')
    assert ops.spectrum_dim_ok(64) and ops.spectrum_dim_ok(8192) and not ops.spectrum_dim_ok(32) and not ops.spectrum_dim_ok(8256)
    with pytest.raises(ValueError, match='multiple of 64'):
        spectrum.covariance(torch.zeros(4, 100), torch.ones(4))
    with pytest.raises(ValueError, match='one weight per row'):
        spectrum.covariance(torch.zeros(4, 64), torch.ones(5))
    for kw, match in ((dict(rank_threshold=0.0), 'rank_threshold'), (dict(rank_threshold=1.5), 'rank_threshold'),
                      (dict(alpha_first=0), 'alpha_first'), (dict(alpha_first=5, alpha_last=11), 'alpha_last')):
        with pytest.raises(ValueError, match=match):
            spectrum.scores(np.ones(64), **kw)


def test_c_boundary_declares_exports_and_refuses():
    from simclr_amd import _lib
    sig = _lib.parse_header()
    for name in ('simclr_spectrum_colsum', 'simclr_spectrum_cov', 'simclr_spectrum_workspace_bytes', 'simclr_spectrum_dim_ok',
                 'simclr_spectrum_colsum_workspace_bytes',
                 'simclr_spectrum_tile_edge', 'simclr_spectrum_row_parts'):
        assert name in sig, name
    L = _lib.lib()
    assert L.abi_version() == 8 == _lib.ABI_VERSION
    assert L.spectrum_workspace_bytes(257, 2048) > 0 and L.spectrum_workspace_bytes(257, 2000) == 0
    assert L.spectrum_workspace_bytes(0, 64) == 0 and L.spectrum_workspace_bytes(65537, 64) == 0 and L.spectrum_workspace_bytes(4, 8256) == 0
    assert L.spectrum_dim_ok(64) == 1 and L.spectrum_dim_ok(8192) == 1 and L.spectrum_dim_ok(96) == 0 and L.spectrum_dim_ok(0) == 0
    for n, D in sr.SHAPES + [sr.PLANTED_SHAPE, (1, 64), (65536, 64), (65536, 128), (65536, 2048), (65536, 8192), (65536, 8128), (31, 8192)]:
        assert L.spectrum_tile_edge(n, D) == sr.tile_edge(n, D), (n, D)
        assert L.spectrum_row_parts(n, D) == sr.row_plan(n, D)[1], (n, D)
        e, (rows, parts) = sr.tile_edge(n, D), sr.row_plan(n, D)
        pairs = (D // e) * (D // e + 1) // 2
        # the workspace holds the centred slab and one fp32 tile per (part, pair); no CU idle wherever the rows allow it
        assert L.spectrum_workspace_bytes(n, D) % 16 == 0 and L.spectrum_workspace_bytes(n, D) >= 4 * n * D + 4 * parts * pairs * e * e
        assert pairs * parts >= min(256, pairs * -(-n // 32))
        # the column sums alone need their row parts, the head of the full workspace: ceil(n / 2048) x (D + 1) doubles
        assert 8 * -(-n // 2048) * (D + 1) <= L.spectrum_colsum_workspace_bytes(n, D) <= 8 * -(-n // 2048) * (D + 1) + 15
        assert L.spectrum_colsum_workspace_bytes(n, D) <= L.spectrum_workspace_bytes(n, D)
    assert L.spectrum_tile_edge(4, 100) == 0 and L.spectrum_row_parts(0, 64) == 0
    assert L.spectrum_colsum_workspace_bytes(4, 100) == 0 and L.spectrum_colsum_workspace_bytes(65537, 64) == 0
    assert L.spectrum_colsum_workspace_bytes(65536, 8192) < 4 << 20 < L.spectrum_workspace_bytes(65536, 8192)
    with pytest.raises(_lib.SimclrHipError, match='multiple of 64'):
        L.spectrum_colsum(None, None, 4, 100, None, 0, None, None)
    with pytest.raises(_lib.SimclrHipError, match='1 <= n <= 65536'):
        L.spectrum_cov(None, None, None, 65537, 64, None, 0, None, None)
    for call in (lambda: L.spectrum_colsum(None, None, 4, 64, None, 0, None, None),
                 lambda: L.spectrum_cov(None, None, None, 4, 64, None, 0, None, None)):
        with pytest.raises(_lib.SimclrHipError, match='null argument'):
            call()
    import ctypes
    fake, odd = ctypes.c_void_p(1 << 20), ctypes.c_void_p((1 << 20) + 4)
    with pytest.raises(_lib.SimclrHipError, match='16-byte aligned'):
        L.spectrum_colsum(fake, odd, 4, 64, fake, 0, fake, None)
    with pytest.raises(_lib.SimclrHipError, match='16-byte aligned'):
        L.spectrum_cov(fake, fake, odd, 4, 64, fake, 0, fake, None)

