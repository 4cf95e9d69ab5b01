"""CPU tests of the representation diagnostics: the three identities the kernels rest on (direct form == Gram form), the hand cases of
tests/golden/REPR_HAND_DERIVED.md in float64, the invariances, every refusal that needs no device, the flags, the metric names under
every loss, the emulation's error budget re-measured, and the emulation mutants against the gates of the device case table."""
import math

import numpy as np
import pytest

from tests import repr_reference as rr


@pytest.fixture(autouse=True)
def _reset_flags():
    from simclr_amd.flags import FLAGS
    FLAGS.reset()
    yield
    FLAGS.reset()


SMALL = [(N, D, t, fam) for N, D, t, fam in rr.CASES if N * D <= 200 * 256]


# ---------------------------------------------------------------------------------------------------------------- identities
def test_distance_identity_needs_no_mean_term():
    z = rr.case_views(65, 128, 'clusters').astype(np.float64)[:65]
    xc = z - z.mean(0)
    G = xc @ xc.T
    r = np.diag(G)
    d2 = ((z[:, None, :] - z[None, :, :]) ** 2).sum(-1)
    assert np.abs(r[:, None] + r[None, :] - 2.0 * G - d2).max() < 1e-14


def test_trace_and_frobenius_identities():
    for fam in rr.FAMILIES:
        z = rr.case_views(63, 64, fam).astype(np.float64)[:63]
        xc = z - z.mean(0)
        G, C = xc @ xc.T, xc.T @ xc / 62.0
        assert abs(np.trace(C) - np.trace(G) / 62.0) < 1e-14 * np.trace(C)
        assert abs((C * C).sum() - (G * G).sum() / 62.0 ** 2) < 1e-13 * (C * C).sum()
        lam = np.linalg.eigvalsh(C)
        pr = np.trace(G) ** 2 / (G * G).sum()
        assert abs(pr - lam.sum() ** 2 / (lam * lam).sum()) < 1e-10 * pr and 1.0 - 1e-9 <= pr <= min(64, 62) + 1e-9


@pytest.mark.parametrize('N,D,t,fam', SMALL, ids=lambda v: str(v))
def test_direct_form_equals_gram_form(N, D, t, fam):
    z = rr.case_views(N, D, fam)
    a, b = rr.direct(z, t), rr.gram(z, t)
    assert np.all(np.abs(a - b) <= 1e-11 * np.maximum(np.abs(a), 1.0)), (a, b)
    assert 0.0 <= a[0] <= 4.0 and -4.0 * t <= a[1] <= 0.0 and a[2] >= 0.0 and 1.0 - 1e-9 <= a[3] <= min(D, N - 1) + 1e-9


# ---------------------------------------------------------------------------------------------------------------- hand cases
def test_hand_signed_basis_rows():
    for f in (rr.direct, rr.gram):
        assert np.abs(f(rr.hand_basis(64), 2.0) - np.array([0.0, -4.0, 1.0, 63.0])).max() < 1e-12
    assert np.abs(rr.direct(rr.hand_basis(64), 5.0)[1] + 10.0) < 1e-12


def test_hand_antipodal_rows():
    want = rr.hand_antipodal_values(64, 64, 2.0)
    assert abs(want[1] - (-0.708801)) < 1e-6 and abs(want[2] - math.sqrt(64 / 63) / 8) < 1e-15
    for f in (rr.direct, rr.gram):
        assert np.abs(f(rr.hand_antipodal(64, 64), 2.0) - want).max() < 1e-12


def test_hand_identical_rows_are_all_zero():
    for f in (rr.direct, rr.gram):
        assert np.abs(f(rr.hand_collapsed(), 2.0)).max() < 1e-12
    assert np.array_equal(rr.emulate(rr.hand_collapsed(), 2.0), np.zeros(4))


def test_two_rows_have_rank_one():
    z = rr.case_views(2, 64, 'gauss')
    for f in (rr.direct, rr.gram):
        assert abs(f(z, 2.0)[3] - 1.0) < 1e-12
    assert abs(rr.emulate(z, 2.0)[3] - 1.0) <= rr.ulp32(1.0)


def test_view_swap_and_image_permutation_change_nothing():
    z = rr.case_views(63, 64, 'gauss').astype(np.float64)
    base = rr.direct(z, 2.0)
    perm = np.random.RandomState(3).permutation(63)
    for other in (np.concatenate([z[63:], z[:63]]), np.concatenate([z[:63][perm], z[63:][perm]])):
        assert np.abs(rr.direct(other, 2.0) - base).max() < 1e-12


def test_scale_of_the_unnormalised_input_changes_nothing():
    h = np.random.RandomState(5).randn(40, 64)
    assert np.abs(rr.direct(rr.normalize(3.0 * h), 2.0) - rr.direct(rr.normalize(h), 2.0)).max() < 1e-13


# ---------------------------------------------------------------------------------------------------------------- refusals, flags, names
def test_abi_refuses_bad_arguments():
    import ctypes
    from simclr_amd import _lib
    L = _lib.lib()
    assert L.repr_workspace_bytes(64, 64) > 0 and L.abi_version() == 8
    for N, D in ((64, 100), (64, 32), (64, 8256), (1, 64), (65537, 64), (0, 64)):
        assert L.repr_workspace_bytes(N, D) == 0, (N, D)
    fake = ctypes.c_void_p(1 << 20)          # never dereferenced: every call below is refused before any launch
    t = ctypes.c_float
    for N, D, tt, args, msg in ((64, 100, 2.0, (fake, fake, fake), 'multiple of 64'), (64, 8256, 2.0, (fake, fake, fake), 'multiple of 64'),
                                (1, 64, 2.0, (fake, fake, fake), '2 <= N <= 65536'), (65537, 64, 2.0, (fake, fake, fake), '2 <= N <= 65536'),
                                (64, 64, 0.0, (fake, fake, fake), r't must lie in \(0, 16\]'), (64, 64, 16.5, (fake, fake, fake), 't must lie'),
                                (64, 64, float('nan'), (fake, fake, fake), 't must lie'), (64, 64, float('inf'), (fake, fake, fake), 't must lie'),
                                (64, 64, -1.0, (fake, fake, fake), 't must lie'),
                                (64, 64, 2.0, (None, fake, fake), 'null argument'), (64, 64, 2.0, (fake, None, fake), 'null argument'),
                                (64, 64, 2.0, (fake, fake, None), 'null argument'),
                                (64, 64, 2.0, (fake, ctypes.c_void_p((1 << 20) + 8), fake), '16-byte aligned')):
        with pytest.raises(_lib.SimclrHipError, match=msg):
            L.repr_stats(args[0], N, D, t(tt), args[1], args[2], None)


def test_the_case_table_reaches_both_tile_edges():
    """The pairs launch has two instantiations; the table holds shapes of both, the 128-wide one with a ragged and a full last tile."""
    from simclr_amd import ops
    assert {s: ops.repr_tile_edge(*s) for s in rr.SHAPES} == rr.EDGES
    assert sorted(s for s, e in rr.EDGES.items() if e == 128) == [(1409, 64), (1536, 64)] and 1409 % 128 == 1 and 1536 % 128 == 0
    assert ops.repr_tile_edge(1408, 64) == 64 and ops.repr_tile_edge(4096, 128) == 128 and ops.repr_tile_edge(1, 64) == 0


def test_ops_predicates():
    from simclr_amd import ops
    assert [D for D in (0, 32, 64, 100, 128, 8192, 8256) if ops.repr_dim_ok(D)] == [64, 128, 8192]
    assert [t for t in (-1.0, 0.0, 1e-3, 2.0, 16.0, 16.5, float('inf'), float('nan')) if ops.repr_t_ok(t)] == [1e-3, 2.0, 16.0]


def _parse(*args):
    from simclr_amd.flags import FLAGS
    FLAGS.reset()
    FLAGS.parse(['--dataset=synthetic'] + list(args))
    return FLAGS


def test_flags_parse_and_default_off():
    from simclr_amd import run
    F = _parse()
    assert F.repr_metrics_steps == 0 and F.repr_uniform_t == 2.0 and run.check_repr_flags() == 0 and run.repr_metrics_steps() == 0
    F = _parse('--repr_metrics_steps=5', '--repr_uniform_t=3.5')
    assert F.repr_metrics_steps == 5 and F.repr_uniform_t == 3.5 and run.check_repr_flags() == 5 and run.repr_metrics_steps() == 5


@pytest.mark.parametrize('args,flag', [
    (['--repr_metrics_steps=-1'], 'repr_metrics_steps'),
    (['--repr_uniform_t=0'], 'repr_uniform_t'), (['--repr_uniform_t=16.5'], 'repr_uniform_t'), (['--repr_uniform_t=nan'], 'repr_uniform_t'),
    (['--repr_uniform_t=-2'], 'repr_uniform_t'),
    (['--repr_metrics_steps=1', '--proj_out_dim=100'], 'repr_metrics_steps'),
    (['--repr_metrics_steps=1', '--proj_out_dim=32'], 'repr_metrics_steps'),
    (['--repr_metrics_steps=1', '--train_batch_size=1'], 'repr_metrics_steps'),
    (['--repr_metrics_steps=1', '--train_batch_size=65537'], 'repr_metrics_steps'),
], ids=lambda v: ','.join(v) if isinstance(v, list) else v)
def test_bad_flags_are_refused_before_any_device_work(args, flag, monkeypatch):
    from simclr_amd import run
    _parse(*args)
    with pytest.raises(ValueError, match='--' + flag):
        run.check_repr_flags()
    # run.main raises the same error, before it touches the device
    monkeypatch.setattr(run, 'init_distributed', lambda: pytest.fail('run.main reached the device work'))
    with pytest.raises(ValueError, match='--' + flag):
        run.main(['--dataset=synthetic'] + args)


def test_finetune_and_eval_ignore_the_flags():
    from simclr_amd import run
    for extra in (['--train_mode=finetune'], ['--mode=eval']):
        _parse('--repr_metrics_steps=-3', '--repr_uniform_t=99', '--proj_out_dim=100', *extra)
        assert run.check_repr_flags() == 0 and run.repr_metrics_steps() is None
        assert not any('repr' in n for n in run.build_metrics())
    # a width the kernels refuse is fine while the measurement is off
    _parse('--proj_out_dim=100')
    assert run.check_repr_flags() == 0


def test_metric_names_with_and_without_the_flag_under_every_loss():
    from simclr_amd import metrics, run
    from simclr_amd import pretrain_losses as loss_lib
    from simclr_amd.flags import FLAGS
    four = [n for n, _ in metrics.REPR_METRICS]
    assert four == ['train/repr_align', 'train/repr_uniform', 'train/repr_std', 'train/repr_rank']
    assert len(loss_lib.LOSSES) >= 9
    for name in loss_lib.LOSSES:
        FLAGS.reset()
        FLAGS.update(contrastive_loss=name)
        off = sorted(run.build_metrics())
        assert not any('repr' in n for n in off)
        FLAGS.update(repr_metrics_steps=0)
        assert sorted(run.build_metrics()) == off
        FLAGS.update(repr_metrics_steps=3)
        on = sorted(run.build_metrics())
        assert on == sorted(off + four), (name, on)
        assert len(on) <= 13 <= 16, (name, on)            # the bank of run.make_single_step holds 16 running sums


def test_handle_refuses_bad_input_before_any_launch():
    import torch
    from simclr_amd import metrics, ops
    for bad, msg in ((torch.zeros(8, 100), 'multiples of 64'), (torch.zeros(7, 64), 'both views'), (torch.zeros(8, 64, dtype=torch.float64), 'both views'),
                     (torch.zeros(64), 'both views')):
        with pytest.raises(ValueError, match=msg):
            metrics.representation_stats(bad)
    for t in (0.0, 17.0, float('nan')):
        with pytest.raises(ValueError, match='t must lie'):
            metrics.representation_stats(torch.zeros(8, 64), t=t)
    for bad, msg in ((torch.zeros(8, 100), 'multiples of 64'), (torch.zeros(2, 64), 'rows per view'), (torch.zeros(7, 64), r'\[2N, D\]'),
                     (torch.zeros(8, 64, dtype=torch.float64), r'\[2N, D\]')):
        with pytest.raises(ValueError, match=msg):
            ops.repr_stats(bad)
    with pytest.raises(ValueError, match='t must lie'):
        ops.repr_stats(torch.zeros(8, 64), t=-1.0)
    with pytest.raises(ValueError, match='rows per view'):
        ops.repr_workspace(1, 64, 'cpu')
    with pytest.raises(ValueError, match='multiples of 64'):
        ops.repr_workspace(8, 96, 'cpu')


# ---------------------------------------------------------------------------------------------------------------- budget and mutants
def test_emulation_error_budget_remeasured():
    """The emulation's error against float64 over the device case table, per output in float32 ulps of the float64 value, stays inside
    the recorded budget (tests/golden/REPR_HAND_DERIVED.md); every case is far from the collapse branch."""
    worst = dict.fromkeys(rr.NAMES, 0.0)
    for c in rr.CASES:
        z, ref, emu, gate = rr.case(*c)
        assert min(rr.trace_cov(z)) > 1e-9, c
        for k, name in enumerate(rr.NAMES):
            worst[name] = max(worst[name], abs(emu[k] - ref[k]) / rr.ulp32(ref[k]))
            assert gate[k] >= rr.ulp32(ref[k])
    print('emulation error, ulps: %s' % worst)
    for name in rr.NAMES:
        assert worst[name] <= rr.EMULATION_BUDGET_ULPS[name], (name, worst[name])


@pytest.mark.parametrize('mutant', sorted(rr.MUTANTS))
def test_comparator_rejects_the_mutant_on_every_case(mutant):
    """A wrong reading of the definition, run through the same emulation, misses the device gate of the output it changes on every case
    of the table (and the unmutated emulation passes it, by construction)."""
    k = rr.NAMES.index(rr.MUTANTS[mutant])
    for c in rr.CASES:
        z, ref, emu, gate = rr.case(*c)
        assert rr.compare(emu, ref, gate)[1].all(), c
        N, D, t, fam = c
        err, ok = rr.compare(rr.emulate(z, t, key=(N, D, fam), mutant=mutant), ref, gate)
        assert not ok[k], (mutant, c, err[k], gate[k])
