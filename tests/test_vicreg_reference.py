"""CPU tests of the VICReg restatement (tests/vicreg_reference.py): the Gram form the kernels of csrc/vicreg.hip run against float64
autograd of the direct D x D form and the case of tests/golden/VICREG_HAND_DERIVED.md, the three facts the kernels build on (no centring
backward, the cancelling subtraction, the replica convention), the error budget the GPU tolerances derive from, and the host-side flag
and argument checks."""
import math
import re

import numpy as np
import pytest
import torch

from tests import vicreg_reference as vr
from tests.vicreg_reference import h_all_of, replica_rows, vicreg_direct, vicreg_direct_torch, vicreg_gram

COEFFS = [(25.0, 25.0, 1.0), (1.0, 0.0, 3.0), (2.0, 4.0, 0.5)]


def _case(n, R, D, seed):
    return [h.astype(np.float64) for h in vr.case_views(n, R, D, seed)]


def _autograd(hs, n, coeffs, eps=1e-4, gamma=1.0):
    h_all = torch.tensor(h_all_of(hs, n), dtype=torch.float64, requires_grad=True)
    loss = vicreg_direct_torch(h_all, *coeffs, eps=eps, gamma=gamma)
    loss.backward()
    return float(loss.detach()), h_all.grad.numpy()


# ---------------------------------------------------------------------------------------------------------------- the forms agree
@pytest.mark.parametrize('coeffs', COEFFS)
@pytest.mark.parametrize('n,R,D', [(2, 1, 64), (5, 1, 64), (70, 1, 128), (4, 2, 16), (3, 3, 24)])
def test_gram_form_equals_autograd_of_the_direct_form(n, R, D, coeffs):
    hs = _case(n, R, D, 1)
    N = n * R
    loss, grad = _autograd(hs, n, coeffs)
    direct, gram = vicreg_direct(hs, *coeffs), vicreg_gram(hs, *coeffs)
    assert abs(direct['loss'] - loss) <= 1e-13 * abs(loss)
    assert abs(np.mean(gram['loss']) - loss) <= 1e-13 * abs(loss)
    assert abs(np.mean(gram['inv']) - direct['inv']) <= 1e-13 * direct['inv']
    assert abs(gram['var'][0] - direct['var']) <= 1e-14
    assert abs(np.mean(gram['cov']) - direct['cov']) <= 1e-13 * direct['frob']
    assert abs(np.mean(gram['minuend']) - direct['frob']) <= 1e-13 * direct['frob']
    for r in range(R):
        assert np.abs(gram['grads'][r] - grad[replica_rows(r, n, N)]).max() <= 1e-13 * np.abs(grad).max()
    # some columns on each side of the hinge, so both branches of the predicate are differentiated
    assert 0.1 < (direct['std'] < 1.0).mean() < 0.9


def test_restatement_equals_the_hand_derived_case():
    """tests/golden/VICREG_HAND_DERIVED.md: N = 3, D = 2, eps = 0, gamma = 3, coefficients (2, 4, 1/2)."""
    h = np.array([[1, 0], [3, 1], [5, 2], [1, 2], [3, 0], [-1, 1]], dtype=np.float64)
    kw = dict(sim_coeff=2.0, std_coeff=4.0, cov_coeff=0.5, eps=0.0, gamma=3.0)
    for ref in (vicreg_direct([h], **kw), {k: v[0] for k, v in vicreg_gram([h], **kw).items() if k in ('loss', 'inv', 'var', 'cov')}):
        assert (ref['loss'], ref['inv'], ref['var'], ref['cov']) == pytest.approx((22.5, 7.0, 1.5, 5.0), rel=1e-15)
    gram = vicreg_gram([h], **kw)
    assert gram['minuend'][0] == pytest.approx(22.0, rel=1e-15)
    assert np.array_equal(gram['xc_all'], [[-2, -1], [0, 0], [2, 1], [0, 1], [2, -1], [-2, 0]])
    assert np.array_equal(gram['stats'], [[[4, 1], [2, 1]], [[4, 1], [2, 1]]])
    assert np.array_equal(gram['gram'][0][0], [[5, 0, -5], [0, 0, 0], [-5, 0, 5]])
    assert np.array_equal(gram['gram'][0][1], [[1, -1, 0], [-1, 5, -4], [0, -4, 4]])
    g = gram['grads'][0]
    assert g[0] == pytest.approx([-0.5, -17.0 / 6.0], rel=1e-15)
    assert g[1] == pytest.approx([0.0, 2.0 / 3.0], rel=1e-15)
    _, grad = _autograd([h], 3, (2.0, 4.0, 0.5), eps=0.0, gamma=3.0)
    assert np.abs(g - grad).max() <= 1e-15


# ---------------------------------------------------------------------------------------------------------------- fact 1: no centring backward
@pytest.mark.parametrize('N,D', [(2, 64), (5, 64), (70, 128)])
def test_the_xc_gradient_has_zero_column_sums_and_needs_no_projection(N, D):
    h = _case(N, 1, D, 2)[0]
    for v in range(2):
        xc, var = vr.center(h[v * N:(v + 1) * N])
        g = vr.xc_gradient(xc, var, np.sqrt(var + 1e-4), N, D, 25.0, 1.0, 1.0)
        assert np.abs(g.sum(axis=0)).max() <= 1e-14 * np.abs(g).max() * N
        projected = g - g.mean(axis=0)                      # the backward of xc = h - colmean(h)
        assert np.abs(projected - g).max() <= 1e-15 * np.abs(g).max() * N
    loss, grad = _autograd([h], N, (25.0, 25.0, 1.0))
    assert np.abs(vicreg_gram([h])['grads'][0] - grad).max() <= 3e-15 * max(1.0, np.abs(grad).max())


# ---------------------------------------------------------------------------------------------------------------- invariances
def test_row_permutation_of_both_views_changes_nothing():
    n, D = 12, 64
    h = _case(n, 1, D, 3)[0]
    perm = np.random.default_rng(0).permutation(n)
    a, b = vicreg_gram([h]), vicreg_gram([np.concatenate([h[:n][perm], h[n:][perm]])])
    for k in ('loss', 'inv', 'var', 'cov'):
        assert abs(a[k][0] - b[k][0]) <= 1e-13 * max(abs(a[k][0]), a['minuend'][0])
    assert np.abs(a['grads'][0][np.concatenate([perm, n + perm])] - b['grads'][0]).max() <= 1e-13 * np.abs(a['grads'][0]).max()


def test_a_constant_added_to_one_view_changes_the_invariance_term_alone():
    n, D = 12, 64
    h = _case(n, 1, D, 4)[0]
    shifted = h.copy()
    shifted[n:] += np.random.default_rng(1).standard_normal(D)
    a, b = vicreg_gram([h]), vicreg_gram([shifted])
    assert abs(a['var'][0] - b['var'][0]) <= 1e-13 and abs(a['cov'][0] - b['cov'][0]) <= 1e-13 * a['minuend'][0]
    assert abs(a['inv'][0] - b['inv'][0]) > 0.1


def test_identical_views_have_zero_invariance_exactly():
    v = np.random.default_rng(5).standard_normal((9, 64))
    ref = vicreg_gram([np.concatenate([v, v])])
    assert ref['inv'][0] == 0.0 and vicreg_direct([np.concatenate([v, v])])['inv'] == 0.0
    assert ref['var'][0] > 0.0 or ref['cov'][0] > 0.0
    emu = vr.vicreg_emulated([np.concatenate([v, v]).astype(np.float32)], 0)
    assert float(emu['inv']) == 0.0


def test_columns_at_or_above_the_hinge_add_no_variance_and_no_gradient():
    """sim_coeff = cov_coeff = 0 leaves the variance term alone: columns with std >= gamma contribute neither value nor gradient."""
    n, D = 20, 64
    h = _case(n, 1, D, 6)[0]
    ref = vicreg_gram([h], 0.0, 25.0, 0.0)
    std = ref['stats'][:, 1]
    above = std >= 1.0
    assert above.any() and (~above).any()
    assert ref['var'][0] == pytest.approx(0.5 * np.maximum(0.0, 1.0 - std)[~above].sum() / D, rel=1e-14)
    g = ref['grads'][0].reshape(2, n, D)
    for v in range(2):
        assert np.all(g[v][:, above[v]] == 0.0) and np.all(np.abs(g[v][:, ~above[v]]).max(axis=0) > 0.0)


def test_a_collapsed_column_gives_the_full_hinge_and_a_finite_zero_gradient():
    n, D, eps = 10, 64, 1e-4
    h = _case(n, 1, D, 7)[0]
    h[:, 3] = 2.5                                         # constant in both views
    ref = vicreg_gram([h], 0.0, 1.0, 0.0, eps=eps)
    assert ref['stats'][0, 0, 3] == 0.0 and ref['stats'][0, 1, 3] == math.sqrt(eps)
    others = np.delete(np.arange(D), 3)
    hinge = np.maximum(0.0, 1.0 - ref['stats'][:, 1])
    assert hinge[0, 3] == hinge[1, 3] == 1.0 - math.sqrt(eps)
    assert ref['var'][0] == pytest.approx(0.5 * (hinge[:, others].sum() + 2.0 * (1.0 - math.sqrt(eps))) / D, rel=1e-14)
    assert np.all(np.isfinite(ref['grads'][0])) and np.all(ref['grads'][0][:, 3] == 0.0)
    zero_eps = vicreg_gram([h], 25.0, 25.0, 1.0, eps=0.0)            # std = 0 exactly: still finite
    assert np.all(np.isfinite(zero_eps['grads'][0])) and zero_eps['stats'][0, 1, 3] == 0.0
    emu = vr.vicreg_emulated([h.astype(np.float32)], 0, eps=0.0)
    assert np.all(np.isfinite(emu['grad']))


# ---------------------------------------------------------------------------------------------------------------- fact 3: replicas
@pytest.mark.parametrize('R', [1, 2, 3])
def test_replica_conventions(R):
    """mean_r loss_r = L, and what the device returns (grad_scale * R * dL/dh_r with grad_scale = 1 / R), summed over the replicas by the
    gradient synchronisation of the parameters, is the gradient of L: the per-replica blocks tile dL/dh_all."""
    n, D, coeffs = 6, 64, (2.0, 4.0, 0.5)
    hs = _case(n, R, D, 20 + R)
    N = R * n
    loss, grad = _autograd(hs, n, coeffs)
    gram = vicreg_gram(hs, *coeffs)
    one = vicreg_gram([h_all_of(hs, n)], *coeffs)                     # the whole batch on one replica
    assert abs(np.mean(gram['loss']) - loss) <= 1e-13 * abs(loss) and abs(one['loss'][0] - loss) <= 1e-13 * abs(loss)
    for k in ('inv', 'cov', 'minuend'):
        assert abs(np.mean(gram[k]) - one[k][0]) <= 1e-13 * one['minuend'][0]
        assert R == 1 or max(gram[k]) - min(gram[k]) > 0.0            # the shares differ: only their mean is the term
    assert all(v == one['var'][0] for v in gram['var'])               # var is the global value on every replica
    tiled = np.zeros((2 * N, D))
    for r in range(R):
        tiled[replica_rows(r, n, N)] = (1.0 / R) * R * gram['grads'][r]
    assert np.abs(tiled - grad).max() <= 1e-13 * np.abs(grad).max()


# ---------------------------------------------------------------------------------------------------------------- fact 2: the subtraction cancels
def test_whitened_case_cancels_and_the_emulation_stays_within_its_budget():
    hs = vr.whitened_views()
    ref = vicreg_gram(hs)
    assert ref['minuend'][0] >= 1000.0 * abs(ref['cov'][0])
    assert ref['minuend'][0] == pytest.approx(2 * 0.81 ** 2, rel=1e-6) and abs(ref['cov'][0]) < 1e-9
    assert ref['stats'][:, 0] == pytest.approx(0.81, rel=1e-6)        # every column sits below the hinge
    measured = vr.measured_whitened_budget()
    print(measured)
    for k, recorded in vr.WHITENED_ERROR.items():
        assert recorded / 4.0 <= measured[k] <= recorded, (k, measured[k], recorded)
        assert vr.WHITENED_TOL[k] == 4.0 * recorded
    # a float32 result of this size is rounding noise of either sign: reported as computed
    emu = vr.vicreg_emulated(hs, 0)
    assert abs(float(emu['cov']) - ref['cov'][0]) <= vr.WHITENED_ERROR['cov'] * ref['minuend'][0]


def test_error_budget_of_every_gpu_case_matches_the_recorded_values():
    """The emulation error of every GPU case, re-measured, against the table of tests/golden/VICREG_HAND_DERIVED.md ("Error budget"),
    from which the GPU tolerances (4x) derive."""
    measured = vr.measured_budget()
    print(measured)
    assert list(measured) == vr.MAIN_SHAPES == list(vr.EMULATION_ERROR)
    for case, worst in measured.items():
        for k, recorded in vr.EMULATION_ERROR[case].items():
            assert 0.5 * recorded <= worst[k] <= recorded, (case, k, worst[k], recorded)
            assert vr.TOL[case][k] == 4.0 * recorded and vr.TOL[case][k] < 5e-6
    centre = vr.measured_center_budget()
    print(centre)
    assert list(centre) == vr.CENTER_SHAPES == list(vr.CENTER_ERROR)
    for case, worst in centre.items():
        for k, recorded in vr.CENTER_ERROR[case].items():
            assert 0.5 * recorded <= worst[k] <= recorded, (case, k, worst[k], recorded)
    table = open(__file__.replace('test_vicreg_reference.py', 'golden/VICREG_HAND_DERIVED.md')).read()
    for (n, N, D, rank), e in vr.EMULATION_ERROR.items():
        row = re.search(r'^\| %d \| %d \| %d \| %d \| (\d+)[^|]*\| (.*) \|$' % (n, N, D, rank), table, re.M)
        assert row and int(row.group(1)) == vr.k_splits(n, N, D)[0], (n, N, D, rank)
        assert [float(x) for x in row.group(2).split(' | ')] == [e[k] for k in ('loss', 'inv', 'var', 'cov', 'grad')]
    for (N, D), e in vr.CENTER_ERROR.items():
        row = re.search(r'^\| %d \| %d \| ([^|]*) \| ([^|]*) \| ([^|]*) \|$' % (N, D), table, re.M)
        assert row and [float(x) for x in row.groups()] == [e[k] for k in ('xc', 'stat_var', 'stat_std')]


def test_split_rule_covers_one_two_and_many_parts_and_a_ragged_last_part():
    splits = {s[:3]: vr.k_splits(*s[:3]) for s in vr.MAIN_SHAPES}
    counts = [S for S, _ in splits.values()]
    assert 1 in counts and 2 in counts and any(S >= 4 for S in counts)
    assert any(S > 1 and D % kc != 0 for (_, _, D), (S, kc) in splits.items())          # the last part is shorter than the others
    for (n, N, D), (S, kc) in splits.items():
        assert kc % 32 == 0 and (S - 1) * kc < D <= S * kc
    assert vr.k_splits(512, 512, 8192) == (8, 1024) and vr.k_splits(512, 4096, 2048) == (1, 2048)
    assert vr.k_splits(256, 2048, 8192) == (1, 8192) and vr.k_splits(512, 512, 128) == (1, 128)


def test_library_split_rule_is_the_restated_one():
    from simclr_amd._lib import lib
    L = lib()
    shapes = [s[:3] for s in vr.MAIN_SHAPES] + [(512, 512, 128), (512, 4096, 2048), (512, 512, 8192), (256, 2048, 8192), (4096, 4096, 8192),
                                                 (70, 140, 8192), (1, 2, 8192), (300, 300, 1024)]
    for n, N, D in shapes:
        assert L.vicreg_k_splits(n, N, D) == vr.k_splits(n, N, D)[0], (n, N, D)
        assert L.vicreg_workspace_bytes(n, N, D) > 0 and L.vicreg_fwd_workgroups(n, N, D) >= 2
    for n, N, D in [(4, 4, 100), (4, 4, 8256), (0, 4, 64), (4, 6, 64), (1, 1, 64)]:
        assert L.vicreg_k_splits(n, N, D) == 0 and L.vicreg_workspace_bytes(n, N, D) == 0 and L.vicreg_gram_pitch(n, N, D) == 0


# ---------------------------------------------------------------------------------------------------------------- flags, refusals, names
def test_vicreg_flags_parse_and_default():
    from simclr_amd import run
    from simclr_amd.flags import FLAGS
    try:
        FLAGS.reset()
        assert FLAGS.contrastive_loss == 'ntxent'
        assert (FLAGS.vicreg_sim_coeff, FLAGS.vicreg_std_coeff, FLAGS.vicreg_cov_coeff) == (25.0, 25.0, 1.0)
        assert not run.vicreg_loss_on()
        FLAGS.parse(['--contrastive_loss=vicreg', '--vicreg_sim_coeff=10', '--vicreg_std_coeff=0', '--vicreg_cov_coeff=2.5', '--proj_out_dim=8192'])
        assert (FLAGS.contrastive_loss, FLAGS.vicreg_sim_coeff, FLAGS.vicreg_std_coeff, FLAGS.vicreg_cov_coeff) == ('vicreg', 10.0, 0.0, 2.5)
        assert run.check_contrastive_loss_flags() is False and run.vicreg_loss_on()
        assert not run.generalized_loss_on() and not run.supcon_loss_on() and not run.barlow_loss_on() and not run.byol_loss_on()
        FLAGS.reset()
        FLAGS.update(contrastive_loss='vicreg', proj_head_mode='none')                 # the encoder width: 2048 for ResNet-50
        assert run.barlow_loss_width() == 2048 and run.check_contrastive_loss_flags() is False
        FLAGS.update(hidden_norm=False, temperature=-1.0)                              # ignored
        assert run.check_contrastive_loss_flags() is False
    finally:
        FLAGS.reset()


def test_metric_names_of_the_vicreg_loss():
    from simclr_amd import run
    from simclr_amd.flags import FLAGS
    try:
        FLAGS.reset()
        FLAGS.update(contrastive_loss='vicreg', proj_out_dim=64)
        assert sorted(run.build_metrics()) == ['train/contrast_loss', 'train/supervised_acc', 'train/supervised_loss', 'train/total_loss',
                                               'train/vicreg_cov', 'train/vicreg_inv', 'train/vicreg_var', 'train/weight_decay']
        FLAGS.update(lineareval_while_pretraining=False)
        assert sorted(run.build_metrics()) == ['train/contrast_loss', 'train/total_loss', 'train/vicreg_cov', 'train/vicreg_inv',
                                               'train/vicreg_var', 'train/weight_decay']
        assert len(run.build_metrics()) <= 16
        FLAGS.update(train_mode='finetune')                              # fine-tuning ignores the flag
        assert sorted(run.build_metrics()) == ['train/supervised_acc', 'train/supervised_loss', 'train/total_loss', 'train/weight_decay']
        assert run.check_contrastive_loss_flags() is False and not run.vicreg_loss_on()
    finally:
        FLAGS.reset()


def test_value_errors_before_any_device_work():
    from simclr_amd import objective, ops, run
    from simclr_amd.flags import FLAGS
    assert (ops.VICREG_DIM_STEP, ops.VICREG_MIN_DIM, ops.VICREG_MAX_DIM) == (64, 64, 8192)
    for D in (100, 8256, 32, 0):
        assert not ops.vicreg_dim_ok(D)
        with pytest.raises(ValueError, match='multiples of 64 in \\[64, 8192\\]'):
            ops._vicreg_check_dim(D)
    for D in (64, 320, 2048, 8192):
        assert ops.vicreg_dim_ok(D)
    h, stats = torch.zeros(8, 64), torch.zeros(2, 2, 64, dtype=torch.float64)
    with pytest.raises(ValueError, match='multiples of 64'):
        objective.add_vicreg_loss(torch.zeros(8, 100))
    with pytest.raises(ValueError, match='global batch of at least 2'):
        objective.add_vicreg_loss(torch.zeros(2, 64))
    for bad in (-1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='finite and >= 0'):
            objective.add_vicreg_loss(h, std_coeff=bad)
        with pytest.raises(ValueError, match='finite and >= 0'):
            ops.vicreg_fwd(h, h, stats, 4, 0, cov_coeff=bad)
        with pytest.raises(ValueError, match='finite and >= 0'):
            ops.vicreg_bwd(h, h, stats, 4, 0, bad, 25.0, 1.0, 1.0, 1.0, None)
    with pytest.raises(ValueError, match='eps must be >= 0'):
        objective.add_vicreg_loss(h, eps=-1e-4)
    with pytest.raises(ValueError, match='eps must be >= 0'):
        ops.vicreg_center(h, eps=-1e-4)
    with pytest.raises(ValueError, match='multiples of 64'):
        ops.vicreg_center(torch.zeros(8, 8256))
    with pytest.raises(ValueError, match='N >= 2'):
        ops.vicreg_center(torch.zeros(2, 64))
    with pytest.raises(ValueError, match='N = R\\*n'):
        ops.vicreg_fwd(torch.zeros(10, 64), torch.zeros(10, 64), stats, 3, 0)          # N = 5 is no multiple of n = 3
    with pytest.raises(ValueError, match='N = R\\*n'):
        ops.vicreg_fwd(h, h, stats, 0, 0)
    with pytest.raises(ValueError, match='N = R\\*n'):
        ops.vicreg_fwd(torch.zeros(2, 64), torch.zeros(2, 64), stats, 1, 0)            # N = 1
    with pytest.raises(ValueError, match='rank 2'):
        ops.vicreg_fwd(h, h, stats, 2, 2)
    with pytest.raises(ValueError, match='float64 stats'):
        ops.vicreg_fwd(h, h, stats.float(), 4, 0)
    base = ['--dataset=synthetic', '--contrastive_loss=vicreg', '--train_steps=1']
    try:
        for extra, msg in ((['--vicreg_sim_coeff=-0.1'], 'vicreg_sim_coeff must be >= 0 and finite'),
                           (['--vicreg_std_coeff=inf'], 'vicreg_std_coeff must be >= 0 and finite'),
                           (['--vicreg_cov_coeff=nan'], 'vicreg_cov_coeff must be >= 0 and finite'),
                           (['--proj_out_dim=100'], 'vicreg needs a loss width'), (['--proj_out_dim=8256'], 'vicreg needs a loss width'),
                           (['--proj_out_dim=32'], 'vicreg needs a loss width'),
                           (['--proj_head_mode=none', '--width_multiplier=8'], 'vicreg needs a loss width'),
                           (['--train_batch_size=1'], 'train_batch_size >= 2')):
            FLAGS.reset()
            with pytest.raises(ValueError, match=msg):
                run.main(base + extra)
        FLAGS.reset()
        FLAGS.update(contrastive_loss='vicreg', train_mode='finetune', proj_out_dim=100, vicreg_sim_coeff=-1.0)
        assert run.check_contrastive_loss_flags() is False
        FLAGS.update(train_mode='pretrain', mode='eval')
        assert run.check_contrastive_loss_flags() is False
    finally:
        FLAGS.reset()


def test_unknown_loss_message_still_matches_the_earlier_patterns():
    from simclr_amd import run
    from simclr_amd.flags import FLAGS
    try:
        FLAGS.reset()
        FLAGS.update(contrastive_loss='vicregg')
        with pytest.raises(ValueError) as e:
            run.check_contrastive_loss_flags()
        msg = str(e.value)
        assert re.search("must be 'dino' or 'ntxent' .*'barlow' or 'byol' or 'mocov2' \\(got 'vicregg'\\), or 'swav'", msg)
        assert re.search("must be 'dino' or 'ntxent' .*'barlow' or 'byol' or 'mocov2' \\(got 'vicregg'\\)", msg)
        assert re.search("'ntxent' or 'generalized' or 'supcon'", msg)
        assert msg.endswith("or 'swav' or 'vicreg'")
    finally:
        FLAGS.reset()


def test_handle_names_of_the_loss():
    """add_vicreg_loss documents the handle the step and the metrics read."""
    from simclr_amd import objective
    doc = objective.add_vicreg_loss.__doc__
    for name in ('.invariance', '.variance', '.covariance', '.centered', '.backward_start', '.backward_finish'):
        assert name in doc, name
    import inspect
    sig = inspect.signature(objective.add_vicreg_loss)
    assert [(k, p.default) for k, p in sig.parameters.items()][1:] == [
        ('sim_coeff', 25.0), ('std_coeff', 25.0), ('cov_coeff', 1.0), ('eps', 1e-4), ('gamma', 1.0), ('strategy', None), ('overlap', None)]
