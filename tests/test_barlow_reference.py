"""tests/barlow_reference.py (the float64 restatement the device tests of the Barlow Twins loss compare against) pinned on the CPU:
both of its forms against torch float64 autograd of the direct D x D form, the case worked on paper in
tests/golden/BARLOW_HAND_DERIVED.md, the invariances of the loss and the per-replica conventions; then the flags, the metric names and
the refusals that precede any device work."""
import numpy as np
import pytest
import torch

from tests.barlow_reference import barlow_direct, barlow_gram, h_all_of, replica_rows


def _case(n, R, D, seed, shift=0.0):
    g = np.random.default_rng(seed)
    return [g.standard_normal((2 * n, D)) + shift for _ in range(R)]


def _torch_direct(hs, lam, ls, eps):
    """L of the direct form with torch operations only; returns (L, on, off, leaves)."""
    R, n = len(hs), hs[0].shape[0] // 2
    N = R * n
    leaves = [torch.tensor(h, dtype=torch.float64, requires_grad=True) for h in hs]
    h_all = torch.cat([h[:n] for h in leaves] + [h[n:] for h in leaves], 0)

    def std(x):
        return (x - x.mean(0)) / torch.sqrt(x.var(0, unbiased=False) + eps)
    C = std(h_all[:N]).t() @ std(h_all[N:]) / N
    on = ((1.0 - torch.diagonal(C)) ** 2).sum()
    off = (C ** 2).sum() - (torch.diagonal(C) ** 2).sum()
    return ls * (on + lam * off), on, off, leaves


@pytest.mark.parametrize('n,R,D,lam,ls', [(5, 1, 64, 0.0051, 1.0), (35, 2, 128, 1.0, 0.024), (256, 1, 64, 0.0051, 1.0), (4, 3, 6, 0.3, 2.0)])
def test_both_forms_equal_autograd_of_the_direct_form(n, R, D, lam, ls):
    hs = _case(n, R, D, n + R + D)
    N = R * n
    L, on, off, leaves = _torch_direct(hs, lam, ls, 1e-5)
    L.backward()
    direct, gram = barlow_direct(hs, lam, ls), barlow_gram(hs, lam, ls)
    Lf, onf, offf = float(L.detach()), float(on.detach()), float(off.detach())
    assert abs(direct['loss'] - Lf) <= 1e-12 * abs(Lf)
    assert abs(direct['on_diag'] - onf) <= 1e-12 * onf and abs(direct['off_diag'] - offf) <= 1e-12 * max(offf, direct['frob'])
    # the per-replica values of the Gram form average to the loss
    assert abs(np.mean(gram['loss']) - Lf) <= 1e-12 * abs(Lf)
    assert abs(np.mean(gram['off_diag']) - offf) <= 1e-11 * direct['frob']
    assert abs(gram['on_diag'][0] - onf) <= 1e-12 * onf
    want = [leaf.grad.numpy() for leaf in leaves]
    scale = max(np.abs(w).max() for w in want)
    for r in range(R):
        assert np.abs(direct['grad_all'][replica_rows(r, n, N)] - want[r]).max() <= 1e-11 * scale
        assert np.abs(gram['grads'][r] - want[r]).max() <= 1e-11 * scale


def test_restatement_equals_the_hand_derived_case():
    """tests/golden/BARLOW_HAND_DERIVED.md: N = 2, D = 2, eps = 0, lambda = 1/2."""
    h = np.array([[0.0, 0.0], [2.0, 4.0], [1.0, 5.0], [3.0, 1.0]])
    lam = 0.5
    for ref in (barlow_direct([h], lam, 1.0, 0.0), barlow_gram([h], lam, 1.0, 0.0)):
        loss = ref['loss'] if np.isscalar(ref['loss']) else ref['loss'][0]
        on = ref['on_diag'] if np.isscalar(ref['on_diag']) else ref['on_diag'][0]
        off = ref['off_diag'] if np.isscalar(ref['off_diag']) else ref['off_diag'][0]
        assert abs(on - 4.0) < 1e-14 and abs(off - 2.0) < 1e-14 and abs(loss - 5.0) < 1e-14
    gram = barlow_gram([h], lam, 1.0, 0.0)
    assert np.abs(gram['zhat_all'] - np.array([[-1.0, -1.0], [1.0, 1.0], [-1.0, 1.0], [1.0, -1.0]])).max() < 1e-15
    assert np.abs(gram['gram'][0] - np.array([[[2.0, -2.0], [-2.0, 2.0]]] * 2)).max() < 1e-14
    want_gz = np.array([[-lam, -lam - 2.0], [lam, lam + 2.0], [-lam, lam + 2.0], [lam, -lam - 2.0]])
    assert np.abs(gram['grads_zhat'][0] - want_gz).max() < 1e-14
    assert np.abs(barlow_direct([h], lam, 1.0, 0.0)['grad_zhat'] - want_gz).max() < 1e-14
    # two rows standardise to -1 / +1 whatever their values: the loss does not depend on h, its gradient is zero
    assert np.abs(gram['grads'][0]).max() < 1e-14


def test_joint_permutation_of_samples_changes_nothing():
    n, D = 9, 8
    hs = _case(n, 1, D, 3)
    perm = np.random.default_rng(1).permutation(n)
    rows = np.concatenate([perm, n + perm])
    a, b = barlow_gram(hs, 0.05), barlow_gram([hs[0][rows]], 0.05)
    assert abs(a['loss'][0] - b['loss'][0]) <= 1e-13 * abs(a['loss'][0])
    assert np.abs(a['grads'][0][rows] - b['grads'][0]).max() <= 1e-13 * np.abs(a['grads'][0]).max()


def test_per_dimension_affine_change_of_hidden_changes_nothing():
    n, D = 12, 6
    hs = _case(n, 1, D, 4)
    g = np.random.default_rng(2)
    scale, shift = g.uniform(0.5, 3.0, size=D), g.standard_normal(D) * 5.0
    a = barlow_direct(hs, 0.05, 1.0, 0.0)
    b = barlow_direct([hs[0] * scale + shift], 0.05, 1.0, 0.0)
    assert abs(a['loss'] - b['loss']) <= 1e-12 * abs(a['loss'])
    assert abs(a['on_diag'] - b['on_diag']) <= 1e-12 * a['on_diag'] and abs(a['off_diag'] - b['off_diag']) <= 1e-12 * a['frob']
    assert np.abs(a['grad_all'] - b['grad_all'] * scale).max() <= 1e-11 * np.abs(a['grad_all']).max()


def test_identical_views_have_a_unit_diagonal():
    n, D = 40, 8                                     # N > D, full rank
    v = np.random.default_rng(6).standard_normal((n, D))
    ref = barlow_gram([np.concatenate([v, v])], 0.0051, 1.0, 0.0)
    assert ref['on_diag'][0] < 1e-24
    assert ref['off_diag'][0] > 0.0


@pytest.mark.parametrize('R', [2, 3])
def test_replica_conventions(R):
    """mean_r loss_r = L, and what the device returns (grad_scale * R * dL/dh_r with grad_scale = 1 / R), summed over the replicas by the
    gradient synchronisation of the parameters, is the gradient of L: the per-replica blocks tile dL/dh_all."""
    n, D, lam, ls = 6, 8, 0.2, 0.5
    hs = _case(n, R, D, 20 + R)
    N = R * n
    one = barlow_direct([h_all_of(hs, n)], lam, ls)               # the whole batch on one replica
    gram = barlow_gram(hs, lam, ls)
    assert abs(np.mean(gram['loss']) - one['loss']) <= 1e-12 * abs(one['loss'])
    assert max(gram['loss']) - min(gram['loss']) > 0.0            # the shares differ: only their mean is the loss
    tiled = np.zeros((2 * N, D))
    for r in range(R):
        tiled[replica_rows(r, n, N)] = (1.0 / R) * R * gram['grads'][r]
    assert np.abs(tiled - one['grad_all']).max() <= 1e-12 * np.abs(one['grad_all']).max()


def test_barlow_flags_parse_and_default():
    from simclr_amd.flags import FLAGS
    try:
        FLAGS.reset()
        assert FLAGS.contrastive_loss == 'ntxent' and FLAGS.bt_lambda == 0.0051 and FLAGS.bt_loss_scaling == 1.0
        FLAGS.parse(['--contrastive_loss=barlow', '--bt_lambda=0.01', '--bt_loss_scaling=0.024', '--proj_out_dim=64'])
        assert (FLAGS.contrastive_loss, FLAGS.bt_lambda, FLAGS.bt_loss_scaling) == ('barlow', 0.01, 0.024)
        from simclr_amd import run
        assert run.check_contrastive_loss_flags() is False and run.barlow_loss_on()
        assert not run.generalized_loss_on() and not run.supcon_loss_on()
        FLAGS.reset()
        FLAGS.update(contrastive_loss='barlow', proj_head_mode='none')                 # the encoder width: 2048 for ResNet-50
        assert run.barlow_loss_width() == 2048 and run.check_contrastive_loss_flags() is False
        FLAGS.update(resnet_depth=18, width_multiplier=2)
        assert run.barlow_loss_width() == 1024
    finally:
        FLAGS.reset()


def test_metric_names_of_the_barlow_loss():
    from simclr_amd import run
    from simclr_amd.flags import FLAGS
    try:
        FLAGS.reset()
        FLAGS.update(contrastive_loss='barlow')
        assert sorted(run.build_metrics()) == ['train/bt_off_diag', 'train/bt_on_diag', 'train/contrast_loss', 'train/supervised_acc',
                                               'train/supervised_loss', 'train/total_loss', 'train/weight_decay']
        FLAGS.update(lineareval_while_pretraining=False)
        assert sorted(run.build_metrics()) == ['train/bt_off_diag', 'train/bt_on_diag', 'train/contrast_loss', 'train/total_loss',
                                               'train/weight_decay']
        assert len(run.build_metrics()) <= 16
        FLAGS.update(train_mode='finetune')                              # fine-tuning ignores the flag
        assert sorted(run.build_metrics()) == ['train/supervised_acc', 'train/supervised_loss', 'train/total_loss', 'train/weight_decay']
        assert run.check_contrastive_loss_flags() is False and not run.barlow_loss_on()
    finally:
        FLAGS.reset()


def test_value_errors_before_any_device_work():
    from simclr_amd import objective, ops, run
    from simclr_amd.flags import FLAGS
    for D in (100, 8256, 32, 0):
        with pytest.raises(ValueError, match='multiples of 64 in \\[64, 8192\\]'):
            ops._bt_check_dim(D)
    for D in (64, 320, 2048, 8192):
        ops._bt_check_dim(D)
    with pytest.raises(ValueError, match='multiples of 64'):
        objective.add_barlow_twins_loss(torch.zeros(8, 100))
    with pytest.raises(ValueError, match='multiples of 64'):
        ops.bt_standardize(torch.zeros(8, 8256))
    with pytest.raises(ValueError, match='N = R\\*n'):
        ops.bt_fwd(torch.zeros(10, 64), 3, 0, 0.0051)                    # N = 5 is no multiple of n = 3
    with pytest.raises(ValueError, match='N = R\\*n'):
        ops.bt_fwd(torch.zeros(8, 64), 0, 0, 0.0051)
    with pytest.raises(ValueError, match='rank 2'):
        ops.bt_fwd(torch.zeros(8, 64), 2, 2, 0.0051)
    with pytest.raises(ValueError, match='float64 colsums'):
        ops.bt_apply(torch.zeros(8, 64), torch.zeros(8, 64), torch.zeros(2, 64), torch.zeros(2, 2, 64), 0)
    base = ['--dataset=synthetic', '--contrastive_loss=barlow', '--train_steps=1']
    try:
        for extra, msg in ((['--bt_lambda=-0.1'], 'bt_lambda must be >= 0'), (['--bt_loss_scaling=0'], 'bt_loss_scaling must be > 0'),
                           (['--proj_out_dim=100'], 'barlow needs a loss width'), (['--proj_out_dim=8256'], 'barlow needs a loss width'),
                           (['--proj_out_dim=32'], 'barlow needs a loss width'),
                           (['--proj_head_mode=none', '--width_multiplier=8'], 'barlow needs a loss width')):
            FLAGS.reset()
            with pytest.raises(ValueError, match=msg):
                run.main(base + extra)
        FLAGS.reset()
        with pytest.raises(ValueError, match="'ntxent' or 'generalized' or 'supcon'"):
            run.main(['--dataset=synthetic', '--contrastive_loss=triplet', '--train_steps=1'])
        FLAGS.reset()
        FLAGS.update(contrastive_loss='barlow', train_mode='finetune', proj_out_dim=100, bt_lambda=-1.0)
        assert run.check_contrastive_loss_flags() is False
    finally:
        FLAGS.reset()
