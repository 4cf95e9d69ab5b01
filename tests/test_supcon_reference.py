"""tests/supcon_reference.py (the float64 restatement the device tests of the supervised contrastive loss compare against) pinned on the
CPU: torch float64 autograd, the case worked on paper in tests/golden/SUPCON_HAND_DERIVED.md, the NT-Xent oracle for all-distinct labels,
the all-equal-labels count, permutation invariance; then the flag, the metric names and the refusals that precede any device work."""
import math

import numpy as np
import pytest
import torch

from oracle import ntxent as ont
from tests.supcon_reference import supcon_reference


def _case(n, R, D, C, seed):
    g = np.random.default_rng(seed)
    hs = [g.standard_normal((2 * n, D)) for _ in range(R)]
    ys = [g.integers(0, C, size=n) for _ in range(R)]
    return hs, ys


def _torch_objective(hs, ys, hidden_norm, T):
    """(1 / R) sum_r loss_r with torch operations only; returns (objective, per-replica losses, leaves)."""
    R, n = len(hs), hs[0].shape[0] // 2
    N = R * n
    leaves = [torch.tensor(h, dtype=torch.float64, requires_grad=True) for h in hs]
    zs = [h / torch.sqrt(torch.clamp((h * h).sum(1, keepdim=True), min=1e-12)) if hidden_norm else h for h in leaves]
    z_all = torch.cat([z[:n] for z in zs] + [z[n:] for z in zs], 0)
    y = torch.tensor(np.concatenate(ys))
    ycol = torch.cat([y, y])
    losses = []
    for r in range(R):
        total = 0.0
        for i in range(2 * n):
            v, s = divmod(i, n)
            self_col = v * N + r * n + s
            keep = torch.ones(2 * N, dtype=torch.bool)
            keep[self_col] = False
            logits = (z_all @ zs[r][i]) / T
            pos = keep & (ycol == ys[r][s])
            total = total + torch.logsumexp(logits[keep], 0) - logits[pos].mean()
        losses.append(total / n)
    return sum(losses) / R, losses, leaves


@pytest.mark.parametrize('hidden_norm', [True, False])
@pytest.mark.parametrize('n,R,D,C,T', [(3, 1, 4, 2, 1.0), (4, 2, 8, 3, 0.1), (5, 3, 6, 1, 0.5), (2, 2, 4, 100, 0.2)])
def test_restatement_equals_autograd(n, R, D, C, T, hidden_norm):
    hs, ys = _case(n, R, D, C, n + R + D)
    ref = supcon_reference(hs, ys, hidden_norm, T)
    obj, losses, leaves = _torch_objective(hs, ys, hidden_norm, T)
    obj.backward()
    for r in range(R):
        assert abs(ref['loss'][r] - float(losses[r].detach())) <= 1e-12 * max(1.0, abs(float(losses[r].detach())))
        want = leaves[r].grad.numpy()
        assert np.abs(ref['grads'][r] - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_restatement_equals_the_hand_derived_case():
    """tests/golden/SUPCON_HAND_DERIVED.md: n = 2, D = 2, T = 1, hidden_norm=False, rows e1, e2, e1, e2."""
    h = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 0.0], [0.0, 1.0]])
    e = math.e
    same = supcon_reference([h], [np.array([7, 7])], False, 1.0)
    assert abs(same['loss'][0] - 2.0 * (math.log(2.0 + e) - 1.0 / 3.0)) < 1e-14
    assert same['acc'] == [1.0] and same['positives'] == [3.0]
    a = e / (2.0 + e) - 1.0 / 3.0
    assert np.abs(same['grads'][0] - np.array([[a, -a], [-a, a], [a, -a], [-a, a]])).max() < 1e-14
    two = supcon_reference([h], [np.array([0, 1])], False, 1.0)
    assert abs(two['loss'][0] - 2.0 * (math.log(2.0 + e) - 1.0)) < 1e-14
    assert two['acc'] == [1.0] and two['positives'] == [1.0]
    b = 2.0 / (2.0 + e)
    assert np.abs(two['grads'][0] - np.array([[-b, b], [b, -b], [-b, b], [b, -b]])).max() < 1e-14
    assert abs(2.0 * (math.log(2.0 + e) - 1.0 / 3.0) - 2.4362227612) < 1e-9


@pytest.mark.parametrize('hidden_norm', [True, False])
@pytest.mark.parametrize('n,R,D,T', [(6, 1, 8, 0.1), (4, 2, 8, 1.0), (3, 3, 4, 0.5)])
def test_distinct_labels_give_the_ntxent_oracle(n, R, D, T, hidden_norm):
    hs, _ = _case(n, R, D, 1, 11 * n + R)
    ys = [np.arange(r * n, (r + 1) * n)[::-1] for r in range(R)]          # all distinct, in no particular order
    ref = supcon_reference(hs, ys, hidden_norm, T)
    losses, grads = ont.contrastive_loss_and_grad(hs, hidden_norm, T)
    for r in range(R):
        one, _, _ = ont.add_contrastive_loss(hs[r], hidden_norm, T, all_hiddens=hs if R > 1 else None, replica_id=r)
        assert abs(ref['loss'][r] - one) <= 1e-12 * max(1.0, abs(one))
        assert abs(ref['loss'][r] - losses[r]) <= 1e-12 * max(1.0, abs(losses[r]))
        assert np.abs(ref['grads'][r] - grads[r]).max() <= 1e-12 * max(1.0, np.abs(grads[r]).max())
        assert ref['positives'][r] == 1.0


def test_equal_labels_make_every_other_column_a_positive():
    n, R = 5, 2
    hs, _ = _case(n, R, 4, 1, 2)
    ref = supcon_reference(hs, [np.full(n, 3)] * R, True, 0.3)
    assert (ref['pcount'] == 2 * n * R - 1).all()
    assert ref['positives'] == [2.0 * n * R - 1] * R and ref['acc'] == [1.0] * R       # no non-positive column: every row is a hit


@pytest.mark.parametrize('hidden_norm', [True, False])
def test_joint_permutation_of_samples_changes_nothing(hidden_norm):
    n, D = 7, 8
    hs, ys = _case(n, 1, D, 3, 5)
    perm = np.random.default_rng(1).permutation(n)
    rows = np.concatenate([perm, n + perm])
    a = supcon_reference(hs, ys, hidden_norm, 0.2)
    b = supcon_reference([hs[0][rows]], [ys[0][perm]], hidden_norm, 0.2)
    assert abs(a['loss'][0] - b['loss'][0]) <= 1e-13 * abs(a['loss'][0])
    assert a['acc'] == b['acc'] and a['positives'] == b['positives']
    assert np.abs(a['grads'][0][rows] - b['grads'][0]).max() <= 1e-13 * np.abs(a['grads'][0]).max()
    # renaming the classes changes nothing either
    c = supcon_reference(hs, [(ys[0] * 17 + 5) % 101], hidden_norm, 0.2)
    assert c['loss'] == a['loss'] and np.array_equal(c['grads'][0], a['grads'][0])


def test_supcon_flag_parses_and_defaults():
    from simclr_amd.flags import FLAGS
    try:
        FLAGS.reset()
        assert FLAGS.contrastive_loss == 'ntxent'
        FLAGS.parse(['--contrastive_loss=supcon', '--temperature=0.2'])
        assert (FLAGS.contrastive_loss, FLAGS.temperature) == ('supcon', 0.2)
        from simclr_amd import run
        assert run.check_contrastive_loss_flags() is False and run.supcon_loss_on() and not run.generalized_loss_on()
    finally:
        FLAGS.reset()


def test_metric_names_of_the_supcon_loss():
    from simclr_amd import run
    from simclr_amd.flags import FLAGS
    try:
        FLAGS.reset()
        FLAGS.update(contrastive_loss='supcon')
        assert sorted(run.build_metrics()) == ['train/contrast_acc', 'train/contrast_loss', 'train/contrast_positives', 'train/supervised_acc',
                                               'train/supervised_loss', 'train/total_loss', 'train/weight_decay']
        FLAGS.update(lineareval_while_pretraining=False)
        assert sorted(run.build_metrics()) == ['train/contrast_acc', 'train/contrast_loss', 'train/contrast_positives', 'train/total_loss',
                                               'train/weight_decay']
        assert len(run.build_metrics()) <= 16
        FLAGS.update(train_mode='finetune')                              # fine-tuning ignores the flag
        assert sorted(run.build_metrics()) == ['train/supervised_acc', 'train/supervised_loss', 'train/total_loss', 'train/weight_decay']
        assert run.check_contrastive_loss_flags() is False and not run.supcon_loss_on()
    finally:
        FLAGS.reset()


def test_value_errors_before_any_device_work():
    from simclr_amd import objective, ops, run
    from simclr_amd.flags import FLAGS
    with pytest.raises(ValueError, match='64/128/256'):
        objective.add_supcon_loss(torch.zeros(8, 100), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match='3 labels for a local batch of 4'):
        objective.add_supcon_loss(torch.zeros(8, 128), torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match='labels_all must hold the N = 4'):
        ops.supcon_fwd(torch.zeros(8, 64), torch.zeros(8, 64), torch.zeros(5, dtype=torch.int32), 0, 1.0)
    with pytest.raises(ValueError, match='N = R\\*n'):
        ops.supcon_fwd(torch.zeros(0, 64), torch.zeros(8, 64), torch.zeros(4, dtype=torch.int32), 0, 1.0)
    try:
        for extra in (['--proj_out_dim=100'], ['--proj_head_mode=none'], ['--proj_out_dim=512']):
            FLAGS.reset()
            with pytest.raises(ValueError, match='supcon needs a projection head of width 64/128/256'):
                run.main(['--dataset=synthetic', '--contrastive_loss=supcon', '--train_steps=1'] + extra)
        FLAGS.reset()
        with pytest.raises(ValueError, match="'ntxent' or 'generalized' or 'supcon'"):
            run.main(['--dataset=synthetic', '--contrastive_loss=triplet', '--train_steps=1'])
        FLAGS.reset()
        FLAGS.update(contrastive_loss='supcon', train_mode='finetune', proj_out_dim=100)
        assert run.check_contrastive_loss_flags() is False
    finally:
        FLAGS.reset()
