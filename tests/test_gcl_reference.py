"""CPU tests of the generalized contrastive loss: the float64 reference tests/gcl_reference.py (the yardstick of tests/test_gpu_gcl.py)
against torch float64 autograd, the hand-derived cases (tests/golden/gcl_hand_cases.json, derived in tests/golden/GCL_HAND_DERIVED.md), the closed forms and the stable tie rule; the new flags; the ValueErrors."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests.gcl_reference import gcl_reference, stable_argsort_columns

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'gcl_hand_cases.json')


def _torch_objective(hs, lam, T, dist, hidden_norm, ls, rand_w, prior):
    """The step's objective (1 / R) sum_r loss_r with torch ops only (sort -> autograd gathers through the permutation)."""
    R, n, D = len(hs), hs[0].shape[0] // 2, hs[0].shape[1]
    zs = [h / h.norm(dim=1, keepdim=True) if hidden_norm else h for h in hs]
    z_all = torch.cat([z[:n] for z in zs] + [z[n:] for z in zs], 0)
    N = R * n
    losses, aligns, dists = [], [], []
    for r, z in enumerate(zs):
        align = ((z[:n] - z[n:]) ** 2).mean() / 2.0
        if dist == 'logsumexp':
            own = torch.cat([z_all[r * n:(r + 1) * n], z_all[N + r * n:N + (r + 1) * n]], 0)
            dm = (torch.logsumexp(own @ z_all.T / T, dim=1) - math.log(D)).mean()
        else:
            pr = prior / prior.norm(dim=1, keepdim=True) if hidden_norm else prior
            ps = torch.sort(z_all @ rand_w, dim=0, stable=True).values
            qs = torch.sort(pr @ rand_w, dim=0).values
            dm = ((qs - ps) ** 2).mean()
        losses.append(ls * (align + lam * dm)); aligns.append(align); dists.append(dm)
    return sum(losses) / R, losses, aligns, dists


@pytest.mark.parametrize('dist', ['logsumexp', 'normal', 'uniform'])
@pytest.mark.parametrize('n,R,D', [(1, 1, 2), (3, 1, 8), (4, 2, 16), (5, 3, 4)])
@pytest.mark.parametrize('hidden_norm', [True, False])
@pytest.mark.parametrize('T,lam,ls', [(0.1, 1.0, 1.0), (1.0, 0.5, 2.0)])
def test_reference_equals_autograd(dist, n, R, D, hidden_norm, T, lam, ls):
    g = torch.Generator().manual_seed(n * 100 + R * 10 + D)
    hs = [torch.randn(2 * n, D, generator=g, dtype=torch.float64).requires_grad_(True) for _ in range(R)]
    M = 2 * n * R
    rand_w = torch.linalg.qr(torch.randn(D, D, generator=g, dtype=torch.float64))[0]
    prior = torch.randn(M, D, generator=g, dtype=torch.float64) if dist != 'uniform' else torch.rand(M, D, generator=g, dtype=torch.float64) * 2 - 1
    obj, losses, aligns, dists = _torch_objective(hs, lam, T, dist, hidden_norm, ls, rand_w, prior)
    grads = torch.autograd.grad(obj, hs)
    ref = gcl_reference([h.detach().numpy() for h in hs], lam, T, dist, hidden_norm, ls, rand_w.numpy(), prior.numpy())
    for r in range(R):
        for key, val in (('loss', losses[r]), ('align', aligns[r]), ('dist', dists[r])):
            assert abs(ref[key][r] - float(val.detach())) <= 1e-12 * max(1.0, abs(float(val.detach()))), (key, r)
        scale = max(float(grads[r].abs().max()), 1e-30)
        # both sides are a few hundred float64 operations on O(1) .. O(|h|^2 / T) numbers; the softmax of un-normalised rows at T = 0.1
        # loses log2(|S / T|) bits before exponentiation
        assert float(np.abs(ref['grads'][r] - grads[r].numpy()).max()) <= 1e-9 * scale + 1e-14, r


def _value(x):
    e = math.e
    return x['const'] + x['sig'] * e / (e + 1) + x['log'] * math.log((e + 1) / 2) if isinstance(x, dict) else float(x)


def test_reference_equals_the_hand_derived_cases():
    with open(GOLDEN) as f:
        cases = json.load(f)['cases']
    assert [c['name'] for c in cases] == ['lse_orthogonal', 'swd_tie']
    for c in cases:
        ref = gcl_reference([np.array(c['hidden'])], c['lambda_weight'], c['temperature'], c['dist'], False, c['loss_scaling'],
                            c.get('rand_w'), c.get('prior'))
        assert abs(ref['align'][0] - _value(c['align'])) <= 1e-15, c['name']
        assert abs(ref['dist'][0] - _value(c['dist_match'])) <= 4e-16, c['name']
        assert abs(ref['loss'][0] - _value(c['loss'])) <= 4e-16, c['name']
        want = np.array([[_value(x) for x in row] for row in c['grad']])
        assert float(np.abs(ref['grads'][0] - want).max()) <= 4e-16, c['name']
        if 'perm' in c:
            assert ref['perm'].tolist() == c['perm']
    # the same two cases as numbers, independent of the file's notation
    r = gcl_reference([np.array([[1.0, 0.0], [0.0, 1.0]])], 1.0, 1.0, 'logsumexp', False, 1.0)
    assert abs(r['loss'][0] - (0.5 + math.log((math.e + 1) / 2))) <= 4e-16
    r = gcl_reference([np.array([[3.0, 1.0], [1.0, 1.0]])], 2.0, 1.0, 'normal', False, 0.5, np.eye(2), np.array([[0.0, 2.0], [2.0, 0.0]]))
    assert r['loss'][0] == 1.5 and r['grads'][0].tolist() == [[1.0, 0.5], [0.0, -0.5]]


def test_logsumexp_closed_forms_and_the_log_of_the_width():
    n, D, T = 8, 64, 0.1
    N = n
    h = np.ones((2 * n, D))
    r = gcl_reference([h], 1.0, T, 'logsumexp', True, 1.0)
    assert r['align'][0] == 0.0
    assert abs(r['dist'][0] - (1 / T + math.log(2 * N / D))) <= 1e-13 and abs(r['dist'][0] - 8.613705638880109) <= 1e-12
    e = np.eye(n, D)
    r = gcl_reference([np.concatenate([e, e])], 1.0, T, 'logsumexp', True, 1.0)
    closed = math.log(2 * math.exp(1 / T) + 2 * N - 2) - math.log(D)
    assert r['align'][0] == 0.0 and abs(r['dist'][0] - closed) <= 1e-13 and abs(closed - 6.5345818) <= 1e-7
    # the constant is the log of the hidden WIDTH, not of the column count: widening the rows with zero columns changes only it
    g = np.random.default_rng(0)
    h = g.standard_normal((6, 8))
    a = gcl_reference([h], 1.0, 0.5, 'logsumexp', True, 1.0)['dist'][0]
    b = gcl_reference([np.pad(h, ((0, 0), (0, 8)))], 1.0, 0.5, 'logsumexp', True, 1.0)['dist'][0]
    assert abs((a - b) - math.log(2)) <= 1e-14


def test_ties_are_ordered_by_row_index():
    P = np.array([[2.0, 0.0, 1.0], [1.0, -0.0, 1.0], [2.0, 0.0, 1.0], [1.0, 0.0, 1.0]])
    perm = stable_argsort_columns(P)
    assert perm.T.tolist() == [[1, 3, 0, 2], [0, 1, 2, 3], [0, 1, 2, 3]]          # -0.0 == 0.0: a tie like any other
    # the gradient depends on the tie order: the stable rule and its reverse give different rows their differences
    h = np.array([[1.0, 5.0], [1.0, 7.0], [1.0, 6.0], [1.0, 8.0]])
    prior = np.array([[0.0, 0.0], [1.0, 0.0], [2.0, 0.0], [3.0, 0.0]])
    a = gcl_reference([h], 1.0, 1.0, 'uniform', False, 1.0, np.eye(2), prior)
    assert a['perm'][:, 0].tolist() == [0, 1, 2, 3]
    b = gcl_reference([h], 1.0, 1.0, 'uniform', False, 1.0, np.eye(2), prior, perm=np.array([[3, 0], [2, 2], [1, 1], [0, 3]]))
    assert a['dist'][0] == b['dist'][0] and np.abs(a['grads'][0] - b['grads'][0]).max() > 0.1


def test_generalized_loss_flags_parse_and_default():
    from simclr_amd.flags import FLAGS
    try:
        FLAGS.reset()
        assert (FLAGS.contrastive_loss, FLAGS.gcl_dist, FLAGS.gcl_lambda, FLAGS.gcl_loss_scaling, FLAGS.gcl_seed) == \
               ('ntxent', 'logsumexp', 1.0, 1.0, 0)
        FLAGS.parse(['--contrastive_loss=generalized', '--gcl_dist', 'uniform', '--gcl_lambda=0.25', '--gcl_loss_scaling=2', '--gcl_seed=7'])
        assert (FLAGS.contrastive_loss, FLAGS.gcl_dist, FLAGS.gcl_lambda, FLAGS.gcl_loss_scaling, FLAGS.gcl_seed) == \
               ('generalized', 'uniform', 0.25, 2.0, 7)
    finally:
        FLAGS.reset()


def test_metric_names_of_the_generalized_loss():
    from simclr_amd import run
    from simclr_amd.flags import FLAGS
    try:
        FLAGS.reset()
        FLAGS.update(contrastive_loss='generalized')
        assert sorted(run.build_metrics()) == ['train/align_loss', 'train/contrast_loss', 'train/dist_loss', 'train/supervised_acc',
                                               'train/supervised_loss', 'train/total_loss', 'train/weight_decay']
        assert len(run.build_metrics()) <= 16
        FLAGS.update(train_mode='finetune')                              # fine-tuning ignores the flag
        assert sorted(run.build_metrics()) == ['train/supervised_acc', 'train/supervised_loss', 'train/total_loss', 'train/weight_decay']
        assert run.check_contrastive_loss_flags() is False
    finally:
        FLAGS.reset()


def test_value_errors_before_any_device_work():
    from simclr_amd import objective, ops, run
    from simclr_amd.flags import FLAGS
    h = torch.zeros(4, 128)
    with pytest.raises(ValueError, match='Unknown prior laplace'):
        objective.generalized_contrastive_loss(h, h, dist='laplace')
    with pytest.raises(ValueError, match='64/128/256'):
        objective.generalized_contrastive_loss(torch.zeros(4, 100), torch.zeros(4, 100), dist='logsumexp')
    with pytest.raises(ValueError, match='8192'):
        ops.swd_sort_match(torch.zeros(4, 8193), torch.zeros(4, 8193), 1.0)
    with pytest.raises(ValueError, match='Unknown prior'):
        gcl_reference([np.zeros((2, 2))], dist='laplace')
    try:
        for extra, msg in ((['--proj_out_dim=100'], '64/128/256'), (['--proj_head_mode=none'], '64/128/256'),
                           (['--gcl_dist=laplace'], 'Unknown prior laplace'),
                           (['--gcl_dist=normal', '--train_batch_size=8192'], 'train_batch_size <= 4096')):
            FLAGS.reset()
            with pytest.raises(ValueError, match=msg):
                run.main(['--dataset=synthetic', '--contrastive_loss=generalized', '--train_steps=1'] + extra)
        FLAGS.reset()
        with pytest.raises(ValueError, match="'ntxent' or 'generalized'"):
            run.main(['--dataset=synthetic', '--contrastive_loss=triplet', '--train_steps=1'])
        FLAGS.reset()
        FLAGS.update(contrastive_loss='generalized', train_mode='finetune', proj_out_dim=100)
        assert run.check_contrastive_loss_flags() is False
    finally:
        FLAGS.reset()


def test_draws_depend_on_seed_and_step_only():
    from simclr_amd.objective import gcl_draws
    w0, p0 = gcl_draws(64, 32, 'normal', 3, 5, 'cpu')
    w1, p1 = gcl_draws(64, 32, 'normal', 3, 5, 'cpu')
    assert torch.equal(w0, w1) and torch.equal(p0, p1)
    for seed, step in ((3, 6), (4, 5)):
        w2, p2 = gcl_draws(64, 32, 'normal', seed, step, 'cpu')
        assert not torch.equal(w0, w2) and not torch.equal(p0, p2)
    assert float((w0.double().T @ w0.double() - torch.eye(64, dtype=torch.float64)).abs().max()) <= 1e-5      # orthogonal (fp32 QR)
    u = gcl_draws(64, 4096, 'uniform', 0, 0, 'cpu')[1]
    assert float(u.min()) >= -1.0 and float(u.max()) <= 1.0 and float(u.min()) < -0.99 and float(u.max()) > 0.99
