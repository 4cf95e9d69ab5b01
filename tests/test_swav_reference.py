"""The float64 restatement tests/swav_reference.py pinned from outside: the potential form against the official Sinkhorn-Knopp iteration,
the analytic gradients against float64 autograd with the codes detached (and AWAY from autograd without the detach), the hand-derived
cases of tests/golden/SWAV_HAND_DERIVED.md, invariances, the replica convention, the freeze boundary, the error budget of the GPU tests'
cases; flags, refusals, names.  No GPU."""
import math

import numpy as np
import pytest
import torch

from tests.swav_reference import (ALPHA_EMULATION_ERROR, ALPHA_TOL, GATE_GRAD, GATE_LOSS, LOSS_CASES, SINK_CASES, alpha_emulation_error,
                                  autograd_gradients, case_gates, case_inputs, codes, gather_view_major, l2_normalize, loss_case_inputs, official_alpha,
                                  prototypes_frozen, sinkhorn_official, sinkhorn_potentials, swav_loss, swav_loss_normalized)


def _scores(z, w):
    return np.asarray(z, np.float64) @ np.asarray(w, np.float64).T


# ---------------------------------------------------------------------------------------------------------------- the Sinkhorn
@pytest.mark.parametrize('n,K,iters,eps,concentrated', [(1, 2, 1, 0.05, False), (1, 4097, 3, 0.05, False), (2, 3, 3, 0.05, False),
                                                        (5, 64, 2, 0.05, False), (33, 65, 3, 0.05, False), (70, 200, 3, 0.05, True),
                                                        (70, 63, 16, 0.05, False), (9, 300, 3, 1.0, False), (64, 7, 1, 0.05, True)])
def test_potential_form_equals_the_official_iteration(n, K, iters, eps, concentrated):
    z, w = case_inputs(n, K, 64, concentrated)
    alpha, _ = sinkhorn_potentials(z, w, eps, iters)
    got = codes(z, w, alpha, eps)
    S = _scores(z, w)
    for v in range(2):
        want = sinkhorn_official(S[v * n:(v + 1) * n], eps, iters)
        assert np.abs(got[v * n:(v + 1) * n] - want).max() <= 1e-12
        assert np.abs(want.sum(1) - 1.0).max() <= 1e-12
        # without the initial Q /= sum(Q) the official column scaling IS alpha; with it, alpha shifted by one constant
        assert np.abs(official_alpha(S[v * n:(v + 1) * n], eps, iters, initial_normalisation=False) - alpha[v]).max() <= 1e-10
        shift = official_alpha(S[v * n:(v + 1) * n], eps, iters, initial_normalisation=True) - alpha[v]
        assert np.ptp(shift) <= 1e-10 and abs(shift.mean() - np.log(np.exp(S[v * n:(v + 1) * n] / eps).sum())) <= 1e-10
        unnormalised = sinkhorn_official(S[v * n:(v + 1) * n], eps, iters, initial_normalisation=False)
        assert np.abs(unnormalised - want).max() <= 1e-12                       # the codes do not see that constant


def test_hand_derived_one_row_per_view_gives_exactly_uniform_codes():
    """SWAV_HAND_DERIVED.md case 1: N = 1 -- alpha_j = -ln K - L_j - beta, so L_j + alpha_j is constant in j for any I >= 1."""
    for K, D in ((2, 64), (63, 128), (4097, 64)):
        z, w = case_inputs(1, K, D)
        for iters in (1, 2, 3, 16):
            alpha, beta = sinkhorn_potentials(z, w, 0.05, iters)
            c = codes(z, w, alpha, 0.05)
            assert np.abs(c - 1.0 / K).max() <= 1e-15
            L = _scores(z, w) / 0.05
            assert np.abs(alpha - (-np.log(K) - L - beta[:, None])).max() <= 1e-12
            ref = swav_loss_normalized(z, w, alpha, 0.1, 0.05)
            assert abs(ref['entropy'] - math.log(K)) <= 1e-12


def test_hand_derived_balanced_scores_are_a_fixed_point():
    """SWAV_HAND_DERIVED.md case 2: N = K, z_g = e_g, w_j = e_j -- exp(L) has equal row and column sums c = e^(1/eps) + K - 1:
    alpha_j = -ln K - ln c, beta stays 0, for every I; the code is softmax(L_g) with e^(1/eps) / c on the diagonal."""
    K, D, eps = 4, 64, 0.05
    w = np.eye(K, D)
    z = np.concatenate([np.eye(K, D), np.eye(K, D)[::-1]])          # view b: another order of the same rows
    c = math.exp(1.0 / eps) + K - 1
    for iters in (1, 2, 3, 7):
        alpha, beta = sinkhorn_potentials(z, w, eps, iters)
        assert np.abs(alpha - (-math.log(K) - math.log(c))).max() <= 1e-12 and np.abs(beta).max() <= 1e-12
        q = codes(z, w, alpha, eps)
        assert np.abs(q[:K].diagonal() - math.exp(1.0 / eps) / c).max() <= 1e-15
        assert np.abs(q[:K].sum(0) - 1.0).max() <= 1e-12                       # column sums N / K = 1


def test_invariances():
    n, K, D, eps = 7, 19, 64, 0.05
    z, w = case_inputs(n, K, D)
    S = _scores(z, w)
    base = sinkhorn_official(S[:n], eps, 3)
    # A constant added to the scores of one PROTOTYPE (a row of the official K x N matrix Q): the first column step absorbs it exactly.
    shifted = sinkhorn_official(S[:n] + np.linspace(-3, 2, K)[None, :] * eps, eps, 3)
    assert np.abs(shifted - base).max() <= 1e-12
    # A constant added to the scores of one SAMPLE is the start beta^(0) = that constant instead of 0: the fixed point does not see it,
    # a finite iteration forgets it geometrically (SWAV_HAND_DERIVED.md, "Invariances")
    gap = []
    for iters in (1, 3, 16, 60):
        per_sample = sinkhorn_official(S[:n] + np.linspace(-3, 2, n)[:, None] * eps, eps, iters)
        gap.append(np.abs(per_sample - sinkhorn_official(S[:n], eps, iters)).max())
    assert gap[0] > 0.1 and gap[1] < gap[0] and gap[2] < 1e-3 * gap[0] and gap[3] <= 1e-12
    # a joint permutation of the prototypes
    perm = np.random.default_rng(3).permutation(K)
    a0, _ = sinkhorn_potentials(z, w, eps, 3)
    a1, _ = sinkhorn_potentials(z, w[perm], eps, 3)
    assert np.abs(a1 - a0[:, perm]).max() <= 1e-12
    r0 = swav_loss_normalized(z, w, a0, 0.1, eps)
    r1 = swav_loss_normalized(z, w[perm], a1, 0.1, eps)
    assert abs(r0['loss'] - r1['loss']) <= 1e-12 and np.abs(r1['grad_w'] - r0['grad_w'][perm]).max() <= 1e-12
    assert np.abs(r1['grad_q'] - r0['grad_q']).max() <= 1e-12
    # a constant added to alpha (the official initial normalisation) changes neither the codes nor the loss
    r2 = swav_loss_normalized(z, w, a0 + 1.2345, 0.1, eps)
    assert abs(r2['loss'] - r0['loss']) <= 1e-12 and abs(r2['entropy'] - r0['entropy']) <= 1e-12


def test_sixteen_iterations_approach_the_equipartition():
    n, K, D, eps = 24, 6, 64, 0.05
    z, w = case_inputs(n, K, D)
    worst = []
    for iters in (1, 3, 16):
        alpha, _ = sinkhorn_potentials(z, w, eps, iters)
        q = codes(z, w, alpha, eps)
        worst.append(max(np.abs(q[:n].sum(0) - n / K).max(), np.abs(q[n:].sum(0) - n / K).max()) / (n / K))
    assert worst[2] < 1e-3 and worst[2] < worst[1] < worst[0]
    # concentrated rows: the potentials of the crowded prototypes sink far below the others
    z, w = case_inputs(70, 200, 128, True)
    alpha, _ = sinkhorn_potentials(z, w, 0.05, 3)
    assert alpha.max() - alpha.min() > 15.0


# ---------------------------------------------------------------------------------------------------------------- loss, gradients
@pytest.mark.parametrize('b,K,T,eps,iters', [(1, 2, 0.1, 0.05, 3), (2, 5, 0.1, 0.05, 3), (5, 11, 0.1, 0.05, 3), (9, 70, 1.0, 1.0, 2),
                                             (6, 3, 0.2, 0.05, 1)])
def test_analytic_gradients_are_the_detached_autograd_and_not_the_full_one(b, K, T, eps, iters):
    qh, w = case_inputs(b, K, 64)
    alpha, _ = sinkhorn_potentials(qh, w, eps, iters)
    ref = swav_loss_normalized(qh, w, alpha, T, eps)
    loss, gq, gw = autograd_gradients(qh, w, T, eps, iters, detach=True)
    assert abs(loss - ref['loss']) <= 1e-12
    assert np.abs(gq - ref['grad_q']).max() <= 1e-12 and np.abs(gw - ref['grad_w']).max() <= 1e-12
    # the rows of the direct form: logsumexp(s) - <code of the other view, s>
    direct = ref['lse_s'] - (np.roll(ref['Pt'], -b, 0) * (qh.astype(np.float64) @ w.astype(np.float64).T / T)).sum(1)
    assert np.abs(direct - ref['rows']).max() <= 1e-12
    if b > 1:
        # N = 1 has constant codes; everywhere else the gradient through the Sinkhorn is another gradient
        loss2, gq2, gw2 = autograd_gradients(qh, w, T, eps, iters, detach=False)
        assert abs(loss2 - loss) <= 1e-12
        assert np.abs(gq2 - ref['grad_q']).max() > 1e-2 * np.abs(ref['grad_q']).max()
        assert np.abs(gw2 - ref['grad_w']).max() > 1e-2 * np.abs(ref['grad_w']).max()


def test_gradients_through_the_normalisations_vs_autograd():
    b, K, D = 4, 9, 64
    g = np.random.default_rng(11)
    q, v = g.standard_normal((2 * b, D)), g.standard_normal((K, D))
    ref = swav_loss(q, v, 0.1, 0.05, 3)
    tq = torch.tensor(q, requires_grad=True)
    tv = torch.tensor(v, requires_grad=True)
    unit = lambda x: x / torch.sqrt(torch.clamp((x * x).sum(-1, keepdim=True), min=1e-12))
    s = unit(tq) @ unit(tv).T / 0.1
    code = torch.tensor(ref['Pt'])
    loss = (torch.logsumexp(s, 1) - (torch.roll(code, -b, 0) * s).sum(1)).mean()
    loss.backward()
    assert abs(float(loss.detach()) - ref['loss']) <= 1e-12
    assert np.abs(tq.grad.numpy() - ref['grad_q']).max() <= 1e-12 and np.abs(tv.grad.numpy() - ref['grad_v']).max() <= 1e-12


def test_swapping_the_views_of_alpha_changes_the_loss():
    """alpha is indexed by the view: fed alpha[::-1], the restatement's row gradient moves by far more than the GPU tests' gate."""
    for case in LOSS_CASES:
        b, K, D, T, eps, conc = case
        if b == 1:
            continue                            # N = 1: alpha only shifts each row's logits by a constant
        qh, w, alpha = loss_case_inputs(*case)
        good = swav_loss_normalized(qh, w, alpha, T, eps)
        bad = swav_loss_normalized(qh, w, alpha[::-1].copy(), T, eps)
        assert np.abs(bad['grad_q'] - good['grad_q']).max() > 50 * GATE_GRAD * np.abs(good['grad_q']).max(), case
        if eps == 0.05 and not conc:
            assert abs(bad['loss'] - good['loss']) > 10 * GATE_LOSS * abs(good['loss']), case


@pytest.mark.parametrize('R', [2, 3])
def test_replica_convention(R):
    """The Sinkhorn on the GATHERED batch, run by every replica: the mean of the replica losses is the loss of the one-process run on the
    gathered batch, the SUM of the replicas' prototype gradients (each with grad_scale 1 / R) is its prototype gradient, a replica's
    row gradient is its slice.  A Sinkhorn per replica is another loss."""
    b, K, D = 3, 17, 16
    g = np.random.default_rng(R)
    qs = [g.standard_normal((2 * b, D)) for _ in range(R)]
    v = g.standard_normal((K, D))
    whole = swav_loss(gather_view_major(qs), v, 0.1, 0.05, 3)
    z_all = gather_view_major([l2_normalize(q)[0] for q in qs])
    assert np.abs(z_all - whole['qh']).max() <= 1e-15
    parts = [swav_loss(q, v, 0.1, 0.05, 3, grad_scale=1.0 / R, z_all=z_all) for q in qs]
    assert all(np.array_equal(p['alpha'], whole['alpha']) for p in parts)
    assert abs(np.mean([p['loss'] for p in parts]) - whole['loss']) < 1e-12
    assert abs(np.mean([p['entropy'] for p in parts]) - whole['entropy']) < 1e-12
    assert np.abs(sum(p['grad_v'] for p in parts) - whole['grad_v']).max() < 1e-12
    for r, p in enumerate(parts):
        idx = np.concatenate([np.arange(r * b, (r + 1) * b), R * b + np.arange(r * b, (r + 1) * b)])
        assert np.abs(p['grad_q'] - whole['grad_q'][idx]).max() < 1e-12
    local = [swav_loss(q, v, 0.1, 0.05, 3, grad_scale=1.0 / R) for q in qs]
    assert max(np.abs(p['alpha'] - whole['alpha']).max() for p in local) > 0.1
    assert abs(np.mean([p['loss'] for p in local]) - whole['loss']) > 1e-3
    assert np.abs(sum(p['grad_v'] for p in local) - whole['grad_v']).max() > 1e-2 * np.abs(whole['grad_v']).max()


def test_freeze_boundary():
    from simclr_amd import model as model_lib
    from simclr_amd.flags import FLAGS
    try:
        FLAGS.reset()
        FLAGS.update(contrastive_loss='swav', swav_freeze_prototypes_epochs=2)
        spe = 10
        for step in (0, 1, 19, 20, 21, 10 ** 6):
            assert model_lib.swav_prototypes_frozen(step, spe) == prototypes_frozen(step, spe, 2) == (step < 20)
        FLAGS.update(swav_freeze_prototypes_epochs=0)
        assert not model_lib.swav_prototypes_frozen(0, spe)
        FLAGS.reset()
        assert model_lib.swav_prototypes_frozen(0, 1) and not model_lib.swav_prototypes_frozen(1, 1)      # the default: one epoch
    finally:
        FLAGS.reset()


# ---------------------------------------------------------------------------------------------------------------- error budget
def test_error_budget_of_the_gpu_cases():
    """The float32 emulation of the restatement over the GPU tests' cases: the loss cases use less than a quarter of the project's gates
    (the 4x-emulation rule is never taken), and the worst alpha error is the figure recorded in SWAV_HAND_DERIVED.md, from which the
    GPU tests' alpha tolerance derives."""
    worst = {}
    for case in LOSS_CASES:
        for name, (gate, err) in case_gates(*case).items():
            project = GATE_LOSS if name in ('loss', 'entropy') else GATE_GRAD
            assert gate == project and err <= project / 4.0, (case, name, err)
            worst[name] = max(worst.get(name, 0.0), err)
    errs = {case: alpha_emulation_error(*case) for case in SINK_CASES}
    worst['alpha'] = max(errs.values())
    print(worst)
    assert 0.6 * ALPHA_EMULATION_ERROR <= worst['alpha'] <= 1.15 * ALPHA_EMULATION_ERROR, errs
    assert ALPHA_TOL == 4.0 * ALPHA_EMULATION_ERROR and ALPHA_TOL < 2e-5
    assert {N for N, *_ in SINK_CASES} == {1, 3, 33, 64, 70} and {K for _, K, *_ in SINK_CASES} == {2, 63, 65, 200, 4097}
    assert {D for _, _, D, *_ in SINK_CASES} == {64, 128, 256} and {I for *_, I, _ in SINK_CASES} == {1, 2, 3}
    assert {e for _, _, _, e, _, _ in SINK_CASES} == {0.05, 1.0} and any(c for *_, c in SINK_CASES)
    assert {b for b, *_ in LOSS_CASES} == {1, 3, 33, 70} and {K for _, K, *_ in LOSS_CASES} == {2, 63, 65, 200, 4097}
    assert {D for _, _, D, *_ in LOSS_CASES} == {64, 128, 256}
    for N, K, D, eps, iters, conc in SINK_CASES:
        if conc:
            z, w = case_inputs(N, K, D, True)
            alpha, _ = sinkhorn_potentials(z, w, eps, iters)
            assert alpha.max() - alpha.min() > 15.0


# ---------------------------------------------------------------------------------------------------------------- flags, names
def test_flags_parse_and_defaults():
    from simclr_amd import run
    from simclr_amd.flags import FLAGS
    try:
        FLAGS.reset()
        assert (FLAGS.swav_num_prototypes, FLAGS.swav_epsilon, FLAGS.swav_temperature, FLAGS.swav_sinkhorn_iterations,
                FLAGS.swav_freeze_prototypes_epochs) == (3000, 0.05, 0.1, 3, 1)
        assert not run.swav_loss_on()
        FLAGS.parse(['--contrastive_loss=swav', '--swav_num_prototypes=4096', '--swav_epsilon=0.03', '--swav_temperature=0.2',
                     '--swav_sinkhorn_iterations=5', '--swav_freeze_prototypes_epochs=0', '--proj_out_dim=256'])
        assert (FLAGS.contrastive_loss, FLAGS.swav_num_prototypes, FLAGS.swav_epsilon, FLAGS.swav_sinkhorn_iterations) == ('swav', 4096, 0.03, 5)
        assert run.check_contrastive_loss_flags() is False and run.swav_loss_on()
        assert not (run.generalized_loss_on() or run.supcon_loss_on() or run.barlow_loss_on() or run.byol_loss_on() or run.moco_loss_on()
                    or run.dino_loss_on())
        FLAGS.update(hidden_norm=False, temperature=-1.0)                 # ignored with this loss
        assert run.check_contrastive_loss_flags() is False
        FLAGS.reset()
        FLAGS.update(contrastive_loss='swav')                             # the defaults: K = 3000, width 128
        assert run.check_contrastive_loss_flags() is False
        for name, values in (('swav_num_prototypes', (2, 1048576)), ('swav_sinkhorn_iterations', (1, 16)), ('proj_out_dim', (64, 128, 256))):
            for v in values:
                FLAGS.update(**{name: v})
                assert run.check_contrastive_loss_flags() is False
    finally:
        FLAGS.reset()


def test_value_errors_before_any_device_work():
    from simclr_amd import ops, run
    from simclr_amd.flags import FLAGS
    base = ['--dataset=synthetic', '--contrastive_loss=swav', '--train_steps=1', '--proj_out_dim=64', '--train_batch_size=16']
    try:
        for extra, msg in ((['--swav_num_prototypes=1'], 'swav_num_prototypes must lie in'), (['--swav_num_prototypes=0'], 'swav_num_prototypes must lie in'),
                           (['--swav_num_prototypes=1048577'], 'swav_num_prototypes must lie in'),
                           (['--swav_epsilon=0'], 'swav_epsilon must be > 0'), (['--swav_epsilon=-0.05'], 'swav_epsilon must be > 0'),
                           (['--swav_epsilon=nan'], 'swav_epsilon must be > 0'),
                           (['--swav_temperature=0'], 'swav_temperature must be > 0'), (['--swav_temperature=nan'], 'swav_temperature must be > 0'),
                           (['--swav_sinkhorn_iterations=0'], 'swav_sinkhorn_iterations must lie in'),
                           (['--swav_sinkhorn_iterations=17'], 'swav_sinkhorn_iterations must lie in'),
                           (['--swav_freeze_prototypes_epochs=-1'], 'swav_freeze_prototypes_epochs must be >= 0'),
                           (['--proj_out_dim=100'], 'swav needs a projection head of width 64/128/256'),
                           (['--proj_out_dim=512'], 'swav needs a projection head of width 64/128/256'),
                           (['--proj_head_mode=none'], 'swav needs a projection head of width 64/128/256')):
            FLAGS.reset()
            with pytest.raises(ValueError, match=msg):
                run.main(base + extra)
        # the message keeps the earlier values' order and names the new one
        FLAGS.reset()
        with pytest.raises(ValueError, match="must be 'dino' or 'ntxent' .*'barlow' or 'byol' or 'mocov2' \\(got 'swavv'\\), or 'swav'"):
            run.main(['--dataset=synthetic', '--contrastive_loss=swavv', '--train_steps=1'])
        # fine-tuning and evaluation ignore every SwAV flag
        bad = dict(proj_out_dim=100, swav_num_prototypes=1, swav_epsilon=-1.0, swav_sinkhorn_iterations=99, swav_freeze_prototypes_epochs=-3)
        FLAGS.reset()
        FLAGS.update(contrastive_loss='swav', train_mode='finetune', **bad)
        assert run.check_contrastive_loss_flags() is False and not run.swav_loss_on()
        FLAGS.reset()
        FLAGS.update(contrastive_loss='swav', mode='eval', **bad)
        assert run.check_contrastive_loss_flags() is False
        # the bindings refuse before they touch the library
        z, w, a = torch.zeros(8, 64), torch.zeros(4, 64), torch.zeros(2, 4)
        with pytest.raises(ValueError, match='widths 64/128/256'):
            ops.swav_fwd(torch.zeros(8, 100), torch.zeros(4, 100), a, 0.1, 0.05)
        with pytest.raises(ValueError, match='b >= 1'):
            ops.swav_fwd(torch.zeros(7, 64), w, a, 0.1, 0.05)
        with pytest.raises(ValueError, match='K in \\[2, 1048576\\]'):
            ops.swav_fwd(z, w[:1], a[:, :1], 0.1, 0.05)
        with pytest.raises(ValueError, match='K in \\[2, 1048576\\]'):
            ops.swav_sinkhorn(z, torch.zeros(4, 128))
        with pytest.raises(ValueError, match='alpha is the contiguous float32'):
            ops.swav_fwd(z, w, torch.zeros(4, 2), 0.1, 0.05)
        with pytest.raises(ValueError, match='alpha is the contiguous float32'):
            ops.swav_bwd_w(z, w, torch.zeros(2, 5), 0.1, 0.05, torch.zeros(8, 2), 1.0, None)
        for T in (0.0, -1.0, float('nan'), float('inf')):
            with pytest.raises(ValueError, match='the temperature must be > 0'):
                ops.swav_fwd(z, w, a, T, 0.05)
            with pytest.raises(ValueError, match='epsilon must be > 0'):
                ops.swav_fwd(z, w, a, 0.1, T)
            with pytest.raises(ValueError, match='epsilon must be > 0'):
                ops.swav_sinkhorn(z, w, T, 3)
            with pytest.raises(ValueError, match='the temperature must be > 0'):
                ops.swav_bwd_q(z, w, z, T, torch.zeros(8, 2), 1.0, None)
        for iters in (0, 17, -1, 2.5):
            with pytest.raises(ValueError, match='iterations lie in \\[1, 16\\]'):
                ops.swav_sinkhorn(z, w, 0.05, iters)
    finally:
        FLAGS.reset()


def test_make_single_step_messages():
    from simclr_amd import run
    from simclr_amd.flags import FLAGS

    class Target:
        queue = center = None
        steps_per_epoch = 10
    try:
        FLAGS.reset()
        FLAGS.update(contrastive_loss='swav', proj_out_dim=64)
        with pytest.raises(ValueError, match='swav needs steps_per_epoch >= 1'):
            run.make_single_step(object(), object(), None)
        with pytest.raises(ValueError, match='swav needs steps_per_epoch >= 1'):
            run.make_single_step(object(), object(), None, steps_per_epoch=0)
        with pytest.raises(ValueError, match='belongs to the BYOL'):                  # no target network with this loss
            run.make_single_step(object(), object(), None, target=Target(), steps_per_epoch=10)
        assert callable(run.make_single_step(object(), object(), None, steps_per_epoch=10))
    finally:
        FLAGS.reset()


def test_metric_names_of_the_swav_loss():
    from simclr_amd import run
    from simclr_amd.flags import FLAGS
    try:
        FLAGS.reset()
        FLAGS.update(contrastive_loss='swav')
        assert sorted(run.build_metrics()) == ['train/contrast_loss', 'train/supervised_acc', 'train/supervised_loss',
                                               'train/swav_code_entropy', 'train/total_loss', 'train/weight_decay']
        FLAGS.update(lineareval_while_pretraining=False)
        assert sorted(run.build_metrics()) == ['train/contrast_loss', 'train/swav_code_entropy', 'train/total_loss', 'train/weight_decay']
        FLAGS.update(train_mode='finetune')                              # fine-tuning ignores the flag
        assert sorted(run.build_metrics()) == ['train/supervised_acc', 'train/supervised_loss', 'train/total_loss', 'train/weight_decay']
    finally:
        FLAGS.reset()


def _built_model(**flags):
    from simclr_amd import model as model_lib
    from simclr_amd.flags import FLAGS
    from simclr_amd.resnet import RT
    FLAGS.reset()
    FLAGS.update(resnet_depth=18, image_size=32, **flags)
    RT.reset()
    RT.device = 'cpu'
    m = model_lib.Model(10)
    m.build_variables()
    return m


def test_the_swav_model_is_the_ntxent_model_plus_the_prototypes_built_last():
    from simclr_amd import model as model_lib
    from simclr_amd.flags import FLAGS
    from simclr_amd.resnet import RT
    try:
        plain = _built_model(contrastive_loss='ntxent', proj_out_dim=64)
        plain_vars = [(v.name, v.value.clone()) for v in plain.variables]
        swav = _built_model(contrastive_loss='swav', proj_out_dim=64, swav_num_prototypes=200)
        assert swav.prediction_head is None and isinstance(swav.prototype_head, model_lib.PrototypeHead)
        names = [v.name for v in swav.variables]
        assert names[:-1] == [n for n, _ in plain_vars] and names[-1] == 'model/prototype_head/kernel:0'
        assert all(torch.equal(v.value, w) for v, (_, w) in zip(swav.variables, plain_vars))
        proto = swav.variables[-1]
        assert proto.shape == (200, 64) and proto.trainable and swav.trainable_variables[-1] is proto
        # the same variable a dino run of that width and table size starts from
        dino = _built_model(contrastive_loss='dino', proj_out_dim=64, dino_out_dim=200)
        assert torch.equal(dino.variables[-1].value, proto.value)
        opt = model_lib.build_optimizer(0.1)
        assert opt._use_weight_decay(proto.name) and opt._do_layer_adaptation(proto.name)
        assert _built_model(contrastive_loss='swav', proj_out_dim=64).prototype_head.num_prototypes == 3000        # the default
        assert _built_model(contrastive_loss='swav', train_mode='finetune', proj_out_dim=64).prototype_head is None
    finally:
        FLAGS.reset()
        RT.reset()
