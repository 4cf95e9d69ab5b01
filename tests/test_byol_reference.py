"""The BYOL restatement (tests/byol_reference.py) pinned on the CPU: against torch float64 autograd, the hand-derived cases of
tests/golden/BYOL_HAND_DERIVED.md and the properties of the loss; the float32 moving average and the tau schedule; then the flags, their
refusals, the metric names and what --contrastive_loss=byol adds to the online model's variables.  No GPU."""
import math

import numpy as np
import pytest
import torch

from tests.byol_reference import EPS, byol_loss, ema_f32, one_minus_tau_f32, tau_schedule


def _torch_loss(q, t):
    """The loss as one would write it in a framework: l2_normalize with a clamped squared norm, squared distance, both directions."""
    b = q.shape[0] // 2

    def l2n(x):
        return x / torch.sqrt(torch.clamp((x * x).sum(-1, keepdim=True), min=EPS))
    qh, th = l2n(q), l2n(t)
    tp = torch.roll(th, -b, 0)
    return ((qh - tp) ** 2).sum() / b, (qh * tp).sum(-1).mean()


@pytest.mark.parametrize('b,D', [(1, 4), (3, 64), (5, 320), (16, 128)])
def test_loss_and_gradient_vs_float64_autograd(b, D):
    g = np.random.default_rng(b * 1000 + D)
    q = g.standard_normal((2 * b, D)) * g.uniform(0.1, 10.0, (2 * b, 1))
    t = g.standard_normal((2 * b, D)) * g.uniform(0.1, 10.0, (2 * b, 1))
    ref = byol_loss(q, t, grad_scale=0.5)
    qt = torch.tensor(q, dtype=torch.float64, requires_grad=True)
    loss, cos = _torch_loss(qt, torch.tensor(t, dtype=torch.float64))
    (0.5 * loss).backward()
    assert abs(ref['loss'] - loss.item()) <= 1e-13 * abs(loss.item())
    assert abs(ref['cosine'] - cos.item()) <= 1e-13
    assert np.abs(ref['grad'] - qt.grad.numpy()).max() <= 1e-12 * np.abs(qt.grad.numpy()).max()
    # |qhat - that|^2 = 2 - 2 cos for unit rows
    assert abs(ref['loss'] - 2.0 * (2.0 - 2.0 * ref['cosine'])) <= 1e-12


def test_eps_branch_vs_float64_autograd():
    """A q row below the epsilon: torch.clamp hands its gradient to the constant, as tf.maximum does."""
    g = np.random.default_rng(7)
    q = g.standard_normal((6, 8))
    q[2] = 1e-8 * g.standard_normal(8)            # sum q^2 ~ 8e-16 < 1e-12
    q[4] = 0.0
    t = g.standard_normal((6, 8))
    ref = byol_loss(q, t)
    qt = torch.tensor(q, dtype=torch.float64, requires_grad=True)
    loss, _ = _torch_loss(qt, torch.tensor(t, dtype=torch.float64))
    loss.backward()
    assert abs(ref['loss'] - loss.item()) <= 1e-13 * loss.item()
    assert np.abs(ref['grad'] - qt.grad.numpy()).max() <= 1e-12 * np.abs(qt.grad.numpy()).max()
    assert np.abs(ref['grad'][4]).max() > 1e5      # the 1e6 of the constant norm


def test_hand_derived_case():
    """tests/golden/BYOL_HAND_DERIVED.md, case 1: q = (3, 4), t = (1, 0) in both rows (b = 1)."""
    q = np.array([[3.0, 4.0], [3.0, 4.0]])
    t = np.array([[1.0, 0.0], [1.0, 0.0]])
    ref = byol_loss(q, t)
    assert np.allclose(ref['rows'], [0.8, 0.8], rtol=0, atol=1e-15)
    assert abs(ref['cosine'] - 0.6) <= 1e-15
    assert abs(ref['loss'] - 1.6) <= 1e-15                      # (1 / b) * (0.8 + 0.8)
    assert np.allclose(ref['grad'], [[-0.256, 0.192]] * 2, rtol=0, atol=1e-15)


def test_hand_derived_zero_row():
    """Case 2: a zero q row: qhat = 0, l = |that|^2 = 1, gradient = 2 (0 - that) / 1e-6."""
    q = np.array([[0.0, 0.0], [3.0, 4.0]])
    t = np.array([[1.0, 0.0], [0.0, 2.0]])
    ref = byol_loss(q, t)
    assert ref['rows'][0] == 1.0                                # row 0 pairs with t row 1: that = (0, 1)
    assert np.allclose(ref['grad'][0], -2e6 * np.array([0.0, 1.0]), rtol=1e-12, atol=0)
    assert np.isfinite(ref['grad']).all() and np.isfinite(ref['loss'])


def test_invariant_under_positive_rescaling_of_any_row():
    g = np.random.default_rng(3)
    q, t = g.standard_normal((8, 16)), g.standard_normal((8, 16))
    base = byol_loss(q, t)
    q2, t2 = q.copy(), t.copy()
    q2[1] *= 7.5
    q2[6] *= 1e-3
    t2[0] *= 123.0
    t2[5] *= 0.25
    other = byol_loss(q2, t2)
    assert abs(other['loss'] - base['loss']) <= 1e-13 and abs(other['cosine'] - base['cosine']) <= 1e-13
    assert np.abs(other['rows'] - base['rows']).max() <= 1e-13


def test_identical_unit_rows_give_zero():
    g = np.random.default_rng(4)
    x = g.standard_normal((4, 32))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    q = np.concatenate([x, x])                   # row r and row r + b are the same vector
    ref = byol_loss(q, q)
    assert ref['loss'] <= 1e-30 and abs(ref['cosine'] - 1.0) <= 1e-15
    assert np.abs(ref['grad']).max() <= 1e-14


@pytest.mark.parametrize('D,factor', [(64, 500.0), (2048, 3000.0)])
def test_fp32_cosine_form_loses_the_near_converged_loss(D, factor):
    """Why the kernel sums squared differences: at t = q + 1e-3 randn, b = 16 (the shapes of the GPU test) the loss is ~2e-6, and
    2 - 2 cos with the cosine accumulated in fp32 the way a kernel's lane would (one running sum) misses the GPU test's 1e-5 gate by more
    than 3000x at D = 2048 (measured 0.17 - 0.42 relative over four seeds) and by more than 500x at D = 64, where 32 times fewer
    roundings enter the sum (measured 0.014 - 0.10)."""
    b = 16
    g = np.random.default_rng(D)
    q = g.standard_normal((2 * b, D)).astype(np.float32)
    t = np.roll((q + 1e-3 * g.standard_normal((2 * b, D))).astype(np.float32), b, axis=0)     # row r of q pairs with row r + b of t
    ref = byol_loss(q, t)
    assert 1e-7 < ref['loss'] < 1e-4
    qh = q / np.sqrt((q * q).sum(-1, keepdims=True, dtype=np.float32))
    th = np.roll(t, -b, axis=0)
    th = th / np.sqrt((th * th).sum(-1, keepdims=True, dtype=np.float32))
    cos32 = np.zeros(2 * b, np.float32)
    for j in range(D):
        cos32 = (cos32 + qh[:, j] * th[:, j]).astype(np.float32)
    loss32 = float((np.float32(2.0) - np.float32(2.0) * cos32).sum(dtype=np.float32)) / b
    assert abs(loss32 - ref['loss']) > factor * 1e-5 * ref['loss']


@pytest.mark.parametrize('R', [2, 3])
def test_mean_of_replica_values_is_the_value_of_the_whole_batch(R):
    """No collective: a replica holds rows [its view-a rows; its view-b rows]; the mean of the R values (and of the cosines) equals the
    value on the gathered batch, and each replica's gradient with grad_scale = 1 / R is its slice of the whole batch's gradient."""
    n, D = 5, 16
    g = np.random.default_rng(R)
    q, t = g.standard_normal((2 * n * R, D)), g.standard_normal((2 * n * R, D))
    whole = byol_loss(q, t)
    N = n * R
    parts = []
    for r in range(R):
        idx = np.concatenate([np.arange(r * n, (r + 1) * n), N + np.arange(r * n, (r + 1) * n)])
        parts.append((idx, byol_loss(q[idx], t[idx], grad_scale=1.0 / R)))
    assert abs(np.mean([p['loss'] for _, p in parts]) - whole['loss']) <= 1e-13
    assert abs(np.mean([p['cosine'] for _, p in parts]) - whole['cosine']) <= 1e-13
    for idx, p in parts:
        assert np.abs(p['grad'] - whole['grad'][idx]).max() <= 1e-14


# ---------------------------------------------------------------------------------------------------------------- EMA, tau
def test_ema_fixed_points_are_bitwise():
    g = np.random.default_rng(9)
    t = g.standard_normal(1000).astype(np.float32) * np.float32(37.0)
    o = g.standard_normal(1000).astype(np.float32)
    assert ema_f32(t, t.copy(), 0.004).tobytes() == t.tobytes()              # o == t
    assert ema_f32(t, o, 0.0).tobytes() == t.tobytes()                       # tau = 1
    moved = ema_f32(t, o, one_minus_tau_f32(0, 10, 0.996))
    assert moved.dtype == np.float32 and not np.array_equal(moved, t)
    assert np.abs(moved.astype(np.float64) - (0.996 * t.astype(np.float64) + 0.004 * o.astype(np.float64))).max() <= 1e-5


def test_tau_schedule():
    for base in (0.0, 0.9, 0.996, 1.0):
        assert tau_schedule(0, 1000, base) == base
        assert tau_schedule(1000, 1000, base) == 1.0
        taus = [tau_schedule(k, 1000, base) for k in range(1001)]
        assert all(b >= a for a, b in zip(taus, taus[1:]))
        assert all(0.0 <= x <= 1.0 for x in taus)
    assert abs(tau_schedule(500, 1000, 0.996) - 0.998) <= 1e-15
    from simclr_amd import model as model_lib
    assert all(model_lib.byol_tau(k, 77, 0.99) == tau_schedule(k, 77, 0.99) for k in range(78))
    assert one_minus_tau_f32(0, 10, 0.996) == np.float32(1.0 - 0.996)


# ---------------------------------------------------------------------------------------------------------------- flags, names
def test_flags_parse_and_defaults():
    from simclr_amd import run
    from simclr_amd.flags import FLAGS
    try:
        FLAGS.reset()
        assert FLAGS.contrastive_loss == 'ntxent' and FLAGS.byol_tau_base == 0.996 and FLAGS.byol_pred_hidden_dim == 4096
        assert not run.byol_loss_on()
        FLAGS.parse(['--contrastive_loss=byol', '--byol_tau_base=0.99', '--byol_pred_hidden_dim=512', '--proj_out_dim=256'])
        assert (FLAGS.contrastive_loss, FLAGS.byol_tau_base, FLAGS.byol_pred_hidden_dim) == ('byol', 0.99, 512)
        assert run.check_contrastive_loss_flags() is False and run.byol_loss_on()
        assert not run.generalized_loss_on() and not run.supcon_loss_on() and not run.barlow_loss_on()
        FLAGS.update(hidden_norm=False, temperature=-3.0)                # ignored with this loss
        assert run.check_contrastive_loss_flags() is False
        FLAGS.reset()
        FLAGS.update(contrastive_loss='byol', proj_head_mode='none')     # the encoder width: 2048 for ResNet-50
        assert run.check_contrastive_loss_flags() is False
        for tau in (0.0, 1.0):
            FLAGS.update(byol_tau_base=tau)
            assert run.check_contrastive_loss_flags() is False
    finally:
        FLAGS.reset()


def test_value_errors_before_any_device_work():
    from simclr_amd import ops, run
    from simclr_amd.flags import FLAGS
    base = ['--dataset=synthetic', '--contrastive_loss=byol', '--train_steps=1', '--proj_out_dim=64']
    try:
        for extra, msg in ((['--byol_tau_base=-0.01'], 'byol_tau_base must lie in'), (['--byol_tau_base=1.5'], 'byol_tau_base must lie in'),
                           (['--byol_tau_base=nan'], 'byol_tau_base must lie in'),
                           (['--byol_pred_hidden_dim=100'], 'byol_pred_hidden_dim must be a multiple of 64'),
                           (['--byol_pred_hidden_dim=32'], 'byol_pred_hidden_dim must be a multiple of 64'),
                           (['--byol_pred_hidden_dim=0'], 'byol_pred_hidden_dim must be a multiple of 64'),
                           (['--byol_pred_hidden_dim=8256'], 'byol_pred_hidden_dim must be a multiple of 64'),
                           (['--proj_out_dim=100'], 'byol needs a loss width'), (['--proj_out_dim=8256'], 'byol needs a loss width'),
                           (['--proj_out_dim=32'], 'byol needs a loss width'),
                           (['--proj_head_mode=none', '--width_multiplier=8'], 'byol needs a loss width')):
            FLAGS.reset()
            with pytest.raises(ValueError, match=msg):
                run.main(base + extra)
        FLAGS.reset()
        with pytest.raises(ValueError, match="'ntxent' or 'generalized' or 'supcon' or 'barlow' or 'byol'"):
            run.main(['--dataset=synthetic', '--contrastive_loss=moco', '--train_steps=1'])
        # fine-tuning and evaluation ignore the loss flags
        FLAGS.reset()
        FLAGS.update(contrastive_loss='byol', train_mode='finetune', proj_out_dim=100, byol_tau_base=2.0, byol_pred_hidden_dim=3)
        assert run.check_contrastive_loss_flags() is False and not run.byol_loss_on()
        FLAGS.reset()
        FLAGS.update(contrastive_loss='byol', mode='eval', proj_out_dim=100, byol_tau_base=2.0, byol_pred_hidden_dim=3)
        assert run.check_contrastive_loss_flags() is False
        # the bindings refuse before they touch the library
        with pytest.raises(ValueError, match='multiples of 64 in \\[64, 8192\\]'):
            ops.byol_fwd(torch.zeros(8, 100), torch.zeros(8, 100))
        with pytest.raises(ValueError, match='one shape'):
            ops.byol_fwd(torch.zeros(8, 64), torch.zeros(8, 128))
        with pytest.raises(ValueError, match='one shape'):
            ops.byol_fwd(torch.zeros(8, 64), torch.zeros(6, 64))
        with pytest.raises(ValueError, match='b >= 1'):
            ops.byol_fwd(torch.zeros(0, 64), torch.zeros(0, 64))
        with pytest.raises(ValueError, match='b >= 1'):
            ops.byol_fwd(torch.zeros(7, 64), torch.zeros(7, 64))
        # a BYOL step without a target network
        FLAGS.reset()
        FLAGS.update(contrastive_loss='byol', proj_out_dim=64)
        with pytest.raises(ValueError, match='needs a target network'):
            run.make_single_step(object(), object(), None)
        FLAGS.reset()
        with pytest.raises(ValueError, match='belongs to the BYOL'):
            run.make_single_step(object(), object(), None, target=object())
    finally:
        FLAGS.reset()


def test_metric_names_of_the_byol_loss():
    from simclr_amd import run
    from simclr_amd.flags import FLAGS
    try:
        FLAGS.reset()
        FLAGS.update(contrastive_loss='byol')
        assert sorted(run.build_metrics()) == ['train/byol_cosine', 'train/contrast_loss', 'train/supervised_acc', 'train/supervised_loss',
                                               'train/total_loss', 'train/weight_decay']
        FLAGS.update(lineareval_while_pretraining=False)
        assert sorted(run.build_metrics()) == ['train/byol_cosine', 'train/contrast_loss', 'train/total_loss', 'train/weight_decay']
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


@pytest.mark.parametrize('extra', [dict(proj_out_dim=64), dict(proj_head_mode='none'), dict(proj_out_dim=128, lineareval_while_pretraining=False)])
def test_byol_adds_only_the_predictor_to_the_online_model(extra):
    """Names and initial values of the online encoder, projection head and supervised head are those of an ntxent model; the predictor's
    four variables come on top, under prediction_head, and are trained, weight-decayed and LARS-adapted by the name rules."""
    from simclr_amd import model as model_lib
    from simclr_amd.flags import FLAGS
    from simclr_amd.resnet import RT
    try:
        plain = _built_model(contrastive_loss='ntxent', **extra)
        assert plain.prediction_head is None
        plain_vars = [(v.name, v.value.clone()) for v in plain.variables]
        byol = _built_model(contrastive_loss='byol', byol_pred_hidden_dim=128, **extra)
        rest = [v for v in byol.variables if 'prediction_head' not in v.name]
        pred = [v for v in byol.variables if 'prediction_head' in v.name]
        assert [v.name for v in rest] == [n for n, _ in plain_vars]
        assert all(torch.equal(v.value, w) for v, (_, w) in zip(rest, plain_vars))
        width = model_lib.projection_width()
        assert width == (512 if extra.get('proj_head_mode') == 'none' else extra['proj_out_dim'])
        assert len(pred) == 6 and all(v.name.startswith('model/prediction_head/') for v in pred)
        shapes = {v.name.split('/')[-1]: v.shape for v in pred if 'l_0' in v.name or 'l_1' in v.name}
        kernels = [v for v in pred if v.name.endswith('kernel:0')]
        assert [k.shape for k in kernels] == [(width, 128), (128, width)]
        assert not any('bias' in v.name for v in pred)                      # l_0's bias is its BatchNorm's beta; l_1 has none
        assert sorted(shapes) == ['beta:0', 'gamma:0', 'kernel:0', 'moving_mean:0', 'moving_variance:0']
        trainable = {v.name for v in byol.trainable_variables}
        assert {v.name for v in pred if 'moving_' not in v.name} <= trainable and len(trainable) == len(plain.trainable_variables) + 4
        opt = model_lib.build_optimizer(0.1)
        for k in kernels:
            assert opt._use_weight_decay(k.name) and opt._do_layer_adaptation(k.name)
        for v in pred:
            if 'batch_normalization' in v.name:
                assert not opt._use_weight_decay(v.name) and not opt._do_layer_adaptation(v.name)
        # fine-tuning ignores the flag: no predictor
        ft = _built_model(contrastive_loss='byol', train_mode='finetune', **{k: v for k, v in extra.items() if k != 'lineareval_while_pretraining'})
        assert ft.prediction_head is None
    finally:
        FLAGS.reset()
        RT.reset()


def test_target_flag_values_build_no_heads_but_the_projection():
    from simclr_amd import model as model_lib
    from simclr_amd.flags import FLAGS
    from simclr_amd.resnet import RT
    try:
        online = _built_model(contrastive_loss='byol', proj_out_dim=64, byol_pred_hidden_dim=64)
        names = [v.name for v in online.resnet_model.variables + online._projection_head.variables]
        with FLAGS.override(**model_lib.target_flag_values()), RT.fresh_names():
            t = model_lib.Model(0)
            t.build_variables()
        assert t.supervised_head is None and t.prediction_head is None
        assert [v.name for v in t.variables] == names
        assert FLAGS.contrastive_loss == 'byol' and FLAGS.lineareval_while_pretraining
    finally:
        FLAGS.reset()
        RT.reset()
