"""CPU tests of the distillation stage: the float64 reference tests/kd_reference.py (the yardstick of tests/test_gpu_distill.py) against
torch autograd, two hand-derived cases and the arg-max tie rule; the new flags; the metric names with and without a teacher."""
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.kd_reference import first_argmax, kd_reference

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'kd_hand_cases.json')


@pytest.mark.parametrize('rows,nclass', [(1, 2), (5, 10), (7, 65), (3, 1000)])
@pytest.mark.parametrize('T', [0.1, 1.0, 4.0])
@pytest.mark.parametrize('gscale', [1.0, 0.5])
def test_reference_equals_autograd(rows, nclass, T, gscale):
    g = torch.Generator().manual_seed(rows * 1000 + nclass)
    s = (torch.randn(rows, nclass, generator=g, dtype=torch.float64) * 3).requires_grad_(True)
    t = torch.randn(rows, nclass, generator=g, dtype=torch.float64) * 3
    # T^2 * mean(CE(softmax(t / T), s / T)): F.cross_entropy with probability targets averages over the rows
    loss = T * T * F.cross_entropy(s / T, F.softmax(t / T, dim=1))
    (grad,) = torch.autograd.grad(loss, s)
    ref = kd_reference(s.detach().numpy(), t.numpy(), T, gscale)
    assert abs(ref['loss'] - float(loss.detach())) <= 1e-12 * max(1.0, abs(float(loss.detach())))
    # both sides form T (q - p) / rows from probabilities <= 1 that carry a few float64 roundings each: where q and p nearly cancel the
    # difference keeps an absolute error of some 2^-53, scaled by T * gscale / rows; 16 such units, plus 1e-13 relative
    scale = float(grad.abs().max())
    bound = 1e-13 * scale * gscale + 16 * 2.0 ** -53 * T * gscale / rows
    assert float(np.abs(ref['dlogits'] - gscale * grad.numpy()).max()) <= bound
    assert ref['agreement'] == float((s.argmax(1) == t.argmax(1)).double().mean())
    assert np.allclose(ref['p'].sum(1), 1) and np.allclose(ref['q'].sum(1), 1)


def _value(x):
    return x['times'] * math.log(x['ln']) if isinstance(x, dict) else float(x)


def test_reference_equals_the_hand_derived_cases():
    with open(GOLDEN) as f:
        cases = json.load(f)['cases']
    assert [c['name'] for c in cases] == ['T1', 'T2']
    for c in cases:
        s = [[_value(x) for x in row] for row in c['student']]
        t = [[_value(x) for x in row] for row in c['teacher']]
        ref = kd_reference(s, t, c['temperature'])
        assert abs(ref['loss'] - _value(c['loss'])) <= 1e-15, c['name']
        assert float(np.abs(ref['dlogits'] - np.array(c['dlogits'])).max()) <= 1e-15, c['name']
        assert ref['agreement'] == c['agreement']
    # the two cases as numbers, independent of the file's notation
    assert abs(kd_reference([[0, 0]], [[math.log(3), 0]], 1.0)['loss'] - math.log(2)) <= 1e-15
    assert abs(kd_reference([[0, 0]], [[2 * math.log(3), 0]], 2.0)['loss'] - 4 * math.log(2)) <= 1e-15


def test_reference_ties_the_lower_column_wins():
    rng = np.random.default_rng(0)
    base = np.clip(rng.standard_normal((6, 80)) * 3, -8, 8)
    tied = base.copy()
    tied[:, 6] = 12.0
    tied[:, 71] = 12.0
    only_lo, only_hi = base.copy(), base.copy()
    only_lo[:, 6] = 12.0
    only_hi[:, 71] = 12.0
    assert (first_argmax(tied) == 6).all() and (first_argmax(tied) == np.argmax(tied, 1)).all()
    # a tie on the student side, on the teacher side, on both: column 6 stands for the tied rows
    assert kd_reference(tied, only_lo, 1.0)['agreement'] == 1.0
    assert kd_reference(tied, only_hi, 1.0)['agreement'] == 0.0
    assert kd_reference(only_lo, tied, 1.0)['agreement'] == 1.0
    assert kd_reference(only_hi, tied, 1.0)['agreement'] == 0.0
    assert kd_reference(tied, tied, 1.0)['agreement'] == 1.0
    mixed = tied.copy()
    mixed[::2] = only_hi[::2]
    assert kd_reference(mixed, tied, 1.0)['agreement'] == 0.5


def test_identical_rows_give_zero_gradient_and_the_entropy():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((4, 10)) * 3
    for T in (0.1, 1.0, 4.0):
        ref = kd_reference(x, x, T)
        p = ref['p']
        ent = -(p * np.log(np.maximum(p, 1e-300))).sum(1)
        assert np.abs(ref['dlogits']).max() <= 1e-16
        assert np.allclose(ref['loss_rows'], T * T * ent, rtol=1e-12, atol=1e-15)


def test_distillation_flags_parse_and_default():
    from simclr_amd.flags import FLAGS
    try:
        FLAGS.reset()
        assert FLAGS.teacher_checkpoint is None and FLAGS.distill_temperature == 1.0
        for n in ('resnet_depth', 'width_multiplier', 'sk_ratio', 'ft_proj_selector'):
            assert getattr(FLAGS, 'teacher_' + n) is None
        FLAGS.parse(['--resnet_depth=18', '--sk_ratio=0.0625', '--ft_proj_selector=1', '--width_multiplier=2'])
        from simclr_amd.model import teacher_flag_values
        tv = teacher_flag_values()
        assert (tv['resnet_depth'], tv['width_multiplier'], tv['sk_ratio'], tv['ft_proj_selector']) == (18, 2, 0.0625, 1)
        assert tv['train_mode'] == 'finetune'
        FLAGS.parse(['--teacher_checkpoint=/some/ckpt-4.pt', '--distill_temperature=2.5', '--teacher_resnet_depth=50',
                     '--teacher_width_multiplier=2', '--teacher_sk_ratio=0.0625', '--teacher_ft_proj_selector=1', '--resnet_depth=18'])
        assert FLAGS.teacher_checkpoint == '/some/ckpt-4.pt' and FLAGS.distill_temperature == 2.5
        assert (FLAGS.teacher_resnet_depth, FLAGS.teacher_width_multiplier, FLAGS.teacher_sk_ratio, FLAGS.teacher_ft_proj_selector) == \
               (50, 2, 0.0625, 1)
        tv = teacher_flag_values()
        assert (tv['resnet_depth'], tv['width_multiplier'], tv['sk_ratio'], tv['ft_proj_selector']) == (50, 2, 0.0625, 1)
        assert FLAGS.resnet_depth == 18 and FLAGS.sk_ratio == 0.0
        with FLAGS.override(**tv):
            assert FLAGS.resnet_depth == 50 and FLAGS.train_mode == 'finetune'
        assert FLAGS.resnet_depth == 18 and FLAGS.train_mode == 'pretrain'
    finally:
        FLAGS.reset()


def test_metric_names_with_and_without_a_teacher():
    from simclr_amd import run
    from simclr_amd.flags import FLAGS
    try:
        FLAGS.reset()
        assert sorted(run.build_metrics()) == ['train/contrast_acc', 'train/contrast_entropy', 'train/contrast_loss',
                                               'train/supervised_acc', 'train/supervised_loss', 'train/total_loss', 'train/weight_decay']
        FLAGS.update(lineareval_while_pretraining=False)
        assert sorted(run.build_metrics()) == ['train/contrast_acc', 'train/contrast_entropy', 'train/contrast_loss',
                                               'train/total_loss', 'train/weight_decay']
        FLAGS.update(train_mode='finetune')
        assert sorted(run.build_metrics()) == ['train/supervised_acc', 'train/supervised_loss', 'train/total_loss', 'train/weight_decay']
        FLAGS.update(teacher_checkpoint='/some/ckpt-4.pt')
        assert sorted(run.build_metrics()) == ['train/distill_agreement', 'train/distill_loss', 'train/total_loss', 'train/weight_decay']
    finally:
        FLAGS.reset()


def test_a_teacher_requires_finetune_before_any_device_work():
    from simclr_amd import run
    from simclr_amd.flags import FLAGS
    try:
        FLAGS.reset()
        with pytest.raises(ValueError, match='train_mode=finetune'):
            run.main(['--dataset=synthetic', '--train_mode=pretrain', '--teacher_checkpoint=/nowhere/ckpt-1.pt', '--train_steps=1'])
        FLAGS.reset()
        FLAGS.update(teacher_checkpoint='/nowhere/ckpt-1.pt', train_mode='pretrain', mode='eval')
        assert run.check_distillation_flags() is False           # --mode=eval ignores the teacher flags
    finally:
        FLAGS.reset()


def test_runtime_fresh_names_scopes_counters_scope_and_seed():
    from simclr_amd.resnet import RT, scope
    RT.reset()
    try:
        assert RT.unique('conv2d') == 'conv2d' and RT.unique('conv2d') == 'conv2d_1'
        RT.seed = 5
        marker = object()
        RT.convs.append(marker)
        with scope('model'):
            with RT.fresh_names():
                assert RT.unique('conv2d') == 'conv2d' and RT.path('x') == 'x'
                RT.seed += 3
                RT.convs.append(marker)
            assert RT.path('x') == 'model/x'
        assert RT.unique('conv2d') == 'conv2d_2' and RT.seed == 5
        assert len(RT.convs) == 2                                # the registry is shared, not scoped
    finally:
        RT.reset()
