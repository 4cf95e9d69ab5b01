"""The MoCo v2 restatement (tests/moco_reference.py) pinned on the CPU: against torch float64 autograd of cross_entropy on the concatenated
logits, the hand-derived cases of tests/golden/MOCO_HAND_DERIVED.md and the properties of the loss; the two float32 forms of a row's loss
near convergence; the queue's initial rows and write position; then the flags, their refusals, the metric names, the online model's
variables and the messages of make_single_step.  No GPU."""
import math

import numpy as np
import pytest
import torch

from tests.moco_reference import (EPS, l2_normalize, moco_logits, moco_loss, moco_loss_normalized, queue_init, queue_ptr, row_loss_f32)

GATE_LOSS = 1e-5          # the GPU tests' loss gate (tests/test_gpu_moco.py)


def _torch_loss(q, t, queue, T):
    """The loss as one would write it in a framework (MoCo's own code): logits = [positive | queue], labels = 0, cross entropy."""
    b = q.shape[0] // 2

    def l2n(x):
        return x / torch.sqrt(torch.clamp((x * x).sum(-1, keepdim=True), min=EPS))
    qh, th = l2n(q), l2n(t).detach()
    tp = torch.roll(th, -b, 0)
    logits = torch.cat([(qh * tp).sum(-1, keepdim=True), qh @ queue.T], 1) / T
    labels = torch.zeros(2 * b, dtype=torch.long)
    loss = torch.nn.functional.cross_entropy(logits, labels, reduction='sum') / b
    acc = (logits[:, 0] >= logits[:, 1:].max(-1).values).double().mean()
    return loss, acc


@pytest.mark.parametrize('b,D,K,T', [(1, 4, 1, 1.0), (3, 64, 5, 0.2), (5, 32, 70, 0.07), (16, 128, 200, 1.0)])
def test_loss_and_gradient_vs_float64_autograd(b, D, K, T):
    g = np.random.default_rng(b * 1000 + D + K)
    q = g.standard_normal((2 * b, D)) * g.uniform(0.1, 10.0, (2 * b, 1))
    t = g.standard_normal((2 * b, D)) * g.uniform(0.1, 10.0, (2 * b, 1))
    queue = queue_init(K, D, 3).astype(np.float64)
    ref = moco_loss(q, t, queue, T, grad_scale=0.5)
    qt = torch.tensor(q, dtype=torch.float64, requires_grad=True)
    loss, acc = _torch_loss(qt, torch.tensor(t, dtype=torch.float64), torch.tensor(queue), T)
    (0.5 * loss).backward()
    assert abs(ref['loss'] - loss.item()) <= 1e-12 * abs(loss.item())
    assert ref['acc'] == acc.item()
    assert np.abs(ref['grad'] - qt.grad.numpy()).max() <= 1e-11 * np.abs(qt.grad.numpy()).max()
    # the gradient wrt the normalised rows, against autograd on rows that are normalised already
    qh, th = l2_normalize(q)[0], l2_normalize(t)[0]
    refn = moco_loss_normalized(qh, th, queue, T, grad_scale=0.5)
    qn = torch.tensor(qh, dtype=torch.float64, requires_grad=True)
    tp = torch.roll(torch.tensor(th), -b, 0)
    logits = torch.cat([(qn * tp).sum(-1, keepdim=True), qn @ torch.tensor(queue).T], 1) / T
    (0.5 * torch.nn.functional.cross_entropy(logits, torch.zeros(2 * b, dtype=torch.long), reduction='sum') / b).backward()
    assert np.abs(refn['grad'] - qn.grad.numpy()).max() <= 1e-11 * np.abs(qn.grad.numpy()).max()
    assert np.abs(ref['grad_qhat'] - refn['grad']).max() <= 1e-15


def test_eps_branch_vs_float64_autograd():
    g = np.random.default_rng(7)
    q = g.standard_normal((6, 8))
    q[2] = 1e-8 * g.standard_normal(8)            # sum q^2 ~ 8e-16 < 1e-12
    q[4] = 0.0
    t = g.standard_normal((6, 8))
    queue = queue_init(9, 8, 1).astype(np.float64)
    ref = moco_loss(q, t, queue, 0.5)
    qt = torch.tensor(q, dtype=torch.float64, requires_grad=True)
    loss, _ = _torch_loss(qt, torch.tensor(t, dtype=torch.float64), torch.tensor(queue), 0.5)
    loss.backward()
    assert abs(ref['loss'] - loss.item()) <= 1e-13 * loss.item()
    assert np.abs(ref['grad'] - qt.grad.numpy()).max() <= 1e-12 * np.abs(qt.grad.numpy()).max()
    assert np.isfinite(ref['grad']).all()


def test_hand_derived_case():
    """tests/golden/MOCO_HAND_DERIVED.md, case 1: q = (3, 4), t = (1, 0) in both rows (b = 1), one queue row (0, 1), T = 1."""
    q = np.array([[3.0, 4.0], [3.0, 4.0]])
    t = np.array([[1.0, 0.0], [1.0, 0.0]])
    queue = np.array([[0.0, 1.0]])
    ref = moco_loss(q, t, queue, 1.0)
    l = math.log1p(math.exp(0.2))                               # s+ = 0.6, s_0 = 0.8
    p0 = 1.0 / (1.0 + math.exp(-0.2))
    assert np.allclose(ref['rows'], [l, l], rtol=0, atol=1e-15)
    assert abs(ref['loss'] - 2.0 * l) <= 1e-15 and abs(ref['loss'] - 1.5962778) <= 1e-7
    assert ref['acc'] == 0.0                                    # 0.6 < 0.8 in both rows
    assert np.allclose(ref['neg_mass'], [p0, p0], rtol=0, atol=1e-15)
    assert np.allclose(ref['grad_qhat'], [[-p0, p0]] * 2, rtol=0, atol=1e-15)
    assert np.allclose(ref['grad'], [[-0.224 * p0, 0.168 * p0]] * 2, rtol=0, atol=1e-15)      # (g - qhat (qhat . g)) / 5
    assert np.allclose(ref['grad'], [[-0.1231628, 0.0923721]] * 2, rtol=0, atol=1e-7)
    assert np.abs((ref['grad'] * q).sum(-1)).max() <= 1e-15     # a gradient through the normalisation is orthogonal to its row


def test_hand_derived_tie():
    """Case 2: the queue row is the positive key: s+ = s_0, l = ln 2, P+ = 1/2, the gradient wrt qhat cancels; equality is a hit.
    T = 1/4 scales the logits and changes nothing of this."""
    q = np.array([[3.0, 4.0], [0.0, 2.0]])
    t = np.array([[0.0, 5.0], [0.0, 5.0]])
    ref = moco_loss(q, t, np.array([[0.0, 1.0]]), 0.25)
    assert np.allclose(ref['rows'], [math.log(2.0)] * 2, rtol=0, atol=1e-15)
    assert abs(ref['loss'] - 2.0 * math.log(2.0)) <= 1e-15 and ref['acc'] == 1.0
    assert np.allclose(ref['neg_mass'], [0.5, 0.5], rtol=0, atol=1e-15) and np.abs(ref['grad']).max() <= 1e-15


@pytest.mark.parametrize('K', [1, 7, 64])
def test_zero_similarity_batch_gives_log_one_plus_K(K):
    """q orthogonal to its key and to every queue row: all K + 1 logits are 0, the positive is in the maximum, l = log(1 + K)."""
    D = 2 * K + 4
    q = np.zeros((4, D))
    q[:, 0] = 1.0
    t = np.zeros((4, D))
    t[:, 1] = 2.0
    queue = np.eye(D)[2:2 + K]
    ref = moco_loss(q, t, queue, 0.1)
    assert np.allclose(ref['rows'], math.log(1.0 + K), rtol=0, atol=1e-15) and abs(ref['loss'] - 2.0 * math.log(1.0 + K)) <= 1e-14
    assert ref['acc'] == 1.0 and np.allclose(ref['neg_mass'], K / (K + 1.0), rtol=0, atol=1e-15)


def test_invariant_under_permutation_of_the_queue_rows():
    g = np.random.default_rng(5)
    q, t = g.standard_normal((8, 16)), g.standard_normal((8, 16))
    queue = queue_init(37, 16, 2).astype(np.float64)
    base = moco_loss(q, t, queue, 0.2)
    other = moco_loss(q, t, queue[g.permutation(37)], 0.2)
    assert abs(other['loss'] - base['loss']) <= 1e-14 and other['acc'] == base['acc']
    assert np.abs(other['grad'] - base['grad']).max() <= 1e-14
    # and the other rows of the batch are no negatives: a row's loss depends on its own pair and the queue only
    q2, t2 = q.copy(), t.copy()
    q2[1] = g.standard_normal(16)
    t2[5] = g.standard_normal(16)                 # rows 1 and 5 are each other's pair (b = 4)
    alone = moco_loss(q2, t2, queue, 0.2)
    keep = [0, 2, 3, 4, 6, 7]
    assert np.abs(alone['rows'][keep] - base['rows'][keep]).max() <= 1e-15


def near_converged(D=64, K=64, b=16, seed=0):
    """The near-converged case of the GPU test: t = q + 1e-3 randn, unit queue rows of another seed -> float32 normalised rows."""
    g = np.random.default_rng(seed)
    q = g.standard_normal((2 * b, D)).astype(np.float32)
    t = np.roll((q + 1e-3 * g.standard_normal((2 * b, D))).astype(np.float32), b, axis=0)     # row r of q pairs with row r + b of t
    qh = l2_normalize(q)[0].astype(np.float32)
    th = l2_normalize(t)[0].astype(np.float32)
    return qh, th, queue_init(K, D, seed + 1000)


NEAR_T = 0.05


def test_naive_fp32_row_loss_loses_the_near_converged_loss_and_the_stable_form_keeps_it():
    """T = 0.05, K = 64, D = 64, b = 16: the loss is 4.6e-6 and 1 - P+ at most 6.2e-6.  From the same float32 logits, logsumexp - s+
    (two numbers ~ 20, ulp 1.9e-6) is off by 1.9e-2 relative; the negatives' sum kept apart (log1p) by 6.0e-8 (measured; recorded in
    tests/golden/MOCO_HAND_DERIVED.md).  1 - P+ formed as one minus exp(s+ - lse) in float32 loses the worst row's coefficient whole (100 %)."""
    b = 16
    qh, th, queue = near_converged()
    ref = moco_loss_normalized(qh, th, queue, NEAR_T)
    assert 1e-6 < ref['loss'] < 1e-5 and ref['acc'] == 1.0
    sp, S, _ = moco_logits(qh, th, queue, NEAR_T)
    stable = row_loss_f32(sp, S, stable=True).astype(np.float64).sum() / b
    naive = row_loss_f32(sp, S, stable=False).astype(np.float64).sum() / b
    err_stable, err_naive = abs(stable - ref['loss']) / ref['loss'], abs(naive - ref['loss']) / ref['loss']
    print('near-converged: loss %.4e  stable fp32 %.3e  naive fp32 %.3e' % (ref['loss'], err_stable, err_naive))
    assert err_stable <= 0.25 * GATE_LOSS
    assert err_naive > 100 * GATE_LOSS
    f = np.float32
    sp32, S32 = sp.astype(f), S.astype(f)
    total = (np.exp(S32 - sp32[:, None]).sum(-1, dtype=f) + f(1.0)).astype(f)             # the positive is every row's maximum
    lse = (sp32 + np.log(total).astype(f)).astype(f)
    one_minus = (f(1.0) - np.exp((sp32 - lse).astype(f)).astype(f)).astype(f)             # P+ = exp(s+ - lse), then one minus it
    err = np.abs(one_minus.astype(np.float64) - ref['neg_mass']) / ref['neg_mass']
    print('1 - P+ by subtraction in fp32: worst relative error %.3e, median %.3e' % (err.max(), np.median(err)))
    assert err.max() >= 1.0                                                               # a row's whole coefficient is lost
    share = (np.exp(S32 - sp32[:, None]).sum(-1, dtype=f) / total).astype(f)   # the negatives' share
    assert (np.abs(share.astype(np.float64) - ref['neg_mass']) / ref['neg_mass']).max() <= 1e-5


@pytest.mark.parametrize('R', [2, 3])
def test_mean_of_replica_values_is_the_value_of_the_whole_batch(R):
    """No collective: the mean of the R replica values equals the value on the gathered batch against the same queue, and a replica's
    gradient with grad_scale = 1 / R is its slice of the whole batch's gradient."""
    n, D = 5, 16
    g = np.random.default_rng(R)
    q, t = g.standard_normal((2 * n * R, D)), g.standard_normal((2 * n * R, D))
    queue = queue_init(11, D, 0).astype(np.float64)
    whole = moco_loss(q, t, queue, 0.3)
    N = n * R
    parts = []
    for r in range(R):
        idx = np.concatenate([np.arange(r * n, (r + 1) * n), N + np.arange(r * n, (r + 1) * n)])
        parts.append((idx, moco_loss(q[idx], t[idx], queue, 0.3, grad_scale=1.0 / R)))
    assert abs(np.mean([p['loss'] for _, p in parts]) - whole['loss']) <= 1e-13
    assert abs(np.mean([p['acc'] for _, p in parts]) - whole['acc']) <= 1e-13
    for idx, p in parts:
        assert np.abs(p['grad'] - whole['grad'][idx]).max() <= 1e-14


# ---------------------------------------------------------------------------------------------------------------- queue
def test_queue_initialisation_is_reproducible_and_unit():
    from simclr_amd import model as model_lib
    a, b = queue_init(100, 64, 0), queue_init(100, 64, 0)
    assert a.dtype == np.float32 and a.shape == (100, 64) and a.tobytes() == b.tobytes()
    assert np.abs(np.sqrt((a.astype(np.float64) ** 2).sum(-1)) - 1.0).max() <= 1e-7
    assert not np.array_equal(a, queue_init(100, 64, 1))
    assert model_lib.moco_queue_init(100, 64, 0).tobytes() == a.tobytes()
    x = np.random.default_rng([0]).standard_normal((100, 64))
    assert np.array_equal(a, (x / np.sqrt((x * x).sum(1, keepdims=True))).astype(np.float32))
    qobj = model_lib.MocoQueue(100, 64, seed=0, device='cpu')
    assert [v.name for v in qobj.variables] == ['moco/queue'] and not qobj.variables[0].trainable
    assert qobj.value.numpy().tobytes() == a.tobytes()
    with pytest.raises(ValueError, match='K >= 1'):
        model_lib.MocoQueue(0, 64, device='cpu')


def test_queue_write_position_and_wrap():
    from simclr_amd import model as model_lib
    K, rows = 24, 8
    assert [queue_ptr(s, rows, K) for s in range(7)] == [0, 8, 16, 0, 8, 16, 0]
    assert all(model_lib.moco_queue_ptr(s, rows, K) == queue_ptr(s, rows, K) for s in range(50))
    assert queue_ptr(10 ** 9 + 1, 1024, 65536) == ((10 ** 9 + 1) * 1024) % 65536
    qobj = model_lib.MocoQueue(K, 4, seed=3, device='cpu')
    want = queue_init(K, 4, 3)
    for step in range(4):                                         # step 3 wraps to row 0
        keys = torch.full((rows, 4), float(step + 1))
        assert qobj.enqueue(keys, step) == queue_ptr(step, rows, K)
        want[queue_ptr(step, rows, K):queue_ptr(step, rows, K) + rows] = step + 1
        assert qobj.value.numpy().tobytes() == want.tobytes()
    with pytest.raises(ValueError, match='not a multiple'):
        qobj.enqueue(torch.zeros(5, 4), 0)
    with pytest.raises(ValueError, match='float32 keys'):
        qobj.enqueue(torch.zeros(8, 3), 0)


# ---------------------------------------------------------------------------------------------------------------- flags, names
def test_flags_parse_and_defaults():
    from simclr_amd import run
    from simclr_amd.flags import FLAGS
    try:
        FLAGS.reset()
        assert (FLAGS.moco_queue_size, FLAGS.moco_momentum, FLAGS.moco_queue_seed) == (65536, 0.999, 0)
        assert not run.moco_loss_on()
        FLAGS.parse(['--contrastive_loss=mocov2', '--moco_queue_size=4096', '--moco_momentum=0.99', '--moco_queue_seed=5',
                     '--proj_out_dim=256', '--train_batch_size=512', '--temperature=0.2'])
        assert (FLAGS.contrastive_loss, FLAGS.moco_queue_size, FLAGS.moco_momentum, FLAGS.moco_queue_seed) == ('mocov2', 4096, 0.99, 5)
        assert run.check_contrastive_loss_flags() is False and run.moco_loss_on()
        assert not (run.generalized_loss_on() or run.supcon_loss_on() or run.barlow_loss_on() or run.byol_loss_on())
        FLAGS.update(hidden_norm=False)                                  # ignored with this loss
        assert run.check_contrastive_loss_flags() is False
        FLAGS.reset()
        FLAGS.update(contrastive_loss='mocov2')                          # the defaults: 65536 = 64 x (2 x 512), width 128
        assert run.check_contrastive_loss_flags() is False
        for m in (0.0, 1.0):
            FLAGS.update(moco_momentum=m)
            assert run.check_contrastive_loss_flags() is False
        FLAGS.update(moco_queue_size=1024)                               # exactly one step's rows
        assert run.check_contrastive_loss_flags() is False
        FLAGS.update(moco_queue_size=1048576)
        assert run.check_contrastive_loss_flags() is False
    finally:
        FLAGS.reset()


def test_value_errors_before_any_device_work():
    from simclr_amd import ops, run
    from simclr_amd.flags import FLAGS
    base = ['--dataset=synthetic', '--contrastive_loss=mocov2', '--train_steps=1', '--proj_out_dim=64', '--train_batch_size=16']
    try:
        for extra, msg in ((['--moco_queue_size=16'], 'moco_queue_size must be a multiple'),          # below 2N = 32
                           (['--moco_queue_size=48'], 'moco_queue_size must be a multiple'),          # no multiple of 32
                           (['--moco_queue_size=0'], 'moco_queue_size must be a multiple'),
                           (['--moco_queue_size=-32'], 'moco_queue_size must be a multiple'),
                           (['--moco_queue_size=1048608'], 'moco_queue_size must be a multiple'),     # a multiple, above 1048576
                           (['--moco_queue_size=64', '--moco_momentum=-0.01'], 'moco_momentum must lie in'),
                           (['--moco_queue_size=64', '--moco_momentum=1.5'], 'moco_momentum must lie in'),
                           (['--moco_queue_size=64', '--moco_momentum=nan'], 'moco_momentum must lie in'),
                           (['--moco_queue_size=64', '--temperature=0'], 'mocov2 needs --temperature > 0'),
                           (['--moco_queue_size=64', '--proj_out_dim=100'], 'mocov2 needs a projection head of width 64/128/256'),
                           (['--moco_queue_size=64', '--proj_out_dim=512'], 'mocov2 needs a projection head of width 64/128/256'),
                           (['--moco_queue_size=64', '--proj_head_mode=none'], 'mocov2 needs a projection head of width 64/128/256')):
            FLAGS.reset()
            with pytest.raises(ValueError, match=msg):
                run.main(base + extra)
        # 'moco' is still no loss; the message names the new value last
        FLAGS.reset()
        with pytest.raises(ValueError, match="'barlow' or 'byol' or 'mocov2' \\(got 'moco'\\)"):
            run.main(['--dataset=synthetic', '--contrastive_loss=moco', '--train_steps=1'])
        # fine-tuning and evaluation ignore the loss flags
        FLAGS.reset()
        FLAGS.update(contrastive_loss='mocov2', train_mode='finetune', proj_out_dim=100, moco_queue_size=3, moco_momentum=2.0)
        assert run.check_contrastive_loss_flags() is False and not run.moco_loss_on()
        FLAGS.reset()
        FLAGS.update(contrastive_loss='mocov2', mode='eval', proj_out_dim=100, moco_queue_size=3, moco_momentum=2.0)
        assert run.check_contrastive_loss_flags() is False
        # the bindings refuse before they touch the library
        z = torch.zeros(8, 64)
        with pytest.raises(ValueError, match='widths 64/128/256'):
            ops.moco_fwd(torch.zeros(8, 100), torch.zeros(8, 100), torch.zeros(4, 100), 1.0)
        with pytest.raises(ValueError, match='one shape'):
            ops.moco_fwd(z, torch.zeros(8, 128), torch.zeros(4, 64), 1.0)
        with pytest.raises(ValueError, match='b >= 1'):
            ops.moco_fwd(torch.zeros(7, 64), torch.zeros(7, 64), torch.zeros(4, 64), 1.0)
        with pytest.raises(ValueError, match='b >= 1'):
            ops.moco_fwd(torch.zeros(0, 64), torch.zeros(0, 64), torch.zeros(4, 64), 1.0)
        with pytest.raises(ValueError, match='K >= 1'):
            ops.moco_fwd(z, z, torch.zeros(0, 64), 1.0)
        with pytest.raises(ValueError, match='K >= 1'):
            ops.moco_fwd(z, z, torch.zeros(4, 128), 1.0)
        for T in (0.0, -1.0, float('nan')):
            with pytest.raises(ValueError, match='temperature must be > 0'):
                ops.moco_fwd(z, z, torch.zeros(4, 64), T)
    finally:
        FLAGS.reset()


def test_make_single_step_messages():
    from simclr_amd import run
    from simclr_amd.flags import FLAGS

    class NoQueue:
        queue = None
    try:
        FLAGS.reset()
        FLAGS.update(contrastive_loss='mocov2', proj_out_dim=64)
        with pytest.raises(ValueError, match='needs a target network'):
            run.make_single_step(object(), object(), None)
        with pytest.raises(ValueError, match='mocov2 needs a target network with a key queue'):
            run.make_single_step(object(), object(), None, target=NoQueue())
        FLAGS.reset()
        FLAGS.update(contrastive_loss='byol', proj_out_dim=64)
        with pytest.raises(ValueError, match='--contrastive_loss=byol needs a target network'):
            run.make_single_step(object(), object(), None)
        for loss in ('ntxent', 'supcon'):
            FLAGS.reset()
            FLAGS.update(contrastive_loss=loss)
            with pytest.raises(ValueError, match='belongs to the BYOL'):
                run.make_single_step(object(), object(), None, target=object())
    finally:
        FLAGS.reset()


def test_metric_names_of_the_moco_loss():
    from simclr_amd import run
    from simclr_amd.flags import FLAGS
    try:
        FLAGS.reset()
        FLAGS.update(contrastive_loss='mocov2')
        assert sorted(run.build_metrics()) == ['train/contrast_acc', 'train/contrast_loss', 'train/supervised_acc', 'train/supervised_loss',
                                               'train/total_loss', 'train/weight_decay']
        FLAGS.update(lineareval_while_pretraining=False)
        assert sorted(run.build_metrics()) == ['train/contrast_acc', 'train/contrast_loss', 'train/total_loss', 'train/weight_decay']
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


def test_the_online_model_is_the_ntxent_model():
    """mocov2 adds nothing to the online model: no predictor, the names and initial values of an ntxent build."""
    from simclr_amd.flags import FLAGS
    from simclr_amd.resnet import RT
    try:
        plain = _built_model(contrastive_loss='ntxent', proj_out_dim=64)
        plain_vars = [(v.name, v.value.clone()) for v in plain.variables]
        moco = _built_model(contrastive_loss='mocov2', proj_out_dim=64)
        assert moco.prediction_head is None
        assert [v.name for v in moco.variables] == [n for n, _ in plain_vars]
        assert all(torch.equal(v.value, w) for v, (_, w) in zip(moco.variables, plain_vars))
        assert [v.name for v in moco.trainable_variables] == [v.name for v in plain.trainable_variables]
        assert not any('moco' in v.name or 'target' in v.name for v in moco.variables)
    finally:
        FLAGS.reset()
        RT.reset()
