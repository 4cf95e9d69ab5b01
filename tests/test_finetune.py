"""train_mode=finetune without a GPU: which variables train for every fine_tune_after_block (tf2/resnet.py:548-691), the variable
set against pretraining, the pretraining guard, and the gradient buckets of GradSync."""
import pytest
import torch

from simclr_amd import model as model_lib
from simclr_amd.flags import FLAGS
from simclr_amd.resnet import RT
from simclr_amd.run import GradSync

KS = [-1, 0, 1, 2, 3, 4, -2, 5]


@pytest.fixture(autouse=True)
def _flags():
    FLAGS.reset()
    RT.reset()
    yield
    FLAGS.reset()
    RT.reset()


def _build(**flags):
    FLAGS.reset()
    FLAGS.update(use_blur=False, **flags)
    RT.reset()
    RT.device = torch.device('cpu')
    m = model_lib.Model(1000)
    m.build_variables()
    return m


def _frozen(name, k):
    """Is the variable `name` frozen at fine_tune_after_block=k (the reference's table)?"""
    if k == -1 or not name.startswith('model/resnet/'):
        return False
    if not 0 <= k <= 3:
        return True                                   # 4, and any other value by the construction at :548-681
    for g in range(1, 5):
        if '/block_group%d/' % g in name:
            return g <= k
    return True                                       # the stem


@pytest.mark.parametrize('k', KS)
def test_trainable_variables_follow_the_freezing_table(k):
    pre = _build(train_mode='pretrain', lineareval_while_pretraining=True)
    ft = _build(train_mode='finetune', fine_tune_after_block=k)
    names = [v.name for v in ft.variables]
    assert names == [v.name for v in pre.variables] and len(names) == len(pre.variables) > 250
    want = [v.name for v in pre.trainable_variables if not _frozen(v.name, k)]
    assert [v.name for v in ft.trainable_variables] == want
    got = {v.name for v in ft.trainable_variables}
    assert any('head_supervised' in n for n in got) and any('projection_head' in n for n in got)
    assert all('moving_' not in n for n in got)
    if k == -1:
        assert len(got) == len(pre.trainable_variables)
    # layer-level freezing: the frozen layers report trainable=False
    rm = ft.resnet_model
    assert rm.stem_conv.trainable == (k == -1)
    for g, bg in enumerate(rm.block_groups, start=1):
        assert bg.trainable == (k == -1 or (0 <= k <= 3 and g > k))
        assert all(b.conv1.trainable == bg.trainable for b in bg.layers)


def test_pretraining_forward_with_layer_freezing_still_raises():
    m = _build(train_mode='pretrain', fine_tune_after_block=2)
    with pytest.raises(ValueError):
        m(torch.zeros(2, 32, 32, 6), training=True)


def test_variables_without_gradient_are_the_projection_layers_above_the_selector():
    for sel, want in [(0, 3), (1, 2), (2, 1), (3, 0)]:
        m = _build(train_mode='finetune', fine_tune_after_block=4, ft_proj_selector=sel)
        layers = {v.name.split('/')[2] for v in m.variables_without_gradient()}
        assert len(layers) == want, (sel, layers)
        assert all(v.name.startswith('model/projection_head/') for v in m.variables_without_gradient())
    m = _build(train_mode='pretrain')
    assert m.variables_without_gradient() == []


@pytest.mark.parametrize('k', KS)
def test_gradient_buckets_cover_exactly_the_trainable_gradients(k):
    m = _build(train_mode='finetune', fine_tune_after_block=k)
    flat = m.allocate_flat_grads()
    sync = GradSync(m, None)
    # contiguous, non-empty, covering the whole flat buffer -- and the flat buffer holds the trainable gradients only
    assert sync.ranges[0][0] == 0 and sync.ranges[-1][1] == flat.numel()
    assert all(a < b for a, b in sync.ranges) and all(b == a2 for (_, b), (a2, _) in zip(sync.ranges[:-1], sync.ranges[1:]))
    assert [id(v) for v in m._flat_order] == [id(v) for v in reversed(m.trainable_variables)]
    assert all(v.grad is None for v in m.variables if v not in m._flat_order)
    used = sum((v.numel() + 63) // 64 * 64 for v in m._flat_order)
    assert used == flat.numel()
    trainable_groups = [g for g in (4, 3, 2, 1) if any('block_group%d/' % g in v.name for v in m._flat_order)]
    assert sorted(sync.stage_to_bucket) == sorted(trainable_groups)
    nstem = 1 if k == -1 else 0
    assert len(sync.ranges) == len(trainable_groups) + nstem + (1 if not trainable_groups else 0)
    # every trainable block group's gradients end in the bucket its stage announces
    base = flat.data_ptr()
    for g in trainable_groups:
        a, b = sync.ranges[sync.stage_to_bucket[g]]
        for v in m._flat_order:
            if 'block_group%d/' % g in v.name:
                off = (v.grad.data_ptr() - base) // 4
                assert a <= off and off + v.numel() <= b


def test_pretraining_buckets_are_unchanged():
    m = _build(train_mode='pretrain')
    flat = m.allocate_flat_grads()
    sync = GradSync(m, None)
    assert len(sync.ranges) == 5 and sync.stage_to_bucket == {4: 0, 3: 1, 2: 2, 1: 3}
    assert sync.ranges[-1][1] == flat.numel()


def test_restore_keeps_a_fresh_supervised_head_of_another_class_count(tmp_path):
    """--checkpoint of a 10-class pretraining run into a 1000-class finetune model: the encoder and projection head restore by name,
    the supervised head of the other shape keeps its initialisation; any other shape difference is still an error."""
    from simclr_amd.checkpoint import Checkpoint, try_restore_from_checkpoint
    FLAGS.reset()
    FLAGS.update(use_blur=False, train_mode='pretrain', lineareval_while_pretraining=True)
    RT.reset()
    RT.device = torch.device('cpu')
    RT.seed = 77                                          # other initial values than the finetune model below
    pre = model_lib.Model(10)
    pre.build_variables()
    path = str(tmp_path / 'pre.pt')
    Checkpoint(model=pre).write(path)
    saved = {v.name: v.value.clone() for v in pre.variables}

    ft = _build(train_mode='finetune', fine_tune_after_block=4)
    head0 = {v.name: v.value.clone() for v in ft.supervised_head.variables}
    _, status = try_restore_from_checkpoint(ft, None, str(tmp_path / 'empty'), path)
    assert status is not None and not status.shape_mismatch
    for v in ft.variables:
        if 'head_supervised' in v.name:
            assert torch.equal(v.value, head0[v.name]), v.name
        else:
            assert torch.equal(v.value, saved[v.name]), v.name

    other = _build(train_mode='finetune', fine_tune_after_block=4, proj_out_dim=64)    # a projection layer of another shape
    with pytest.raises(ValueError):
        try_restore_from_checkpoint(other, None, str(tmp_path / 'empty2'), path)
