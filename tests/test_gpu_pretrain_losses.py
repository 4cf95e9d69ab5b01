"""Every row of simclr_amd/pretrain_losses.py through run.make_single_step on the device (pytest -m gpu): the shape of what the step
returns, the row's (metric name, attribute) pairs against the running means, and the handles of step 1 read again after step 2 -- the
step re-points them at a per-step copy, so they must outlive the arena the next step refills.  A handle test: no reference, no
tolerance, every comparison is bitwise."""
import pytest
import torch

from tests.gpu_checks import DEV, structured_images

pytestmark = pytest.mark.gpu
B, SIZE, NCLS, STEPS, SPE = 8, 32, 4, 10, 1
NAMES = ['ntxent', 'generalized', 'supcon', 'barlow', 'vicreg', 'byol', 'mocov2', 'dino', 'swav']
EXTRA = {'byol': dict(byol_pred_hidden_dim=64), 'mocov2': dict(moco_queue_size=32), 'dino': dict(dino_out_dim=64),
         'swav': dict(swav_num_prototypes=16)}


@pytest.fixture(autouse=True)
def _exact_f32_matmul():
    from simclr_amd import ops
    from simclr_amd.flags import FLAGS
    from simclr_amd.resnet import RT
    ops.set_f32_matmul('exact')
    yield
    FLAGS.reset()
    RT.reset()
    ops.set_f32_matmul('exact')


def _batch(seed):
    g = torch.Generator().manual_seed(seed)
    images = structured_images(B, SIZE, 2, g)
    ids = torch.randint(0, NCLS, (B,), generator=g)
    return images.to(DEV), {'labels': torch.nn.functional.one_hot(ids, NCLS).float().to(DEV)}


def _build(name):
    """The step of loss `name`, its target built the way the suite of that loss builds it."""
    from simclr_amd import model as model_lib
    from simclr_amd.flags import FLAGS
    from simclr_amd.resnet import RT
    from simclr_amd.run import make_single_step
    FLAGS.reset()
    FLAGS.update(resnet_depth=18, image_size=SIZE, compute_dtype='f32', f32_matmul='exact', train_mode='pretrain', train_steps=STEPS,
                 train_batch_size=B, proj_out_dim=64, use_blur=False, contrastive_loss=name, **EXTRA.get(name, {}))
    RT.reset()
    RT.device = torch.device(DEV)
    model = model_lib.Model(NCLS)
    target = None
    if name == 'byol':
        target = model_lib.TargetNetwork(model, STEPS)
    elif name == 'mocov2':
        queue = model_lib.MocoQueue(FLAGS.moco_queue_size, FLAGS.proj_out_dim, FLAGS.moco_queue_seed)
        target = model_lib.TargetNetwork(model, STEPS, queue=queue)
    elif name == 'dino':
        target = model_lib.TargetNetwork(model, STEPS, center=model_lib.DinoCenter(FLAGS.dino_out_dim), steps_per_epoch=SPE)
    return make_single_step(model, model_lib.build_optimizer(0.1), None, target=target, steps_per_epoch=SPE if name == 'swav' else None)


@pytest.mark.parametrize('name', NAMES)
def test_step_logs_the_pairs_of_its_row_and_its_handles_outlive_the_next_step(name):
    from simclr_amd.pretrain_losses import LOSSES
    spec = LOSSES[name]
    step = _build(name)
    out = step(*_batch(31))
    torch.cuda.synchronize()

    # ---- step 1: the public shape of the step, and every pair of the row against the running mean of its name
    assert sorted(out) == ['con_loss', 'logits_con', 'sup_loss', 'total_loss', 'weight_decay']
    assert (out['logits_con'] is None) == (name != 'ntxent')
    con, sup = out['con_loss'], out['sup_loss']
    pairs = [(n, con, attr) for n, attr in spec.metrics] + [(n, out['logits_con'], attr) for n, attr in spec.logits_metrics]
    assert pairs[0][0] == 'train/contrast_loss' and pairs[0][2] == 'value' and len(pairs) >= 2
    assert sorted(step.metrics) == sorted([n for n, _, _ in pairs] + ['train/supervised_acc', 'train/supervised_loss',
                                                                      'train/total_loss', 'train/weight_decay'])
    handles = {n: getattr(owner, attr) for n, owner, attr in pairs}
    handles.update({'train/supervised_loss': sup.value, 'train/supervised_acc': sup.acc, 'train/total_loss': out['total_loss']})
    if torch.is_tensor(out['weight_decay']):
        handles['train/weight_decay'] = out['weight_decay']
    for n, h in handles.items():
        assert step.metrics[n].result() == float(h), n
    first = {n: h.detach().clone() for n, h in handles.items()}

    # ---- step 2, another batch: the arena is refilled, the handles of step 1 still read the values of step 1
    out2 = step(*_batch(32))
    torch.cuda.synchronize()
    assert out2['con_loss'] is not con
    for n, h in handles.items():
        assert torch.equal(h, first[n]), n
    for n, owner, attr in pairs:                                      # read through the owner again: the attribute itself was re-pointed
        assert torch.equal(getattr(owner, attr), first[n]), n
