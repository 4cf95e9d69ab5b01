"""train_mode=finetune on the device (pytest -m gpu): one step against a float64 autograd oracle composed from
oracle/model_torch.Builder pieces, frozen and no-gradient-path variables, the pretrain -> finetune round trip through run.main,
determinism, and the absence of backward work in the frozen prefix (tf2/model.py:238-280, tf2/run.py:577-622,
tf2/resnet.py:548-691)."""
import glob
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.gpu_checks import DEV, structured_images

pytestmark = pytest.mark.gpu

WD, LR, MOM = 1e-4, 0.1, 0.9


def _setup(depth, size, k, sel, f32_matmul='exact', optimizer='lars', num_classes=10, batch=16):
    from simclr_amd import model as model_lib
    from simclr_amd.flags import FLAGS
    from simclr_amd.resnet import RT
    FLAGS.reset()
    FLAGS.update(resnet_depth=depth, image_size=size, compute_dtype='f32', f32_matmul=f32_matmul, use_blur=False,
                 weight_decay=WD, train_batch_size=batch, train_mode='finetune', fine_tune_after_block=k,
                 ft_proj_selector=sel, optimizer=optimizer, momentum=MOM)
    RT.reset()
    RT.device = torch.device(DEV)
    model = model_lib.Model(num_classes)
    with torch.no_grad():
        model(torch.zeros(2, size, size, 3, device=DEV), training=False)      # builds the variables (inference: nothing moves)
    return model


def _oracle(cfg, params, state, images, labels, trainable, head_wd=True):
    """float64 autograd of the finetune loss: supervised CE on hiddens_list[ft_proj_selector] + LARS weight decay of the head kernel
    (head_wd=False: CE alone).  No stop_gradient is needed: it only cuts gradients of variables that are frozen anyway."""
    from oracle.model_torch import Builder
    p = {n: t.double().clone().requires_grad_(n in trainable) for n, t in params.items()}
    s = {n: t.double().clone() for n, t in state.items()}
    b = Builder(cfg, params=p, state=s, dtype=torch.float64)
    b.training = True
    b.scope.append('model')
    h = b.resnet(images.double())
    _, sup_in = b.projection_head(h)
    b.scope.append('head_supervised')
    logits = b.linear_layer(sup_in, cfg.num_classes)
    b.scope.pop()
    b.scope.pop()
    ce = F.cross_entropy(logits, labels.argmax(1))
    hk = [n for n in p if 'head_supervised' in n and 'kernel' in n][0]
    loss = ce + WD * (p[hk] ** 2).sum() / 2 if head_wd else ce
    names = [n for n in p if n in trainable]
    grads = torch.autograd.grad(loss, [p[n] for n in names], allow_unused=True)
    return dict(loss=float(ce.detach()), logits=logits.detach(), new_state=b.new_state,
                grads={n: (g if g is not None else torch.zeros_like(p[n])) for n, g in zip(names, grads)})


CASES = [
    (18, 32, -1, 0, 'exact'),
    (18, 32, 2, 1, 'exact'),
    (18, 32, 4, 0, 'exact'),
    (18, 32, 0, 1, 'f16x3_3'),
    (50, 48, 2, 0, 'exact'),
    (50, 48, 4, 1, 'f16x3_3'),
]


@pytest.mark.parametrize('depth,size,k,sel,mode', CASES)
def test_finetune_step_matches_float64_oracle(depth, size, k, sel, mode):
    from oracle.lars import lars_apply
    from oracle.model_torch import Config, init_model
    from simclr_amd import model as model_lib
    from simclr_amd.resnet import RT
    from simclr_amd.run import make_single_step
    batch, ncls = 16, 10
    cfg = Config(resnet_depth=depth, image_size=size, num_classes=ncls, weight_decay=WD, ft_proj_selector=sel)
    params, state = init_model(cfg, seed=3)
    g = torch.Generator().manual_seed(7)
    images = structured_images(batch, size, 1, g)
    labels = F.one_hot(torch.randint(0, ncls, (batch,), generator=g), ncls).float()

    model = _setup(depth, size, k, sel, mode)
    allv = dict(params)
    allv.update(state)
    assert sorted(v.name for v in model.variables) == sorted(allv)
    for v in model.variables:
        v.value.copy_(allv[v.name].to(DEV))
    RT.weights_version += 1
    trainable = {v.name for v in model.trainable_variables}
    nograd = {v.name for v in model.variables_without_gradient()}
    before = {v.name: v.value.clone() for v in model.variables}

    opt = model_lib.build_optimizer(LR)
    step = make_single_step(model, opt, None)
    out = step(images.to(DEV), {'labels': labels.to(DEV)})
    torch.cuda.synchronize()
    ref = _oracle(cfg, params, state, images, labels, trainable - nograd)

    tight = mode == 'exact'
    loss = float(out['sup_loss'].value)
    assert abs(loss - ref['loss']) <= 1e-3 * abs(ref['loss']), (loss, ref['loss'])
    # every gradient: 1 - cos over all trainable tensors, and each tensor against the global gradient norm
    gv = {v.name: v.grad.double().cpu() for v in model.trainable_variables if v.name not in nograd}
    flat_g = torch.cat([gv[n].reshape(-1) for n in sorted(gv)])
    flat_r = torch.cat([ref['grads'][n].reshape(-1) for n in sorted(gv)])
    cos = float(flat_g @ flat_r / (flat_g.norm() * flat_r.norm()))
    assert 1 - cos <= (1e-6 if tight else 1e-4), cos
    gnorm = float(flat_r.norm())
    worst = max(float((gv[n] - ref['grads'][n]).abs().max()) for n in gv) / gnorm
    assert worst <= (1e-3 if tight else 3e-3), worst
    # moving statistics of every BatchNorm, frozen ones included
    for v in model.variables:
        if 'moving_' in v.name:
            r = ref['new_state'][v.name]
            err = float((v.value.double().cpu() - r).abs().max()) / max(float(r.abs().max()), 1e-3)
            assert err <= (1e-4 if tight else 1e-3), (v.name, err)
    # frozen: bitwise unchanged, no gradient buffer; no gradient path: unchanged under LARS; trainable: the LARS update
    for v in model.variables:
        if 'moving_' in v.name:
            continue
        if v.name not in trainable:
            assert torch.equal(v.value, before[v.name]) and v.grad is None, v.name
        elif v.name in nograd:
            assert torch.equal(v.value, before[v.name]), v.name
        else:
            want, _ = lars_apply(v.name, params[v.name].double().numpy(), ref['grads'][v.name].numpy(), np.zeros(v.shape), LR,
                                 momentum=MOM, weight_decay=WD,
                                 exclude_from_weight_decay=['batch_normalization', 'bias', 'head_supervised'])
            got = v.value.double().cpu().numpy()
            den = max(float(np.abs(want).max()), 1e-6)
            assert float(np.abs(got - want).max()) / den <= (1e-5 if tight else 1e-4), v.name


def test_momentum_moves_only_the_kernels_without_gradient_path_by_weight_decay():
    from simclr_amd import model as model_lib
    from simclr_amd.run import make_single_step
    model = _setup(18, 32, 4, 1, optimizer='momentum')
    g = torch.Generator().manual_seed(1)
    images = structured_images(16, 32, 1, g).to(DEV)
    labels = F.one_hot(torch.randint(0, 10, (16,), generator=g), 10).float().to(DEV)
    before = {v.name: v.value.clone() for v in model.variables}
    nograd = model.variables_without_gradient()
    assert nograd
    make_single_step(model, model_lib.build_optimizer(LR), None)(images, {'labels': labels})
    torch.cuda.synchronize()
    for v in nograd:
        if 'batch_normalization' in v.name:
            assert torch.equal(v.value, before[v.name]), v.name
        else:
            # Keras SGD(nesterov) from a zero slot with g = wd * w: w - lr * (1 + momentum) * g
            want = before[v.name].double() * (1 - LR * (1 + MOM) * WD)
            assert torch.allclose(v.value.double(), want, rtol=1e-6, atol=1e-9), v.name
            assert not torch.equal(v.value, before[v.name])
    for v in model.resnet_model.variables:
        if 'moving_' not in v.name:
            assert torch.equal(v.value, before[v.name]), v.name


def test_momentum_step_of_the_trainable_variables_matches_the_oracle():
    """optimizer=momentum (Keras SGD, nesterov, tf2/model.py:31-32) with k=2, ft_proj_selector=1: the trainable variables -- group 3 / 4,
    projection layer nl_0, the supervised head -- move by the oracle's CE gradient plus add_weight_decay's L2 term wd * w on every
    non-BatchNorm variable (tf2/model.py:62-69); the LARS-only head term is not added."""
    from oracle.model_torch import Config, init_model
    from simclr_amd import model as model_lib
    from simclr_amd.resnet import RT
    from simclr_amd.run import make_single_step
    cfg = Config(resnet_depth=18, image_size=32, num_classes=10, weight_decay=WD, ft_proj_selector=1)
    params, state = init_model(cfg, seed=4)
    g = torch.Generator().manual_seed(8)
    images = structured_images(16, 32, 1, g)
    labels = F.one_hot(torch.randint(0, 10, (16,), generator=g), 10).float()
    model = _setup(18, 32, 2, 1, optimizer='momentum')
    allv = dict(params)
    allv.update(state)
    for v in model.variables:
        v.value.copy_(allv[v.name].to(DEV))
    RT.weights_version += 1
    trainable = {v.name for v in model.trainable_variables}
    nograd = {v.name for v in model.variables_without_gradient()}
    out = make_single_step(model, model_lib.build_optimizer(LR), None)(images.to(DEV), {'labels': labels.to(DEV)})
    torch.cuda.synchronize()
    ref = _oracle(cfg, params, state, images, labels, trainable - nograd, head_wd=False)
    assert abs(float(out['sup_loss'].value) - ref['loss']) <= 1e-3 * ref['loss']
    checked = 0
    for v in model.trainable_variables:
        if v.name in nograd:
            continue
        w0 = params[v.name].double()
        gr = ref['grads'][v.name] + (0.0 if 'batch_normalization' in v.name else WD * w0)
        want = w0 - LR * (1 + MOM) * gr                      # accum = -lr g from a zero slot; w += m * accum - lr * g
        err = float((v.value.double().cpu() - want).abs().max()) / max(float(want.abs().max()), 1e-6)
        assert err <= 1e-5, (v.name, err)
        checked += 1
    assert checked > 20 and any('head_supervised' in n for n in trainable - nograd)


def test_build_variables_matches_the_lazy_build_of_a_forward_pass():
    """Model.build_variables (no device work) creates the variables a first forward pass creates: names, shapes, initial values."""
    from simclr_amd import model as model_lib
    from simclr_amd.flags import FLAGS
    from simclr_amd.resnet import RT
    for depth, size, k, sel in ((18, 32, 2, 1), (50, 64, -1, 0)):
        built = []
        for lazy in (True, False):
            FLAGS.reset()
            FLAGS.update(resnet_depth=depth, image_size=size, use_blur=False, train_mode='finetune', fine_tune_after_block=k,
                         ft_proj_selector=sel)
            RT.reset()
            RT.device = torch.device(DEV)
            m = model_lib.Model(1000)
            if lazy:
                with torch.no_grad():
                    m(torch.zeros(2, size, size, 3, device=DEV), training=False)
            else:
                m.build_variables()
            built.append({v.name: v.value.clone() for v in m.variables})
        a, b = built
        assert list(a) == list(b)
        assert all(a[n].shape == b[n].shape and torch.equal(a[n], b[n]) for n in a), [n for n in a if not torch.equal(a[n], b[n])][:3]
    FLAGS.reset()
    RT.reset()


def test_two_finetune_steps_on_the_same_inputs_are_bitwise_identical():
    from simclr_amd import model as model_lib
    from simclr_amd.resnet import RT
    from simclr_amd.run import make_single_step
    model = _setup(18, 32, 2, 1, f32_matmul='f16x3_3')
    g = torch.Generator().manual_seed(2)
    images = structured_images(16, 32, 1, g).to(DEV)
    labels = F.one_hot(torch.randint(0, 10, (16,), generator=g), 10).float().to(DEV)
    init = {v.name: v.value.clone() for v in model.variables}
    results = []
    for _ in range(2):
        for v in model.variables:
            v.value.copy_(init[v.name])
        RT.weights_version += 1
        opt = model_lib.build_optimizer(LR)
        out = make_single_step(model, opt, None)(images, {'labels': labels})
        torch.cuda.synchronize()
        results.append((out['sup_loss'].value.clone(), {v.name: v.value.clone() for v in model.variables},
                        {v.name: v.grad.clone() for v in model.trainable_variables}))
        model._flat_grads = None
    (l0, w0, g0), (l1, w1, g1) = results
    # the loss scalar is a float atomicAdd over rows (simclr_bias_softmax_xent): its last bits follow the row order; the
    # gradients and the updated weights do not depend on it and are compared bit for bit
    assert abs(float(l0) - float(l1)) <= 1e-6 * abs(float(l0))
    assert all(torch.equal(w0[n], w1[n]) for n in w0)
    assert all(torch.equal(g0[n], g1[n]) for n in g0)


def _count_backward(monkeypatch):
    """Record every layer-level backward entry of the encoder: (layer name, need_dx)."""
    from simclr_amd import ops, resnet
    calls = []

    def wrap(cls, meth):
        orig = getattr(cls, meth)

        def f(self, *a, **kw):
            name = getattr(self, '_name', None) or getattr(self, '_base', '?')
            calls.append((meth, name, kw.get('need_dx', True)))
            return orig(self, *a, **kw)
        monkeypatch.setattr(cls, meth, f)
    for m in ('backward', 'backward_folded'):
        wrap(resnet.Conv2dFixedPadding, m)
    for m in ('backward', 'backward_fused', 'bwd_reduce'):
        wrap(resnet.BatchNormRelu, m)
    stem_ops = []
    for name in ('stem_conv_wgrad', 'maxpool_bwd', 'bn_bwd_reduce_pool', 'bn_bwd_apply_pool'):
        orig = getattr(ops, name)
        monkeypatch.setattr(ops, name, (lambda o, n: (lambda *a, **kw: (stem_ops.append(n), o(*a, **kw))[1]))(orig, name))
    return calls, stem_ops


@pytest.mark.parametrize('k', [4, 2])
def test_no_backward_work_in_the_frozen_prefix(monkeypatch, k):
    from simclr_amd import model as model_lib
    from simclr_amd.run import make_single_step
    model = _setup(50, 64, k, 0, f32_matmul='f16x3_3')
    calls, stem_ops = _count_backward(monkeypatch)
    g = torch.Generator().manual_seed(4)
    images = structured_images(8, 64, 1, g).to(DEV)
    labels = F.one_hot(torch.randint(0, 10, (8,), generator=g), 10).float().to(DEV)
    make_single_step(model, model_lib.build_optimizer(LR), None)(images, {'labels': labels})
    torch.cuda.synchronize()
    enc = [c for c in calls if c[1].startswith('model/resnet/')]
    assert not stem_ops
    if k == 4:
        assert not enc
        return
    assert enc
    for _, name, _ in enc:
        assert '/block_group3/' in name or '/block_group4/' in name, name
    first = model.resnet_model.block_groups[2].layers[0]
    entry = [c for c in enc if c[1] in (first.conv1._name, first.shortcut.conv._name)]
    assert entry and all(nd is False for _, _, nd in entry), entry
    # the trainable layers had their weight gradients written
    for v in model.resnet_model.trainable_variables:
        assert v.grad is not None and bool(torch.isfinite(v.grad).all()), v.name


def test_pretrain_then_finetune_round_trip_through_main(tmp_path):
    from simclr_amd import run
    from simclr_amd.checkpoint import try_restore_from_checkpoint
    from simclr_amd import model as model_lib
    from simclr_amd.flags import FLAGS
    from simclr_amd.resnet import RT
    common = ['--dataset=synthetic', '--resnet_depth=18', '--image_size=32', '--train_batch_size=16', '--eval_batch_size=16', '--eval_steps=1',
              '--use_blur=False', '--compute_dtype=f32', '--checkpoint_steps=2']
    pre_dir, ft_dir = str(tmp_path / 'pre'), str(tmp_path / 'ft')
    FLAGS.reset()
    run.main(common + ['--train_mode=pretrain', '--train_steps=2', '--model_dir=' + pre_dir, '--mode=train'])
    ckpts = sorted(glob.glob(os.path.join(pre_dir, 'ckpt-*.pt')))
    assert ckpts
    saved = torch.load(ckpts[-1], map_location='cpu')['model']

    # restore by hand the way main does it, then one step: the zeroed head gives uniform logits
    FLAGS.reset()
    FLAGS.parse(common + ['--train_mode=finetune', '--fine_tune_after_block=2', '--zero_init_logits_layer=True'])
    RT.reset()
    RT.device = torch.device(DEV)
    model = model_lib.Model(10)
    with torch.no_grad():
        model(torch.zeros(2, 32, 32, 3, device=DEV), training=False)
    opt = model_lib.build_optimizer(0.1)
    try_restore_from_checkpoint(model, opt, str(tmp_path / 'scratch'), ckpts[-1], 5, True)
    for v in model.resnet_model.variables + model._projection_head.variables:
        assert torch.equal(v.value.cpu(), saved[v.name]), v.name
    assert all(float(v.value.abs().sum()) == 0 for v in model.supervised_head.variables)
    data = run.synthetic_batches(16, 32, 10, RT.device, views=1)
    out = run.make_single_step(model, opt, None)(*next(data))
    assert abs(float(out['sup_loss'].value) - math.log(10)) <= 1e-6

    FLAGS.reset()
    result = run.main(common + ['--train_mode=finetune', '--fine_tune_after_block=2', '--checkpoint=' + ckpts[-1],
                                '--zero_init_logits_layer=True', '--mode=train_then_eval', '--train_steps=2',
                                '--model_dir=' + ft_dir])
    assert result is not None and 'eval/label_top_1_accuracy' in result
    with open(os.path.join(ft_dir, 'result.json')) as f:
        assert 'eval/label_top_1_accuracy' in json.load(f)
    FLAGS.reset()
