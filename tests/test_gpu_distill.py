"""The distillation (self-training) stage on the device (pytest -m gpu): simclr_kd_softmax_xent through the C ABI against the float64
reference tests/kd_reference.py, then the step -- make_single_step(..., teacher=...) against the plain fine-tuning step, a real frozen
teacher (model.Teacher), strict restore, run.main end to end and two replicas over gloo
(tf2/colabs/distillation_self_training.ipynb:803-808, 908-919)."""
import glob
import hashlib
import json
import math
import os
import shutil
import socket

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.gpu_checks import DEV, _dn, _res, _tol, structured_images
from tests.kd_reference import kd_reference

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
SENT = 7.5
WD, LR, MOM = 1e-4, 0.1, 0.9


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


def _assert(results):
    for r in results:
        print('%-4s %-86s err=%.3e tol=%.3e' % ('ok' if r['ok'] else 'FAIL', r['name'], r['err'], r['tol']))
    bad = [r for r in results if not r['ok']]
    assert not bad, '\n'.join('%s err=%.3e tol=%.3e' % (r['name'], r['err'], r['tol']) for r in bad)


# ---------------------------------------------------------------------------------------------------------------- kernel level
def _call(zs, bs, zt, bt, nclass, T, gscale, out, dl=None):
    """simclr_kd_softmax_xent through the C ABI.  dlogits is followed by 64 sentinel elements; returns (dlogits view, tail view)."""
    from simclr_amd import ops
    from simclr_amd._lib import lib
    rows, cpad_s = zs.shape
    buf = torch.full((rows * cpad_s + 64,), SENT, device=DEV, dtype=zs.dtype) if dl is None else dl
    lib().kd_softmax_xent(ops._p(zs), ops._p(bs), ops._p(zt), ops._p(bt), rows, nclass, cpad_s, zt.shape[1], float(T), float(gscale),
                          ops._p(buf), ops._p(out), ops.dt(zs), ops.dt(zt), ops._s())
    return buf[:rows * cpad_s].view(rows, cpad_s), buf[rows * cpad_s:]


def _inputs(rows, nclass, cpad_s, cpad_t, dts, dtt, mode, g):
    """(zs, bias_s, zt, bias_t) on the host.  Logits of sigma 3; the pad columns of both inputs hold NaN: whoever reads them shows it.
    mode: 'normal' | 'identical' (teacher rows = student rows) | 'zero' | 'large' (magnitude 80) | 'tie_cross' (maxima in columns
    6 and 71: two lanes) | 'tie_same' (6 and 70: one lane) | 'nobias'."""
    zs = torch.randn(rows, cpad_s, generator=g) * 3
    zt = torch.randn(rows, cpad_t, generator=g) * 3
    bs = 0.1 * torch.randn(nclass, generator=g)
    bt = 0.1 * torch.randn(nclass, generator=g)
    if mode == 'identical':
        zs = zs.bfloat16().float()                       # the same values in either storage type
        zt = torch.zeros(rows, cpad_t)
        zt[:, :nclass] = zs[:, :nclass]
        bt = bs.clone()
    elif mode == 'zero':
        zs[:], zt[:], bs[:], bt[:] = 0, 0, 0, 0
    elif mode == 'large':
        zs = torch.where(torch.rand(rows, cpad_s, generator=g) < 0.5, -80.0, 80.0) + torch.randn(rows, cpad_s, generator=g)
        zt = torch.where(torch.rand(rows, cpad_t, generator=g) < 0.5, -80.0, 80.0) + torch.randn(rows, cpad_t, generator=g)
    elif mode in ('tie_cross', 'tie_same'):
        lo, hi = (6, 71) if mode == 'tie_cross' else (6, 70)
        assert nclass > hi
        zs, zt = zs.clamp(-8, 8), zt.clamp(-8, 8)
        bs[lo] = bs[hi] = bt[lo] = bt[hi] = 0.25         # 11.75 + 0.25 = 12 exactly in bf16 and fp32: true ties, above everything else
        idx = torch.arange(rows) % 4
        # student: tie in rows 0, 1 (mod 4), the higher column alone in row 2, the lower alone in row 3; teacher: tie in the even rows,
        # the lower column alone in the odd rows.  "The lower column wins" makes the rows 0, 1, 3 (mod 4) agree and row 2 disagree.
        zs[:, lo] = torch.where(idx == 2, 3.0, 11.75)
        zs[:, hi] = torch.where(idx == 3, 3.0, 11.75)
        zt[:, lo] = 11.75
        zt[:, hi] = torch.where(idx % 2 == 1, 3.0, 11.75)
    elif mode == 'nobias':
        bs = bt = None
    else:
        assert mode == 'normal', mode
    zs[:, nclass:] = float('nan')
    zt[:, nclass:] = float('nan')
    return zs.to(dts), bs, zt.to(dtt), bt


def check_kd(rows, nclass, cpad_s, cpad_t, dts, dtt, T, gscale=1.0, mode='normal', seed=0):
    g = torch.Generator().manual_seed(seed)
    zs, bs, zt, bt = _inputs(rows, nclass, cpad_s, cpad_t, dts, dtt, mode, g)
    s = zs.double()[:, :nclass] + (bs.double() if bs is not None else 0)
    t = zt.double()[:, :nclass] + (bt.double() if bt is not None else 0)
    ref = kd_reference(s.numpy(), t.numpy(), T, gscale)
    init = torch.tensor([0.5, 0.25, SENT, SENT])
    out = init.clone().to(DEV)
    dev = [x.to(DEV) if x is not None else None for x in (zs, bs, zt, bt)]
    dl, tail = _call(*dev, nclass, T, gscale, out[:2])
    dl2, tail2 = _call(*dev, nclass, T, gscale, out[:2])          # the second call adds onto the un-zeroed out
    torch.cuda.synchronize()
    tag = '%dx%d(%d,%d) %s/%s T%g g%g %s' % (rows, nclass, cpad_s, cpad_t, _dn(dts), _dn(dtt), T, gscale, mode)
    o = out.double().cpu()
    # as for simclr_bias_softmax_xent (gpu_checks.check_xent): out[1] is 2 * rows float atomic adds of 0 or 1 / rows onto the initial
    # value, each rounding to 2^-24 of a running value below init + 2
    acc_bound = 2 * rows * 2.0 ** -24 * (float(init[1]) + 2.0)
    res = [_res('kd_loss_two_calls ' + tag, o[0], float(init[0]) + 2 * ref['loss'], _tol(F32)),
           _res('kd_agreement_two_calls ' + tag, o[1], float(init[1]) + 2 * ref['agreement'], 0, acc_bound),
           _res('kd_dlogits ' + tag, dl[:, :nclass], ref['dlogits'], _tol(dts), 1e-7),
           _res('kd_dlogits_pad ' + tag, dl[:, nclass:], torch.zeros(rows, cpad_s - nclass), 0, 0),
           _res('kd_dlogits_repeat ' + tag, dl2, dl, 0, 0),
           _res('kd_sentinels ' + tag, torch.cat([tail.float(), tail2.float(), out[2:]]), torch.full((130,), SENT), 0, 0)]
    if mode == 'identical':
        p = ref['p']
        ent = -(p * np.log(np.maximum(p, 1e-300))).sum(1).mean()
        res += [_res('kd_identical_zero_gradient ' + tag, dl[:, :nclass], torch.zeros(rows, nclass), 0, 1e-7),
                _res('kd_identical_entropy ' + tag, o[0], float(init[0]) + 2 * T * T * ent, _tol(F32))]
    if mode == 'zero':
        res += [_res('kd_zero_loss ' + tag, o[0], float(init[0]) + 2 * T * T * math.log(nclass), _tol(F32)),
                _res('kd_zero_agreement ' + tag, o[1], float(init[1]) + 2.0, 0, acc_bound)]
    if mode in ('tie_cross', 'tie_same'):
        want = float((torch.arange(rows) % 4 != 2).double().mean())
        assert ref['agreement'] == want, (ref['agreement'], want)
    return res


SHAPES = [(10, 16, 64), (10, 64, 16), (1000, 1008, 1024), (1000, 1024, 1008), (64, 64, 64), (65, 128, 80)]
DTYPES = [(F32, F32), (F32, BF), (BF, F32), (BF, BF)]


@pytest.mark.parametrize('dts,dtt', DTYPES)
@pytest.mark.parametrize('nclass,cpad_s,cpad_t', SHAPES)
def test_kd_kernel_vs_float64(nclass, cpad_s, cpad_t, dts, dtt):
    """Fewer classes than lanes, exactly one pass, one class into the second pass, many passes, unequal pitches; a lone row, a partly
    filled last workgroup (four rows each), many workgroups; three temperatures; gscale 1 and 0.5."""
    res = []
    for rows in (1, 5, 63, 126):
        for T in (0.1, 1.0, 4.0):
            for gscale in (1.0, 0.5):
                res += check_kd(rows, nclass, cpad_s, cpad_t, dts, dtt, T, gscale, seed=rows)
    _assert(res)


@pytest.mark.parametrize('dts,dtt', DTYPES)
@pytest.mark.parametrize('mode', ['identical', 'zero', 'large', 'nobias'])
def test_kd_kernel_special_inputs(mode, dts, dtt):
    res = []
    for nclass, cpad_s, cpad_t in ((10, 16, 64), (1000, 1008, 1024), (65, 128, 80)):
        for T in (0.1, 1.0, 4.0):
            res += check_kd(63, nclass, cpad_s, cpad_t, dts, dtt, T, mode=mode, seed=3)
    _assert(res)


@pytest.mark.parametrize('dts,dtt', DTYPES)
@pytest.mark.parametrize('mode', ['tie_cross', 'tie_same'])
def test_kd_kernel_ties_the_lower_column_wins(mode, dts, dtt):
    res = []
    for nclass, cpad_s, cpad_t in ((1000, 1008, 1024), (80, 128, 80)):
        res += check_kd(63, nclass, cpad_s, cpad_t, dts, dtt, 1.0, mode=mode, seed=4)
        res += check_kd(10, nclass, cpad_s, cpad_t, dts, dtt, 4.0, gscale=0.5, mode=mode, seed=5)
    _assert(res)


@pytest.mark.parametrize('nclass', [2048, 1500])
def test_kd_kernel_more_classes_than_the_register_path_holds(nclass):
    """Above 1024 classes the kernel reads its inputs again in every pass instead of keeping the row in registers."""
    _assert(check_kd(5, nclass, nclass + 16, nclass, F32, BF, 1.0) + check_kd(9, nclass, nclass, nclass + 48, BF, F32, 0.1, gscale=0.5))


@pytest.mark.parametrize('dtype', [F32, BF])
@pytest.mark.parametrize('nclass,cpad', [(10, 16), (1000, 1008)])
def test_kd_kernel_with_a_one_hot_teacher_equals_the_supervised_kernel(nclass, cpad, dtype):
    """Teacher logits 60 at the label column and 0 elsewhere, T = 1: p is one-hot in fp32 (in float64 the loss differs from the plain
    cross entropy by 0, the gradient by 3e-26), so loss and dlogits must equal what simclr_bias_softmax_xent returns for those labels,
    within that kernel's own tolerances (gpu_checks.check_xent)."""
    from simclr_amd import ops
    rows = 63
    g = torch.Generator().manual_seed(11)
    z = (torch.randn(rows, cpad, generator=g) * 3).to(dtype).to(DEV)
    bias = (0.1 * torch.randn(nclass, generator=g)).to(DEV)
    labels = torch.randint(0, nclass, (rows,), generator=g).int()
    zt = (60.0 * F.one_hot(labels.long(), nclass).float()).to(DEV)
    for gscale in (1.0, 0.5):
        o_sup = torch.zeros(2, device=DEV)
        o_kd = torch.zeros(2, device=DEV)
        d_sup = ops.bias_softmax_xent(z, bias, labels.to(DEV), nclass, gscale, o_sup)
        d_kd = ops.kd_softmax_xent(z, bias, zt, None, nclass, 1.0, gscale, o_kd)
        torch.cuda.synchronize()
        tag = '%dx%d %s g%g' % (rows, nclass, _dn(dtype), gscale)
        _assert([_res('kd_onehot_loss ' + tag, o_kd[0], o_sup[0], _tol(F32)),
                 _res('kd_onehot_agreement_is_accuracy ' + tag, o_kd[1], o_sup[1], 0, 2 * rows * 2.0 ** -24),
                 _res('kd_onehot_dlogits ' + tag, d_kd[:, :nclass], d_sup[:, :nclass], _tol(dtype), 1e-7),
                 _res('kd_onehot_dlogits_pad ' + tag, d_kd[:, nclass:], torch.zeros(rows, cpad - nclass), 0, 0)])


def test_kd_kernel_refuses_bad_arguments():
    from simclr_amd import ops
    from simclr_amd._lib import SimclrHipError, lib
    z = torch.zeros(4, 16, device=DEV)
    out = torch.zeros(2, device=DEV)
    with pytest.raises(SimclrHipError, match='temperature'):
        _call(z, None, z, None, 10, 0.0, 1.0, out)
    with pytest.raises(SimclrHipError, match='temperature'):
        _call(z, None, z, None, 10, -1.0, 1.0, out)
    with pytest.raises(SimclrHipError, match='row pitch below nclass'):
        _call(z, None, z, None, 17, 1.0, 1.0, out)
    with pytest.raises(SimclrHipError, match='row pitch below nclass'):
        _call(torch.zeros(4, 32, device=DEV), None, z, None, 17, 1.0, 1.0, out)
    with pytest.raises(SimclrHipError, match='null argument'):
        lib().kd_softmax_xent(ops._p(z), None, ops._p(z), None, 4, 10, 16, 16, 1.0, 1.0, None, ops._p(out), 0, 0, ops._s())
    with pytest.raises(SimclrHipError, match='bad shape'):
        lib().kd_softmax_xent(ops._p(z), None, ops._p(z), None, 0, 10, 16, 16, 1.0, 1.0, ops._p(z.clone()), ops._p(out), 0, 0, ops._s())
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0


def test_add_kd_loss_handle_and_class_count_check():
    from simclr_amd import objective as obj_lib
    from simclr_amd.model import SupLogits
    g = torch.Generator().manual_seed(2)
    zs = (torch.randn(8, 64, generator=g) * 3).to(DEV)
    zt = (torch.randn(8, 16, generator=g) * 3).to(DEV)
    bs = (0.1 * torch.randn(10, generator=g)).to(DEV)
    bt = (0.1 * torch.randn(10, generator=g)).to(DEV)
    loss = obj_lib.add_kd_loss(SupLogits(zs, bs, 10), SupLogits(zt, bt, 10), 2.0)
    ref = kd_reference((zs[:, :10] + bs).double().cpu().numpy(), (zt[:, :10] + bt).double().cpu().numpy(), 2.0)
    dl = loss.backward()
    assert dl.shape == zs.shape and dl.dtype == zs.dtype
    _assert([_res('add_kd_loss value', loss.value, ref['loss'], _tol(F32)),
             _res('add_kd_loss acc', loss.acc, ref['agreement'], 0, 1e-6),
             _res('add_kd_loss dlogits', dl[:, :10], ref['dlogits'], _tol(F32), 1e-7)])
    with pytest.raises(ValueError, match='10 classes.*7'):
        obj_lib.add_kd_loss(SupLogits(zs, bs, 10), SupLogits(zt, None, 7), 1.0)


# ---------------------------------------------------------------------------------------------------------------- step level
B, NCLS, SIZE = 8, 10, 32


def _flags(depth=18, k=-1, sel=0, optimizer='lars', sk=0.0, f32_matmul='exact', **kw):
    from simclr_amd.flags import FLAGS
    FLAGS.reset()
    FLAGS.update(resnet_depth=depth, image_size=SIZE, compute_dtype='f32', f32_matmul=f32_matmul, use_blur=False, weight_decay=WD,
                 train_batch_size=B, train_mode='finetune', fine_tune_after_block=k, ft_proj_selector=sel, optimizer=optimizer,
                 momentum=MOM, sk_ratio=sk, **kw)
    return FLAGS


def _fresh_runtime():
    from simclr_amd.resnet import RT
    RT.reset()
    RT.device = torch.device(DEV)
    return RT


def _build_model():
    from simclr_amd import model as model_lib
    model = model_lib.Model(NCLS)
    with torch.no_grad():
        model(torch.zeros(2, SIZE, SIZE, 3, device=DEV), training=False)      # builds the variables (inference: nothing moves)
    return model


def _batches(n, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        images = structured_images(B, SIZE, 1, g).to(DEV)
        labels = F.one_hot(torch.randint(0, NCLS, (B,), generator=g), NCLS).float().to(DEV)
        out.append((images, labels))
    return out


def _rel_l2(a, b):
    return float((a.double() - b.double()).norm()) / max(float(b.double().norm()), 1e-30)


def _run_steps(batches, teacher=None, perturb=False, monkeypatch=None):
    """A fresh student under the current flags, three steps; returns after step 1 and step 3 the flat gradient buffer and every
    variable.  perturb: the fine-tuning step with the loss gradient moved by one fp32 ulp (towards +inf)."""
    from simclr_amd import model as model_lib
    from simclr_amd import objective as obj_lib
    from simclr_amd.run import make_single_step
    _fresh_runtime()
    model = _build_model()
    if perturb:
        orig = obj_lib.add_supervised_loss

        def moved(labels, logits):
            loss = orig(labels=labels, logits=logits)
            d = loss.backward()
            v = d[:, :NCLS]
            v.copy_(torch.nextafter(v, torch.full_like(v, float('inf'))))
            return loss
        monkeypatch.setattr(obj_lib, 'add_supervised_loss', moved)
    step = make_single_step(model, model_lib.build_optimizer(LR), None, teacher=teacher)
    snaps = {}
    for i, (images, labels) in enumerate(batches):
        step.current_labels = labels
        out = step(images, {'labels': labels})
        if i in (0, 2):
            torch.cuda.synchronize()
            snaps[i] = (model._flat_grads.clone(), torch.cat([v.value.reshape(-1) for v in model.variables]).clone(), out)
    if perturb:
        monkeypatch.setattr(obj_lib, 'add_supervised_loss', orig)
    return snaps, step


@pytest.mark.parametrize('optimizer', ['lars', 'momentum'])
@pytest.mark.parametrize('k,sel', [(-1, 0), (-1, 1), (4, 0), (4, 1)])
def test_distillation_step_with_a_one_hot_teacher_equals_the_finetune_step(monkeypatch, optimizer, k, sel):
    """make_single_step(..., teacher=stub), the stub returning 60 * onehot(labels), T = 1: the step is the plain fine-tuning step on the
    same batches and labels.  Bound: five times the relative L2 difference between the fine-tuning step and the fine-tuning step with
    its loss gradient moved by one fp32 ulp, measured here in the same process on the same batches -- what a last-bit difference of
    the loss gradient does to the flattened gradients and the variables after one and after three steps.  (On an MI355X that floor came
    out at 0.8e-7 ... 2.0e-6 for the gradients and 4e-10 ... 8e-8 for the variables over the eight cases, the distillation step at no
    more than 1.24 times it.)"""
    from simclr_amd.model import SupLogits
    _flags(k=k, sel=sel, optimizer=optimizer)
    batches = _batches(3, seed=21)
    plain, _ = _run_steps(batches)
    moved, _ = _run_steps(batches, perturb=True, monkeypatch=monkeypatch)
    box = {}

    def stub(features):
        lab = [l for im, l in batches if im is features][0]
        z = torch.zeros(B, 64, device=DEV)
        z[:, :NCLS] = 60.0 * lab
        box['calls'] = box.get('calls', 0) + 1
        return SupLogits(z, None, NCLS)
    kd, step = _run_steps(batches, teacher=stub)
    assert box['calls'] == 3
    assert sorted(step.metrics) == ['train/distill_agreement', 'train/distill_loss', 'train/total_loss', 'train/weight_decay']
    for i in (0, 2):
        for j, what in ((0, 'gradients'), (1, 'variables')):
            floor = _rel_l2(moved[i][j], plain[i][j])
            got = _rel_l2(kd[i][j], plain[i][j])
            print('%s k=%d sel=%d step %d %s: one-ulp floor %.3e, distillation vs fine-tuning %.3e' % (optimizer, k, sel, i + 1, what, floor, got))
            assert floor > 0
            assert got <= 5 * floor, (i, what, got, floor)
        a, b = kd[i][2], plain[i][2]
        assert abs(float(a['sup_loss'].value) - float(b['sup_loss'].value)) <= 2e-5 * abs(float(b['sup_loss'].value))
        assert abs(float(a['total_loss']) - float(b['total_loss'])) <= 2e-5 * abs(float(b['total_loss']))
    m = step.metrics
    assert abs(m['train/total_loss'].result() - m['train/distill_loss'].result() - m['train/weight_decay'].result()) \
        <= 1e-5 * abs(m['train/total_loss'].result())


def _teacher_checkpoint(path, depth, sk=0.0, sel=0, steps=2, f32_matmul='exact'):
    """A short fine-tuning run of the teacher's architecture, saved as a checkpoint.  Returns {name: tensor} of the saved model."""
    from simclr_amd import model as model_lib
    from simclr_amd.checkpoint import Checkpoint
    from simclr_amd.run import make_single_step
    _flags(depth=depth, sk=sk, sel=sel, f32_matmul=f32_matmul)
    _fresh_runtime()
    model = _build_model()
    opt = model_lib.build_optimizer(LR)
    step = make_single_step(model, opt, None)
    for images, labels in _batches(steps, seed=31):
        step(images, {'labels': labels})
    torch.cuda.synchronize()
    Checkpoint(model=model, optimizer=opt).write(path)
    return torch.load(path, map_location='cpu')['model']


def _layers(layer):
    out = [layer]
    for l in layer.sublayers():
        out.extend(_layers(l))
    return out


@pytest.mark.parametrize('teacher_sk,mode', [(0.0, 'f16x3_3'), (0.0625, 'exact')])
def test_real_teacher_is_frozen_restored_and_feeds_the_step(tmp_path, monkeypatch, teacher_sk, mode):
    """Teacher ResNet-50 (plain, and with selective kernels), student ResNet-18.  'f16x3_3' is the product's default arithmetic: the
    teacher's inference forward and the student's training step then select different modes within one step."""
    from simclr_amd import model as model_lib
    from simclr_amd import objective as obj_lib
    from simclr_amd import resnet
    from simclr_amd.checkpoint import Checkpoint
    from simclr_amd.run import make_single_step
    ckpt = str(tmp_path / 'teacher.pt')
    saved = _teacher_checkpoint(ckpt, 50, sk=teacher_sk, f32_matmul=mode)
    batches = _batches(3, seed=41)

    # the restored teacher called alone, training=False: the logits the step must be fed with
    RT = _fresh_runtime()
    alone = _build_model()
    Checkpoint(model=alone).restore(ckpt, model_only=True).assert_consumed()
    alone_logits = [alone(im, training=False)[1].z.clone() for im, _ in batches]
    assert sorted(v.name for v in alone.variables) == sorted(saved)
    # the student built alone: names and initial values
    _flags(depth=18, f32_matmul=mode)
    _fresh_runtime()
    student_alone = {v.name: v.value.clone() for v in _build_model().variables}

    FLAGS = _flags(depth=18, f32_matmul=mode, teacher_resnet_depth=50, teacher_sk_ratio=teacher_sk, distill_temperature=2.0)
    RT = _fresh_runtime()
    teacher = model_lib.Teacher(NCLS, ckpt)
    assert FLAGS.resnet_depth == 18 and FLAGS.sk_ratio == 0.0
    model = _build_model()
    now = {v.name: v.value for v in model.variables}
    assert list(now) == list(student_alone) and all(torch.equal(now[n], student_alone[n]) for n in now)
    tvars = teacher.model.variables
    assert sorted(v.name for v in tvars) == sorted(saved) and len(tvars) > len(now)
    assert all(torch.equal(v.value.cpu(), saved[v.name]) for v in tvars)
    assert not teacher.model.trainable_variables

    seen = []
    orig = obj_lib.add_kd_loss

    def recording(student_logits, teacher_logits, temperature):
        loss = orig(student_logits, teacher_logits, temperature)
        seen.append(dict(s=student_logits.dense().double().cpu(), t=teacher_logits.dense().double().cpu(), tz=teacher_logits.z.clone(),
                         T=temperature, dl=loss.backward()))
        return loss
    monkeypatch.setattr(obj_lib, 'add_kd_loss', recording)
    opt = model_lib.build_optimizer(LR)
    step = make_single_step(model, opt, None, teacher=teacher)
    convs = [l for l in _layers(teacher.model) if isinstance(l, resnet.Conv2dFixedPadding) and getattr(l, 'w_t', None) is not None]
    dense = [l for l in _layers(teacher.model) if isinstance(l, model_lib.LinearLayer)]
    assert len(convs) > 40 and dense
    marks = []
    for images, labels in batches:
        step(images, {'labels': labels})
        torch.cuda.synchronize()
        marks.append(([(c._version, c.w_t.data_ptr(), c.w_d.data_ptr()) for c in convs], [(d._version, d.w_t.data_ptr()) for d in dense],
                      RT.weights_version))
    # fed with the restored model's inference logits, bit for bit; the gradient that enters the student's backward is the reference's
    res = []
    for i, rec in enumerate(seen):
        assert rec['T'] == 2.0
        assert torch.equal(rec['tz'], alone_logits[i]), i
        ref = kd_reference(rec['s'].numpy(), rec['t'].numpy(), 2.0)
        res.append(_res('step %d dlogits vs float64' % (i + 1), rec['dl'][:, :NCLS], ref['dlogits'], _tol(F32), 1e-7))
        res.append(_res('step %d dlogits pad' % (i + 1), rec['dl'][:, NCLS:], torch.zeros(B, rec['dl'].shape[1] - NCLS), 0, 0))
    _assert(res)
    # frozen: every teacher variable, moving statistics included, bitwise unchanged; nothing kept for a backward pass
    assert all(torch.equal(v.value.cpu(), saved[v.name]) for v in tvars)
    for l in _layers(teacher.model):
        for a in ('saved', 'out', 'relu_bits', '_prep'):
            assert getattr(l, a, None) is None, (type(l).__name__, a)
    assert not teacher.model.resnet_model.endpoints
    # outside the student's training state
    tids = {id(v) for v in tvars}
    assert not tids & {id(v) for v in model.trainable_variables} and not tids & {id(v) for v in model.variables}
    assert not tids & set(opt._slots)
    state = Checkpoint(model=model, optimizer=opt).state_dict()
    assert sorted(state['model']) == sorted(student_alone) and set(state['optimizer']['slots']) <= set(student_alone)
    assert all(v.grad is None for v in tvars)
    # compute copies: written at the teacher's first forward after the restore, then never again while the optimizer stepped
    assert marks[0][2] < marks[1][2] < marks[2][2]
    assert marks[0][0] == marks[1][0] == marks[2][0] and marks[0][1] == marks[1][1] == marks[2][1]
    # the student moved
    assert any(not torch.equal(v.value, student_alone[v.name]) for v in model.trainable_variables)


def test_teacher_restore_is_strict(tmp_path):
    from simclr_amd import model as model_lib
    ckpt = str(tmp_path / 'teacher.pt')
    _teacher_checkpoint(ckpt, 18, steps=1)
    state = torch.load(ckpt, map_location='cpu')
    head = [n for n in state['model'] if 'head_supervised' in n]
    assert len(head) == 2
    no_head = dict(state, model={n: t for n, t in state['model'].items() if n not in head})
    torch.save(no_head, str(tmp_path / 'no_head.pt'))
    other = dict(state, model={n: (t[..., :7].clone() if n in head else t) for n, t in state['model'].items()})
    torch.save(other, str(tmp_path / 'seven_classes.pt'))
    _flags(depth=18)
    _fresh_runtime()
    with pytest.raises(ValueError, match=r'missing variables \[.*head_supervised'):
        model_lib.Teacher(NCLS, str(tmp_path / 'no_head.pt'))
    _fresh_runtime()
    with pytest.raises(ValueError, match=r'another shape.*head_supervised'):
        model_lib.Teacher(NCLS, str(tmp_path / 'seven_classes.pt'))
    _fresh_runtime()
    # a student-sized file for a teacher of another architecture names the first variables it lacks
    _flags(depth=18, teacher_resnet_depth=50)
    with pytest.raises(ValueError, match='missing variables'):
        model_lib.Teacher(NCLS, ckpt)
    _flags(depth=18)
    _fresh_runtime()
    model_lib.Teacher(NCLS, ckpt)


def test_run_main_distils_resumes_and_writes_finetune_checkpoints(tmp_path):
    from simclr_amd import model as model_lib
    from simclr_amd import run
    from simclr_amd.checkpoint import INDEX_NAME, Checkpoint
    from simclr_amd.flags import FLAGS
    common = ['--dataset=synthetic', '--resnet_depth=18', '--image_size=32', '--train_batch_size=8', '--eval_batch_size=8', '--eval_steps=1',
              '--use_blur=False', '--compute_dtype=f32', '--checkpoint_steps=2', '--train_mode=finetune']
    t_dir, d_dir, r_dir = (str(tmp_path / n) for n in ('teacher', 'distill', 'resumed'))
    FLAGS.reset()
    run.main(common + ['--train_steps=2', '--model_dir=' + t_dir, '--mode=train'])
    t_ckpt = sorted(glob.glob(os.path.join(t_dir, 'ckpt-*.pt')))[-1]

    FLAGS.reset()
    with pytest.raises(ValueError, match='train_mode=finetune'):
        run.main([a for a in common if 'train_mode' not in a] + ['--train_mode=pretrain', '--teacher_checkpoint=' + t_ckpt,
                                                                  '--train_steps=1'])
    distill = common + ['--teacher_checkpoint=' + t_ckpt, '--distill_temperature=2.0', '--train_steps=4', '--mode=train_then_eval']
    FLAGS.reset()
    result = run.main(distill + ['--model_dir=' + d_dir])
    assert result is not None and 'eval/label_top_1_accuracy' in result and result['global_step'] == 4
    with open(os.path.join(d_dir, 'result.json')) as f:
        on_disk = json.load(f)
    assert {'eval/label_top_1_accuracy', 'eval/label_top_5_accuracy', 'eval/regularization_loss'} <= set(on_disk)
    full = torch.load(os.path.join(d_dir, 'ckpt-4.pt'), map_location='cpu')
    assert not any('teacher' in n for n in full['model'])

    # a run stopped after step 2 (its directory holds ckpt-2 alone) and started again
    os.makedirs(r_dir)
    shutil.copy(os.path.join(d_dir, 'ckpt-2.pt'), os.path.join(r_dir, 'ckpt-2.pt'))
    with open(os.path.join(r_dir, INDEX_NAME), 'w') as f:
        json.dump({'model_checkpoint_path': 'ckpt-2.pt', 'all_model_checkpoint_paths': ['ckpt-2.pt']}, f)
    FLAGS.reset()
    run.main(distill + ['--model_dir=' + r_dir])
    again = torch.load(os.path.join(r_dir, 'ckpt-4.pt'), map_location='cpu')
    assert sorted(again['model']) == sorted(full['model'])
    assert all(torch.equal(again['model'][n], full['model'][n]) for n in full['model'])
    assert all(torch.equal(again['optimizer']['slots'][n], full['optimizer']['slots'][n]) for n in full['optimizer']['slots'])
    assert again['optimizer']['iterations'] == full['optimizer']['iterations'] == 4

    # the checkpoint of a distillation run is a fine-tuning checkpoint
    FLAGS.reset()
    FLAGS.parse(common)
    _fresh_runtime()
    model = _build_model()
    opt = model_lib.build_optimizer(0.1)
    Checkpoint(model=model, optimizer=opt).restore(os.path.join(d_dir, 'ckpt-4.pt')).assert_consumed()
    assert int(opt.iterations) == 4


# ---------------------------------------------------------------------------------------------------------------- two replicas
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    try:
        import torch.distributed as dist
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        torch.cuda.set_device(0)
        dist.init_process_group('gloo', rank=rank, world_size=world)
        from simclr_amd import comm
        from simclr_amd import model as model_lib
        from simclr_amd.run import make_single_step
        FLAGS = _flags(depth=18, k=2, sel=1, distill_temperature=2.0)
        FLAGS.update(train_batch_size=world * B)
        RT = _fresh_runtime()
        strategy = comm.Strategy()
        RT.strategy = strategy
        teacher = model_lib.Teacher(NCLS)                      # same seed on every rank: the same (untrained) teacher
        model = _build_model()
        counts = {'inside': 0, 'outside': 0, 'on': False}
        for name in ('all_reduce', 'all_gather', 'all_gather_into_tensor', 'reduce_scatter_tensor', 'broadcast', 'reduce_scatter',
                     'all_to_all_single'):
            orig = getattr(dist, name)
            setattr(dist, name, (lambda o: (lambda *a, **kw: (counts.__setitem__('inside' if counts['on'] else 'outside',
                                                                                  counts['inside' if counts['on'] else 'outside'] + 1),
                                                               o(*a, **kw))[1]))(orig))

        def watched(features):
            counts['on'] = True
            try:
                return teacher(features)
            finally:
                counts['on'] = False
        step = make_single_step(model, model_lib.build_optimizer(LR), strategy, teacher=watched)
        g = torch.Generator().manual_seed(51)
        losses = []
        for _ in range(2):
            images = structured_images(world * B, SIZE, 1, g)
            out = step(images[rank * B:(rank + 1) * B].to(DEV), {'labels': None})          # labels are not read
            losses.append(float(out['sup_loss'].value))
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for v in model.variables:
            h.update(v.value.cpu().numpy().tobytes())
        res = dict(digest=h.hexdigest(), inside=counts['inside'], outside=counts['outside'], losses=losses,
                   finite=all(bool(torch.isfinite(v.value).all()) for v in model.variables))
        dist.destroy_process_group()
        q.put((rank, 'ok', res))
    except Exception:  # noqa
        import traceback
        q.put((rank, 'FAIL', traceback.format_exc()))


def test_two_replica_distillation_step():
    import torch.multiprocessing as mp
    os.environ['SIMCLR_PEER_STATS'] = '0'          # the statistics travel over gloo (the peer-mapped exchange has its own tests)
    try:
        ctx = mp.get_context('spawn')
        q = ctx.Queue()
        port = _free_port()
        procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
        for p in procs:
            p.start()
        res = [q.get(timeout=600) for _ in procs]
        for p in procs:
            p.join(timeout=60)
    finally:
        os.environ.pop('SIMCLR_PEER_STATS', None)
    assert all(r[1] == 'ok' for r in res), res
    a, b = res[0][2], res[1][2]
    assert a['inside'] == 0 and b['inside'] == 0, (a, b)         # the teacher's forward issues no collective
    assert a['outside'] > 0 and b['outside'] > 0                   # the student's statistics and gradients do
    assert a['finite'] and b['finite'] and all(math.isfinite(x) for x in a['losses'] + b['losses'])
    assert a['digest'] == b['digest']                              # the student's variables: bitwise equal on both ranks
