"""The oracle against the REFERENCE'S OWN SOURCE (tests/golden/reference_pin.npz).

The fixtures were produced in the build container by importing /root/reference/tf2/{objective,lars_optimizer,metrics,resnet,
data_util,model}.py unmodified on top of oracle/tfshim.py (a float64 numpy stand-in for the TensorFlow / Keras calls they make) --
tests/golden/make_reference_golden.py.  Here every fixture is recomputed with oracle/*.py and must agree.  The suite uses the committed
fixtures only; regenerating them from a reference checkout is `python tests/golden/make_reference_golden.py --check`."""
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SCRIPT = os.path.join(HERE, 'golden', 'make_reference_golden.py')


def _script():
    spec = importlib.util.spec_from_file_location('make_reference_golden', SCRIPT)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_oracle_reproduces_the_reference_source_fixtures():
    m = _script()
    ref = dict(np.load(m.OUT_NPZ))
    orc = m.oracle_cases()
    assert set(ref) == set(orc), (sorted(set(ref) - set(orc))[:5], sorted(set(orc) - set(ref))[:5])
    assert len(ref) >= 307 and 'step_r18_img_R1_grad_fd' in ref and 'step_r50_R1_grad_fd' in ref
    bad = [(k, m.compare(ref[k], orc[k], k)) for k in sorted(ref) if m.compare(ref[k], orc[k], k) > m.tolerance(k)]
    assert not bad, bad[:10]
    # what the table covers (a fixture file that silently lost a family would pass the loop above)
    fam = {k.split('_')[0].rstrip('0123456789') for k in ref}
    assert {'ntx', 'ntxr', 'sup', 'lars', 'sched', 'blur', 'conv', 'bn', 'r', 'aug', 'augeval', 'step', 'twoview'} <= fam, fam
    for tag in ('r18_cifar', 'r50', 'r50_sk', 'r34_w2', 'r18_localbn'):
        assert len(ref[tag + '_names']) == {'r18_cifar': 121, 'r50': 281, 'r50_sk': 387, 'r34_w2': 196, 'r18_localbn': 119}[tag]
        assert list(ref[tag + '_names']) == list(orc[tag + '_names'])       # variable names as the reference's layer construction yields them


def test_variable_names_follow_the_lars_name_filters():
    """the name filters of tf2/model.py:39-41 ('batch_normalization', 'bias', 'head_supervised') meet the names the reference's own
    layer construction produced: BatchNorm variables carry 'sync_batch_normalization' (global_bn), the linear-eval head 'head_supervised'"""
    ref = dict(np.load(_script().OUT_NPZ))
    names = list(ref['r50_names'])
    bn = [n for n in names if n.endswith(('gamma:0', 'beta:0'))]
    assert bn and all('batch_normalization' in n for n in bn)
    assert [n for n in names if 'head_supervised' in n] == ['head_supervised/linear_layer/dense_3/bias:0', 'head_supervised/linear_layer/dense_3/kernel:0']
    assert sum(n.endswith('kernel:0') for n in names) == 53 + 3 + 1          # 53 convolutions, 3 projection-head layers, the linear-eval head


# ---- the PRODUCT's Python mirrors (simclr_amd/*.py, no HIP call involved) against the same fixtures --------------------------------
def test_product_schedule_matches_the_reference_source():
    """simclr_amd.model.WarmUpAndCosineDecay / get_train_steps vs what tf2/model.py:72-110 itself returned"""
    from simclr_amd import model as model_lib
    from simclr_amd.flags import FLAGS
    m = _script()
    ref = dict(np.load(m.OUT_NPZ))
    try:
        for i, s in enumerate(m.SCHED):
            FLAGS.reset()
            FLAGS.update(learning_rate_scaling=s['scaling'], train_batch_size=s['batch'], warmup_epochs=s['warmup_epochs'],
                         train_epochs=s['train_epochs'], train_steps=s['train_steps'])
            sched = model_lib.WarmUpAndCosineDecay(s['base_lr'], s['num_examples'])
            got = np.array([float(sched(st)) for st in m.SCHED_STEPS])
            assert np.abs(got - ref['sched%d_lr' % i]).max() <= 1e-12 * max(1.0, np.abs(ref['sched%d_lr' % i]).max()), i
            assert model_lib.get_train_steps(s['num_examples']) == int(ref['sched%d_total_steps' % i])
    finally:
        FLAGS.reset()


def test_product_lars_name_filters_match_the_reference_source():
    """simclr_amd.model.build_optimizer's LARSOptimizer decides per variable name exactly as tf2/lars_optimizer.py:139-157 did on the
    names tf2/resnet.py / tf2/model.py produced (sync_batch_normalization gammas / betas, biases, the linear-eval head)"""
    from simclr_amd import model as model_lib
    from simclr_amd.flags import FLAGS
    ref = dict(np.load(_script().OUT_NPZ))
    try:
        FLAGS.reset()
        FLAGS.update(weight_decay=1e-4)
        opt = model_lib.build_optimizer(0.1)
        for tag in ('r18_cifar', 'r50', 'r50_sk', 'r34_w2', 'r18_localbn'):
            names = list(ref[tag + '_lars_names'])
            assert [bool(opt._use_weight_decay(n)) for n in names] == list(ref[tag + '_lars_decays']), tag
            assert [bool(opt._do_layer_adaptation(n)) for n in names] == list(ref[tag + '_lars_adapts']), tag
            assert 0 < sum(ref[tag + '_lars_decays']) < len(names)
    finally:
        FLAGS.reset()


def test_product_metrics_match_the_reference_source():
    """simclr_amd.metrics.update_pretrain_metrics_train / update_finetune_metrics_train (dense-tensor path) vs tf2/metrics.py:22-55"""
    import torch
    from simclr_amd import metrics as pm
    m = _script()
    ref = dict(np.load(m.OUT_NPZ))

    class Rec:
        def __init__(self):
            self.v = []

        def update_state(self, x):
            self.v.append(float(x))
    for i in range(len(m.NTX)):
        acc, ent = Rec(), Rec()
        pm.update_pretrain_metrics_train(Rec(), acc, ent, torch.tensor(float(ref['ntx%d_loss' % i])),
                                         torch.from_numpy(ref['ntx%d_logits_ab' % i]), torch.from_numpy(ref['ntx%d_labels' % i]))
        assert abs(acc.v[0] - float(ref['ntx%d_acc' % i])) <= 1e-6 and abs(ent.v[0] - float(ref['ntx%d_entropy' % i])) <= 1e-9
    rng = m._rng(20)
    logits, lab = rng.standard_normal((9, 5)) * 3, np.eye(5)[rng.integers(0, 5, 9)]
    acc = Rec()
    pm.update_finetune_metrics_train(Rec(), acc, torch.tensor(float(ref['sup_loss'])), torch.from_numpy(lab), torch.from_numpy(logits))
    assert abs(acc.v[0] - float(ref['sup_acc'])) <= 1e-6


def test_product_model_names_match_the_reference_source():
    """simclr_amd.model.Model (constructed on the CPU: names only, no kernel runs) numbers its layers exactly as the reference's Keras
    layer construction did -- the variable names are what checkpoints and the LARS name filters key on"""
    import torch
    from simclr_amd import model as model_lib
    from simclr_amd.flags import FLAGS
    from simclr_amd.resnet import RT
    m = _script()
    ref = dict(np.load(m.OUT_NPZ))
    try:
        for mm in m.MODELS:
            FLAGS.reset()
            FLAGS.update(use_blur=False, resnet_depth=mm['depth'], image_size=mm['size'], sk_ratio=mm['sk'],
                         **{flag: mm[k] for k, flag in m.MODEL_FLAGS.items() if k in mm})
            RT.reset()
            net = model_lib.Model(mm['classes'])
            names = sorted(n[len('model/'):] if n.startswith('model/') else n for n in (v.name for v in net.variables)) if net.variables else None
            if not names:
                pytest.skip('the product builds its variables lazily on the first forward (needs the GPU)')
            assert names == list(ref[mm['tag'] + '_names']), mm['tag']
    finally:
        FLAGS.reset()
        RT.reset()


def test_product_centre_crop_boxes_match_the_reference_source():
    """simclr_amd.data_util.center_crop_boxes (the host side of the evaluation preprocessing) vs the box tf2/data_util.py:175-243
    (_compute_crop_shape + center_crop) itself handed to crop_to_bounding_box, for landscape / portrait / square / extreme sources"""
    from simclr_amd import data_util as pdu
    m = _script()
    ref = dict(np.load(m.OUT_NPZ))
    for i, (sh, sw, size) in enumerate(m.AUG_EVAL):
        box = ref['augeval%d_box' % i]
        assert box.shape[0] == 1 and int(box[0, 0]) == m.ASKED_KINDS['cropbox']
        got = pdu.center_crop_boxes([sh], [sw], size, size)[0]
        assert [int(v) for v in got] == [int(v) for v in box[0, 1:5]], (sh, sw, size, got, box[0, 1:5])
