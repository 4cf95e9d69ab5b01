"""Golden vectors of train_mode='finetune' produced by the REFERENCE'S OWN SOURCE FILES.  TEST INFRASTRUCTURE ONLY.

    python tests/golden/make_finetune_golden.py            # rewrites tests/golden/finetune_pin.npz

The reference's tf2/{objective,lars_optimizer,metrics,resnet,data_util,model}.py are imported UNMODIFIED on top of oracle/tfshim.py, and the
training step is the `single_step` of tf2/run.py:557-622 itself -- through make_reference_golden.py's machinery (flag defaults, the
`_single_step` extraction, the `*_img` variable tables and inputs), which this script imports and does not change.  Per case
(model tag, fine_tune_after_block, ft_proj_selector), on the first view of the case's images and its labels:
  <case>_sup / <case>_sup_eval      supervised logits of Model.__call__ (tf2/model.py:268-270) in training / inference mode
  <case>_moving_checksum            [sum, sum |.|] of every BatchNorm moving statistic after ONE training forward, sorted by name
  <case>_metrics                    supervised_loss, supervised_acc, weight_decay, total_loss of single_step (tf2/run.py:595-613)
  <case>_grad_fd                    <d total_loss / d variable, direction> by central differences of single_step, along unit directions
                                    on TRAINABLE variables (tf2/resnet.py:548-691; names chosen here, not taken from tfshim's `trainable`)
What is not pinned: which variables train (tfshim's `trainable` does not propagate the way Keras' does) -- tests/test_finetune.py
checks the product's trainable set against the freezing table of tf2/resnet.py.
"""
import importlib
import os
import sys
import warnings
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import make_reference_golden as mrg  # noqa: E402

OUT_NPZ = os.path.join(HERE, 'finetune_pin.npz')
# (case tag, model tag of make_reference_golden.MODELS, fine_tune_after_block, ft_proj_selector, [(variable, directions)])
CASES = [
    ('ft_r18_k2_s1', 'r18_img', 2, 1,
     [('resnet/block_group3/residual_block_4/conv2d_fixed_padding_11/conv2d_11/kernel:0', 1),
      ('resnet/block_group3/residual_block_4/conv2d_fixed_padding_12/conv2d_12/kernel:0', 1),
      ('resnet/block_group4/residual_block_7/batch_norm_relu_19/sync_batch_normalization_19/gamma:0', 1),
      ('projection_head/nl_0/dense/kernel:0', 1),
      ('projection_head/nl_0/batch_norm_relu_21/sync_batch_normalization_21/beta:0', 1),
      ('head_supervised/linear_layer/dense_3/kernel:0', 1),
      ('head_supervised/linear_layer/dense_3/bias:0', 1)]),
    ('ft_r18_km1_s0', 'r18_img', -1, 0,
     [('resnet/conv2d_fixed_padding/conv2d/kernel:0', 1),
      ('resnet/block_group1/residual_block/conv2d_fixed_padding_2/conv2d_2/kernel:0', 1),
      ('resnet/batch_norm_relu/sync_batch_normalization/gamma:0', 1),
      ('head_supervised/linear_layer/dense_3/kernel:0', 1)]),
    ('ft_r18_k4_s0', 'r18_img', 4, 0,
     [('head_supervised/linear_layer/dense_3/kernel:0', 2),
      ('head_supervised/linear_layer/dense_3/bias:0', 1)]),
]
METRICS = ['supervised_loss', 'supervised_acc', 'weight_decay', 'total_loss']
WEIGHT_DECAY = 1e-4


def fd_directions(case, shapes):
    """[(variable name, unit-norm direction)], deterministic by name (as make_reference_golden.grad_fd_directions)."""
    tag, _, _, _, vars_ = next(c for c in CASES if c[0] == case)
    out = []
    for name, k in vars_:
        for j in range(k):
            d = np.random.default_rng([zlib.crc32(('%s#%s#%d' % (tag, name, j)).encode()), 7]).standard_normal(tuple(shapes[name]))
            out.append((name, d / np.sqrt((d * d).sum())))
    return out


def model_case(tag):
    return next(m for m in mrg.MODELS if m['tag'] == tag)


def case_inputs(m):
    """The case's images, first view only ([b, H, W, 3]: finetune feeds one view, tf2/data.py:52-58), and its labels."""
    images, labels = mrg._model_inputs(m)
    return np.ascontiguousarray(images[..., :3]), labels


def reference_cases(ref_dir=mrg.REFERENCE):
    from oracle import tfshim
    tf, FLAGS = tfshim.install()
    for k, v in mrg.FLAG_DEFAULTS.items():
        setattr(FLAGS, k, v)
    sys.path.insert(0, os.path.join(ref_dir, 'tf2'))
    try:
        for mname in ('objective', 'lars_optimizer', 'metrics', 'resnet', 'data_util', 'model'):
            sys.modules.pop(mname, None)
        objective, lars_optimizer, metrics, resnet, data_util, model = (
            importlib.import_module(n) for n in ('objective', 'lars_optimizer', 'metrics', 'resnet', 'data_util', 'model'))
    finally:
        sys.path.pop(0)
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        FLAGS.use_blur = False
        for case, tag, k, sel, _ in CASES:
            m = model_case(tag)
            FLAGS.resnet_depth, FLAGS.image_size, FLAGS.sk_ratio = m['depth'], m['size'], m['sk']
            for key, flag in mrg.MODEL_FLAGS.items():
                setattr(FLAGS, flag, m.get(key, mrg.FLAG_DEFAULTS[flag]))
            FLAGS.train_mode, FLAGS.fine_tune_after_block, FLAGS.ft_proj_selector = 'finetune', k, sel
            FLAGS.weight_decay = WEIGHT_DECAY
            _, params, state, _ = mrg._oracle_model(m)
            allv = {**params, **state}
            images, labels = case_inputs(m)
            x = tf.constant(images)

            def build():
                tfshim.reset_uids()
                net = model.Model(m['classes'])
                net(x, training=False)                                   # builds the variables (inference: nothing moves)
                vs = list(tfshim.CREATED_VARIABLES)
                for v in vs:
                    v.assign(allv['model/' + v.name].numpy())
                return net, vs
            net, vs = build()
            proj, sup = net(x, training=True)
            assert proj is None
            out[case + '_sup'] = sup.numpy()
            out[case + '_moving_checksum'] = np.array([[float(v.numpy().sum()), float(np.abs(v.numpy()).sum())]
                                                       for v in sorted(vs, key=lambda v: v.name) if 'moving_' in v.name])
            _, sup_e = net(x, training=False)
            out[case + '_sup_eval'] = sup_e.numpy()
            # tf2/run.py single_step on fresh variables
            net, vs = build()
            opt = tfshim.RecordingOptimizer()
            strategy = tfshim.Strategy(1)
            ns = dict(tf=tf, FLAGS=FLAGS, logging=sys.modules['absl.logging'], metrics=metrics, obj_lib=objective, model_lib=model,
                      optimizer=opt, steps_per_loop=100, model=net, strategy=strategy)
            step = mrg._single_step(ref_dir, ns)
            shards = [(x, {'labels': tf.constant(labels)})]

            def run():
                mets = {key: tfshim._Mean('train/' + key) for key in mrg.STEP_METRICS}
                for key in mrg.STEP_METRICS:
                    ns[key + '_metric'] = mets[key]
                strategy.run(step, shards)
                return {key: float(mets[key].result()) for key in METRICS}
            base_m = run()
            out[case + '_metrics'] = np.array([base_m[key] for key in METRICS])
            byname = {v.name: v for v in vs}
            g = []
            for name, d in fd_directions(case, {n: v.value.shape for n, v in byname.items()}):
                v = byname[name]
                base = v.numpy().copy()
                vals = []
                for sgn in (+1.0, -1.0):
                    v.assign(base + sgn * mrg.GRAD_FD_STEP * d)
                    vals.append(run()['total_loss'])
                v.assign(base)
                g.append((vals[0] - vals[1]) / (2.0 * mrg.GRAD_FD_STEP))
            out[case + '_grad_fd'] = np.array(g)
        for key in ('resnet_depth', 'image_size', 'sk_ratio', 'use_blur', 'train_mode', 'fine_tune_after_block', 'weight_decay') + \
                tuple(mrg.MODEL_FLAGS.values()):
            setattr(FLAGS, key, mrg.FLAG_DEFAULTS[key])
    return out


def main():
    out = reference_cases()
    np.savez_compressed(OUT_NPZ, **out)
    print('wrote %s (%d arrays)' % (OUT_NPZ, len(out)))


if __name__ == '__main__':
    main()
