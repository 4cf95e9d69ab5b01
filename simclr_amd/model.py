"""Model assembly -- drop-in mirror of /root/reference/tf2/model.py on the HIP kernels.

Mirrors `build_optimizer` (:29-44), `add_weight_decay` (:47-69), `get_train_steps` (:72-75),
`WarmUpAndCosineDecay` (:78-116), `LinearLayer` (:119-154), `ProjectionHead` (:157-213),
`SupervisedHead` (:216-225) and `Model` (:228-280) with the reference's names, argument
order and defaults.  Forward results are plain device tensors; each class also carries the
hand-written backward that `tape.gradient` (tf2/run.py:621) would derive.
"""
import math

import torch

from . import data_util, lars_optimizer, ops, optimizers, resnet
from .flags import FLAGS, aug_plan, check_dropblock_flags
from .lars_optimizer import Variable
from .resnet import RT, Act, Layer, PackedInput, scope


def build_optimizer(learning_rate):
    """Returns the optimizer (tf2/model.py:29-44)."""
    if FLAGS.optimizer == 'lars':
        return lars_optimizer.LARSOptimizer(
            learning_rate,
            momentum=FLAGS.momentum,
            weight_decay=FLAGS.weight_decay,
            exclude_from_weight_decay=['batch_normalization', 'bias', 'head_supervised'])
    elif FLAGS.optimizer == 'momentum':                                                     # :31-32
        # l2: the gradient of add_weight_decay's loss term for the non-LARS optimizers (:62-69), applied inside the update kernel
        return optimizers.SGD(learning_rate, FLAGS.momentum, nesterov=True, l2=FLAGS.weight_decay)
    elif FLAGS.optimizer == 'adam':                                                         # :33-34
        return optimizers.Adam(learning_rate, l2=FLAGS.weight_decay)
    else:
        raise ValueError('Unknown optimizer {}'.format(FLAGS.optimizer))


def add_weight_decay(model, adjust_per_optimizer=True):
    """Compute weight decay from flags (tf2/model.py:47-69).  Returns a float32 device scalar
    (or 0).  With LARS only the supervised head's non-bias variables contribute (:49-60); the
    matching gradient term wd*w is added by Model.backward."""
    if adjust_per_optimizer and 'lars' in FLAGS.optimizer:
        vs = [v for v in model.trainable_variables if 'head_supervised' in v.name and 'bias' not in v.name]
    else:
        vs = [v for v in model.trainable_variables if 'batch_normalization' not in v.name]
    if not vs:
        return 0
    nv = len(vs)
    out = ops.step_scalars(nv + 1, vs[0].value.device)
    for i, v in enumerate(vs):
        ops.l2_loss_f32(v.value, out[i:i + 1])          # tf.nn.l2_loss = sum(v^2)/2
    if nv > 16:                                         # SGD / Adam: every non-BN variable contributes
        return FLAGS.weight_decay * out[:nv].sum()
    # weight_decay * add_n(l2 losses) (:58-60 / :66-68) in one launch
    ops.accumulate_scalars([out[j:j + 1] for j in range(nv)], scales=[FLAGS.weight_decay] * nv, total=out[nv:nv + 1],
                           total_mask=(1 << nv) - 1)
    return out[nv]


def get_train_steps(num_examples):
    """Determine the number of training steps (tf2/model.py:72-75)."""
    return FLAGS.train_steps or (num_examples * FLAGS.train_epochs // FLAGS.train_batch_size + 1)


class WarmUpAndCosineDecay:
    """Applies a warmup schedule on a given learning rate decay schedule (tf2/model.py:78-116)."""

    def __init__(self, base_learning_rate, num_examples, name=None):
        self.base_learning_rate = base_learning_rate
        self.num_examples = num_examples
        self._name = name

    def __call__(self, step):
        warmup_steps = int(round(FLAGS.warmup_epochs * self.num_examples // FLAGS.train_batch_size))   # :89-91
        if FLAGS.learning_rate_scaling == 'linear':
            scaled_lr = self.base_learning_rate * FLAGS.train_batch_size / 256.
        elif FLAGS.learning_rate_scaling == 'sqrt':
            scaled_lr = self.base_learning_rate * math.sqrt(FLAGS.train_batch_size)
        else:
            raise ValueError('Unknown learning rate scaling {}'.format(FLAGS.learning_rate_scaling))
        learning_rate = (step / float(warmup_steps) * scaled_lr if warmup_steps else scaled_lr)
        total_steps = get_train_steps(self.num_examples)
        decay_steps = total_steps - warmup_steps
        # tf.keras.experimental.CosineDecay(scaled_lr, decay_steps)(step - warmup_steps), alpha=0
        # decay_steps <= 0 (train_steps <= warmup_steps): the reference divides 0/0 here; the decay is then complete
        s = min(max(step - warmup_steps, 0), decay_steps)
        frac = (s / decay_steps) if decay_steps > 0 else 1.0
        cosine = scaled_lr * 0.5 * (1.0 + math.cos(math.pi * frac))
        return learning_rate if step < warmup_steps else cosine                       # :107-108

    def get_config(self):
        return {'base_learning_rate': self.base_learning_rate, 'num_examples': self.num_examples}


class LinearLayer(Layer):  # tf2/model.py:119-154
    def __init__(self, num_classes, use_bias=True, use_bn=False, name='linear_layer', **kwargs):
        # Note: use_bias is ignored for the dense layer when use_bn=True (it is used for BN's center).
        # pad_multiple: the compute copies pad the class dimension to this multiple (64: the data gradient's reduction
        # dimension, conv2d_dgrad needs Cout % 64 == 0 in bf16 / % 32 in fp32)
        self.pad_multiple = kwargs.get('pad_multiple', 16)
        self.num_classes = num_classes
        self.use_bias = use_bias
        self.use_bn = use_bn
        self._name = name
        with scope(name):
            if self.use_bn:
                self.bn_relu = resnet.BatchNormRelu(relu=False, center=use_bias)      # :134-135
            self._dense = RT.unique('dense')
            self._path = RT.path(self._dense)
        self.kernel = None
        self.bias = None
        self._version = -1
        self.saved = None

    def build(self, cin):
        n = self.num_classes(cin) if callable(self.num_classes) else self.num_classes
        self.nout = n
        pm = self.pad_multiple
        self.npad = (n + pm - 1) // pm * pm
        RT.seed += 1
        g = torch.Generator().manual_seed(RT.seed)
        w = torch.randn(cin, n, generator=g) * 0.01                   # RandomNormal(stddev=.01), :145
        self.kernel = Variable(self._path + '/kernel:0', w.to(RT.device))
        if self.use_bias and not self.use_bn:                        # :146
            self.bias = Variable(self._path + '/bias:0', torch.zeros(n, device=RT.device))
        self.cin = cin

    def _refresh(self, dtype):
        """Compute copies of the fp32 master weight in the dtype of the layer's input."""
        if self._version == RT.weights_version and getattr(self, '_dtype', None) == dtype:
            return
        if not self.trainable and self._version >= 0 and getattr(self, '_frozen_key', None) == (RT.frozen_version, dtype):
            return                  # frozen (the distillation teacher): the optimizer step did not change this weight
        self._frozen_key = None if self.trainable else (RT.frozen_version, dtype)
        w4 = self.kernel.value.view(1, 1, self.cin, self.nout)
        if self.npad == self.nout:
            self.w_t = ops.prep_weights(w4, 0, dtype)
        else:   # class dimension padded to a multiple of pad_multiple with zero rows
            self.w_t = torch.zeros(self.npad, self.cin, device=RT.device, dtype=dtype)
            ops.prep_weights(w4, 0, dtype, out=self.w_t[:self.nout])
        # class dimension padded: the data-gradient copy is made on first use (LinearLayer.backward(need_dx=True), finetune)
        self.w_d = ops.prep_weights(w4, 1, dtype) if self.npad == self.nout else None
        self._version = RT.weights_version
        self._dtype = dtype

    def __call__(self, inputs, training, relu=False):
        """inputs: [V, C] tensor.  Returns [V, n] tensor (dense [+BN [+relu]])."""
        assert inputs.dim() == 2, inputs.shape
        V, cin = inputs.shape
        if self.kernel is None:
            self.build(cin)
        self._refresh(inputs.dtype)
        x4 = inputs.view(V, 1, 1, cin)
        stats = ops.conv_stats(V, self.npad, RT.device) if (self.use_bn and training) else None
        y, stats, sums = ops.conv2d_fwd_with_stats(x4, self.w_t, 1, 1, 1, 0, 1, 1, stats)
        y = y.view(V, self.npad)
        self.saved = dict(x=x4)
        if self.use_bn:
            return self.bn_relu(Act(y, stats, sums=sums), training, relu=relu).t
        return y

    def backward(self, dy, need_dx=True):
        if self.use_bn:
            dy, _ = self.bn_relu.backward(dy)
        V = dy.shape[0]
        dy4 = dy.view(V, 1, 1, self.npad)
        x4 = self.saved['x']
        self.saved = None
        g = self.kernel.ensure_grad()
        if self.npad == self.nout:
            ops.conv2d_wgrad(x4, dy4, 1, 1, 1, 0, out=g)
        else:
            tmp = ops.conv2d_wgrad(x4, dy4, 1, 1, 1, 0)
            g.copy_(tmp[:, :self.nout])
        if self.bias is not None:
            ops.colsum(dy, self.nout, self.bias.ensure_grad())
        if not need_dx:
            return None
        if self.w_d is None:
            # [cin, npad] with zero columns for the padded classes (the padded columns of dy are zero as well)
            self.w_d = ops.prep_weights(self.kernel.value.view(1, 1, self.cin, self.nout), 1, dy.dtype, cout_p=self.npad)
        return ops.conv2d_dgrad(dy4, self.w_d, 1, 1, 1, 0, 1, 1).view(V, self.cin)


class ProjectionHead(Layer):  # tf2/model.py:157-213
    def __init__(self, **kwargs):
        out_dim = FLAGS.proj_out_dim
        self.linear_layers = []
        with scope('projection_head'):
            if FLAGS.proj_head_mode == 'none':
                pass  # directly use the output hiddens as hiddens
            elif FLAGS.proj_head_mode == 'linear':
                self.linear_layers = [LinearLayer(num_classes=out_dim, use_bias=False, use_bn=True, name='l_0')]
            elif FLAGS.proj_head_mode == 'nonlinear':
                for j in range(FLAGS.num_proj_layers):
                    if j != FLAGS.num_proj_layers - 1:
                        # for the middle layers, use bias and relu for the output.
                        self.linear_layers.append(LinearLayer(num_classes=lambda cin: int(cin), use_bias=True,
                                                              use_bn=True, name='nl_%d' % j))
                    else:
                        # for the final layer, neither bias nor relu is used.
                        self.linear_layers.append(LinearLayer(num_classes=FLAGS.proj_out_dim, use_bias=False,
                                                              use_bn=True, name='nl_%d' % j))
            else:
                raise ValueError('Unknown head projection mode {}'.format(FLAGS.proj_head_mode))

    def __call__(self, inputs, training):
        if FLAGS.proj_head_mode == 'none':
            return inputs, inputs  # directly use the output hiddens as hiddens
        self._in_dtype = inputs.dtype
        if FLAGS.head_dtype == 'f32' and inputs.dtype != torch.float32:
            inputs = ops.cast(inputs, torch.float32)          # heads in fp32 on top of a bf16 encoder
        hiddens_list = [inputs]
        if FLAGS.proj_head_mode == 'linear':
            # The reference returns None here (list.append, tf2/model.py:198-199); we return the
            # evidently intended pair instead of reproducing the bug.
            hiddens_list.append(self.linear_layers[0](hiddens_list[-1], training))
        else:
            n = FLAGS.num_proj_layers
            for j in range(n):
                hiddens_list.append(self.linear_layers[j](hiddens_list[-1], training, relu=(j != n - 1)))
        # The first element is the output of the projection head, the second the finetune-head input.
        return hiddens_list[-1], hiddens_list[FLAGS.ft_proj_selector]

    def backward(self, d, upto=None):
        """d: gradient wrt hiddens_list[upto] (default: the projection output).  Only layers 0 .. upto-1 run their
        backward -- finetune mode's gradient enters at ft_proj_selector (tf2/model.py:268-270)."""
        layers = self.linear_layers if upto is None else self.linear_layers[:upto]
        for layer in reversed(layers):
            d = layer.backward(d)
        if self.linear_layers and d.dtype != self._in_dtype:
            d = ops.cast(d, self._in_dtype)
        return d


def pretrain_loss():
    """Name of the active pretraining loss (--contrastive_loss), or None outside a pretraining run: train_mode=finetune has no
    contrastive loss and ignores the flag.  The one statement of that switch: the model reads it to decide which heads it carries,
    run.py to pick the row of pretrain_losses.LOSSES."""
    return getattr(FLAGS, 'contrastive_loss', 'ntxent') if FLAGS.train_mode == 'pretrain' else None


def byol_on():
    """--contrastive_loss=byol in a pretraining run: the online model carries a predictor and the step needs a TargetNetwork."""
    return pretrain_loss() == 'byol'


def moco_on():
    """--contrastive_loss=mocov2 in a pretraining run: the step needs a TargetNetwork with a MocoQueue; the online model is the ntxent
    model (no predictor)."""
    return pretrain_loss() == 'mocov2'


def dino_on():
    """--contrastive_loss=dino in a pretraining run: the model carries a PrototypeHead and the step needs a TargetNetwork with a
    DinoCenter; no predictor."""
    return pretrain_loss() == 'dino'


def dino_teacher_temp(step, steps_per_epoch):
    """Teacher temperature of DINO at optimizer step `step`: linear from --dino_warmup_teacher_temp to --dino_teacher_temp over
    --dino_warmup_teacher_temp_epochs * steps_per_epoch steps, then constant.  Formed in double, cast to float32 once."""
    import numpy as np
    final, warm = float(FLAGS.dino_teacher_temp), float(FLAGS.dino_warmup_teacher_temp)
    n = int(FLAGS.dino_warmup_teacher_temp_epochs) * int(steps_per_epoch)
    if n <= 0 or int(step) >= n:
        return float(np.float32(final))
    return float(np.float32(warm + (final - warm) * (float(int(step)) / float(n))))


def dino_last_layer_frozen(step, steps_per_epoch):
    """True while the prototypes take no update: step < --dino_freeze_last_layer_epochs * steps_per_epoch."""
    return int(step) < int(FLAGS.dino_freeze_last_layer_epochs) * int(steps_per_epoch)


def swav_on():
    """--contrastive_loss=swav in a pretraining run: the model carries a PrototypeHead; no target network, no predictor."""
    return pretrain_loss() == 'swav'


def swav_prototypes_frozen(step, steps_per_epoch):
    """True while the SwAV prototypes take no update: step < --swav_freeze_prototypes_epochs * steps_per_epoch."""
    return int(step) < int(FLAGS.swav_freeze_prototypes_epochs) * int(steps_per_epoch)


class PrototypeHead(Layer):
    """The prototype layer of DINO (Caron et al. 2021): ONE variable [K, D] whose rows, l2-normalised every step, score the
    l2-normalised projection output -- the paper's weight-normalised last layer with norm_last_layer=True (gain fixed at 1).  The
    variable is initialised as a LinearLayer kernel of that shape (RandomNormal(stddev=.01)) and is trained, weight-decayed and
    LARS-adapted by the name rules that cover the projection head's kernels.

    A call returns the normalised rows [K, D] (tf.math.l2_normalize, epsilon 1e-12) and keeps them for `backward(dws)`, which writes
    the gradient of the raw variable into its gradient slot.  The [2b, K] logits are never formed here: the loss kernels sweep them."""

    def __init__(self, num_prototypes, **kwargs):
        self.num_prototypes = int(num_prototypes)
        with scope('prototype_head'):
            self._path = RT.path('kernel:0')
        self.kernel = None
        self.saved = None

    def build(self, width):
        RT.seed += 1
        g = torch.Generator().manual_seed(RT.seed)
        w = torch.randn(self.num_prototypes, int(width), generator=g) * 0.01          # as LinearLayer.build
        self.kernel = Variable(self._path, w.to(RT.device))

    def __call__(self, width=None):
        if self.kernel is None:
            self.build(projection_width() if width is None else width)
        w, inv = ops.l2norm_fwd(self.kernel.value)
        self.saved = (w, inv)
        return w

    def backward(self, dws):
        """dws: gradient wrt the normalised rows [K, D] -> written into the variable's gradient slot (and returned)."""
        w, inv = self.saved
        self.saved = None
        g = self.kernel.ensure_grad()
        g.copy_(ops.l2norm_bwd(w, inv, dws))
        return g


def projection_width():
    """Width of the block the pretraining loss reads: proj_out_dim, or the encoder's pooled output for proj_head_mode=none.  The one
    statement of that rule: the start-up checks of run.check_contrastive_loss_flags and the predictor's output layer both call it."""
    if FLAGS.proj_head_mode == 'none':
        return (512 if FLAGS.resnet_depth in (18, 34) else 2048) * FLAGS.width_multiplier
    return FLAGS.proj_out_dim


class PredictionHead(Layer):
    """The predictor of BYOL (Grill et al. 2020, section 3.3) on the online projection output: dense + BN + ReLU of width
    byol_pred_hidden_dim, then a dense layer back to the loss width.  The paper's output layer has a bias; LinearLayer without
    BatchNorm applies none (tf2/model.py:146 creates it only with use_bias=True), and this one is built without.  Trained,
    weight-decayed and LARS-adapted by the name rules of the projection head's layers."""

    def __init__(self, **kwargs):
        with scope('prediction_head'):
            self.linear_layers = [LinearLayer(num_classes=FLAGS.byol_pred_hidden_dim, use_bias=True, use_bn=True, name='l_0'),
                                  LinearLayer(num_classes=projection_width(), use_bias=False, use_bn=False, name='l_1')]

    def __call__(self, inputs, training):
        hidden = self.linear_layers[0](inputs, training, relu=True)
        return self.linear_layers[1](hidden, training)

    def backward(self, dq):
        """dq: gradient wrt the predictor's output -> gradient wrt its input (the online projection output)."""
        return self.linear_layers[0].backward(self.linear_layers[1].backward(dq))


class SupLogits:
    """Supervised-head output before the bias add; bias + softmax-CE + gradient are one fused
    launch in objective.add_supervised_loss."""

    def __init__(self, z, bias, num_classes):
        self.z, self.bias, self.num_classes = z, bias, num_classes

    def dense(self):
        return self.z[:, :self.num_classes].float() + self.bias


class SupervisedHead(Layer):  # tf2/model.py:216-225
    def __init__(self, num_classes, name='head_supervised', **kwargs):
        with scope(name):
            # finetune: the gradient flows through this layer into the projection head / encoder (no stop_gradient)
            self.linear_layer = LinearLayer(num_classes, pad_multiple=64 if FLAGS.train_mode == 'finetune' else 16)

    def __call__(self, inputs, training):
        z = self.linear_layer(inputs, training)
        return SupLogits(z, self.linear_layer.bias.value, self.linear_layer.nout)

    def backward(self, dlogits):
        self.linear_layer.backward(dlogits, need_dx=False)      # stop_gradient on the input, :276-277


class Model(Layer):
    """Resnet model with projection or supervised layer (tf2/model.py:228-280)."""

    def __init__(self, num_classes, **kwargs):
        RT.strategy = kwargs.get('strategy', RT.strategy)
        with scope('model'):
            keep_probs, dropblock_size = check_dropblock_flags()
            self.resnet_model = resnet.resnet(resnet_depth=FLAGS.resnet_depth,
                                              width_multiplier=FLAGS.width_multiplier,
                                              cifar_stem=FLAGS.image_size <= 32,
                                              dropblock_keep_probs=keep_probs, dropblock_size=dropblock_size)
            self._projection_head = ProjectionHead()
            self.supervised_head = None
            if FLAGS.train_mode == 'finetune' or FLAGS.lineareval_while_pretraining:
                self.supervised_head = SupervisedHead(num_classes)
            # BYOL: constructed last, so every other layer keeps the name (and, built after them, the initial value) of an ntxent run
            self.prediction_head = PredictionHead() if byol_on() else None
            # DINO: constructed (and, by TargetNetwork, built) LAST for the same reason
            self.prototype_head = PrototypeHead(FLAGS.dino_out_dim) if dino_on() else None
            # SwAV: the same layer under the same name, built last too (at its first call, or by build_variables)
            if swav_on():
                self.prototype_head = PrototypeHead(FLAGS.swav_num_prototypes)
        self._flat_grads = None

    def __call__(self, inputs, training, blur=True, supervised=True):
        """inputs: float32 [b, H, W, 3k] in [0,1].  Returns (projection_head_outputs float32
        [k*b, proj_out_dim], supervised_head_outputs SupLogits) like tf2/model.py:241-280.
        blur=False: the caller drew the random blur already (the BYOL step hands the online and the target network the same pixels).
        supervised=False (pretraining): the linear-eval head does not run (the second, local-view pass of SwAV multi-crop)."""
        if training and FLAGS.train_mode == 'pretrain':
            if FLAGS.fine_tune_after_block > -1:
                raise ValueError('Does not support layer freezing during pretraining,'
                                 'should set fine_tune_after_block<=-1 for safety.')
        if inputs.dim() != 4 or inputs.shape[3] % 3 != 0:
            raise ValueError('The input channels dimension must be statically known '
                             f'(got input shape {tuple(inputs.shape)})')
        # (evaluation passes do not go through ops.begin_step.)  Inference mode normalises with the MOVING statistics, so nothing bounds the
        # activations to fp16's range (a freshly initialised network's moving averages do not normalise at all): the split-fp16 forward is
        # for training-mode BatchNorm only, an inference forward runs its fp32 products as six bf16 terms instead (same accuracy class).
        ops.select_f32_matmul(inference=not training)
        if blur and training and FLAGS.train_mode == 'pretrain':
            # batch_random_blur on the device (tf2/model.py:255-258), fused over the k views, and the plan's solarization in its
            # last pass; --use_blur=False without solarization launches nothing
            inputs = data_util.apply_view_plan(inputs, aug_plan(), height=FLAGS.image_size)
        num_transforms = inputs.shape[3] // 3
        k, s = self.resnet_model.stem_kernel_stride
        # (training: the 7x7 stem's weight gradient reads the image as bf16 pieces in the three-term modes -- written by the packing pass)
        rm = self.resnet_model
        ps_cout = rm.stem_conv.filters if (training and rm.stem_trainable and not rm.stem_pre and not rm.cifar_stem) else 0
        packed = PackedInput(inputs.contiguous(), num_transforms, k, s, RT.dtype, presplit_for_cout=ps_cout)   # split + concat, :250-259
        hiddens = self.resnet_model(packed, training=training)                     # :262
        proj, sup_in = self._projection_head(hiddens, training)                    # :265-266
        if FLAGS.train_mode == 'finetune':
            # one view, no stop_gradient: the supervised head reads hiddens_list[ft_proj_selector] (:268-270).  Every projection
            # layer ran (its BatchNorm moving statistics moved); the ones at and above the selector get no gradient.
            for l in self._projection_head.linear_layers[FLAGS.ft_proj_selector:]:
                l.release()
            return None, self.supervised_head(sup_in, training)
        self._proj_is_encoder = proj is hiddens
        self._proj_dtype = proj.dtype
        proj32 = ops.cast(proj, torch.float32) if proj.dtype != torch.float32 else proj
        sup_out = None
        if FLAGS.train_mode == 'pretrain' and FLAGS.lineareval_while_pretraining and supervised:
            sup_out = self.supervised_head(sup_in, training)                       # stop_gradient, :276-278
        return proj32, sup_out

    def features(self, inputs):
        """inputs: float32 [b, H, W, 3] in [0,1].  The encoder alone in inference mode (moving BatchNorm statistics, no blur): the
        pooled `hiddens` the heads read, as float32 [b, C].  Neither head runs, no activation is kept and no variable or moving
        statistic moves, so a call between two training steps leaves the next step what it is without the call
        (simclr_amd/knn.py: the frozen features of the weighted k-NN evaluation)."""
        if inputs.dim() != 4 or inputs.shape[3] != 3:
            raise ValueError(f'features() reads single-view batches [b, H, W, 3] (got input shape {tuple(inputs.shape)})')
        ops.select_f32_matmul(inference=True)
        k, s = self.resnet_model.stem_kernel_stride
        packed = PackedInput(inputs.contiguous(), 1, k, s, RT.dtype)
        hiddens = self.resnet_model(packed, training=False)
        out = ops.cast(hiddens, torch.float32) if hiddens.dtype != torch.float32 else hiddens.clone()
        self.release()
        return out

    def predict(self, projection_head_outputs, training=True):
        """BYOL: the predictor on the online projection output, float32 [2b, D] -> float32 [2b, D]."""
        return self.prediction_head(projection_head_outputs, training)

    def backward_predictor(self, dq):
        """Gradient wrt the predictor's output -> d_proj for Model.backward (the predictor's weight gradients are written)."""
        return self.prediction_head.backward(dq)

    def backward_supervised(self, d_sup):
        """Backward of the linear-eval head alone (its input is stop_gradient'ed, tf2/model.py:276-277)."""
        if d_sup is not None:
            self.supervised_head.backward(d_sup)
            if 'lars' in FLAGS.optimizer and FLAGS.weight_decay:   # d/dw of add_weight_decay, :49-60
                k = self.supervised_head.linear_layer.kernel
                ops.axpy_f32(FLAGS.weight_decay * self._wd_grad_scale, k.value, k.grad)

    def backward(self, d_proj, d_sup=None, on_stage=None):
        """d_proj: float32 [k*b, proj_out_dim]; d_sup: gradient wrt the supervised logits.
        train_mode=finetune: d_proj is None and d_sup carries the whole gradient (backward_finetune)."""
        if FLAGS.train_mode == 'finetune':
            return self.backward_finetune(d_sup, on_stage)
        self.backward_supervised(d_sup)
        d = ops.cast(d_proj, self._proj_dtype) if self._proj_dtype != torch.float32 else d_proj
        d = self._projection_head.backward(d)
        self.resnet_model.backward(d, on_stage=on_stage)

    def backward_finetune(self, d_sup, on_stage=None):
        """tape.gradient of the finetune loss (tf2/run.py:577-622): the supervised head (weights and, where anything below it
        trains, its input), the projection head from ft_proj_selector downwards, then the encoder up to its first frozen layer."""
        rm = self.resnet_model
        sel = FLAGS.ft_proj_selector
        encoder_trains = rm.first_trainable_group < len(rm.block_groups)
        need_dx = encoder_trains or any(l.trainable_variables for l in self._projection_head.linear_layers[:sel])
        lin = self.supervised_head.linear_layer
        d = lin.backward(d_sup, need_dx=need_dx)
        if 'lars' in FLAGS.optimizer and FLAGS.weight_decay:       # d/dw of add_weight_decay, :49-60
            ops.axpy_f32(FLAGS.weight_decay * self._wd_grad_scale, lin.kernel.value, lin.kernel.grad)
        if not need_dx:
            return
        d = self._projection_head.backward(d, upto=sel)
        if encoder_trains:
            rm.backward(d, on_stage=on_stage)

    def variables_without_gradient(self):
        """finetune: the projection-head variables at and above ft_proj_selector, which no path connects to the loss (tape.gradient
        returns None for them; the L2 term of add_weight_decay may still give the kernels a gradient, see run.make_single_step)."""
        if FLAGS.train_mode != 'finetune':
            return []
        return [v for l in self._projection_head.linear_layers[FLAGS.ft_proj_selector:] for v in l.trainable_variables]

    def build_variables(self):
        """Create every variable from the layer configuration alone -- no device work, in the order (and with the initial values) of
        the lazy build of the first forward pass.  Plain ResNet encoders (no selective kernels)."""
        rm = self.resnet_model
        if rm.stem_pre or FLAGS.sk_ratio > 0:
            raise NotImplementedError('build_variables: selective-kernel / ResNet-D encoders build at their first forward pass')
        c = rm.stem_conv
        c.build(3)
        rm.stem_bn.build(c.filters, c.cout_p)
        cin = c.filters
        for g in rm.block_groups:
            for b in g.layers:
                # the forward's build order: shortcut conv and conv1 read the block input, then conv2 (and conv3) in sequence
                chain = [b.conv1, b.conv2] + ([b.conv3] if isinstance(b, resnet.BottleneckBlock) else [])
                pairs = list(zip(chain, [b.bn1, b.bn2] + ([b.bn3] if len(chain) == 3 else [])))
                if b.shortcut is not None:
                    pairs.insert(0, (b.shortcut.conv, b.shortcut.bn))
                    b.shortcut.conv.build(cin)
                x = cin
                for cv in chain:
                    cv.build(x)
                    x = cv.filters
                for cv, bn in pairs:
                    bn.build(cv.filters, cv.cout_p)
                cin = x
        feats = [cin]
        for l in self._projection_head.linear_layers:
            l.build(feats[-1])
            if l.use_bn:
                l.bn_relu.build(l.npad)
            feats.append(l.npad)
        if self.supervised_head is not None:
            sel = FLAGS.ft_proj_selector if FLAGS.proj_head_mode != 'none' else 0
            self.supervised_head.linear_layer.build(feats[sel])
        if self.prediction_head is not None:
            l0, l1 = self.prediction_head.linear_layers
            l0.build(feats[-1])
            l0.bn_relu.build(l0.npad)
            l1.build(l0.npad)
        if self.prototype_head is not None:
            self.prototype_head.build(feats[-1])

    def release(self):
        super().release()
        rm = self.resnet_model
        rm.endpoints.clear()
        rm._final = rm._pool = None

    _wd_grad_scale = 1.0   # set to 1/num_replicas by the step (loss / R, tf2/run.py:617)

    def allocate_flat_grads(self):
        """One flat fp32 buffer for every trainable gradient (ordered last-layer-first so the
        gradient all-reduce can be bucketed along the backward pass)."""
        vs = list(reversed(self.trainable_variables))
        offs, total = [], 0
        for v in vs:
            offs.append(total)
            total += (v.numel() + 63) // 64 * 64
        flat = torch.zeros(total, device=vs[0].value.device, dtype=torch.float32)
        for v, o in zip(vs, offs):
            v.grad = flat[o:o + v.numel()].view(v.value.shape)
        self._flat_grads = flat
        self._flat_order = vs
        self._flat_offsets = offs
        return flat


def teacher_flag_values():
    """The flag values the distillation teacher is built and called under: its own architecture flags (--teacher_*, each defaulting
    to the student's), the structure of a fine-tuned model, everything else shared with the student."""
    def pick(name):
        v = getattr(FLAGS, 'teacher_' + name)
        return getattr(FLAGS, name) if v is None else v
    return dict(train_mode='finetune', fine_tune_after_block=-1, resnet_depth=pick('resnet_depth'),
                width_multiplier=pick('width_multiplier'), sk_ratio=pick('sk_ratio'), ft_proj_selector=pick('ft_proj_selector'),
                dropblock_keep_probs='')        # the teacher never trains: no DropBlock site


class Teacher:
    """The frozen fine-tuned network of the self-training stage (tf2/colabs/distillation_self_training.ipynb:908-919): a second Model
    in the process, built under `teacher_flag_values()` and under the variable names it has when built alone (RT.fresh_names), so that
    its own checkpoint restores by name and the student's names and initial values are those of a run without a teacher.  The whole
    model is `trainable = False`; a call is an inference forward (moving BatchNorm statistics) that keeps no activations.

    Construct it BEFORE the student: its one build-forward runs here.  `checkpoint`: restored strictly -- a teacher variable that the
    file lacks or holds with another shape raises, the supervised head included."""

    def __init__(self, num_classes, checkpoint=None, image_size=None):
        self.flag_values = teacher_flag_values()
        size = image_size or FLAGS.image_size
        with FLAGS.override(**self.flag_values), RT.fresh_names():
            self.model = Model(num_classes)
            self.model.trainable = False
            for l in _all_layers(self.model):
                l.inference_only = True
            # variables exist only after the first forward pass (lazy build)
            self.model(torch.zeros(2, size, size, 3, device=RT.device), training=False)
            self.model.release()
        if checkpoint:
            self.restore(checkpoint)

    def restore(self, path):
        from .checkpoint import Checkpoint
        status = Checkpoint(model=self.model).restore(path, model_only=True)
        if status.missing_in_checkpoint or status.shape_mismatch:
            raise ValueError('teacher checkpoint %s does not hold the teacher (flags %s): missing variables %s, variables of another '
                             'shape (name, in the file, in the model) %s'
                             % (path, self.flag_values, status.missing_in_checkpoint[:8], status.shape_mismatch[:8]))
        return status

    def __call__(self, features):
        """features [b, H, W, 3] -> SupLogits of the frozen teacher."""
        with FLAGS.override(**self.flag_values):
            _, logits = self.model(features, training=False)
        self.model.release()
        return logits


def byol_tau(step, total_steps, tau_base):
    """Decay of the target network's moving average at optimizer step `step` of `total_steps` (Grill et al. 2020, section 3.3):
    1 - (1 - tau_base) * (cos(pi * step / total_steps) + 1) / 2, in double.  tau_0 = tau_base, tau_K = 1."""
    return 1.0 - (1.0 - float(tau_base)) * (math.cos(math.pi * float(step) / float(total_steps)) + 1.0) / 2.0


def target_flag_values():
    """The flag values the BYOL target network is built and called under: a plain pretraining encoder and projection head of the
    online architecture -- no supervised head, no predictor, no DropBlock site."""
    return dict(train_mode='pretrain', contrastive_loss='dino' if dino_on() else 'ntxent', lineareval_while_pretraining=False,
                fine_tune_after_block=-1, dropblock_keep_probs='')


def moco_queue_ptr(step, rows_per_step, K):
    """Row of the queue the keys of optimizer step `step` (optimizer.iterations before its increment) are written at.  No pointer is
    stored: a resumed run continues by construction.  K is a multiple of rows_per_step, so a step's rows never wrap."""
    return (int(step) * int(rows_per_step)) % int(K)


def moco_queue_init(K, D, seed):
    """The initial queue of MoCo: K random unit rows -- numpy.random.default_rng([seed]).standard_normal((K, D)), l2-normalised in
    float64 and cast to float32 once.  A function of (K, D, seed) alone: identical on every replica."""
    import numpy as np
    x = np.random.default_rng([int(seed)]).standard_normal((int(K), int(D)))
    return (x / np.sqrt(np.maximum((x * x).sum(axis=1, keepdims=True), 1e-12))).astype(np.float32)


class MocoQueue:
    """The ring buffer of momentum keys of MoCo (He et al. 2020): a device fp32 [K, D] tensor of l2-normalised rows, exposed as ONE
    non-trainable Variable `moco/queue` (checkpointed with the target network; no optimizer slot, no weight decay, no gradient).
    enqueue(keys_all, step) overwrites the rows [ptr, ptr + 2N), ptr = moco_queue_ptr(step, 2N, K), with the gathered keys of the
    step in the NT-Xent gather layout (every replica's view-a rows, then every replica's view-b rows): one device-to-device slice copy
    on the step's stream."""

    NAME = 'moco/queue'

    def __init__(self, K, D, seed=0, device=None):
        K, D = int(K), int(D)
        if K < 1 or D < 1:
            raise ValueError('MocoQueue: need K >= 1 rows of width D >= 1 (got K = %d, D = %d)' % (K, D))
        self.K, self.D, self.seed = K, D, int(seed)
        self.variable = Variable(self.NAME, torch.empty(K, D, device=device or RT.device, dtype=torch.float32), False)
        self.reset()

    def reset(self):
        """Back to the seeded random unit rows."""
        self.variable.value.copy_(torch.from_numpy(moco_queue_init(self.K, self.D, self.seed)))

    @property
    def value(self):
        return self.variable.value

    @property
    def variables(self):
        return [self.variable]

    def ptr(self, step, rows):
        return moco_queue_ptr(step, rows, self.K)

    def enqueue(self, keys_all, step):
        rows = keys_all.shape[0]
        if keys_all.dim() != 2 or keys_all.shape[1] != self.D or keys_all.dtype != torch.float32:
            raise ValueError('MocoQueue.enqueue: need float32 keys [2N, %d] (got %s %s)' % (self.D, tuple(keys_all.shape), keys_all.dtype))
        if rows < 1 or self.K % rows:
            raise ValueError('MocoQueue.enqueue: the queue size %d is not a multiple of the %d rows of a step' % (self.K, rows))
        ptr = self.ptr(step, rows)
        self.variable.value[ptr:ptr + rows].copy_(keys_all)
        return ptr


class SupportQueue(MocoQueue):
    """The support set of NNCLR (--nn_queue_size): MocoQueue's ring under the variable name `nnclr/queue` -- a device fp32 [K, D]
    tensor of unit rows, seeded random directions at the start, not trainable (no optimizer slot, no weight decay, no gradient).
    enqueue(z_all[:N], step) overwrites the rows [ptr, ptr + N), ptr = moco_queue_ptr(step, N, K), with the view-a rows of the step's
    GLOBAL batch: every replica writes the same rows, so the queues stay bitwise equal without a collective."""

    NAME = 'nnclr/queue'

    def checkpointable(self, model):
        """The object run.main hands the checkpoint: the model's variables, then `nnclr/queue`."""
        return _WithSupport(model, self)


class _WithSupport:
    """What an NNCLR checkpoint holds: every variable of the model under its own name (the optimizer's slots hang on these very
    objects), then `nnclr/queue`.  Evaluation, --knn_eval and fine-tuning read such a file as a plain pretraining checkpoint: the one
    name they do not know is left unused."""

    def __init__(self, model, support):
        self.model, self.support = model, support
        self.supervised_head = model.supervised_head

    @property
    def variables(self):
        return self.model.variables + self.support.variables


class DinoCenter:
    """The centre of the DINO teacher (Caron et al. 2021, eq. 4): a device fp32 [K] vector, zeros at the start, exposed as ONE
    non-trainable Variable `dino/center` (checkpointed with the target network; no optimizer slot, no weight decay, no gradient) and
    identical on every replica: update() reads the GLOBAL mean of the normalised target projections.
    update(wt, kbar, momentum): c <- c + (1 - m) (wt . kbar - c) in one launch (ops.dino_center), with wt the normalised target
    prototypes THE FORWARD USED -- the caller runs it after the backward (which recomputes the teacher softmax from the centre)."""

    NAME = 'dino/center'

    def __init__(self, K, device=None):
        K = int(K)
        if K < 2:
            raise ValueError('DinoCenter: need K >= 2 prototypes (got %d)' % K)
        self.K = K
        self.variable = Variable(self.NAME, torch.zeros(K, device=device or RT.device, dtype=torch.float32), False)

    def reset(self):
        self.variable.value.zero_()

    @property
    def value(self):
        return self.variable.value

    @property
    def variables(self):
        return [self.variable]

    def update(self, wt, kbar, momentum):
        return ops.dino_center(wt, kbar, self.variable.value, momentum)


class _WithTarget:
    """What a BYOL / MoCo checkpoint holds: every variable of the online model under its own name (the optimizer's slots hang on these
    very objects), every target variable under the prefix `target/` and, with a queue attached, `moco/queue`."""

    def __init__(self, model, target):
        self.model, self.target = model, target
        self.supervised_head = model.supervised_head
        self._target_variables = [Variable(TargetNetwork.PREFIX + v.name, v.value, False) for v in target.model.variables]
        if target.queue is not None:
            self._target_variables += target.queue.variables
        if getattr(target, 'center', None) is not None:
            self._target_variables += target.center.variables

    @property
    def variables(self):
        return self.model.variables + self._target_variables


class TargetNetwork:
    """The momentum target network of BYOL: a second encoder and projection head (no supervised head, no predictor), built under
    `target_flag_values()` and RT.fresh_names() -- its variables carry the online names, the online model's names and initial values
    are those of a run without a target.  The whole model is `trainable = False`: nothing of it reaches trainable_variables, the flat
    gradient buffer, the optimizer's table or add_weight_decay.

    It is not frozen through fine_tune_after_block (Model.__call__ refuses that flag in pretraining): the layer switch alone makes
    every block release what it kept, and `stem_trainable = False` drops the stem's pooling tap ids.

    A call is a TRAINING-mode forward (batch statistics, SyncBN over the replicas, the target's own moving statistics move) on pixels
    the caller has blurred already; it returns the float32 [2b, D] projection output and keeps no activation.

    update(step) moves every trainable variable of the online encoder and projection head into its target namesake,
    t + (1 - tau_step) * (o - t), in one launch, and marks the target's compute copies stale: RT.optimizer_stepped() leaves frozen
    layers' copies alone, and these masters change every step.

    --contrastive_loss=mocov2 (MoCo v2) uses the same network: the online model then has no predictor, the decay is the constant
    --moco_momentum instead of BYOL's cosine schedule, and `queue` (a MocoQueue) is checkpointed with it."""

    PREFIX = 'target/'

    def __init__(self, online_model, total_steps, image_size=None, queue=None, center=None, steps_per_epoch=None):
        self.moco = moco_on()
        self.dino = dino_on()
        if online_model.prediction_head is None and not (self.moco or self.dino):
            raise ValueError('TargetNetwork: the online model has no predictor (it was built without --contrastive_loss=byol)')
        if self.dino and getattr(online_model, 'prototype_head', None) is None:
            raise ValueError('TargetNetwork: the online model has no prototype head (it was built without --contrastive_loss=dino)')
        if self.dino and (steps_per_epoch is None or int(steps_per_epoch) < 1):
            raise ValueError('TargetNetwork: --contrastive_loss=dino needs steps_per_epoch >= 1 (the teacher temperature and the '
                             'freeze of the prototypes count epochs)')
        self.queue = queue                    # model.MocoQueue (mocov2) or None: listed by checkpointable()
        self.center = center                  # model.DinoCenter (dino) or None: listed by checkpointable()
        self.steps_per_epoch = None if steps_per_epoch is None else int(steps_per_epoch)
        # mocov2: the constant --moco_momentum m; 1 - m is formed in double and cast to float32 once
        self._moco_omt = None
        if self.moco:
            import numpy as np
            self._moco_omt = float(np.float32(1.0 - float(FLAGS.moco_momentum)))
        self.online = online_model
        self.total_steps = max(int(total_steps), 1)
        self.flag_values = target_flag_values()
        size = image_size or FLAGS.image_size
        zeros = None
        if online_model.resnet_model.stem_conv.kernel is None:
            # variables exist only after the first forward pass (lazy build); inference mode: no statistic moves
            zeros = torch.zeros(2, size, size, 3, device=RT.device)
            online_model(zeros, training=False)
            online_model.release()
        if online_model.prediction_head is not None and online_model.prediction_head.linear_layers[0].kernel is None:
            # after the encoder, the projection head and the supervised head: their initial values are those of an ntxent run
            online_model.prediction_head(torch.zeros(2, projection_width(), device=RT.device), training=False)
            online_model.prediction_head.release()
        if self.dino and online_model.prototype_head.kernel is None:
            online_model.prototype_head.build(projection_width())       # last: every other initial value is that of an ntxent run
        with FLAGS.override(**self.flag_values), RT.fresh_names():
            self.model = Model(0)
            self.model.trainable = False
            self.model.resnet_model.stem_trainable = False
            self.model(zeros if zeros is not None else torch.zeros(2, size, size, 3, device=RT.device), training=False)
            self.model.release()
            if self.dino:
                self.model.prototype_head.build(projection_width())
        heads = [online_model._projection_head] + ([online_model.prototype_head] if self.dino else [])
        online = {v.name: v for v in online_model.resnet_model.variables + [v for h in heads for v in h.variables]}
        self._pairs = []                      # (target variable, online variable) by name, every variable of the target
        for v in self.model.variables:
            o = online.get(v.name)
            if o is None or o.shape != v.shape:
                raise ValueError('TargetNetwork: target variable %s has no online namesake of its shape' % v.name)
            self._pairs.append((v, o))
        trained = {id(v) for v in online_model.resnet_model.trainable_variables + [v for h in heads for v in h.trainable_variables]}
        self._ema_pairs = [(t, o) for t, o in self._pairs if id(o) in trained]
        self._tables = ops.EmaTables()
        self.copy_from_online()

    def copy_from_online(self):
        """Every target variable (moving statistics included) becomes a bitwise copy of its online namesake."""
        for t, o in self._pairs:
            t.value.copy_(o.value)
        self._invalidate()

    def _invalidate(self):
        for l in _all_layers(self.model):
            if '_version' in l.__dict__:
                l._frozen_key = None
                l._dtype = None

    @property
    def variables(self):
        return self.model.variables

    def checkpointable(self):
        """The object run.main hands the checkpoint: online variables + `target/`-prefixed target variables (+ `moco/queue` when a
        queue is attached)."""
        return _WithTarget(self.online, self)

    def tau(self, step):
        """BYOL's cosine schedule to 1, from --byol_tau_base or (dino) from --dino_momentum."""
        return byol_tau(step, self.total_steps, FLAGS.dino_momentum if self.dino else FLAGS.byol_tau_base)

    def prototypes(self):
        """dino: the row-normalised prototypes of the target network, float32 [K, D]; nothing is kept."""
        w = self.model.prototype_head()
        self.model.prototype_head.saved = None
        return w

    def update(self, step):
        """After optimizer.apply_gradients of step `step` (optimizer.iterations before its increment).  tau is formed on the host in
        double; 1 - tau is cast to float32 once.  The decay is chosen by the loss: BYOL's cosine schedule, or the constant
        --moco_momentum of mocov2."""
        import numpy as np
        omt = self._moco_omt if self.moco else float(np.float32(1.0 - self.tau(step)))
        self._tables.run([t.value for t, _ in self._ema_pairs], [o.value for _, o in self._ema_pairs], omt)
        self._invalidate()
        return omt

    def __call__(self, features):
        """features [b, H, W, 6] (blurred by the caller) -> float32 [2b, D] projection output of the target network."""
        with FLAGS.override(**self.flag_values):
            proj, _ = self.model(features, training=True, blur=False)
        self.model.release()
        return proj


def _all_layers(layer):
    out = [layer]
    for l in layer.sublayers():
        out.extend(_all_layers(l))
    return out
