"""The training step and driver -- mirror of /root/reference/tf2/run.py for the hot path.

`make_single_step` restates `single_step` (tf2/run.py:557-622) line for line on the HIP
kernels: model forward, contrastive + supervised losses, metrics, weight decay, loss / R,
backward (hand-written, replaces tape.gradient :621), cross-replica gradient SUM (implicit in
apply_gradients :614-622; here a bucketed RCCL all-reduce overlapped with the rest of the
backward pass), LARS.  `main` accepts the reference's flags (simclr_amd/flags.py) and mirrors the
driver (run.py:450-664): `--dataset=synthetic` feeds random two-view batches of the right shape,
any other `--dataset` is read from `--data_dir` in the array format of simclr_amd/data.py
(tfds / TFRecord readers and JPEG decode are out of scope, as is the SavedModel export).
"""
import json
import logging
import sys
import time
import types

import torch
import torch.distributed as dist

from . import data_util, metrics, ops
from . import model as model_lib
from . import objective as obj_lib
from . import pretrain_losses as loss_lib
from .comm import Strategy, collectives_on, num_replicas
from .flags import FLAGS, aug_plan, check_dropblock_flags, local_crop_flags
from .resnet import RT, join_wgrad_stream, set_dropblock_step


# One predicate (model.pretrain_loss) and one table (pretrain_losses.LOSSES) say which loss a pretraining run trains; the names below
# are that predicate spelt per loss.  train_mode=finetune has no contrastive loss and ignores --contrastive_loss.
def _loss_on(name):
    return lambda: model_lib.pretrain_loss() == name


generalized_loss_on, supcon_loss_on = _loss_on('generalized'), _loss_on('supcon')
barlow_loss_on, vicreg_loss_on = _loss_on('barlow'), _loss_on('vicreg')
# the model reads the same switches to decide which heads it carries
byol_loss_on, moco_loss_on, dino_loss_on, swav_loss_on = model_lib.byol_on, model_lib.moco_on, model_lib.dino_on, model_lib.swav_on
barlow_loss_width = model_lib.projection_width      # the width of the block every pretraining loss reads, under its first name


def swav_local_crops():
    """L of SwAV multi-crop in a pretraining run (0: off); train_mode=finetune and --mode=eval ignore the flags."""
    if FLAGS.train_mode != 'pretrain' or FLAGS.mode == 'eval':
        return 0
    return int(getattr(FLAGS, 'swav_local_crops', 0))


def check_swav_local_flags():
    """Raise before any device work when the multi-crop flags name something the step does not cover.  Returns L."""
    L = swav_local_crops()
    if not 0 <= L <= ops.SWAV_MAX_LOCAL_CROPS:
        raise ValueError('--swav_local_crops must lie in [0, %d] (got %r)' % (ops.SWAV_MAX_LOCAL_CROPS, FLAGS.swav_local_crops))
    if L == 0:
        return 0
    if FLAGS.contrastive_loss != 'swav':
        raise ValueError('--swav_local_crops belongs to --contrastive_loss=swav (got %r): multi-crop is built for SwAV only'
                         % FLAGS.contrastive_loss)
    size = FLAGS.swav_local_crop_size
    stride = 1 if FLAGS.image_size <= 32 else 2           # the stem's: resnet.Resnet.stem_kernel_stride
    if not 1 <= size <= FLAGS.image_size or size % stride:
        raise ValueError('--swav_local_crop_size must lie in [1, image_size = %d] and be a multiple of the stem stride %d (got %r)'
                         % (FLAGS.image_size, stride, size))
    lo, hi = FLAGS.swav_local_crop_min_scale, FLAGS.swav_local_crop_max_scale
    if not 0.0 < lo < hi <= 1.0:                          # (NaN fails the comparison)
        raise ValueError('the local crop scales need 0 < --swav_local_crop_min_scale < --swav_local_crop_max_scale <= 1 (got %r, %r)'
                         % (lo, hi))
    if any(p is not None for p in (check_dropblock_flags()[0] or [])):
        raise ValueError('--swav_local_crops with an active DropBlock is refused: the noise of a site is a function of (seed, step, '
                         'replica, site) and would repeat in the second encoder pass')
    return L


def dino_local_crops():
    """L of DINO multi-crop in a pretraining run (0: off); train_mode=finetune and --mode=eval ignore the flags."""
    if FLAGS.train_mode != 'pretrain' or FLAGS.mode == 'eval':
        return 0
    return int(getattr(FLAGS, 'dino_local_crops', 0))


def check_dino_local_flags():
    """check_swav_local_flags for the --dino_local_crop* flags.  Returns L."""
    L = dino_local_crops()
    if not 0 <= L <= ops.DINO_MAX_LOCAL_CROPS:
        raise ValueError('--dino_local_crops must lie in [0, %d] (got %r)' % (ops.DINO_MAX_LOCAL_CROPS, FLAGS.dino_local_crops))
    if L == 0:
        return 0
    if FLAGS.contrastive_loss != 'dino':
        raise ValueError('--dino_local_crops belongs to --contrastive_loss=dino (got %r); SwAV has --swav_local_crops, no other loss '
                         'has multi-crop' % FLAGS.contrastive_loss)
    size = FLAGS.dino_local_crop_size
    stride = 1 if FLAGS.image_size <= 32 else 2           # the stem's: resnet.Resnet.stem_kernel_stride
    if not 1 <= size <= FLAGS.image_size or size % stride:
        raise ValueError('--dino_local_crop_size must lie in [1, image_size = %d] and be a multiple of the stem stride %d (got %r)'
                         % (FLAGS.image_size, stride, size))
    lo, hi = FLAGS.dino_local_crop_min_scale, FLAGS.dino_local_crop_max_scale
    if not 0.0 < lo < hi <= 1.0:                          # (NaN fails the comparison)
        raise ValueError('the local crop scales need 0 < --dino_local_crop_min_scale < --dino_local_crop_max_scale <= 1 (got %r, %r)'
                         % (lo, hi))
    if any(p is not None for p in (check_dropblock_flags()[0] or [])):
        raise ValueError('--dino_local_crops with an active DropBlock is refused: the noise of a site is a function of (seed, step, '
                         'replica, site) and would repeat in the second encoder pass')
    return L


def local_crop_plan():
    """(L, size, min_scale, max_scale) of the active multi-crop: the --swav_local_crop* flags under --contrastive_loss=swav, the
    --dino_local_crop* flags under dino, L = 0 under every other loss, in fine-tuning and in --mode=eval."""
    L, size, lo, hi = local_crop_flags()
    if FLAGS.train_mode != 'pretrain' or FLAGS.mode == 'eval':
        L = 0
    return L, size, lo, hi


def check_contrastive_loss_flags():
    """Raise before any device work when the pretraining loss flags name something the kernels do not cover: the multi-crop flags,
    the loss name, then --hard_negative_beta / --debiased_tau_plus, --nn_queue_size and the check of that loss's row of
    pretrain_losses.LOSSES (a pretraining run outside --mode=eval only).
    Returns True for the generalized loss in such a run, False otherwise (model.pretrain_loss() tells the others)."""
    check_swav_local_flags()
    check_dino_local_flags()
    if FLAGS.contrastive_loss not in loss_lib.LOSSES:
        raise ValueError("--contrastive_loss must be 'dino' or 'ntxent' or 'generalized' or 'supcon' or 'barlow' or 'byol' or 'mocov2' (got %r), "
                         "or 'swav' or 'vicreg'" % FLAGS.contrastive_loss)
    spec = loss_lib.active()
    if spec is None or FLAGS.mode == 'eval':
        return False
    loss_lib.check_ntxent_corrections()
    loss_lib.check_nn_positives()
    if spec.check is not None:
        spec.check()
    return spec is loss_lib.LOSSES['generalized']


def repr_metrics_steps():
    """K of --repr_metrics_steps in a pretraining run (0: off); train_mode=finetune and --mode=eval ignore the flag.  The one reader of
    the flag: check_repr_flags and build_metrics call it."""
    if FLAGS.train_mode != 'pretrain' or FLAGS.mode == 'eval':
        return None
    return FLAGS.repr_metrics_steps


def check_repr_flags():
    """--repr_metrics_steps / --repr_uniform_t (metrics.representation_stats), checked before any device work.  Returns K."""
    K = repr_metrics_steps()
    if K is None:
        return 0
    if K < 0:
        raise ValueError('--repr_metrics_steps must be >= 0 (got %r): 0 is off, K measures every K-th step' % (K,))
    if not ops.repr_t_ok(FLAGS.repr_uniform_t):
        raise ValueError('--repr_uniform_t must lie in (0, %g] (got %r)' % (ops.REPR_MAX_T, FLAGS.repr_uniform_t))
    if K > 0:
        width = model_lib.projection_width()
        if not ops.repr_dim_ok(width):
            raise ValueError('--repr_metrics_steps=%d needs a loss width that is a multiple of %d in [%d, %d] (got %d from '
                             'proj_head_mode=%r, proj_out_dim=%d): the diagnostics kernels take those widths only'
                             % (K, ops.REPR_DIM_STEP, ops.REPR_MIN_DIM, ops.REPR_MAX_DIM, width, FLAGS.proj_head_mode, FLAGS.proj_out_dim))
        if not ops.REPR_MIN_ROWS <= FLAGS.train_batch_size <= ops.REPR_MAX_ROWS:
            raise ValueError('--repr_metrics_steps=%d needs %d <= --train_batch_size <= %d (got %r): the pairwise terms run over the '
                             'global batch' % (K, ops.REPR_MIN_ROWS, ops.REPR_MAX_ROWS, FLAGS.train_batch_size))
    return int(K)


def build_metrics():
    """The metric set of tf2/run.py:534-549; the pretraining names are those of the loss's row of pretrain_losses.LOSSES, and with
    --repr_metrics_steps > 0 the four of metrics.REPR_METRICS."""
    names = ['train/weight_decay', 'train/total_loss']
    spec = loss_lib.active()
    if spec is not None:
        names += [n for n, _ in spec.metrics + spec.logits_metrics]
        if (repr_metrics_steps() or 0) > 0:
            names += [n for n, _ in metrics.REPR_METRICS]
    if FLAGS.train_mode == 'finetune' and getattr(FLAGS, 'teacher_checkpoint', None):
        names += ['train/distill_loss', 'train/distill_agreement']       # distillation: the teacher replaces the labels
    elif FLAGS.train_mode == 'finetune' or FLAGS.lineareval_while_pretraining:
        names += ['train/supervised_loss', 'train/supervised_acc']
    return {n: metrics.Mean(n) for n in names}


class GradSync:
    """Collective B: SUM of every trainable gradient across replicas (tf2/run.py:614-622).

    Gradients live in ONE flat fp32 buffer ordered last-layer-first, cut into buckets at block
    group boundaries; each bucket's all-reduce is issued asynchronously as soon as the backward
    pass has produced it, so xGMI traffic overlaps the remaining dgrad/wgrad kernels.  Frozen
    block groups (finetune, fine_tune_after_block) have no gradients and no bucket; buckets the
    backward pass never announced (the whole encoder frozen) are issued by `wait`."""

    def __init__(self, model, strategy):
        self.strategy = strategy
        self.flat = model._flat_grads
        order, offs = model._flat_order, model._flat_offsets
        cuts = [0]
        self.stage_to_bucket = {}
        for g in (4, 3, 2, 1):                # a bucket ends where a (trainable) block group ends
            mk = 'block_group%d' % g
            idx = [i for i, v in enumerate(order) if mk in v.name]
            if not idx:
                continue
            last = idx[-1]
            end = offs[last + 1] if last + 1 < len(order) else self.flat.numel()
            self.stage_to_bucket[g] = len(cuts) - 1
            cuts.append(end)
        self._groups = len(cuts) - 1
        cuts.append(self.flat.numel())
        self.ranges = [(a, b) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
        self.works = []
        self.issued = set()

    def on_stage(self, stage):
        """Called by the backward pass after block group `stage` (4..1) is done; 0 = stem done."""
        if not collectives_on(self.strategy):
            return
        join_wgrad_stream()          # this bucket's weight gradients may still be running on the side stream
        if stage == 0:
            idx = len(self.ranges) - 1 if len(self.ranges) > self._groups else None
        else:
            idx = self.stage_to_bucket.get(stage)
        if idx is None or idx >= len(self.ranges):
            return
        self._issue(idx)

    def _issue(self, idx):
        a, b = self.ranges[idx]
        self.issued.add(idx)
        self.works.append(dist.all_reduce(self.flat[a:b], op=dist.ReduceOp.SUM,
                                          group=getattr(self.strategy, 'grad_group', self.strategy.group), async_op=True))

    def wait(self):
        if collectives_on(self.strategy):
            for idx in range(len(self.ranges)):
                if idx not in self.issued:
                    self._issue(idx)
        self.issued = set()
        for w in self.works:
            w.wait()
        self.works = []


def check_distillation_flags():
    """A teacher needs the fine-tuning path: raise before any device work otherwise.  --mode=eval ignores the teacher flags."""
    if FLAGS.teacher_checkpoint and FLAGS.mode != 'eval':
        if FLAGS.train_mode != 'finetune':
            raise ValueError('--teacher_checkpoint distils into the fine-tuning path: it requires --train_mode=finetune (got %r)'
                             % FLAGS.train_mode)
        if not FLAGS.distill_temperature > 0:
            raise ValueError('--distill_temperature must be positive (got %r)' % FLAGS.distill_temperature)
        return True
    return False


SYNTHETIC_KNN_BANK_BATCHES = 8     # --dataset=synthetic: eval batches in the k-NN bank (plumbing only; every batch distinct)


def check_knn_flags(num_train_examples=None):
    """--knn_eval (simclr_amd/knn.py), checked before any device work.  Returns the number of bank examples (None with the flag off, or
    when the size of --train_split is not known yet)."""
    if not FLAGS.knn_eval:
        return None
    if not 1 <= FLAGS.knn_k <= ops.KNN_MAX_K:
        raise ValueError('--knn_k must be 1..%d (got %d): the top-k kernel sorts a query\'s candidates in LDS' % (ops.KNN_MAX_K, FLAGS.knn_k))
    if not FLAGS.knn_temperature > 0:
        raise ValueError('--knn_temperature must be > 0 (got %r)' % (FLAGS.knn_temperature,))
    if FLAGS.knn_bank_examples < 0:
        raise ValueError('--knn_bank_examples must be >= 0 (got %d)' % FLAGS.knn_bank_examples)
    if num_train_examples is None:
        bank = FLAGS.knn_bank_examples or None
    else:
        if FLAGS.knn_bank_examples > num_train_examples:
            raise ValueError('--knn_bank_examples=%d exceeds the %d examples of --train_split=%s'
                             % (FLAGS.knn_bank_examples, num_train_examples, FLAGS.train_split))
        bank = FLAGS.knn_bank_examples or int(num_train_examples)
    if bank is not None and bank < FLAGS.knn_k:
        raise ValueError('the k-NN bank would hold %d examples, fewer than --knn_k=%d' % (bank, FLAGS.knn_k))
    return bank


def check_logreg_flags(num_train_examples=None):
    """--logreg_eval (simclr_amd/logreg.py), checked before any device work.  Returns the number of bank examples (None with the flag
    off, in --mode=train, or for the whole split when its size is not known yet)."""
    if not FLAGS.logreg_eval or FLAGS.mode == 'train':
        return None
    from . import logreg as logreg_lib
    for l2 in logreg_lib.parse_l2_list(FLAGS.logreg_l2):
        logreg_lib.check_fit_arguments(l2, FLAGS.logreg_max_iterations, FLAGS.logreg_tolerance, FLAGS.logreg_history)
    if FLAGS.logreg_bank_examples < 0:
        raise ValueError('--logreg_bank_examples must be >= 0 (got %d)' % FLAGS.logreg_bank_examples)
    width = (512 if FLAGS.resnet_depth in (18, 34) else 2048) * FLAGS.width_multiplier
    if not ops.logreg_dim_ok(width):
        raise ValueError('--logreg_eval needs an encoder width that is a multiple of %d in [%d, %d] (resnet_depth=%d, width_multiplier=%d '
                         'give %d)' % (ops.LOGREG_DIM_STEP, ops.LOGREG_MIN_DIM, ops.LOGREG_MAX_DIM, FLAGS.resnet_depth,
                                       FLAGS.width_multiplier, width))
    if num_train_examples is None:
        return FLAGS.logreg_bank_examples or None
    if FLAGS.logreg_bank_examples > num_train_examples:
        raise ValueError('--logreg_bank_examples=%d exceeds the %d examples of --train_split=%s'
                         % (FLAGS.logreg_bank_examples, num_train_examples, FLAGS.train_split))
    return FLAGS.logreg_bank_examples or int(num_train_examples)


def check_logreg_classes(num_classes):
    if FLAGS.logreg_eval and FLAGS.mode != 'train' and not ops.LOGREG_MIN_CLASSES <= num_classes <= ops.LOGREG_MAX_CLASSES:
        raise ValueError('--logreg_eval takes %d..%d classes (the dataset has %d)' % (ops.LOGREG_MIN_CLASSES, ops.LOGREG_MAX_CLASSES, num_classes))


def check_kmeans_flags(num_train_examples=None, num_classes=None):
    """--kmeans_eval (simclr_amd/kmeans.py), checked before any device work.  Returns the number of bank examples (None with the flag
    off, in --mode=train, or for the whole split when its size is not known yet).  K = --kmeans_k, or the class count once it is
    known."""
    if not FLAGS.kmeans_eval or FLAGS.mode == 'train':
        return None
    from . import kmeans as kmeans_lib
    K = int(FLAGS.kmeans_k) or num_classes
    if FLAGS.kmeans_k < 0 or (K is not None and not ops.KMEANS_MIN_K <= K <= ops.KMEANS_MAX_K):
        raise ValueError('--kmeans_k must be 0 (the class count) or %d..%d (got %d%s)'
                         % (ops.KMEANS_MIN_K, ops.KMEANS_MAX_K, FLAGS.kmeans_k, '' if FLAGS.kmeans_k else '; the dataset has %r classes' % K))
    kmeans_lib.check_fit_arguments(K or ops.KMEANS_MIN_K, FLAGS.kmeans_seed, FLAGS.kmeans_restarts, FLAGS.kmeans_max_iterations,
                                   FLAGS.kmeans_tolerance)
    if FLAGS.kmeans_bank_examples < 0:
        raise ValueError('--kmeans_bank_examples must be >= 0 (got %d)' % FLAGS.kmeans_bank_examples)
    width = (512 if FLAGS.resnet_depth in (18, 34) else 2048) * FLAGS.width_multiplier
    if not ops.kmeans_dim_ok(width):
        raise ValueError('--kmeans_eval needs an encoder width that is a multiple of %d in [%d, %d] (resnet_depth=%d, width_multiplier=%d '
                         'give %d)' % (ops.KMEANS_DIM_STEP, ops.KMEANS_MIN_DIM, ops.KMEANS_MAX_DIM, FLAGS.resnet_depth,
                                       FLAGS.width_multiplier, width))
    if num_train_examples is None:
        bank = FLAGS.kmeans_bank_examples or None
    else:
        if FLAGS.kmeans_bank_examples > num_train_examples:
            raise ValueError('--kmeans_bank_examples=%d exceeds the %d examples of --train_split=%s'
                             % (FLAGS.kmeans_bank_examples, num_train_examples, FLAGS.train_split))
        bank = FLAGS.kmeans_bank_examples or int(num_train_examples)
    if bank is not None and K is not None and K > bank:
        raise ValueError('--kmeans_k: %d clusters exceed the %d bank examples (--kmeans_bank_examples)' % (K, bank))
    return bank


def check_spectrum_flags(num_train_examples=None):
    """--spectrum_eval (simclr_amd/spectrum.py), checked before any device work.  Returns the number of bank examples (None with the flag
    off, in --mode=train, or for the whole split when its size is not known yet)."""
    if not FLAGS.spectrum_eval or FLAGS.mode == 'train':
        return None
    from . import spectrum as spectrum_lib
    spectrum_lib.check_score_arguments(FLAGS.spectrum_rank_threshold, FLAGS.spectrum_alpha_first, FLAGS.spectrum_alpha_last)
    if FLAGS.spectrum_bank_examples < 0:
        raise ValueError('--spectrum_bank_examples must be >= 0 (got %d)' % FLAGS.spectrum_bank_examples)
    width = (512 if FLAGS.resnet_depth in (18, 34) else 2048) * FLAGS.width_multiplier
    if not ops.spectrum_dim_ok(width):
        raise ValueError('--spectrum_eval needs an encoder width that is a multiple of %d in [%d, %d] (resnet_depth=%d, width_multiplier=%d '
                         'give %d)' % (ops.SPECTRUM_DIM_STEP, ops.SPECTRUM_MIN_DIM, ops.SPECTRUM_MAX_DIM, FLAGS.resnet_depth,
                                       FLAGS.width_multiplier, width))
    if num_train_examples is None:
        bank = FLAGS.spectrum_bank_examples or None
    else:
        if FLAGS.spectrum_bank_examples > num_train_examples:
            raise ValueError('--spectrum_bank_examples=%d exceeds the %d examples of --train_split=%s'
                             % (FLAGS.spectrum_bank_examples, num_train_examples, FLAGS.train_split))
        bank = FLAGS.spectrum_bank_examples or int(num_train_examples)
    if bank is not None and bank < 2:
        raise ValueError('--spectrum_bank_examples: a covariance needs at least 2 bank examples (got %d)' % bank)
    return bank


def all_reduce_stats_async(tensor, strategy):
    """SUM of a small statistics tensor over the replicas on the route the SyncBN sums and the Barlow Twins column sums use, started
    now; returns a zero-argument function that waits for it and returns the tensor.  One replica: nothing to do."""
    if not collectives_on(strategy):
        return lambda: tensor
    if strategy.peer_stats is not None and strategy.peer_stats.usable(tensor):
        strategy.all_reduce_sum(tensor)            # the peer-mapped exchange is stream-ordered: the host does not wait
        return lambda: tensor
    strategy.stat_collectives += 1
    work = dist.all_reduce(tensor, op=dist.ReduceOp.SUM, group=strategy.stat_group, async_op=True)

    def wait():
        work.wait()
        return tensor
    return wait


def make_single_step(model, optimizer, strategy, all_metrics=None, teacher=None, target=None, steps_per_epoch=None, support=None):
    """Returns single_step(features, labels) -- tf2/run.py:557-622.
    A pretraining step trains the row of pretrain_losses.LOSSES that model.pretrain_loss() names: the row's `call` makes the loss, its
    (metric name, attribute) pairs are logged and re-pointed by one loop each; the phases that differ between losses (below) are
    explicit code in the step, keyed on what the loss uses: a target, a queue, a centre, prototypes that can be frozen.
    target: model.TargetNetwork (or a stand-in with its __call__ / update), required by --contrastive_loss=byol.  The step is then:
    blur once, target forward (training mode, nothing kept), online forward on the same pixels, predictor, add_byol_loss, the usual
    backward entering through the predictor, optimizer, target.update(step).
    --contrastive_loss=mocov2 needs a target with a model.MocoQueue attached (target.queue).  The step is: blur once, target forward
    and release, normalise the keys and start their asynchronous all-gather (nothing in the loss waits for it), online forward,
    add_moco_loss against the queue, backward, optimizer, target.update(step), then wait for the gather and queue.enqueue.
    --contrastive_loss=dino needs a target with a model.DinoCenter attached (target.center) and its steps_per_epoch.  The step is: blur
    once, target forward and release, normalise the keys and start the asynchronous all-reduce of their mean, online forward, normalise
    both prototype tables, add_dino_loss, backward (loss kernels, the normalisations, the heads, the encoder), gradient synchronisation,
    optimizer (without the prototypes while they are frozen), target.update(step), THEN wait for the mean and move the centre.
    --contrastive_loss=swav needs no target (passing one is refused) and steps_per_epoch >= 1, which the freeze of the prototypes counts.
    support: model.SupportQueue, required while --nn_queue_size is nonzero in an NT-Xent pretraining run and refused otherwise.  The
    step is then: online forward, normalise and gather, the exact top-1 search of the local rows in the queue AS IT STANDS,
    add_nn_contrastive_loss, backward, optimizer, then support.enqueue of the global batch's view-a rows.
    The step is the NT-Xent step with add_swav_loss in place of the loss: online forward, normalise the rows and the prototypes, gather
    the normalised block, the Sinkhorn on it, the loss on the local rows, backward, gradient synchronisation, optimizer (without the
    prototypes while they are frozen).
    --swav_local_crops=L > 0 (multi-crop): features = (globals [b, H, W, 6], locals [b, h, h, 3L]).  The layers keep the activations of
    ONE pending forward, so the step has two passes: pass A is the swav step on the global views up to model.backward with
    grad_scale 1 / (R (V - 1)), V = 2 + L (the supervised head trains here only); the flat gradient buffer is saved and zeroed; pass B
    blurs the local views at their own size, forwards them in training mode (BatchNorm on statistics of its own), add_swav_local_loss
    against pass A's codes, backward without the supervised head; the saved buffer is added back, the gradients are all-reduced ONCE
    (after the add: the sum is linear, one reduction is cheaper than two), then one optimizer step.
    --repr_metrics_steps=K > 0: a step with (step + 1) % K == 0 is measured.  Right after the online forward the projection is
    normalised into a tensor of its own and its gather starts; after the loss call metrics.representation_stats' kernels run on the
    gathered block.  Read-only: nothing the step reads is written, and the weights are bitwise those of K = 0.  The four values go
    through the metric bank on measured steps only, and the handle is returned under `repr_stats` (None on other steps).
    --dino_local_crops=L > 0: the same two passes under --contrastive_loss=dino, pass B's loss being add_dino_local_loss against pass
    A's teacher rows.  The teacher sees the global views only: the target forward, the keys, their mean and the centre are pass A's.
    target.update(step), the wait for the mean and the centre update stay after the optimizer step, that is after pass B, whose
    backward reads the centre, the keys and the target prototypes again.  train/dino_teacher_entropy is pass A's.
    teacher: a callable features -> SupLogits (model.Teacher, or a stub).  The step is then the fine-tuning step with the supervised
    loss replaced by add_kd_loss(student logits, teacher(features), FLAGS.distill_temperature) -- the self-training step of
    tf2/colabs/distillation_self_training.ipynb:908-919; labels are not read."""
    if teacher is not None and FLAGS.train_mode != 'finetune':
        raise ValueError('a distillation teacher requires train_mode=finetune (got %r)' % FLAGS.train_mode)
    if all_metrics is not None:
        m = all_metrics
    elif teacher is not None:
        m = {n: metrics.Mean(n) for n in ('train/weight_decay', 'train/total_loss', 'train/distill_loss', 'train/distill_agreement')}
    else:
        m = build_metrics()
    state = {'sync': None}
    RT.strategy = strategy
    check_contrastive_loss_flags()
    name = model_lib.pretrain_loss()          # None: fine-tuning, no contrastive loss
    spec = loss_lib.active()
    if name == 'swav' and (steps_per_epoch is None or int(steps_per_epoch) < 1):
        raise ValueError('--contrastive_loss=swav needs steps_per_epoch >= 1 (the freeze of the prototypes counts epochs): '
                         'make_single_step(..., steps_per_epoch=n)')
    if spec is not None and spec.check_target is not None:
        spec.check_target(target)
    elif target is not None:
        raise ValueError('a target network belongs to the BYOL pretraining step (got contrastive_loss=%r, train_mode=%r)'
                         % (FLAGS.contrastive_loss, FLAGS.train_mode))
    nn_positives = loss_lib.nn_positives_on()
    if nn_positives and (support is None or getattr(support, 'enqueue', None) is None):
        raise ValueError('--nn_queue_size=%d needs a support queue: make_single_step(..., support=model.SupportQueue(K, D, seed))'
                         % FLAGS.nn_queue_size)
    if not nn_positives and support is not None:
        raise ValueError('a support queue belongs to the NT-Xent pretraining step under a nonzero --nn_queue_size (got '
                         'contrastive_loss=%r, train_mode=%r, nn_queue_size=%r)'
                         % (FLAGS.contrastive_loss, FLAGS.train_mode, FLAGS.nn_queue_size))
    dropblock = any(p is not None for p in (check_dropblock_flags()[0] or []))
    local_crops = local_crop_plan()[0]
    aug_plan()                                # (raises for malformed augmentation flags; the steps resolve the plan as they read it)
    repr_every = check_repr_flags() if spec is not None else 0

    def single_step(features, labels):
        # optimizer.iterations is a host int that apply_gradients increments: every "before the increment" read of the step is this
        # value, and a restored run continues what derives from it (DropBlock noise, SWD draws, temperatures, freezes, tau, queue row)
        step = int(getattr(optimizer, 'iterations', 0))
        local_features = None
        if local_crops:
            features, local_features = features
            if local_features.dim() != 4 or local_features.shape[3] != 3 * local_crops or local_features.shape[0] != features.shape[0]:
                raise ValueError('--%s_local_crops=%d: the step reads (globals [b, H, W, 6], locals [b, h, h, %d]) (got locals %s)'
                                 % (name, local_crops, 3 * local_crops, tuple(local_features.shape)))
        ops.begin_step(features.device)
        if dropblock:
            # the noise of a DropBlock site is a function of (dropblock_seed, global step, replica, site): the restored step continues it
            set_dropblock_step(step)
        teacher_logits = None
        if teacher is not None:
            # the frozen teacher's inference forward (it selects its own arithmetic); the student's forward below selects the
            # training arithmetic again, for the rest of the step
            teacher_logits = teacher(features)
        c = types.SimpleNamespace(model=model, target=target, strategy=strategy, steps_per_epoch=steps_per_epoch, step=step,
                                  labels=labels, target_outputs=None, keys=None, frozen=False, logits_con=None, support=support)
        if target is not None:
            # one draw of the random blur (and of the plan's solarization) for both networks (Model.__call__ would draw its own
            # inside each): view a stays channels 0:3 -- rows [0, b) of both projections
            features = data_util.apply_view_plan(features, aug_plan(), height=FLAGS.image_size)
            c.target_outputs = target(features)        # released before the online forward: the two activation sets never coexist
            if name == 'mocov2':
                # the keys of this step, and their gather for the enqueue at the END of the step: in flight during the online forward,
                # the loss and the whole backward -- the loss reads the local keys and the queue as it stands
                c.keys, _ = ops.l2norm_fwd(c.target_outputs.contiguous())
                moco_gather = obj_lib.gather_hidden(c.keys, strategy, async_op=True)
            if name == 'dino':
                # the mean of this step's keys over the GLOBAL batch -- the one vector the centre update at the END of the step needs:
                # formed in double in a fixed order, its all-reduce in flight during the online forward, the loss and the backward
                c.keys, _ = ops.l2norm_fwd(c.target_outputs.contiguous())
                dino_kbar = ops.dino_key_mean(c.keys, c.keys.shape[0] * num_replicas(strategy))
                dino_kbar_wait = all_reduce_stats_async(dino_kbar, strategy)
            projection_head_outputs, supervised_head_outputs = model(features, training=True, blur=False)
        else:
            projection_head_outputs, supervised_head_outputs = model(features, training=True)   # :577-578
        R = num_replicas(strategy)
        con_loss = sup_loss = None
        sup_box = {}
        # the label-free diagnostics of a measured step: the online projection (before the predictor under byol, the online side under
        # mocov2 / dino, pass A's global views under multi-crop); the gather is in flight during the loss
        repr_finish = repr_handle = None
        if repr_every and (step + 1) % repr_every == 0 and projection_head_outputs is not None:
            repr_finish = metrics.start_representation_stats(projection_head_outputs, strategy, FLAGS.repr_uniform_t)

        def supervised_part():
            if teacher_logits is not None:
                sup_box['loss'] = obj_lib.add_kd_loss(supervised_head_outputs, teacher_logits, FLAGS.distill_temperature)
            elif supervised_head_outputs is not None:
                l = labels['labels'] if isinstance(labels, dict) else labels
                # pretraining: labels are reused for both views (tf2/run.py:599-600: l = concat([l, l], 0)); finetune: one view
                sup_box['loss'] = obj_lib.add_supervised_loss(labels=l, logits=supervised_head_outputs)   # :601
        if projection_head_outputs is not None:
            # collective A (all-gather of the hidden block) is in flight while the supervised loss is computed
            c.outputs, c.overlap = projection_head_outputs, supervised_part
            if spec.frozen is not None:
                c.frozen = spec.frozen(c)
            con_loss = spec.call(c)
        else:
            supervised_part()
        if repr_finish is not None:
            repr_handle = repr_finish()
        sup_loss = sup_box.get('loss')
        weight_decay = model_lib.add_weight_decay(model, adjust_per_optimizer=True)         # :609-610

        # ---- backward of (loss / R): tf2/run.py:617-621 ----
        if model._flat_grads is None:
            model.allocate_flat_grads()
            state['sync'] = GradSync(model, strategy)
            # finetune: variables no path connects to the loss get no gradient -- tape.gradient returns None and apply_gradients
            # drops the pair, so they stay bitwise unchanged; with momentum / Adam the L2 term of add_weight_decay (tf2/model.py:62-69)
            # still gives their non-BatchNorm kernels the gradient wd * w, which the update kernel adds
            lars = isinstance(optimizer, model_lib.lars_optimizer.LARSOptimizer)
            skip = {id(v) for v in model.variables_without_gradient()
                    if lars or not getattr(optimizer, '_takes_l2', lambda n: False)(v.name)}
            state['apply'] = [v for v in model._flat_order if id(v) not in skip]
        sync = state['sync']
        model._wd_grad_scale = 1.0 / R
        # NT-Xent backward launches the reduce-scatter of the key-side gradient (transpose of collective A); the
        # supervised head's backward (independent: stop_gradient, tf2/model.py:276-277) runs while it is in flight
        # multi-crop: the global views carry 1 / (V - 1) of the loss, and the one gradient all-reduce comes after pass B
        share = 1.0 / (1 + local_crops)
        on_stage = sync.on_stage if not local_crops else None
        if con_loss is not None:
            con_loss.backward_start(share / R)
        d_sup = sup_loss.backward() if sup_loss is not None else None
        if FLAGS.train_mode == 'finetune':
            # no stop_gradient: supervised head -> projection head below ft_proj_selector -> trainable encoder layers
            model.backward(None, d_sup, on_stage=sync.on_stage)
        else:
            model.backward_supervised(d_sup)
            d_proj = con_loss.backward_finish() if con_loss is not None else None
            if name == 'byol':
                d_proj = model.backward_predictor(d_proj)
            model.backward(d_proj, None, on_stage=on_stage)
        join_wgrad_stream()
        if local_crops:
            # ---- pass B: the local views through the encoder a second time, against the codes of pass A ----
            # Every weight-gradient launch OVERWRITES its slot (the flat buffer is never cleared between steps), so pass A's gradients
            # are set aside; the buffer is zeroed because pass B writes no supervised-head (and no frozen-prototype) slot
            saved_grads = model._flat_grads.clone()
            model._flat_grads.zero_()
            # Model.__call__ blurs at FLAGS.image_size: the local views are blurred here, at their own size (probability 0.5 and no
            # solarization under every recipe)
            local_features = data_util.apply_view_plan(local_features, aug_plan(), local=True)
            local_outputs, _ = model(local_features, training=True, blur=False, supervised=False)
            global_loss = con_loss
            if name == 'dino':
                # the teacher rows are pass A's (the global keys, the target prototypes and the centre as they stand: all three move
                # only after the optimizer step below); frozen last layer: pass B writes no prototype gradient either
                local_loss = obj_lib.add_dino_local_loss(local_outputs, global_loss, model.prototype_head, strategy=strategy,
                                                         update_prototypes=not c.frozen)
            else:
                local_loss = obj_lib.add_swav_local_loss(local_outputs, global_loss, model.prototype_head,
                                                         temperature=FLAGS.swav_temperature, strategy=strategy,
                                                         update_prototypes=not c.frozen)
            model.backward(local_loss.backward(1.0 / R), None, on_stage=None)
            join_wgrad_stream()
            ops.axpy_f32(1.0, saved_grads, model._flat_grads)
            # train/contrast_loss is the total: global / (V - 1) + local
            total_con = torch.empty(1, device=features.device, dtype=torch.float32)
            ops.accumulate_scalars([global_loss.value.reshape(-1)[:1], local_loss.value.reshape(-1)[:1]], scales=[share, 1.0],
                                   total=total_con, total_mask=3)
            con_loss = obj_lib._Loss(total_con, None)
            con_loss.entropy = global_loss.entropy                                 # pass A's: the teacher / the codes see the globals only
            if name == 'dino':
                con_loss.keys, con_loss.target_prototypes = global_loss.keys, global_loss.target_prototypes
            else:
                con_loss.alpha = global_loss.alpha
            con_loss.global_loss, con_loss.local_loss = global_loss, local_loss
        sync.wait()
        if c.frozen:
            # the frozen prototypes take no update at all -- no gradient, no weight decay, no momentum: the pair is dropped, as
            # apply_gradients drops a variable without a gradient.  Online and target copies stay bitwise what they are.
            frozen_id = id(model.prototype_head.kernel)
            optimizer.apply_gradients([(v.grad, v) for v in state['apply'] if id(v) != frozen_id])
        else:
            optimizer.apply_gradients([(v.grad, v) for v in state['apply']])               # :622
        if target is not None:
            target.update(step)
        if name == 'mocov2':
            # The enqueue comes AFTER the backward: the backward recomputes the logits from the queue, and a queue that already held
            # this step's keys would silently differentiate another loss (every query would find its own positive among the negatives).
            target.queue.enqueue(moco_gather(), step)
        if nn_positives:
            # The enqueue comes AFTER the backward, which recomputes the logits from the neighbour rows it gathered (a copy: the queue
            # itself is not re-read), and after the search of this step: a row never finds itself.  Every replica writes the same N rows.
            support.enqueue(con_loss.gathered[:con_loss.gathered.shape[0] // 2], step)
        if name == 'dino':
            # The centre moves AFTER the backward, which recomputes the teacher softmax from it (moved earlier, the step would
            # differentiate another loss in silence), and it reads the target prototypes the FORWARD used, not the ones update() left.
            target.center.update(con_loss.target_prototypes, dino_kbar_wait(), FLAGS.dino_center_momentum)
        RT.optimizer_stepped()
        ops.end_step()
        if strategy is not None:
            strategy.check_health()          # a timed-out statistics exchange of an earlier step raises here (no device sync)

        # ---- metrics (device scalars, no sync): tf2/run.py:587-613 -- update_pretrain_metrics_train,
        # update_finetune_metrics_train, weight_decay and total_loss = the sum of the loss terms, in two launches:
        # total first, then every running sum (metrics.Mean.attach / bump)
        if state.get('bank') is None or state['bank'].device != features.device:
            state['bank'] = torch.zeros(16, device=features.device, dtype=torch.float32)
            state['zero'] = torch.zeros(1, device=features.device, dtype=torch.float32)
            for i, nm in enumerate(sorted(m)):
                m[nm].attach(state['bank'], i)
        order = sorted(m)
        wd_t = weight_decay.reshape(-1)[:1] if torch.is_tensor(weight_decay) else state['zero']
        total = torch.empty(1, device=features.device, dtype=torch.float32)
        terms = [wd_t] + ([con_loss.value.reshape(-1)[:1]] if con_loss is not None else []) + \
                ([sup_loss.value.reshape(-1)[:1]] if sup_loss is not None else [])
        ops.accumulate_scalars(terms, total=total, total_mask=(1 << len(terms)) - 1)
        vals = {'train/weight_decay': wd_t, 'train/total_loss': total}
        # the (metric name, attribute) pairs of the loss's row of pretrain_losses.LOSSES, read from the loss handle and (NT-Xent) the logits
        pairs = spec.metrics if con_loss is not None else ()
        logits_pairs = spec.logits_metrics if c.logits_con is not None else ()
        for nm, attr in pairs:
            vals[nm] = getattr(con_loss, attr).reshape(-1)[:1]
        for nm, attr in logits_pairs:
            vals[nm] = getattr(c.logits_con, attr).reshape(-1)[:1]
        sup_names = ('train/distill_loss', 'train/distill_agreement') if teacher is not None else \
                    ('train/supervised_loss', 'train/supervised_acc')
        if sup_loss is not None:
            vals[sup_names[0]] = sup_loss.value.reshape(-1)[:1]
            vals[sup_names[1]] = sup_loss.acc.reshape(-1)[:1]
        if repr_handle is not None:
            for nm, attr in metrics.REPR_METRICS:
                vals[nm] = getattr(repr_handle, attr)
        names = [nm for nm in order if nm in vals]
        # one launch: bank[index(name)] += value(name); the metrics absent this step keep their sums
        srcs = [vals.get(nm, state['zero']) for nm in order]
        assert len(order) <= 16, 'the metric bank holds 16 running sums (simclr_accumulate_scalars)'
        # The loss / metric scalars above are views into the per-step arena, which the NEXT step zeroes and refills: the same
        # launch writes them into `keep` (a fresh tensor per step) and the handles this function returns are re-pointed at
        # it, so a caller may hold them across steps (deferred .item() logging, trajectory lists).
        keep = torch.empty(len(order), device=features.device, dtype=torch.float32)
        ops.accumulate_scalars(srcs, dst=state['bank'], copy=keep)
        for nm in names:
            m[nm].bump()
        at = {nm: keep[i:i + 1] for i, nm in enumerate(order) if nm in vals}
        # Per name: a caller who passes an `all_metrics` without some name of the row still has every handle whose name it did pass
        # re-pointed (the handles of the names it left out keep reading the arena, as they must: nothing copied them).
        for nm, attr in pairs:
            if nm in at:
                setattr(con_loss, attr, at[nm])
        if logits_pairs and all(nm in at for nm, _ in logits_pairs):
            c.logits_con.keep(*(at[nm] for nm, _ in logits_pairs))                # LazyLogits.keep(acc, entropy): both or neither
        if sup_loss is not None and sup_names[0] in at:
            sup_loss.value = at[sup_names[0]]
            if sup_names[1] in at:
                sup_loss.acc = at[sup_names[1]]
        if torch.is_tensor(weight_decay) and 'train/weight_decay' in at:
            weight_decay = at['train/weight_decay']
        out = dict(con_loss=con_loss, sup_loss=sup_loss, weight_decay=weight_decay, total_loss=total, logits_con=c.logits_con)
        if repr_every:
            out['repr_stats'] = repr_handle
        return out

    single_step.metrics = m
    return single_step


def synthetic_batches(batch, image_size, num_classes, device, seed=0, pool=2, views=2, local_crops=0, local_size=None):
    """i.i.d. U[0,1) two-view batches [b, H, W, 6] + one-hot labels; views=1: the single-view
    [b, H, W, 3] batches of train_mode=finetune (tf2/data.py:52-58).  local_crops = L > 0 (SwAV / DINO multi-crop): features =
    (globals [b, H, W, 6], locals [b, h, h, 3L]); the local tensors are drawn AFTER every global tensor and label from the same
    seeded generator, so the globals and labels are those of a run without local crops."""
    g = torch.Generator(device='cpu').manual_seed(seed)
    feats = [torch.rand(batch, image_size, image_size, 3 * views, generator=g).to(device) for _ in range(pool)]
    labs = [torch.nn.functional.one_hot(torch.randint(0, num_classes, (batch,), generator=g), num_classes)
            .float().to(device) for _ in range(pool)]
    if local_crops:
        locs = [torch.rand(batch, local_size, local_size, 3 * local_crops, generator=g).to(device) for _ in range(pool)]
        feats = list(zip(feats, locs))
    i = 0
    while True:
        yield feats[i % pool], {'labels': labs[i % pool]}
        i += 1


def init_distributed():
    """One process per GPU (torchrun): RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* from the env.
    SIMCLR_DIST_BACKEND=gloo: the ranks talk over gloo and, with SIMCLR_SHARE_GPU=1, all sit on cuda:0 -- the way the
    multi-rank launch path is exercised on a single-GPU box (RCCL refuses two ranks on one device).
    SIMCLR_FORCE_COLLECTIVES=1 with WORLD_SIZE=1: a one-rank RCCL communicator whose collectives are all issued."""
    import os
    world = int(os.environ.get('WORLD_SIZE', '1'))
    force = os.environ.get('SIMCLR_FORCE_COLLECTIVES') == '1'
    if world <= 1 and not force:
        return None
    backend = os.environ.get('SIMCLR_DIST_BACKEND', 'nccl')
    share = os.environ.get('SIMCLR_SHARE_GPU') == '1'
    local = 0 if share else int(os.environ.get('LOCAL_RANK', '0'))
    torch.cuda.set_device(local)
    if not dist.is_initialized():
        if world <= 1:
            os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
            os.environ.setdefault('MASTER_PORT', '29533')
            os.environ.setdefault('RANK', '0')
            os.environ.setdefault('WORLD_SIZE', '1')
        if backend == 'nccl':
            dist.init_process_group('nccl', device_id=torch.device('cuda', local))
        else:
            dist.init_process_group(backend)
    return Strategy()


def json_serializable(val):      # tf2/run.py:340-345
    try:
        json.dumps(val)
        return True
    except TypeError:
        return False


def synthetic_eval_batches(batch, image_size, num_classes, device, seed=0, pool=2):
    """Single-view eval batches [b, H, W, 3] + one-hot labels (the eval pipeline feeds one centre crop,
    tf2/data.py:52-62 with is_training=False)."""
    g = torch.Generator(device='cpu').manual_seed(seed)
    feats = [torch.rand(batch, image_size, image_size, 3, generator=g).to(device) for _ in range(pool)]
    labs = [torch.nn.functional.one_hot(torch.randint(0, num_classes, (batch,), generator=g), num_classes)
            .float().to(device) for _ in range(pool)]
    i = 0
    while True:
        yield feats[i % pool], {'labels': labs[i % pool]}
        i += 1


def _check_device_health(strategy):
    """Synchronise and raise if any in-kernel bounded wait of this process ever timed out: the peer-mapped SyncBN exchange
    (comm.PeerStats: NaN-poisoned statistics) or a split-tail partner of the persistent convolution grid (wrong tile)."""
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    if strategy is not None:
        strategy.check_health(wait=True)
    ops.check_split_tail_health()


def perform_evaluation(model, data, eval_steps, ckpt, strategy, model_dir=None):
    """tf2/run.py:348-432: restore `ckpt` (weights + global step), run `eval_steps` batches through
    model(features, training=False), accumulate eval/label_top_1_accuracy, eval/label_top_5_accuracy and
    eval/regularization_loss, write result.json, result_<step>.json and flags.json into model_dir.
    `data`: iterator of (features [b,H,W,3], {'labels': one-hot}).  Returns the result dict (None when skipped)."""
    from .checkpoint import Checkpoint
    import os
    if FLAGS.train_mode == 'pretrain' and not FLAGS.lineareval_while_pretraining:
        logging.info('Skipping eval during pretraining without linear eval.')          # :350-352
        return None
    regularization_loss = metrics.Mean('eval/regularization_loss')
    label_top_1_accuracy = metrics.Accuracy('eval/label_top_1_accuracy')
    label_top_5_accuracy = metrics.TopKCategoricalAccuracy(5, 'eval/label_top_5_accuracy')
    all_metrics = [regularization_loss, label_top_1_accuracy, label_top_5_accuracy]
    global_step = 0
    restored = False
    for i in range(eval_steps):
        features, labels = next(data)
        _, supervised_head_outputs = model(features, training=False)                 # :379
        assert supervised_head_outputs is not None
        if not restored and ckpt:
            # variables exist only after the first forward pass (lazy build): restore, then redo this batch
            logging.info('Restoring from %s', ckpt)
            c = Checkpoint(model=model)
            c.restore(ckpt, model_only=False).expect_partial()                       # :369-373
            global_step = c.global_step
            restored = True
            _, supervised_head_outputs = model(features, training=False)
        restored = True
        outputs = supervised_head_outputs.dense()
        l = labels['labels']
        # 'mask': per-sample weights of a padded last batch (simclr_amd/data.py); absent = every sample counts
        metrics.update_finetune_metrics_eval(label_top_1_accuracy, label_top_5_accuracy, outputs, l, labels.get('mask'))   # :383-384
        reg_loss = model_lib.add_weight_decay(model, adjust_per_optimizer=True)      # :385
        regularization_loss.update_state(reg_loss)
        logging.info('Completed eval for %d / %d steps', i + 1, eval_steps)
    if hasattr(data, 'close'):
        data.close()                     # the input pipeline's worker threads
    # replicas evaluate disjoint shards: the accuracies are ratios of summed counts
    if strategy is not None and num_replicas(strategy) > 1:
        for m in (label_top_1_accuracy, label_top_5_accuracy):
            t = m.totals().to(RT.device)
            strategy.all_reduce_sum(t)
            m._hits, m._count = t[:1], float(t[1].item())
    writer = metrics.JsonlSummaryWriter(model_dir) if (model_dir and (strategy is None or strategy.rank == 0)) else None
    metrics.log_and_write_metrics_to_summary(all_metrics, global_step, writer)           # :400-403
    if writer is not None:
        writer.close()
    result = {m.name: float(m.result()) for m in all_metrics}
    result['global_step'] = int(global_step)
    logging.info(result)
    if model_dir and (strategy is None or strategy.rank == 0):
        os.makedirs(model_dir, exist_ok=True)
        for name in ('result.json', 'result_%d.json' % result['global_step']):       # :410-418
            with open(os.path.join(model_dir, name), 'w') as f:
                json.dump({k: float(v) for k, v in result.items()}, f)
        with open(os.path.join(model_dir, 'flags.json'), 'w') as f:                  # :419-427
            json.dump({k: v for k, v in FLAGS.flag_values_dict().items() if json_serializable(v)}, f)
    return result


def main(argv):
    """tf2/run.py:450-664: train (with checkpoints every checkpoint_steps / checkpoint_epochs and resume from
    model_dir), eval, or train_then_eval -- on synthetic batches (--dataset=synthetic) or on the array dataset
    <data_dir>/<dataset> (simclr_amd/data.py), whose training stream starts at the restored global step."""
    from .checkpoint import try_restore_from_checkpoint
    from . import data as data_lib
    import math
    FLAGS.parse(argv)
    logging.basicConfig(level=logging.INFO)
    distill = check_distillation_flags()
    check_contrastive_loss_flags()
    aug_plan()                                # a malformed --aug_recipe / --blur_probs / ... raises here, before any device work
    check_dropblock_flags()
    check_knn_flags()
    check_logreg_flags()
    check_kmeans_flags()
    check_spectrum_flags()
    check_repr_flags()
    builder = None
    if FLAGS.dataset != 'synthetic':
        # before any device work: a missing / unset --data_dir raises here, naming the expected layout and the converter
        builder = data_lib.ArrayDatasetBuilder(FLAGS.dataset, FLAGS.data_dir)                 # :471-472
        for sp in ([FLAGS.train_split] if FLAGS.mode != 'eval' else []) + ([FLAGS.eval_split] if FLAGS.mode != 'train' else []):
            builder.split(sp)
        if FLAGS.knn_eval and FLAGS.mode != 'train':
            builder.split(FLAGS.train_split)
            check_knn_flags(builder.info.splits[FLAGS.train_split].num_examples)
        if FLAGS.logreg_eval and FLAGS.mode != 'train':
            builder.split(FLAGS.train_split)
            check_logreg_flags(builder.info.splits[FLAGS.train_split].num_examples)
            check_logreg_classes(builder.info.features['label'].num_classes)
        if FLAGS.kmeans_eval and FLAGS.mode != 'train':
            builder.split(FLAGS.train_split)
            check_kmeans_flags(builder.info.splits[FLAGS.train_split].num_examples, builder.info.features['label'].num_classes)
        if FLAGS.spectrum_eval and FLAGS.mode != 'train':
            builder.split(FLAGS.train_split)
            check_spectrum_flags(builder.info.splits[FLAGS.train_split].num_examples)
    else:
        if FLAGS.knn_eval:
            check_knn_flags(SYNTHETIC_KNN_BANK_BATCHES * FLAGS.eval_batch_size)
        check_logreg_flags(SYNTHETIC_KNN_BANK_BATCHES * FLAGS.eval_batch_size)
        check_kmeans_flags(SYNTHETIC_KNN_BANK_BATCHES * FLAGS.eval_batch_size, 10 if FLAGS.image_size <= 32 else 1000)
        check_spectrum_flags(SYNTHETIC_KNN_BANK_BATCHES * FLAGS.eval_batch_size)
    strategy = init_distributed()
    R = num_replicas(strategy)
    rank0 = strategy is None or strategy.rank == 0
    if builder is not None:
        num_classes = builder.info.features['label'].num_classes                              # :475
        num_train_examples = builder.info.splits[FLAGS.train_split].num_examples if FLAGS.train_split in builder.info.splits else 0
        num_eval_examples = builder.info.splits[FLAGS.eval_split].num_examples if FLAGS.eval_split in builder.info.splits else 0
    else:
        num_classes = 10 if FLAGS.image_size <= 32 else 1000
        num_train_examples = 50000 if FLAGS.image_size <= 32 else 1281167
        num_eval_examples = 10000 if FLAGS.image_size <= 32 else 50000
    train_steps = model_lib.get_train_steps(num_train_examples)
    eval_steps = FLAGS.eval_steps or int(math.ceil(num_eval_examples / FLAGS.eval_batch_size))   # :476-478
    epoch_steps = int(round(num_train_examples / FLAGS.train_batch_size))                     # :479
    checkpoint_steps = FLAGS.checkpoint_steps or (FLAGS.checkpoint_epochs * epoch_steps)      # :486-487
    if builder is not None and FLAGS.mode != 'train':
        eval_steps = min(eval_steps, data_lib.eval_num_steps(num_eval_examples, FLAGS.eval_batch_size))   # one pass at most

    def eval_data():
        if builder is not None:
            return data_lib.build_distributed_dataset(builder, FLAGS.eval_batch_size, False, strategy)
        return synthetic_eval_batches(FLAGS.eval_batch_size // R, FLAGS.image_size, num_classes, RT.device, seed=100 + rep)

    def bank_iterator(n_bank, subset, knn_lib):
        """This replica's shard of the bank under evaluation preprocessing: n_bank examples of --train_split (`subset`: the first
        positions of the epoch-0 permutation), or, with --dataset=synthetic, whole batches of random images."""
        if builder is not None:
            split = builder.split(FLAGS.train_split, cache=FLAGS.cache_dataset)
            if subset:
                sel = knn_lib.knn_bank_indices(FLAGS.data_seed, split.index.shape[0], n_bank)
                split = data_lib.Split(split.index[sel], split.images)
            # evaluation preprocessing of the TRAINING split; the last batch is padded with weight 0 and trimmed from the bank
            return data_lib.DatasetIterator(split, num_classes, FLAGS.eval_batch_size, False, replica=rep, num_replicas=R, device=RT.device)
        import itertools
        steps = int(math.ceil(n_bank / FLAGS.eval_batch_size))
        return itertools.islice(synthetic_eval_batches(FLAGS.eval_batch_size // R, FLAGS.image_size, num_classes, RT.device,
                                                       seed=7000 + rep, pool=steps), steps)

    def knn_evaluation(ckpt, result):
        """--knn_eval: the weighted k-NN evaluation after perform_evaluation (which may have skipped); the union of both results."""
        from . import knn as knn_lib
        # --dataset=synthetic: at most SYNTHETIC_KNN_BANK_BATCHES batches, each drawn once -- a longer bank would only repeat them
        n_bank = check_knn_flags(num_train_examples if builder is not None else SYNTHETIC_KNN_BANK_BATCHES * FLAGS.eval_batch_size)
        bank_data = bank_iterator(n_bank, FLAGS.knn_bank_examples, knn_lib)
        knn_result = knn_lib.perform_knn_evaluation(model, bank_data, eval_data(), eval_steps, ckpt, strategy, FLAGS.model_dir)
        return dict(result or {}, **knn_result)

    def logreg_evaluation(ckpt, result):
        """--logreg_eval: the cached-feature linear probe, after perform_evaluation (which may have skipped) and the k-NN vote; the
        union of the results.  --dataset=synthetic: the bank of the k-NN path."""
        from . import knn as knn_lib
        from . import logreg as logreg_lib
        n_bank = check_logreg_flags(num_train_examples if builder is not None else SYNTHETIC_KNN_BANK_BATCHES * FLAGS.eval_batch_size)
        check_logreg_classes(num_classes)
        bank_data = bank_iterator(n_bank, FLAGS.logreg_bank_examples, knn_lib)
        logreg_result = logreg_lib.perform_logreg_evaluation(model, bank_data, eval_data(), eval_steps, ckpt, strategy, FLAGS.model_dir)
        return dict(result or {}, **logreg_result)

    def kmeans_evaluation(ckpt, result):
        """--kmeans_eval: the k-means clustering evaluation, after perform_evaluation (which may have skipped), the k-NN vote and the
        probe; the union of the results.  --dataset=synthetic: the bank of the k-NN path."""
        from . import kmeans as kmeans_lib
        from . import knn as knn_lib
        n_bank = check_kmeans_flags(num_train_examples if builder is not None else SYNTHETIC_KNN_BANK_BATCHES * FLAGS.eval_batch_size,
                                    num_classes)
        bank_data = bank_iterator(n_bank, FLAGS.kmeans_bank_examples, knn_lib)
        kmeans_result = kmeans_lib.perform_kmeans_evaluation(model, bank_data, eval_data(), eval_steps, ckpt, strategy, FLAGS.model_dir)
        return dict(result or {}, **kmeans_result)

    def spectrum_evaluation(ckpt, result):
        """--spectrum_eval: the eigen-spectrum evaluation, after the k-means evaluation; the union of the results.
        --dataset=synthetic: the bank of the k-NN path."""
        from . import knn as knn_lib
        from . import spectrum as spectrum_lib
        n_bank = check_spectrum_flags(num_train_examples if builder is not None else SYNTHETIC_KNN_BANK_BATCHES * FLAGS.eval_batch_size)
        bank_data = bank_iterator(n_bank, FLAGS.spectrum_bank_examples, knn_lib)
        spectrum_result = spectrum_lib.perform_spectrum_evaluation(model, bank_data, ckpt, strategy, FLAGS.model_dir)
        return dict(result or {}, **spectrum_result)
    RT.reset()
    RT.strategy = strategy
    RT.device = torch.device('cuda', torch.cuda.current_device())
    # the teacher is built, run once and restored BEFORE the student exists: the student's names and initial values are those of a
    # run without a teacher
    teacher = model_lib.Teacher(num_classes, FLAGS.teacher_checkpoint) if distill else None
    model = model_lib.Model(num_classes)
    rep = 0 if strategy is None else strategy.rank

    if FLAGS.mode == 'eval':                                                             # :482-496 (one pass over
        from .checkpoint import CheckpointManager, Checkpoint                            #  the latest checkpoint)
        mgr = CheckpointManager(Checkpoint(model=model), FLAGS.model_dir, FLAGS.keep_checkpoint_max)
        ckpt = FLAGS.checkpoint or mgr.latest_checkpoint
        result = perform_evaluation(model, eval_data(), eval_steps, ckpt, strategy, FLAGS.model_dir)
        if FLAGS.knn_eval:
            result = knn_evaluation(ckpt, result)
        if FLAGS.logreg_eval:
            result = logreg_evaluation(ckpt, result)
        if FLAGS.kmeans_eval:
            result = kmeans_evaluation(ckpt, result)
        if FLAGS.spectrum_eval:
            result = spectrum_evaluation(ckpt, result)
        if rank0:
            print(json.dumps(result), flush=True)
        return result

    learning_rate = model_lib.WarmUpAndCosineDecay(FLAGS.learning_rate, num_train_examples)
    optimizer = model_lib.build_optimizer(learning_rate)
    # a loss with a momentum target network builds it after the online model (whose variables it makes exist first); SwAV has none,
    # and the freeze of its prototypes counts epochs
    spec = loss_lib.active()
    target = spec.make_target(model, train_steps, epoch_steps) if spec is not None and spec.make_target is not None else None
    # --nn_queue_size: the support queue of NNCLR, seeded (the same on every replica) and checkpointed after the model's variables
    support = (model_lib.SupportQueue(FLAGS.nn_queue_size, model_lib.projection_width(), FLAGS.nn_queue_seed)
               if loss_lib.nn_positives_on() else None)
    step_fn = make_single_step(model, optimizer, strategy, teacher=teacher, target=target,
                               steps_per_epoch=max(epoch_steps, 1) if swav_loss_on() else None, support=support)
    per_replica = FLAGS.train_batch_size // R                                   # tf2/data.py:45
    data = None
    if builder is None:
        data = synthetic_batches(per_replica, FLAGS.image_size, num_classes, RT.device, seed=rep,
                                 views=1 if FLAGS.train_mode == 'finetune' else 2,
                                 local_crops=local_crop_plan()[0], local_size=local_crop_plan()[1])
    manager = None
    summary_writer = metrics.JsonlSummaryWriter(FLAGS.model_dir) if (FLAGS.model_dir and rank0) else None   # :526
    log_every = FLAGS.checkpoint_steps or 10
    step = 0
    if FLAGS.model_dir:
        # Build the variables with a forward-only pass in inference mode (no statistics or moving averages move), then
        # restore BEFORE step 0 as tf2/run.py:520-521 does: the latest checkpoint of model_dir (weights, BN moving
        # statistics, LARS slots, step) or, failing that, the weights of --checkpoint (slots stay zero, step 0).
        model(torch.zeros(2, FLAGS.image_size, FLAGS.image_size, 3, device=RT.device), training=False)
        if swav_loss_on() and model.prototype_head.kernel is None:
            model.prototype_head.build(model_lib.projection_width())    # last: every other initial value is that of an ntxent run
        saved = target.checkpointable() if target is not None else support.checkpointable(model) if support is not None else model
        manager, status = try_restore_from_checkpoint(saved, optimizer, FLAGS.model_dir, FLAGS.checkpoint,
                                                      FLAGS.keep_checkpoint_max, FLAGS.zero_init_logits_layer)
        if target is not None and status is not None:
            # --checkpoint, or a file without these entries: the copy of the online model is made after the restore; likewise the
            # seeded queue (a weights-only restore may have filled it from the file) and the zero centre.  In this order.
            missing = status.missing_in_checkpoint
            for part, absent, reset in (
                    (target, lambda: any(n.startswith(target.PREFIX) for n in missing), target.copy_from_online),
                    (target.queue, lambda: target.queue.NAME in missing, lambda: target.queue.reset()),
                    (target.center, lambda: target.center.NAME in missing, lambda: target.center.reset())):
                if part is not None and (not manager.latest_checkpoint or absent()):
                    reset()
        if support is not None and status is not None and (not manager.latest_checkpoint
                                                           or support.NAME in status.missing_in_checkpoint):
            support.reset()          # --checkpoint (a weights-only restore may have filled it), or a file without the queue: the seeded rows
        if status is not None and manager.latest_checkpoint:
            step = int(optimizer.iterations)
            logging.info('restored %s; continuing from step %d', manager.latest_checkpoint, step)
    if builder is not None:
        # the batch of step s depends on (data_seed, s, replica) only: starting at the restored step continues the same data
        data = data_lib.build_distributed_dataset(builder, FLAGS.train_batch_size, True, strategy, start_step=step)
    t0 = time.time()
    while step < train_steps:
        features, labels = next(data)
        step_fn(features, labels)
        step += 1
        if step % log_every == 0:
            torch.cuda.synchronize()
            ops.check_split_tail_health()        # a split-tail partner that never arrived is an error, not a silent wrong tile
            dt = time.time() - t0
            t0 = time.time()
            if rank0:
                # a window without a measured step has no representation diagnostics: the keys are left out, never written as 0.0
                logged = {k: v for k, v in step_fn.metrics.items() if v._count or k not in dict(metrics.REPR_METRICS)}
                vals = {k: v.result() for k, v in logged.items()}
                vals.update(step=step, images_per_sec=FLAGS.train_batch_size * log_every / dt,
                            learning_rate=learning_rate(step))
                print(json.dumps(vals), flush=True)
                if summary_writer is not None:                                              # :645-652
                    metrics.log_and_write_metrics_to_summary(list(logged.values()), step, summary_writer)
                    summary_writer.scalar('learning_rate', learning_rate(step), step)
                    summary_writer.flush()
            for v in step_fn.metrics.values():
                v.reset_states()
        if manager is not None and (step % checkpoint_steps == 0 or step == train_steps):   # :640-648 (every steps_per_loop)
            # A timed-out statistics exchange poisons that step's statistics -- and the weights -- with NaN, and the per-step
            # health check only sees the PREVIOUS step's copy: synchronise and inspect the sticky device counters NOW, so that a
            # poisoned state is never written as `latest` (nor rotates a good checkpoint out).  Raises -> nothing is saved.
            _check_device_health(strategy)
            # every replica records the new checkpoint (same name everywhere), replica 0 alone writes it: otherwise
            # the other replicas' `latest_checkpoint` would still name the resume point in train_then_eval
            manager.save(step, write=rank0)
            if strategy is not None:
                dist.barrier()
    _check_device_health(strategy)       # time-outs of the last steps are reported too (the loop may end between two log intervals)
    if builder is not None:
        data.close()
    if FLAGS.mode == 'train_then_eval' and manager is not None:                           # :657-660
        result = perform_evaluation(model, eval_data(), eval_steps, manager.latest_checkpoint, strategy, FLAGS.model_dir)
        if FLAGS.knn_eval:
            result = knn_evaluation(manager.latest_checkpoint, result)
        if FLAGS.logreg_eval:
            result = logreg_evaluation(manager.latest_checkpoint, result)
        if FLAGS.kmeans_eval:
            result = kmeans_evaluation(manager.latest_checkpoint, result)
        if FLAGS.spectrum_eval:
            result = spectrum_evaluation(manager.latest_checkpoint, result)
        if rank0:
            print(json.dumps(result), flush=True)
        return result
    return None


if __name__ == '__main__':
    main(sys.argv[1:])
