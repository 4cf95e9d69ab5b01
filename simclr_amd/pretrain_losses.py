"""The table of pretraining losses: one row of LOSSES per --contrastive_loss name, holding what is declarative about that loss.

run.py reads it: check_contrastive_loss_flags runs the row's `check`, build_metrics lists the row's metric names, single_step calls
the row's `call` and fills / re-points the row's (metric name, attribute) pairs, main builds the target network from `make_target`.
The phases of the step that really differ between losses (target prelude, predictor backward, frozen prototypes, enqueue, centre
update, multi-crop) are explicit code in run.make_single_step, not rows here.  Every `call` reaches the loss through the `objective`
module at call time (obj_lib.add_*), never through a function object captured at import.
"""
import collections

from . import model as model_lib
from . import objective as obj_lib
from . import ops
from .flags import FLAGS


# ------------------------------------------------------------------------------------------- start-up checks (before any device work)
def _need_head_width(name, dims, kernels):
    if FLAGS.proj_head_mode == 'none' or FLAGS.proj_out_dim not in dims:
        raise ValueError('--contrastive_loss=%s needs a projection head of width %s (got proj_head_mode=%r, proj_out_dim=%d): '
                         'the %s kernels are instantiated for those widths only'
                         % (name, '/'.join(map(str, dims)), FLAGS.proj_head_mode, FLAGS.proj_out_dim, kernels))


def _need_loss_width(name, ok, step, lo, hi, takers):
    width = model_lib.projection_width()
    if not ok(width):
        raise ValueError('--contrastive_loss=%s needs a loss width that is a multiple of %d in [%d, %d] (got %d from '
                         'proj_head_mode=%r, proj_out_dim=%d): the %s take those widths only'
                         % (name, step, lo, hi, width, FLAGS.proj_head_mode, FLAGS.proj_out_dim, takers))


def _need_range(names, ok, what):
    for name in names:
        if not ok(getattr(FLAGS, name)):
            raise ValueError('--%s must %s (got %r)' % (name, what, getattr(FLAGS, name)))


# (test, wording) for _need_range; NaN fails every one of them
_POSITIVE_FINITE = (lambda x: 0.0 < x < float('inf'), 'be > 0 and finite')
_UNIT_INTERVAL = (lambda x: 0.0 <= x <= 1.0, 'lie in [0, 1]')
_NON_NEGATIVE = (lambda x: not x < 0, 'be >= 0')


def _check_swav():
    if not 2 <= FLAGS.swav_num_prototypes <= ops.SWAV_MAX_PROTOTYPES:
        raise ValueError('--swav_num_prototypes must lie in [2, %d] (got %r)' % (ops.SWAV_MAX_PROTOTYPES, FLAGS.swav_num_prototypes))
    _need_range(('swav_epsilon', 'swav_temperature'), *_POSITIVE_FINITE)
    if not 1 <= FLAGS.swav_sinkhorn_iterations <= ops.SWAV_MAX_ITERS:
        raise ValueError('--swav_sinkhorn_iterations must lie in [1, %d] (got %r)' % (ops.SWAV_MAX_ITERS, FLAGS.swav_sinkhorn_iterations))
    _need_range(('swav_freeze_prototypes_epochs',), *_NON_NEGATIVE)
    _need_head_width('swav', ops.SWAV_DIMS, 'SwAV')


def _check_dino():
    if not 2 <= FLAGS.dino_out_dim <= ops.DINO_MAX_OUT_DIM:
        raise ValueError('--dino_out_dim must lie in [2, %d] (got %r)' % (ops.DINO_MAX_OUT_DIM, FLAGS.dino_out_dim))
    _need_range(('dino_student_temp', 'dino_teacher_temp', 'dino_warmup_teacher_temp'), *_POSITIVE_FINITE)
    _need_range(('dino_center_momentum', 'dino_momentum'), *_UNIT_INTERVAL)
    _need_range(('dino_warmup_teacher_temp_epochs', 'dino_freeze_last_layer_epochs'), *_NON_NEGATIVE)
    _need_head_width('dino', ops.DINO_DIMS, 'DINO')


def _check_moco():
    rows = 2 * FLAGS.train_batch_size               # the global 2N rows a step enqueues
    K = FLAGS.moco_queue_size
    if rows < 2 or K < rows or K % rows != 0 or K > ops.MOCO_MAX_QUEUE:
        raise ValueError('--moco_queue_size must be a multiple of 2 x train_batch_size = %d, at least that and at most %d (got %r): '
                         'the ring never wraps inside a step' % (rows, ops.MOCO_MAX_QUEUE, K))
    _need_range(('moco_momentum',), *_UNIT_INTERVAL)
    if not FLAGS.temperature > 0:
        raise ValueError('--contrastive_loss=mocov2 needs --temperature > 0 (got %r)' % (FLAGS.temperature,))
    _need_head_width('mocov2', ops.MOCO_DIMS, 'MoCo')


def _check_byol():
    _need_range(('byol_tau_base',), *_UNIT_INTERVAL)
    if not ops.byol_dim_ok(FLAGS.byol_pred_hidden_dim):
        raise ValueError('--byol_pred_hidden_dim must be a multiple of %d in [%d, %d] (got %r)'
                         % (ops.BYOL_DIM_STEP, ops.BYOL_MIN_DIM, ops.BYOL_MAX_DIM, FLAGS.byol_pred_hidden_dim))
    _need_loss_width('byol', ops.byol_dim_ok, ops.BYOL_DIM_STEP, ops.BYOL_MIN_DIM, ops.BYOL_MAX_DIM, 'BYOL kernels and the predictor')


def _check_vicreg():
    _need_range(('vicreg_sim_coeff', 'vicreg_std_coeff', 'vicreg_cov_coeff'), ops.vicreg_coeff_ok, 'be >= 0 and finite')
    _need_loss_width('vicreg', ops.vicreg_dim_ok, ops.VICREG_DIM_STEP, ops.VICREG_MIN_DIM, ops.VICREG_MAX_DIM, 'VICReg kernels')
    if FLAGS.train_batch_size < 2:
        raise ValueError('--contrastive_loss=vicreg needs --train_batch_size >= 2 (got %r): the variance over the global batch is '
                         'the unbiased one' % (FLAGS.train_batch_size,))


def _check_barlow():
    _need_range(('bt_lambda',), *_NON_NEGATIVE)
    _need_range(('bt_loss_scaling',), lambda x: x > 0, 'be > 0')
    _need_loss_width('barlow', ops.bt_dim_ok, ops.BT_DIM_STEP, ops.BT_MIN_DIM, ops.BT_MAX_DIM, 'Barlow Twins kernels')


def ntxent_corrections_on():
    """A nonzero --hard_negative_beta or --debiased_tau_plus (NaN counts: the check refuses it) in an NT-Xent pretraining run outside
    --mode=eval: the step trains add_hard_negative_contrastive_loss.  Fine-tuning and evaluation ignore the two flags."""
    return (model_lib.pretrain_loss() == 'ntxent' and FLAGS.mode != 'eval'
            and not (FLAGS.hard_negative_beta == 0 and FLAGS.debiased_tau_plus == 0))


def check_ntxent_corrections():
    """The start-up check of --hard_negative_beta / --debiased_tau_plus, run for every pretraining loss: the two flags correct NT-Xent
    and nothing else."""
    beta, tau_plus = FLAGS.hard_negative_beta, FLAGS.debiased_tau_plus
    if beta == 0 and tau_plus == 0:
        return
    _need_range(('hard_negative_beta',), ops.hcl_beta_ok, 'be >= 0 and finite')
    _need_range(('debiased_tau_plus',), ops.hcl_tau_plus_ok, 'lie in [0, 1)')
    if model_lib.pretrain_loss() != 'ntxent':
        raise ValueError('--hard_negative_beta and --debiased_tau_plus correct NT-Xent: a nonzero value needs --contrastive_loss=ntxent '
                         '(got %r with hard_negative_beta=%r, debiased_tau_plus=%r)' % (FLAGS.contrastive_loss, beta, tau_plus))
    if not FLAGS.hidden_norm:
        raise ValueError('--hard_negative_beta / --debiased_tau_plus need --hidden_norm=true: the floor M exp(-1 / temperature) of the '
                         'negative term assumes dot products >= -1')
    width = model_lib.projection_width()
    if width not in ops.HCL_DIMS:
        raise ValueError('--hard_negative_beta / --debiased_tau_plus need a loss width of %s (got %d from proj_head_mode=%r, '
                         'proj_out_dim=%d): the hard-negative / debiased NT-Xent kernels are instantiated for those widths only'
                         % ('/'.join(map(str, ops.HCL_DIMS)), width, FLAGS.proj_head_mode, FLAGS.proj_out_dim))
    if FLAGS.train_batch_size < 2:
        raise ValueError('--hard_negative_beta / --debiased_tau_plus need --train_batch_size >= 2 (got %r): a row needs a negative'
                         % (FLAGS.train_batch_size,))
    if not FLAGS.temperature > 0:
        raise ValueError('--hard_negative_beta / --debiased_tau_plus need --temperature > 0 (got %r)' % (FLAGS.temperature,))


def nn_positives_on():
    """A nonzero --nn_queue_size in an NT-Xent pretraining run outside --mode=eval: the step trains add_nn_contrastive_loss against a
    model.SupportQueue.  Fine-tuning and evaluation ignore the flag."""
    return model_lib.pretrain_loss() == 'ntxent' and FLAGS.mode != 'eval' and FLAGS.nn_queue_size != 0


def check_nn_positives():
    """The start-up check of --nn_queue_size, run for every pretraining loss: the flag replaces NT-Xent's anchors and nothing else."""
    K = FLAGS.nn_queue_size
    if K == 0:
        return
    if model_lib.pretrain_loss() != 'ntxent':
        raise ValueError('--nn_queue_size draws the positives of NT-Xent from a support queue: a nonzero value needs '
                         '--contrastive_loss=ntxent (got %r with nn_queue_size=%r)' % (FLAGS.contrastive_loss, K))
    if not (FLAGS.hard_negative_beta == 0 and FLAGS.debiased_tau_plus == 0):
        raise ValueError('--nn_queue_size does not combine with --hard_negative_beta / --debiased_tau_plus (got %r with %r / %r): '
                         'the corrected NT-Xent contrasts a block against itself' % (K, FLAGS.hard_negative_beta, FLAGS.debiased_tau_plus))
    if FLAGS.train_batch_size < 2:
        raise ValueError('--nn_queue_size needs --train_batch_size >= 2 (got %r): a row needs a negative' % (FLAGS.train_batch_size,))
    rows = FLAGS.train_batch_size                   # the global N view-a rows a step enqueues
    if K < rows or K % rows != 0 or K > ops.MOCO_MAX_QUEUE:
        raise ValueError('--nn_queue_size must be a multiple of train_batch_size = %d, at least that and at most %d (got %r): '
                         'the ring never wraps inside a step' % (rows, ops.MOCO_MAX_QUEUE, K))
    if not FLAGS.hidden_norm:
        raise ValueError('--nn_queue_size needs --hidden_norm=true: the nearest neighbour is the largest dot product of unit rows')
    width = model_lib.projection_width()
    if width not in ops.NNCLR_DIMS:
        raise ValueError('--nn_queue_size needs a loss width of %s (got %d from proj_head_mode=%r, proj_out_dim=%d): the NNCLR kernels '
                         'are instantiated for those widths only'
                         % ('/'.join(map(str, ops.NNCLR_DIMS)), width, FLAGS.proj_head_mode, FLAGS.proj_out_dim))
    if not FLAGS.temperature > 0:
        raise ValueError('--nn_queue_size needs --temperature > 0 (got %r)' % (FLAGS.temperature,))


def _check_generalized():
    if FLAGS.gcl_dist not in obj_lib.GCL_DISTS:
        raise ValueError('Unknown prior {}'.format(FLAGS.gcl_dist))
    _need_head_width('generalized', ops.GCL_DIMS, 'generalized-loss')
    if FLAGS.gcl_dist != 'logsumexp' and 2 * FLAGS.train_batch_size > ops.SWD_MAX_ROWS:
        raise ValueError('--gcl_dist=%s sorts the 2 x train_batch_size global rows of every projected dimension in LDS: '
                         'train_batch_size <= %d (got %d)' % (FLAGS.gcl_dist, ops.SWD_MAX_ROWS // 2, FLAGS.train_batch_size))


# ------------------------------------------------------------------------------------------------------------- the call into objective
# c: the namespace run.single_step fills for one step -- model, target, strategy, steps_per_epoch; step (optimizer.iterations before
# its increment: a restored run continues every schedule derived from it); outputs (the online projection), labels, overlap (the
# supervised part, run while collective A is in flight); target_outputs and keys (losses with a target); frozen (losses with
# prototypes); support (the model.SupportQueue of --nn_queue_size, or None);
# logits_con (None; NT-Xent sets it).  Each function returns the loss handle.
def _ntxent(c):
    if nn_positives_on():                 # --nn_queue_size: the anchors are the rows' nearest neighbours in c.support
        return obj_lib.add_nn_contrastive_loss(c.outputs, c.support.value, temperature=FLAGS.temperature, strategy=c.strategy,
                                               overlap=c.overlap)
    if ntxent_corrections_on():           # --hard_negative_beta / --debiased_tau_plus: the same logits, another loss over them
        con_loss, c.logits_con, _ = obj_lib.add_hard_negative_contrastive_loss(
            c.outputs, temperature=FLAGS.temperature, beta=FLAGS.hard_negative_beta, tau_plus=FLAGS.debiased_tau_plus,
            strategy=c.strategy, overlap=c.overlap)
        return con_loss
    con_loss, c.logits_con, _ = obj_lib.add_contrastive_loss(                           # tf2/run.py:582-586
        c.outputs, hidden_norm=FLAGS.hidden_norm, temperature=FLAGS.temperature, strategy=c.strategy, overlap=c.overlap)
    return con_loss


def _generalized(c):
    obj_lib.set_gcl_step(c.step)          # the draws of the SWD priors are a function of (gcl_seed, global step)
    return obj_lib.generalized_loss_of_block(
        c.outputs, lambda_weight=FLAGS.gcl_lambda, temperature=FLAGS.temperature, dist=FLAGS.gcl_dist,
        hidden_norm=FLAGS.hidden_norm, loss_scaling=FLAGS.gcl_loss_scaling, strategy=c.strategy, overlap=c.overlap)


def _supcon(c):
    # the labels define the positives, whether or not the supervised head trains on them too
    return obj_lib.add_supcon_loss(c.outputs, c.labels['labels'] if isinstance(c.labels, dict) else c.labels,
                                   hidden_norm=FLAGS.hidden_norm, temperature=FLAGS.temperature, strategy=c.strategy, overlap=c.overlap)


def _barlow(c):
    return obj_lib.add_barlow_twins_loss(c.outputs, lambda_weight=FLAGS.bt_lambda, loss_scaling=FLAGS.bt_loss_scaling,
                                         strategy=c.strategy, overlap=c.overlap)


def _vicreg(c):
    return obj_lib.add_vicreg_loss(c.outputs, sim_coeff=FLAGS.vicreg_sim_coeff, std_coeff=FLAGS.vicreg_std_coeff,
                                   cov_coeff=FLAGS.vicreg_cov_coeff, strategy=c.strategy, overlap=c.overlap)


def _byol(c):
    return obj_lib.add_byol_loss(c.model.predict(c.outputs), c.target_outputs, strategy=c.strategy, overlap=c.overlap)


def _moco(c):
    return obj_lib.add_moco_loss(c.outputs, c.target_outputs, c.target.queue.value, temperature=FLAGS.temperature,
                                 strategy=c.strategy, overlap=c.overlap, keys=c.keys)


def _dino(c):
    return obj_lib.add_dino_loss(
        c.outputs, c.target_outputs, c.model.prototype_head, c.target.prototypes(), c.target.center.value,
        student_temp=FLAGS.dino_student_temp, teacher_temp=model_lib.dino_teacher_temp(c.step, c.target.steps_per_epoch),
        strategy=c.strategy, overlap=c.overlap, keys=c.keys, update_prototypes=not c.frozen)


def _swav(c):
    return obj_lib.add_swav_loss(
        c.outputs, c.model.prototype_head, temperature=FLAGS.swav_temperature, epsilon=FLAGS.swav_epsilon,
        sinkhorn_iterations=FLAGS.swav_sinkhorn_iterations, strategy=c.strategy, overlap=c.overlap, update_prototypes=not c.frozen)


# ---------------------------------------------------------------------------------------------------------------- the target networks
# make_target(model, train_steps, epoch_steps): what run.main builds after the online model (whose variables it makes exist first);
# check_target(target): what make_single_step refuses.
def _moco_target(model, train_steps, epoch_steps):
    # the same target network under a constant momentum, and the queue of its keys (seeded: the same on every replica)
    return model_lib.TargetNetwork(model, train_steps,
                                   queue=model_lib.MocoQueue(FLAGS.moco_queue_size, FLAGS.proj_out_dim, FLAGS.moco_queue_seed))


def _dino_target(model, train_steps, epoch_steps):
    # the same target network under BYOL's cosine schedule from --dino_momentum, prototypes included, and the teacher's centre
    return model_lib.TargetNetwork(model, train_steps, center=model_lib.DinoCenter(FLAGS.dino_out_dim),
                                   steps_per_epoch=max(epoch_steps, 1))


def _check_byol_target(target):
    if target is None:
        raise ValueError('--contrastive_loss=byol needs a target network: '
                         'make_single_step(..., target=model.TargetNetwork(model, steps))')


def _check_moco_target(target):
    if target is None or getattr(target, 'queue', None) is None:
        raise ValueError('--contrastive_loss=mocov2 needs a target network with a key queue: make_single_step(..., '
                         'target=model.TargetNetwork(model, steps, queue=model.MocoQueue(K, D, seed)))')


def _check_dino_target(target):
    if target is None or getattr(target, 'center', None) is None or not getattr(target, 'steps_per_epoch', None):
        raise ValueError('--contrastive_loss=dino needs a target network with a centre: make_single_step(..., '
                         'target=model.TargetNetwork(model, steps, center=model.DinoCenter(K), steps_per_epoch=n))')


# -------------------------------------------------------------------------------------------------------------------------- the table
# call: c -> loss handle;  check: the start-up check, run in a pretraining run outside --mode=eval;
# metrics: (metric name, attribute of the loss handle), train/contrast_loss -> .value first, which every loss logs;
# logits_metrics: the same, read from the LazyLogits NT-Xent alone returns (no other loss has logits to score);
# make_target / check_target: losses with a momentum target network;
# frozen: c -> True while the loss's prototypes take no update (losses with a prototype head).
LossSpec = collections.namedtuple('LossSpec', 'call check metrics logits_metrics make_target check_target frozen',
                                  defaults=((), None, None, None))


def _row(call, check, *metrics, **kw):
    return LossSpec(call, check, (('train/contrast_loss', 'value'),) + metrics, **kw)


LOSSES = {
    'ntxent': _row(_ntxent, None,
                   logits_metrics=(('train/contrast_acc', 'contrast_acc'), ('train/contrast_entropy', 'contrast_entropy'))),
    'generalized': _row(_generalized, _check_generalized, ('train/align_loss', 'align'), ('train/dist_loss', 'dist_match')),
    'supcon': _row(_supcon, lambda: _need_head_width('supcon', ops.SUPCON_DIMS, 'supervised contrastive'),
                   ('train/contrast_acc', 'acc'), ('train/contrast_positives', 'positives')),
    # no logits to score: the two raw sums / the three raw terms / the mean cosine of the paired rows instead
    'barlow': _row(_barlow, _check_barlow, ('train/bt_on_diag', 'on_diag'), ('train/bt_off_diag', 'off_diag')),
    'vicreg': _row(_vicreg, _check_vicreg,
                   ('train/vicreg_inv', 'invariance'), ('train/vicreg_var', 'variance'), ('train/vicreg_cov', 'covariance')),
    'byol': _row(_byol, _check_byol, ('train/byol_cosine', 'cosine'), check_target=_check_byol_target,
                 make_target=lambda model, train_steps, epoch_steps: model_lib.TargetNetwork(model, train_steps)),
    # positive against the best queue row; no entropy
    'mocov2': _row(_moco, _check_moco, ('train/contrast_acc', 'acc'), make_target=_moco_target, check_target=_check_moco_target),
    # log K = uniform teacher / codes, 0 = one-hot collapse
    'dino': _row(_dino, _check_dino, ('train/dino_teacher_entropy', 'entropy'),
                 make_target=_dino_target, check_target=_check_dino_target,
                 frozen=lambda c: model_lib.dino_last_layer_frozen(c.step, c.target.steps_per_epoch)),
    'swav': _row(_swav, _check_swav, ('train/swav_code_entropy', 'entropy'),
                 frozen=lambda c: model_lib.swav_prototypes_frozen(c.step, c.steps_per_epoch)),
}


# the ntxent row while --hard_negative_beta / --debiased_tau_plus is nonzero: one more metric, everything else the row's own
_NTXENT_CORRECTED = LOSSES['ntxent']._replace(metrics=LOSSES['ntxent'].metrics + (('train/contrast_floor_share', 'floor_share'),))


# the ntxent row while --nn_queue_size is nonzero: the loss scores its own logits (no LazyLogits), and reports how close the neighbours are
_NTXENT_NN = LOSSES['ntxent']._replace(
    metrics=LOSSES['ntxent'].metrics + (('train/contrast_acc', 'acc'), ('train/nn_similarity', 'nn_sim')), logits_metrics=())


def active():
    """The row of the active pretraining loss, or None outside a pretraining run."""
    if nn_positives_on():
        return _NTXENT_NN
    if ntxent_corrections_on():
        return _NTXENT_CORRECTED
    return LOSSES.get(model_lib.pretrain_loss())
