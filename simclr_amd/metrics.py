"""Training metrics -- mirror of /root/reference/tf2/metrics.py for the pretraining step.

`Mean` stands in for tf.keras.metrics.Mean (running mean, `update_state` / `result` /
`reset_states`); values stay on the device until `result()` so the step never syncs.
"""
import logging

import torch


class Mean:
    def __init__(self, name):
        self.name = name
        self._bank = None
        self.reset_states()

    def reset_states(self):
        self._sum = None
        self._count = 0
        if getattr(self, '_bank', None) is not None:
            self._bank[0][self._bank[1]] = 0.0

    def attach(self, sums, index):
        """Batched bookkeeping (run.make_single_step): this metric's running sum is element `index` of the device tensor
        `sums`, which ONE simclr_accumulate_scalars launch per step updates for all metrics; `bump()` counts the update."""
        if self._bank is not None and self._bank[0] is not sums:
            # re-attached to another step function's bank: carry the sum accumulated so far over instead of dropping it
            prev = self._bank[0][self._bank[1]].detach().reshape(1).clone()
            self._sum = prev if self._sum is None else self._sum + prev.to(self._sum.device)
        self._bank = (sums, index)

    def bump(self):
        self._count += 1

    def update_state(self, value):
        if hasattr(value, 'value'):
            value = value.value
        if not torch.is_tensor(value):
            value = torch.tensor(float(value))
        v = value.detach().reshape(-1)[:1].clone()
        self._sum = v if self._sum is None else self._sum + v.to(self._sum.device)
        self._count += 1

    def result(self):
        if self._count == 0:
            return 0.0
        tot = float(self._sum.item()) if self._sum is not None else 0.0
        if getattr(self, '_bank', None) is not None:
            tot += float(self._bank[0][self._bank[1]].item())
        return tot / self._count


class Accuracy:
    """tf.keras.metrics.Accuracy: running mean of (y_true == y_pred) over all samples seen."""

    def __init__(self, name):
        self.name = name
        self.reset_states()

    def reset_states(self):
        self._hits = None
        self._count = 0

    def update_state(self, y_true, y_pred, sample_weight=None):
        self._add(y_true.reshape(-1) == y_pred.reshape(-1), sample_weight)

    def _add(self, hit, sample_weight):
        """sample_weight (optional, one per sample; stays on the device): hits and count are weighted sums, so a padded eval
        batch whose padding carries weight 0 counts every example once."""
        if sample_weight is None:
            h = hit.sum().to(torch.float64).reshape(1)
            self._count = self._count + hit.numel()
        else:
            w = sample_weight.reshape(-1).to(torch.float64)
            h = (hit.reshape(-1).to(torch.float64) * w).sum().reshape(1)
            self._count = self._count + w.sum().reshape(1)
        self._hits = h if self._hits is None else self._hits + h

    def totals(self):
        """(hits, count) as a fp64 tensor -- what a multi-replica eval all-reduces."""
        dev = self._hits.device if self._hits is not None else 'cpu'
        h = self._hits if self._hits is not None else torch.zeros(1, dtype=torch.float64)
        c = self._count if torch.is_tensor(self._count) else torch.tensor([float(self._count)], dtype=torch.float64)
        return torch.cat([h.to(dev), c.to(dev)])

    def result(self):
        t = self.totals()
        return float(t[0].item()) / max(float(t[1].item()), 1.0)


class TopKCategoricalAccuracy(Accuracy):
    """tf.keras.metrics.TopKCategoricalAccuracy(k): one-hot labels, a sample counts when its target class is
    among the k largest predictions (ties resolved like tf.math.in_top_k: strictly-greater count < k)."""

    def __init__(self, k, name):
        self.k = k
        super().__init__(name)

    def update_state(self, y_true, y_pred, sample_weight=None):
        target = y_true.argmax(1)
        tv = y_pred.gather(1, target[:, None])
        self._add((y_pred > tv).sum(1) < self.k, sample_weight)


def update_finetune_metrics_eval(label_top_1_accuracy_metrics, label_top_5_accuracy_metrics, outputs, labels, weights=None):
    """tf2/metrics.py:58-62.  outputs: dense logits [b, C]; labels: one-hot [b, C]; weights: optional per-sample weights
    (0 for the padding of a last eval batch)."""
    label_top_1_accuracy_metrics.update_state(labels.argmax(1), outputs.argmax(1), weights)
    label_top_5_accuracy_metrics.update_state(labels, outputs, weights)


def update_pretrain_metrics_train(contrast_loss, contrast_acc, contrast_entropy, loss, logits_con, labels_con):
    """Updated pretraining metrics (tf2/metrics.py:23-36).  The accuracy (argmax(labels) ==
    argmax(logits_ab), :28-31) and the entropy of softmax(logits_ab) (:33-35) come fused out of
    the loss kernels when `logits_con` is the lazy handle."""
    contrast_loss.update_state(loss)
    if hasattr(logits_con, 'contrast_acc'):
        contrast_acc.update_state(logits_con.contrast_acc)
        contrast_entropy.update_state(logits_con.contrast_entropy)
        return
    acc = (labels_con.argmax(1) == logits_con.argmax(1)).float().mean()
    contrast_acc.update_state(acc)
    p = torch.softmax(logits_con, -1)
    contrast_entropy.update_state(-(p * torch.log(p + 1e-8)).sum(-1).mean())


def update_finetune_metrics_train(supervised_loss_metric, supervised_acc_metric, loss, labels, logits):
    """tf2/metrics.py:49-55."""
    supervised_loss_metric.update_state(loss)
    if hasattr(loss, 'acc'):
        supervised_acc_metric.update_state(loss.acc)
        return
    acc = (labels.argmax(1) == logits.argmax(1)).float().mean()
    supervised_acc_metric.update_state(acc)


REPR_METRICS = (('train/repr_align', 'align'), ('train/repr_uniform', 'uniform'), ('train/repr_std', 'std'), ('train/repr_rank', 'rank'))


class ReprStats:
    """What representation_stats returns: `values` fp32 [4] = {align, uniform, std, rank} on the device, the four as one-element
    views of it, `normalized` [2n, D] (the l2-normalised local block) and `gathered` [2N, D] (the block the kernels read)."""

    def __init__(self, values, normalized, gathered):
        self.values, self.normalized, self.gathered = values, normalized, gathered
        self.align, self.uniform, self.std, self.rank = (values[i:i + 1] for i in range(4))


def representation_stats(hidden, strategy=None, t=2.0):
    """Label-free diagnostics of an embedding batch (csrc/repr.hip), comparable across every pretraining loss.
    hidden [2n, D]: this replica's projections, view a in rows [0, n), view b in rows [n, 2n); always l2-normalised here.  The
    normalised block is gathered over the replicas (view-major, comm.gather_hidden) and every replica runs the kernels on the whole
    [2N, D] block: no collective beyond the gather, and the four values are bitwise the same everywhere.
      align   = mean_i |z_a,i - z_b,i|^2                                       [0, 4], 0 = the views agree
      uniform = mean over the views of log mean_{a != b} exp(-t |z_a - z_b|^2)   [-4t, 0], 0 = one point
      std     = sqrt(D) x the mean per-feature standard deviation              about 1 healthy, 0 collapsed
      rank    = the participation ratio of the covariance spectrum             [1, min(D, N-1)], 0 for a collapsed view
    Takes no gradient, keeps no state and writes nothing it was given."""
    return start_representation_stats(hidden, strategy, t)()


def start_representation_stats(hidden, strategy=None, t=2.0):
    """representation_stats in two halves: checks, normalises and starts the gather now; the zero-argument function it returns waits
    for the gather, runs the kernels and returns the handle (the training step puts the loss between the two)."""
    from . import ops
    from .comm import gather_hidden
    if not torch.is_tensor(hidden) or hidden.dim() != 2 or hidden.shape[0] < 2 or hidden.shape[0] % 2 or hidden.dtype != torch.float32:
        raise ValueError('representation_stats: hidden holds both views, float32 [2n, D] with n >= 1 (got %s %s)'
                         % (tuple(getattr(hidden, 'shape', ())), getattr(hidden, 'dtype', type(hidden))))
    if not ops.repr_dim_ok(hidden.shape[1]):
        raise ValueError('representation_stats supports widths that are multiples of %d in [%d, %d] (got %d)'
                         % (ops.REPR_DIM_STEP, ops.REPR_MIN_DIM, ops.REPR_MAX_DIM, hidden.shape[1]))
    if not ops.repr_t_ok(t):
        raise ValueError('representation_stats: t must lie in (0, %g] (got %r)' % (ops.REPR_MAX_T, t))
    z, _ = ops.l2norm_fwd(hidden.detach().contiguous())
    wait = gather_hidden(z, strategy, async_op=True)

    def finish():
        z_all = wait()
        return ReprStats(ops.repr_stats(z_all, t), z, z_all)
    return finish


class JsonlSummaryWriter:
    """Stand-in for tf.summary.create_file_writer(model_dir) (tf2/run.py:356, :526): every scalar becomes one JSON
    line {"step": s, "tag": name, "value": v} in <model_dir>/summaries.jsonl (TensorBoard-importable, grep-able).
    Callable as writer(name, value, step) -- the hook log_and_write_metrics_to_summary expects."""

    def __init__(self, model_dir, filename='summaries.jsonl'):
        import os
        os.makedirs(model_dir, exist_ok=True)
        self.path = os.path.join(model_dir, filename)
        self._f = open(self.path, 'a')

    def scalar(self, name, value, step):
        import json
        self._f.write(json.dumps({'step': int(step), 'tag': name, 'value': float(value)}) + '\n')

    __call__ = scalar

    def flush(self):
        self._f.flush()

    def close(self):
        self._f.close()


def _float_metric_value(metric):
    return float(metric.result())


def log_and_write_metrics_to_summary(all_metrics, global_step, writer=None):
    """tf2/metrics.py:70-74: log every metric; `writer` (optional) is a callable(name, value, step)."""
    for metric in all_metrics:
        metric_value = _float_metric_value(metric)
        logging.info('Step: [%d] %s = %f', global_step, metric.name, metric_value)
        if writer is not None:
            writer(metric.name, metric_value, global_step)
