"""Weighted k-NN evaluation of the frozen encoder (Wu et al. 2018, "Unsupervised Feature Learning via Non-Parametric Instance
Discrimination"): the head-free quality monitor of self-supervised pretraining.

A query is classified by its k most similar bank rows (cosine similarity of the pooled encoder features), each voting for its class
with weight exp(similarity / temperature).  Nothing is trained and nothing is tuned.  The similarity GEMM, the streaming top-k and the
vote are HIP kernels (csrc/knn.hip: ops.knn_topk, ops.knn_vote); this module extracts the features, shards the work over the replicas
and counts the hits.
"""
import json
import logging
import os

import numpy as np
import torch

from . import ops
from .comm import num_replicas
from .flags import FLAGS
from .resnet import RT


def knn_bank_indices(data_seed, num_examples, num_bank):
    """Examples of the training split in the bank: all of them (num_bank = 0) or the first num_bank positions of the epoch-0
    permutation of the input pipeline -- a class-balanced sample whatever the order of the split on disk."""
    from .data import epoch_permutation
    if not num_bank:
        return np.arange(num_examples, dtype=np.int64)
    if num_bank > num_examples:
        raise ValueError('knn_bank_examples=%d exceeds the %d examples of the split' % (num_bank, num_examples))
    return epoch_permutation(data_seed, 0, num_examples)[:num_bank].astype(np.int64)


def knn_predict(queries, bank, bank_labels, num_classes, k=200, temperature=0.07):
    """queries [Q, D], bank [N, D] fp32 rows (expected L2-normalised; not normalised here), bank_labels [N] class ids.  Returns
    (pred5 [Q, 5] int32, score5 [Q, 5] fp32): the five best classes by (vote score descending, class id ascending), -1 / 0 past the
    number of classes."""
    top_val, top_idx = ops.knn_topk(queries, bank, k)
    top_label = bank_labels.to(torch.int32)[top_idx.long()].contiguous()        # the label gather is a torch index
    return ops.knn_vote(top_val, top_label, num_classes, temperature)


def extract_features(model, data, steps=None, normalize=True):
    """One pass of an eval-style iterator of (features [b, H, W, 3], {'labels': one-hot, 'mask': weights}) through model.features.
    `steps`: batches to read (None: until the iterator ends).  Returns (L2-normalised features [n, C] fp32, labels [n] int64,
    weights [n] fp32); a padded last batch keeps its rows, with weight 0 (absent 'mask' = every sample counts).  normalize=False
    returns the pooled features as they are (simclr_amd/logreg.py standardises them instead)."""
    feats, labels, weights = [], [], []
    i = 0
    while steps is None or i < steps:
        try:
            x, lab = next(data)
        except StopIteration:
            break
        h = model.features(x)
        z = ops.l2norm_fwd(h)[0] if normalize else h
        feats.append(z)
        labels.append(lab['labels'].argmax(1))
        w = lab.get('mask')
        weights.append(torch.ones(z.shape[0], device=z.device, dtype=torch.float32) if w is None else w.to(torch.float32))
        i += 1
    if hasattr(data, 'close'):
        data.close()
    if not feats:
        raise ValueError('extract_features: the iterator gave no batch')
    return torch.cat(feats), torch.cat(labels), torch.cat(weights)


def gather_bank(feats, labels, weights, strategy=None, batch=None):
    """The bank every replica classifies against: all replicas' rows with a non-zero weight.  Each replica passes the rows of ITS
    shard (equal counts: the eval iterator pads); `batch` = rows per replica per step, so that the gathered rows are put back in
    split order (step, replica, row) -- the order one process would have produced -- before the padding is trimmed off."""
    R = num_replicas(strategy)
    if R > 1:
        n = feats.shape[0]
        feats = strategy.all_gather_concat(feats.contiguous())
        labels = strategy.all_gather_concat(labels.contiguous())
        weights = strategy.all_gather_concat(weights.contiguous())
        b = batch or n
        if n % b:
            raise ValueError('gather_bank: %d rows per replica are not whole batches of %d' % (n, b))
        order = torch.arange(R * n, device=feats.device).view(R, n // b, b).permute(1, 0, 2).reshape(-1)
        feats, labels, weights = feats[order], labels[order], weights[order]
    keep = weights > 0
    return feats[keep].contiguous(), labels[keep].contiguous()


def knn_hit_counts(queries, labels, weights, bank, bank_labels, num_classes, k, temperature):
    """fp64 [top-1 hits, top-5 hits, examples] of one query batch, each example counted with its weight."""
    pred5, _ = knn_predict(queries, bank, bank_labels, num_classes, k, temperature)
    hit = pred5.long() == labels.view(-1, 1)
    w = weights.to(torch.float64)
    return torch.stack([(hit[:, 0].to(torch.float64) * w).sum(), (hit.any(1).to(torch.float64) * w).sum(), w.sum()])


def reduce_hit_counts(counts, strategy=None):
    """Replicas classify disjoint query shards: the accuracies are ratios of summed counts (as run.perform_evaluation)."""
    if strategy is not None and num_replicas(strategy) > 1:
        counts = counts.to(RT.device if RT.device is not None else counts.device)
        strategy.all_reduce_sum(counts)
    return counts


def perform_knn_evaluation(model, bank_data, eval_data, eval_steps, ckpt, strategy, model_dir=None):
    """Restore `ckpt` as run.perform_evaluation does, encode `bank_data` (this replica's shard of --train_split under EVALUATION
    preprocessing) into the bank, all-gather it, classify `eval_steps` batches of `eval_data` and write
    eval/knn_top_1_accuracy, eval/knn_top_5_accuracy and global_step to knn_result.json / knn_result_<step>.json (replica 0)."""
    from .checkpoint import Checkpoint
    global_step = 0
    if ckpt:
        # variables exist only after the first forward pass (lazy build), the heads' included
        # (run.main calls this right after perform_evaluation, which has restored the same file when it did not skip: restoring
        # again costs one small forward and keeps this function usable on its own)
        model(torch.zeros(2, FLAGS.image_size, FLAGS.image_size, 3, device=RT.device), training=False)
        model.release()
        logging.info('Restoring from %s', ckpt)
        c = Checkpoint(model=model)
        c.restore(ckpt, model_only=False).expect_partial()
        global_step = c.global_step
    feats, labels, weights = extract_features(model, bank_data)
    bank, bank_labels = gather_bank(feats, labels, weights, strategy, batch=getattr(bank_data, 'b', None))
    del feats
    if bank.shape[0] < FLAGS.knn_k:
        raise ValueError('the k-NN bank holds %d examples, fewer than --knn_k=%d' % (bank.shape[0], FLAGS.knn_k))
    counts = torch.zeros(3, device=bank.device, dtype=torch.float64)
    for i in range(eval_steps):
        try:
            x, lab = next(eval_data)
        except StopIteration:
            break
        num_classes = lab['labels'].shape[1]
        z, _ = ops.l2norm_fwd(model.features(x))
        w = lab.get('mask')
        w = torch.ones(z.shape[0], device=z.device) if w is None else w
        counts += knn_hit_counts(z, lab['labels'].argmax(1), w, bank, bank_labels, num_classes, FLAGS.knn_k, FLAGS.knn_temperature)
        logging.info('Completed k-NN eval for %d / %d steps', i + 1, eval_steps)
    if hasattr(eval_data, 'close'):
        eval_data.close()
    counts = reduce_hit_counts(counts, strategy).cpu()
    n = max(float(counts[2]), 1.0)
    result = {'eval/knn_top_1_accuracy': float(counts[0]) / n, 'eval/knn_top_5_accuracy': float(counts[1]) / n,
              'global_step': int(global_step)}
    logging.info(result)
    if model_dir and (strategy is None or strategy.rank == 0):
        os.makedirs(model_dir, exist_ok=True)
        for name in ('knn_result.json', 'knn_result_%d.json' % result['global_step']):
            with open(os.path.join(model_dir, name), 'w') as f:
                json.dump({k: float(v) for k, v in result.items()}, f)
    return result
