"""Eigen-spectrum evaluation of the frozen encoder: how many dimensions of the encoder output are in use.  The definitions are this
project's own choices, not a restatement of a paper's protocol.

  rows         h_n = model.features(image) under evaluation preprocessing, NOT normalised (knn.extract_features(normalize=False))
  counted      a row counts once when its weight is > 0 and not at all otherwise; S = the counted rows of all replicas
  mean         mu = (1 / S) sum h_n                              float64
  covariance   C = (1 / (S - 1)) sum (h_n - mu)(h_n - mu)^T      float64 [D, D]
  spectrum     lambda_1 >= ... >= lambda_D = numpy.linalg.eigvalsh(C) on replica 0, negative values set to 0 and counted

The column sums and the centred product are HIP kernels (csrc/spectrum.hip: ops.spectrum_colsum, ops.spectrum_cov).  The kernel centres
with mu32 = fp32(mu); the exact correction - S delta delta^T, delta = mu - mu32, is applied here in float64 (sum (h - mu32) = S delta).
Replicas hold disjoint shards of the bank: one float64 all-reduce of [D + 1] and one of [D D], the bank is never gathered.  The
eigenvalues travel from replica 0 to the others through a zero-filled buffer and an all-reduce (the way kmeans.fit shares its start
rows), so every replica holds the same bits.
"""
import json
import logging
import os

import numpy as np
import torch

from . import ops
from ._lib import lib
from .comm import num_replicas, replica_id
from .flags import FLAGS
from .resnet import RT

SLAB_ROWS = ops.SPECTRUM_MAX_ROWS      # rows per kernel call
COLLAPSE_TRACE = 1e-12                 # tr C at or below this: one point, every score 0 (the rule of train/repr_rank)
RANKME_EPS = 1e-7
ALPHA_MIN_POINTS = 8

RESULT_KEYS = ('eval/spectrum_rankme', 'eval/spectrum_participation_ratio', 'eval/spectrum_numerical_rank', 'eval/spectrum_top1_share',
               'eval/spectrum_dims_90', 'eval/spectrum_dims_99', 'spectrum/trace', 'spectrum/rows', 'spectrum/dim',
               'spectrum/negative_eigenvalues', 'global_step')
ALPHA_KEY = 'eval/spectrum_alpha'      # absent when the fit would have fewer than ALPHA_MIN_POINTS points


def check_score_arguments(rank_threshold, alpha_first, alpha_last, name='--spectrum_'):
    if not 0.0 < float(rank_threshold) < 1.0:               # NaN fails the comparison
        raise ValueError('%srank_threshold must lie in (0, 1) (got %r)' % (name, rank_threshold))
    if int(alpha_first) < 1:
        raise ValueError('%salpha_first must be >= 1 (got %r)' % (name, alpha_first))
    if int(alpha_last) != 0 and int(alpha_last) < int(alpha_first) + ALPHA_MIN_POINTS - 1:
        raise ValueError('%salpha_last must be 0 (the numerical rank) or >= %salpha_first + %d (got %r with first = %r)'
                         % (name, name, ALPHA_MIN_POINTS - 1, alpha_last, alpha_first))


def _slabs(n):
    return [(o, min(n, o + SLAB_ROWS)) for o in range(0, n, SLAB_ROWS)]


def _all_reduce(t, strategy):
    if strategy is not None and num_replicas(strategy) > 1:
        strategy.all_reduce_sum(t)
    return t


def covariance(feats, weights, strategy=None):
    """(C float64 [D, D] on the device, S, mu float64 [D]) of this replica's rows feats [n, D] fp32 and weights [n] (every replica
    passes its shard; padding rows carry weight 0).  Two passes over the slabs, one all-reduce of [D + 1] and one of [D D]."""
    if not torch.is_tensor(feats) or feats.dim() != 2:
        raise ValueError('covariance: need feats [n, D]')
    n, D = feats.shape
    if not ops.spectrum_dim_ok(D):
        raise ValueError('covariance: the width must be a multiple of %d in [%d, %d] (got %d)'
                         % (ops.SPECTRUM_DIM_STEP, ops.SPECTRUM_MIN_DIM, ops.SPECTRUM_MAX_DIM, D))
    if feats.dtype != torch.float32 or not torch.is_tensor(weights) or tuple(weights.shape) != (n,):
        raise ValueError('covariance: need float32 rows and one weight per row')
    x = feats.contiguous()
    w = weights.to(torch.float32).contiguous()
    dev = x.device
    slabs = _slabs(n)
    ws = None
    if n:
        nbytes = max(lib().spectrum_workspace_bytes(e - o, D) for o, e in (slabs[0], slabs[-1]))
        ws = torch.empty((nbytes + 7) // 8, device=dev, dtype=torch.float64)
    sums = torch.zeros(D + 1, device=dev, dtype=torch.float64)
    for i, (o, e) in enumerate(slabs):
        ops.spectrum_colsum(x[o:e], w[o:e], sums, accumulate=i > 0, ws=ws)
    _all_reduce(sums, strategy)
    S = float(sums[D])
    if not S >= 2:
        raise ValueError('covariance: %r rows of weight > 0; a covariance needs at least 2' % S)
    mu = sums[:D] / S
    mu32 = mu.to(torch.float32)
    cov = torch.zeros(D, D, device=dev, dtype=torch.float64)
    for i, (o, e) in enumerate(slabs):
        ops.spectrum_cov(x[o:e], w[o:e], mu32, cov, accumulate=i > 0, ws=ws)
    _all_reduce(cov.view(-1), strategy)
    delta = mu - mu32.to(torch.float64)
    C = (cov - S * torch.outer(delta, delta)) / (S - 1.0)
    return C, S, mu


def eigenvalues(C, strategy=None):
    """numpy float64 [D], descending: numpy.linalg.eigvalsh of C on replica 0, shared with the other replicas through a zero buffer and
    an all-reduce (the other addends are exact zeros: every replica holds the same bits)."""
    D = C.shape[0]
    buf = torch.zeros(D, device=C.device, dtype=torch.float64)
    if replica_id(strategy) == 0:
        lam = np.linalg.eigvalsh(C.detach().cpu().numpy().astype(np.float64))[::-1].copy()
        buf.copy_(torch.from_numpy(lam))
    _all_reduce(buf, strategy)
    return buf.cpu().numpy()


def scores(lam, rank_threshold=1e-6, alpha_first=10, alpha_last=0):
    """The scores of a spectrum, in float64 on the host.  lam: eigenvalues in any order; negative values are set to 0 and counted."""
    check_score_arguments(rank_threshold, alpha_first, alpha_last, name='scores: ')
    lam = np.sort(np.asarray(lam, np.float64).reshape(-1))[::-1].copy()
    negative = int((lam < 0).sum())
    lam[lam < 0] = 0.0
    D = lam.shape[0]
    trace = float(lam.sum())
    out = {'spectrum/trace': trace, 'spectrum/dim': int(D), 'spectrum/negative_eigenvalues': negative}
    if not trace > COLLAPSE_TRACE:
        out.update({'eval/spectrum_rankme': 0.0, 'eval/spectrum_participation_ratio': 0.0, 'eval/spectrum_numerical_rank': 0,
                    'eval/spectrum_top1_share': 0.0, 'eval/spectrum_dims_90': 0, 'eval/spectrum_dims_99': 0})
        return out
    sigma = np.sqrt(lam)
    p = sigma / sigma.sum() + RANKME_EPS
    out['eval/spectrum_rankme'] = float(np.exp(-(p * np.log(p)).sum()))
    out['eval/spectrum_participation_ratio'] = float(trace * trace / (lam * lam).sum())
    rank = int((lam > float(rank_threshold) * lam[0]).sum())
    out['eval/spectrum_numerical_rank'] = rank
    out['eval/spectrum_top1_share'] = float(lam[0] / trace)
    cum = np.cumsum(lam)
    for key, share in (('eval/spectrum_dims_90', 0.9), ('eval/spectrum_dims_99', 0.99)):
        out[key] = int(min(D, np.searchsorted(cum, share * trace, side='left') + 1))
    last = min(int(alpha_last) or rank, rank)
    first = int(alpha_first)
    if last - first + 1 >= ALPHA_MIN_POINTS:
        i = np.arange(first, last + 1, dtype=np.float64)
        u, v = np.log(i), np.log(lam[first - 1:last])
        u = u - u.mean()
        out[ALPHA_KEY] = float(-(u * (v - v.mean())).sum() / (u * u).sum())
    return out


def perform_spectrum_evaluation(model, bank_data, ckpt, strategy, model_dir=None):
    """Restore `ckpt` as knn.perform_knn_evaluation does, encode `bank_data` (this replica's shard of --train_split under EVALUATION
    preprocessing), take the covariance of the unnormalised features over all replicas, its eigenvalues and their scores, and write
    spectrum_result.json / spectrum_result_<step>.json (replica 0): the keys of RESULT_KEYS (and ALPHA_KEY when the fit has enough
    points) plus `eigenvalues`, the D values in descending order.  No label is read."""
    from .checkpoint import Checkpoint
    from .knn import extract_features
    global_step = 0
    if ckpt:
        model(torch.zeros(2, FLAGS.image_size, FLAGS.image_size, 3, device=RT.device), training=False)
        model.release()
        logging.info('Restoring from %s', ckpt)
        c = Checkpoint(model=model)
        c.restore(ckpt, model_only=False).expect_partial()
        global_step = c.global_step
    x, _, weights = extract_features(model, bank_data, normalize=False)
    if not ops.spectrum_dim_ok(x.shape[1]):
        raise ValueError('--spectrum_eval needs an encoder width that is a multiple of 64 in [64, 8192] (got %d)' % x.shape[1])
    C, S, _ = covariance(x, weights, strategy)
    lam = eigenvalues(C, strategy)
    result = scores(lam, FLAGS.spectrum_rank_threshold, FLAGS.spectrum_alpha_first, FLAGS.spectrum_alpha_last)
    result.update({'spectrum/rows': int(S), 'global_step': int(global_step)})
    logging.info(result)
    if model_dir and (strategy is None or strategy.rank == 0):
        os.makedirs(model_dir, exist_ok=True)
        for name in ('spectrum_result.json', 'spectrum_result_%d.json' % result['global_step']):
            with open(os.path.join(model_dir, name), 'w') as f:
                json.dump(dict(result, eigenvalues=[float(max(v, 0.0)) for v in lam]), f)
    return result
