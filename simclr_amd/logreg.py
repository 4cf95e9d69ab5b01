"""Cached-feature linear probe of the frozen encoder: encode the training split once under evaluation preprocessing, then fit an
l2-regularised multinomial logistic regression on the cached features with L-BFGS (the transfer protocol of the SimCLR paper, as
defined for this project in DESIGN.md section 30).

  rows         h = model.features(x), NOT l2-normalised, standardised per column with the bank's mean and biased variance
  objective    f(W, b) = (1 / S) sum_n w_n (logsumexp_c s_nc - s_n,y_n) + (l2 / 2) (|W|_F^2 + |b|^2),   s_nc = x_n . W_c + b_c
  solver       L-BFGS (two-loop recursion, history m) from theta = 0 with Armijo backtracking

The two products of an evaluation (the logits X W^T and the gradient G^T X) are HIP kernels (csrc/logreg.hip: ops.logreg_fwd,
ops.logreg_bwd); the vectors of the recursion live on the device in float64.  Replicas hold disjoint shards of the bank: one all-reduce
of a flat [C D + C + 3] buffer per evaluation, the bank is never gathered.
"""
import json
import logging
import math
import os

import torch

from . import ops
from ._lib import lib
from .comm import num_replicas
from .flags import FLAGS
from .resnet import RT

SLAB_ROWS = ops.LOGREG_MAX_ROWS      # rows per kernel call
VAR_EPS = 1e-6                       # x = (h - mu) / sqrt(var + VAR_EPS)
ARMIJO_C1 = 1e-4
MAX_HALVINGS = 30
CURVATURE_EPS = 1e-10                # a pair with s.y <= CURVATURE_EPS |s| |y| is not stored

RESULT_KEYS = ('eval/logreg_top_1_accuracy', 'eval/logreg_top_5_accuracy', 'eval/logreg_loss', 'logreg/train_loss',
               'logreg/train_top_1_accuracy', 'logreg/iterations', 'logreg/evaluations', 'logreg/grad_norm', 'logreg/converged',
               'logreg/l2', 'global_step')


def parse_l2_list(text):
    """--logreg_l2: one value or a comma list of finite numbers > 0, in the order given."""
    parts = [p.strip() for p in str(text).split(',')]
    if not parts or any(not p for p in parts):
        raise ValueError('--logreg_l2 must be a number > 0 or a comma list of them (got %r)' % (text,))
    out = []
    for p in parts:
        try:
            v = float(p)
        except ValueError:
            raise ValueError('--logreg_l2: %r is not a number (got %r)' % (p, text))
        if not (v > 0.0 and math.isfinite(v)):
            raise ValueError('--logreg_l2 values must be finite numbers > 0 (got %r)' % (p,))
        out.append(v)
    return out


def check_fit_arguments(l2, max_iterations, tolerance, history, name='--logreg_'):
    if not (isinstance(l2, (int, float)) and l2 > 0.0 and math.isfinite(l2)):
        raise ValueError('%sl2 must be a finite number > 0 (got %r)' % (name, l2))
    if not 1 <= int(max_iterations) <= 10000:
        raise ValueError('%smax_iterations must be 1..10000 (got %r)' % (name, max_iterations))
    if not 0.0 < float(tolerance) < 1.0:                    # NaN fails the comparison
        raise ValueError('%stolerance must lie in (0, 1) (got %r)' % (name, tolerance))
    if not 1 <= int(history) <= 64:
        raise ValueError('%shistory must be 1..64 (got %r)' % (name, history))


def _slabs(n):
    return [(o, min(n, o + SLAB_ROWS)) for o in range(0, n, SLAB_ROWS)]


def _all_reduce(t, strategy):
    if strategy is not None and num_replicas(strategy) > 1:
        strategy.all_reduce_sum(t)
    return t


def standardize_stats(feats, weights, strategy=None):
    """(mu [D], var [D]) in float64: the mean and the biased variance of the rows of weight > 0 over all replicas, slab by slab in a
    fixed order; the per-replica sums are all-reduced in float64."""
    D = feats.shape[1]
    keep = (weights > 0).to(torch.float64)
    acc = torch.zeros(D + 1, device=feats.device, dtype=torch.float64)
    for o, e in _slabs(feats.shape[0]):
        acc[:D] += (feats[o:e].to(torch.float64) * keep[o:e, None]).sum(0)
        acc[D] += keep[o:e].sum()
    _all_reduce(acc, strategy)
    count = float(acc[D])
    if not count > 0:
        raise ValueError('standardize_stats: no row has a weight > 0')
    mu = acc[:D] / count
    sq = torch.zeros(D, device=feats.device, dtype=torch.float64)
    for o, e in _slabs(feats.shape[0]):
        sq += (((feats[o:e].to(torch.float64) - mu) ** 2) * keep[o:e, None]).sum(0)
    _all_reduce(sq, strategy)
    return mu, sq / count


def standardize(feats, mu, var):
    """fp32 x = (h - mu) / sqrt(var + 1e-6), formed in float64 slab by slab and rounded once."""
    scale = 1.0 / torch.sqrt(var + VAR_EPS)
    out = torch.empty(feats.shape, device=feats.device, dtype=torch.float32)
    for o, e in _slabs(feats.shape[0]):
        out[o:e] = ((feats[o:e].to(torch.float64) - mu) * scale).to(torch.float32)
    return out


_BUFFERS = {}


def _buffers(first, last, D, C, device):
    """One store / lse / workspace per (slab rows, rows of the last slab, D, C, device), reused by every slab of every evaluation: the
    workspace holds the larger of the two needs (the need is not monotone in n: the forward tile edge depends on it)."""
    key = (first, last, D, C, str(device))
    if key not in _BUFFERS:
        _BUFFERS.clear()
        nbytes = max(lib().logreg_workspace_bytes(n, D, C) for n in (first, last))
        _BUFFERS[key] = (torch.empty(first, ops.logreg_store_pitch(C), device=device, dtype=torch.float32),
                         torch.empty(first, device=device, dtype=torch.float64),
                         torch.empty((nbytes + 7) // 8, device=device, dtype=torch.float64))
    return _BUFFERS[key]


def _check_bank(x, labels, weights, C):
    if labels.dtype != torch.int32 or weights.dtype != torch.float32 or labels.shape[0] != x.shape[0] or weights.shape[0] != x.shape[0]:
        raise ValueError('logreg: need int32 labels and float32 weights, one per row of x')
    if x.shape[0] and (int(labels.min()) < 0 or int(labels.max()) >= C):
        raise ValueError('logreg: labels must lie in [0, %d) (got %d .. %d)' % (C, int(labels.min()), int(labels.max())))


def value_and_grad(x, labels, weights, W, b, l2, inv_S, want_grad=True, strategy=None):
    """One evaluation of f at (W [C, D], b [C]) over this replica's rows x [n, D] (fp32, standardised), labels int32 in [0, C) -- checked
    by the caller, see fit -- and weights fp32.  Returns (f, grad, hits, weight): f a float (float64 arithmetic), grad the flat float64
    [C D + C] device vector [dW; db] (None without want_grad), hits = the weighted top-1 hits and weight = the weight total, both over all
    replicas."""
    C, D = W.shape
    flat = torch.zeros(C * D + C + 3, device=W.device, dtype=torch.float64)
    n = x.shape[0]
    if n:
        slabs = _slabs(n)
        store, lse, ws = _buffers(slabs[0][1] - slabs[0][0], slabs[-1][1] - slabs[-1][0], D, C, x.device)
        dW = torch.empty(C, D, device=W.device, dtype=torch.float32) if want_grad else None
        db = torch.empty(C, device=W.device, dtype=torch.float32) if want_grad else None
        for i, (o, e) in enumerate(slabs):
            # a ragged last slab uses the head of store and lse; the workspace is sized for both slab lengths
            out, _, g = ops.logreg_fwd(x[o:e], W, b, labels[o:e], weights[o:e], inv_S, 1 if want_grad else 0, store, lse[:e - o], ws,
                                       check_labels=False)
            flat[C * D + C:] += out
            if want_grad:
                ops.logreg_bwd(g, x[o:e], C, dW, db, accumulate=i > 0, ws=ws)
        if want_grad:
            flat[:C * D] = dW.view(-1)
            flat[C * D:C * D + C] = db
    _all_reduce(flat, strategy)
    theta = torch.cat([W.reshape(-1), b]).to(torch.float64)
    tail = flat[C * D + C:].cpu()
    f = float(tail[0]) * inv_S + 0.5 * l2 * float(torch.dot(theta, theta))
    grad = flat[:C * D + C] + l2 * theta if want_grad else None
    return f, grad, float(tail[1]), float(tail[2])


class LogregFit:
    """What fit returns: W [C, D], b [C] fp32 device tensors and the record of the solve."""

    def __init__(self, W, b, loss, train_top_1, iterations, evaluations, grad_norm, converged, losses):
        self.W, self.b, self.loss, self.train_top_1 = W, b, loss, train_top_1
        self.iterations, self.evaluations, self.grad_norm, self.converged, self.losses = iterations, evaluations, grad_norm, converged, losses


def _direction(g, pairs):
    """-H g by the two-loop recursion; pairs = [(s, y, 1 / s.y)] oldest first; gamma = s.y / y.y of the newest pair.  float64, on the
    device, no host round trip."""
    q = g.clone()
    alphas = []
    for s, y, rho in reversed(pairs):
        a = rho * torch.dot(s, q)
        q -= a * y
        alphas.append(a)
    if pairs:
        s, y, rho = pairs[-1]
        q *= 1.0 / (rho * torch.dot(y, y))
    for (s, y, rho), a in zip(pairs, reversed(alphas)):
        q += (a - rho * torch.dot(y, q)) * s
    return -q


def search_direction(g, pairs):
    """(d, g.d, pairs): the L-BFGS direction; one that is not a descent direction (a history spoilt by rounding) drops the history
    and gives steepest descent."""
    d = _direction(g, pairs)
    gd = float(torch.dot(g, d))
    if not gd < 0.0:
        pairs, d = [], -g
        gd = float(torch.dot(g, d))
    return d, gd, pairs


def fit(x, labels, weights, num_classes, l2, max_iterations=200, tolerance=1e-5, history=10, strategy=None, init=None):
    """Minimise f over this replica's standardised rows x [n, D] (every replica passes its shard).  init = (W, b) warm-starts; the
    default start is 0.  Returns a LogregFit."""
    check_fit_arguments(l2, max_iterations, tolerance, history, name='fit: ')
    C, D = int(num_classes), x.shape[1]
    ops._logreg_check_shape(max(min(x.shape[0], SLAB_ROWS), 1), D, C)
    labels = labels.to(torch.int32).contiguous()
    weights = weights.to(torch.float32).contiguous()
    x = x.contiguous()
    _check_bank(x, labels, weights, C)
    total = _all_reduce(weights.to(torch.float64).sum().view(1), strategy)
    S = float(total)
    if not S > 0:
        raise ValueError('fit: the weights sum to %r' % S)
    inv_S = 1.0 / S
    theta = torch.zeros(C * D + C, device=x.device, dtype=torch.float32)
    if init is not None:
        W0, b0 = init
        if tuple(W0.shape) != (C, D) or tuple(b0.shape) != (C,):
            raise ValueError('fit: init must be (W [%d, %d], b [%d])' % (C, D, C))
        theta = torch.cat([W0.reshape(-1), b0]).to(device=x.device, dtype=torch.float32)

    def split(t):
        return t[:C * D].view(C, D), t[C * D:].contiguous()

    def evaluate(t, want_grad):
        W, b = split(t)
        return value_and_grad(x, labels, weights, W, b, l2, inv_S, want_grad, strategy)

    f, g, hits, _ = evaluate(theta, True)
    evaluations, iterations, converged, losses, pairs = 1, 0, False, [], []
    while True:
        gnorm = float(g.abs().max())
        if gnorm <= tolerance * max(1.0, abs(f)):
            converged = True
            break
        if iterations >= max_iterations:
            break
        d, gd, pairs = search_direction(g, pairs)
        t = min(1.0, 1.0 / float(torch.linalg.vector_norm(g))) if iterations == 0 else 1.0
        theta64 = theta.to(torch.float64)
        accepted = None
        for _ in range(MAX_HALVINGS + 1):
            trial = (theta64 + t * d).to(torch.float32)
            ft = evaluate(trial, False)[0]
            evaluations += 1
            if ft <= f + ARMIJO_C1 * t * gd:
                accepted = trial
                break
            t *= 0.5
        if accepted is None:
            break
        f_new, g_new, hits, _ = evaluate(accepted, True)      # the value of a gradient evaluation is bitwise the trial's
        evaluations += 1
        s = accepted.to(torch.float64) - theta64
        y = g_new - g
        sy = float(torch.dot(s, y))
        if sy > CURVATURE_EPS * float(torch.linalg.vector_norm(s)) * float(torch.linalg.vector_norm(y)):
            pairs.append((s, y, 1.0 / sy))
            pairs = pairs[-int(history):]
        theta, f, g = accepted, f_new, g_new
        iterations += 1
        losses.append(f)
    W, b = split(theta)
    return LogregFit(W.contiguous(), b, f, hits / S, iterations, evaluations, float(g.abs().max()), converged, losses)


def score(x, labels, weights, W, b):
    """fp64 [loss sum, top-1 hits, top-5 hits, weight] of standardised rows x under (W, b): the loss and the top-1 count from the
    kernel's three doubles, top-5 by torch.topk on the stored logits."""
    C, D = W.shape
    labels = labels.to(torch.int32).contiguous()
    weights = weights.to(torch.float32).contiguous()
    _check_bank(x, labels, weights, C)
    counts = torch.zeros(4, device=x.device, dtype=torch.float64)
    for o, e in _slabs(x.shape[0]):
        out, _, logits = ops.logreg_fwd(x[o:e].contiguous(), W, b, labels[o:e], weights[o:e], 1.0, 2, check_labels=False)
        top5 = torch.topk(logits[:, :C], min(5, C), dim=1).indices
        hit5 = (top5 == labels[o:e, None].long()).any(1).to(torch.float64)
        counts += torch.stack([out[0], out[1], (hit5 * weights[o:e].to(torch.float64)).sum(), out[2]])
    return counts


def perform_logreg_evaluation(model, bank_data, eval_data, eval_steps, ckpt, strategy, model_dir=None):
    """Restore `ckpt` as knn.perform_knn_evaluation does, encode `bank_data` (this replica's shard of --train_split under EVALUATION
    preprocessing), standardise, fit one probe per value of --logreg_l2 (each warm-started from the one before), score `eval_steps`
    batches of `eval_data` under each and write logreg_result.json / logreg_result_<step>.json (replica 0): the keys of RESULT_KEYS for
    the LAST l2 plus `fits`, one such record per value.  Nothing is selected."""
    from .checkpoint import Checkpoint
    from .knn import extract_features, reduce_hit_counts
    l2s = parse_l2_list(FLAGS.logreg_l2)
    global_step = 0
    if ckpt:
        model(torch.zeros(2, FLAGS.image_size, FLAGS.image_size, 3, device=RT.device), training=False)
        model.release()
        logging.info('Restoring from %s', ckpt)
        c = Checkpoint(model=model)
        c.restore(ckpt, model_only=False).expect_partial()
        global_step = c.global_step
    feats, labels, weights = extract_features(model, bank_data, normalize=False)
    if not ops.logreg_dim_ok(feats.shape[1]):
        raise ValueError('--logreg_eval needs an encoder width that is a multiple of 64 in [64, 8192] (got %d)' % feats.shape[1])
    mu, var = standardize_stats(feats, weights, strategy)
    x = standardize(feats, mu, var)
    del feats
    queries, num_classes = [], None
    for i in range(eval_steps):
        try:
            xe, lab = next(eval_data)
        except StopIteration:
            break
        num_classes = lab['labels'].shape[1]
        h = model.features(xe)
        w = lab.get('mask')
        w = torch.ones(h.shape[0], device=h.device) if w is None else w
        queries.append((standardize(h, mu, var), lab['labels'].argmax(1), w.to(torch.float32)))
        logging.info('Encoded %d / %d evaluation steps for the linear probe', i + 1, eval_steps)
    if hasattr(eval_data, 'close'):
        eval_data.close()
    if num_classes is None:
        raise ValueError('perform_logreg_evaluation: the evaluation iterator gave no batch')
    fits, init = [], None
    for l2 in l2s:
        res = fit(x, labels, weights, num_classes, l2, FLAGS.logreg_max_iterations, FLAGS.logreg_tolerance, FLAGS.logreg_history,
                  strategy, init)
        init = (res.W, res.b)
        counts = torch.zeros(4, device=x.device, dtype=torch.float64)
        for q, ql, qw in queries:
            counts += score(q, ql, qw, res.W, res.b)
        counts = reduce_hit_counts(counts, strategy).cpu()
        n = max(float(counts[3]), 1.0)
        fits.append({'eval/logreg_top_1_accuracy': float(counts[1]) / n, 'eval/logreg_top_5_accuracy': float(counts[2]) / n,
                     'eval/logreg_loss': float(counts[0]) / n, 'logreg/train_loss': float(res.loss),
                     'logreg/train_top_1_accuracy': float(res.train_top_1), 'logreg/iterations': int(res.iterations),
                     'logreg/evaluations': int(res.evaluations), 'logreg/grad_norm': float(res.grad_norm),
                     'logreg/converged': bool(res.converged), 'logreg/l2': float(l2), 'global_step': int(global_step)})
        logging.info(fits[-1])
    _BUFFERS.clear()
    result = dict(fits[-1])
    if model_dir and (strategy is None or strategy.rank == 0):
        os.makedirs(model_dir, exist_ok=True)
        for name in ('logreg_result.json', 'logreg_result_%d.json' % result['global_step']):
            with open(os.path.join(model_dir, name), 'w') as f:
                json.dump(dict(result, fits=fits), f)
    return result
