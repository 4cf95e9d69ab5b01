"""k-means clustering evaluation of the frozen encoder: cluster the l2-normalised features of the training split with spherical k-means,
then score the clusters against the labels (NMI, ARI, cluster accuracy) -- the unsupervised protocol, as defined for this project in
DESIGN.md section 31.

  rows         x = l2norm(model.features(image)) under evaluation preprocessing (knn.extract_features)
  assignment   a_n = argmax_k x_n . c_k, ties to the lowest k
  objective    J = (1 / S) sum_n w_n (1 - x_n . c_{a_n}),   S = sum_n w_n
  update       s_k = sum_{n: a_n = k} w_n x_n in float64, c_k = fp32(s_k / |s_k|); a cluster with no weight or |s_k|^2 <= 1e-24 keeps
               its previous centroid (counted in empty_clusters); nothing is split or re-seeded

The assignment (an [n, D] x [D, K] product with a fused arg-max) and the update (a segmented row sum) are HIP kernels
(csrc/kmeans.hip: ops.kmeans_assign, ops.kmeans_update, ops.kmeans_finish).  Replicas hold disjoint shards of the bank: one all-reduce
of a flat float64 [K D + K + 3] buffer per iteration, the bank is never gathered, and every replica takes the same decisions on the
same bits.
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

SLAB_ROWS = ops.KMEANS_MAX_ROWS      # rows per kernel call
MAX_RESTARTS = 16
MAX_ITERATIONS = 1000

RESULT_KEYS = ('eval/kmeans_nmi', 'eval/kmeans_ari', 'eval/kmeans_top_1_accuracy', 'kmeans/inertia', 'kmeans/iterations',
               'kmeans/converged', 'kmeans/empty_clusters', 'kmeans/restart', 'kmeans/k', 'global_step')
MATCHED_KEY = 'eval/kmeans_matched_accuracy'       # present only when K == num_classes and scipy imports


def check_fit_arguments(k, seed, restarts, max_iterations, tolerance, name='--kmeans_'):
    if not ops.KMEANS_MIN_K <= int(k) <= ops.KMEANS_MAX_K:
        raise ValueError('%sk must be %d..%d (got %r)' % (name, ops.KMEANS_MIN_K, ops.KMEANS_MAX_K, k))
    if not 1 <= int(restarts) <= MAX_RESTARTS:
        raise ValueError('%srestarts must be 1..%d (got %r)' % (name, MAX_RESTARTS, restarts))
    if not 1 <= int(max_iterations) <= MAX_ITERATIONS:
        raise ValueError('%smax_iterations must be 1..%d (got %r)' % (name, MAX_ITERATIONS, max_iterations))
    if not 0.0 <= float(tolerance) < 1.0:                   # NaN fails the comparison
        raise ValueError('%stolerance must lie in [0, 1) (got %r)' % (name, tolerance))
    if not 0 <= int(seed) < 2 ** 63:
        raise ValueError('%sseed must be >= 0 (got %r)' % (name, seed))


def _slabs(n):
    return [(o, min(n, o + SLAB_ROWS)) for o in range(0, n, SLAB_ROWS)]


def _all_reduce(t, strategy):
    if strategy is not None and num_replicas(strategy) > 1:
        strategy.all_reduce_sum(t)
    return t


def shard_positions(n, batch, strategy=None):
    """Global position of each of this replica's n rows when every step deals `batch` rows to each replica in replica order (the
    layout of the evaluation iterators): step * batch * R + rank * batch + row."""
    R, rank = num_replicas(strategy), replica_id(strategy)
    i = np.arange(n, dtype=np.int64)
    return (i // batch) * batch * R + rank * batch + i % batch


def start_positions(candidates, k, seed, restart):
    """The global positions restart `restart` starts from: the first k entries of a permutation, drawn from
    numpy.random.default_rng([seed, restart]), of `candidates` (the ascending global positions of the rows of weight > 0)."""
    candidates = np.asarray(candidates, np.int64)
    if k > len(candidates):
        raise ValueError('kmeans: k = %d exceeds the %d rows of weight > 0' % (k, len(candidates)))
    perm = np.random.default_rng([int(seed), int(restart)]).permutation(len(candidates))
    return candidates[perm[:k]]


def _workspace(first, last, D, K, device):
    nbytes = max(lib().kmeans_workspace_bytes(n, D, K) for n in (first, last))
    return torch.empty((nbytes + 7) // 8, device=device, dtype=torch.float64)


class KMeansFit:
    """What fit returns: centroids [K, D] fp32 on the device and the record of the winning restart; restarts = one dict
    (inertia, iterations, converged, empty_clusters) per restart."""

    def __init__(self, centroids, inertia, iterations, converged, empty_clusters, restart, restarts, inertias):
        self.centroids, self.inertia, self.iterations, self.converged = centroids, inertia, iterations, converged
        self.empty_clusters, self.restart, self.restarts, self.inertias = empty_clusters, restart, restarts, inertias


def lloyd(x, weights, centroids, max_iterations, tolerance, strategy=None):
    """Lloyd iterations from `centroids` [K, D] over this replica's rows.  Returns (centroids, J, iterations, converged, empties, Js,
    assignments): J, the assignments and the empty-cluster count belong to the centroids returned."""
    n, D = x.shape
    K = centroids.shape[0]
    dev = x.device
    c = centroids.contiguous()
    assign = torch.full((max(n, 1),), -1, device=dev, dtype=torch.int32)[:n]
    best = torch.empty(n, device=dev, dtype=torch.float32)
    sums = torch.zeros(K, D, device=dev, dtype=torch.float64)
    wsum = torch.zeros(K, device=dev, dtype=torch.float64)
    slabs = _slabs(n)
    ws = _workspace(slabs[0][1] - slabs[0][0], slabs[-1][1] - slabs[-1][0], D, K, dev) if n else ops.kmeans_workspace(1, D, K, dev)
    J_prev, Js, converged, iterations, empties, J = None, [], False, 0, 0, float('nan')
    for it in range(1, int(max_iterations) + 1):
        flat = torch.zeros(K * D + K + 3, device=dev, dtype=torch.float64)
        if n:
            for i, (o, e) in enumerate(slabs):
                _, _, out = ops.kmeans_assign(x[o:e], c, weights[o:e], assign[o:e], best[o:e], ws)
                flat[K * D + K:] += out
                ops.kmeans_update(x[o:e], weights[o:e], assign[o:e], K, sums, wsum, accumulate=i > 0)
            flat[:K * D] = sums.view(-1)
            flat[K * D:K * D + K] = wsum
        _all_reduce(flat, strategy)
        c_next, out2 = ops.kmeans_finish(flat[:K * D].view(K, D), flat[K * D:K * D + K], c, ws=ws)
        tail = torch.cat([flat[K * D + K:], out2]).cpu()
        S, changed, empties = float(tail[1]), float(tail[2]), int(tail[3])
        if not S > 0:
            raise ValueError('kmeans: the weights sum to %r' % S)
        J = float(tail[0]) / S
        iterations = it
        Js.append(J)
        if changed == 0 or (J_prev is not None and J_prev - J <= tolerance * max(J_prev, 1e-30)):
            converged = True
            break
        if it == int(max_iterations):
            break
        c, J_prev = c_next, J
    return c, J, iterations, converged, empties, Js, assign


def fit(x, weights, k, seed=0, restarts=1, max_iterations=50, tolerance=1e-6, strategy=None, init=None, positions=None):
    """Spherical k-means over this replica's unit rows x [n, D] fp32 (every replica passes its shard; padding rows carry weight 0).
    positions: int64 [n] global positions of the rows (default: shard_positions with one batch of n rows per replica); the start rows
    are chosen among the global positions of weight > 0, so the start is the same for any sharding.  init = centroids [K, D] replaces
    the start rule (one restart).  Returns a KMeansFit: the restart with the lowest final J, ties to the lowest restart."""
    check_fit_arguments(k, seed, restarts, max_iterations, tolerance, name='fit: ')
    K = int(k)
    if not torch.is_tensor(x) or x.dim() != 2:
        raise ValueError('fit: need x [n, D]')
    n, D = x.shape
    ops._kmeans_check_shape(max(min(n, SLAB_ROWS), 1), D, K)
    x = x.contiguous()
    weights = weights.to(torch.float32).contiguous()
    if x.dtype != torch.float32 or weights.shape[0] != n:
        raise ValueError('fit: need float32 rows and one weight per row')
    R = num_replicas(strategy)
    starts = []
    if init is not None:
        if tuple(init.shape) != (K, D):
            raise ValueError('fit: init must be centroids [%d, %d]' % (K, D))
        starts.append(init.to(device=x.device, dtype=torch.float32).contiguous())
    else:
        pos = shard_positions(n, max(n, 1), strategy) if positions is None else np.asarray(positions, np.int64)
        if pos.shape != (n,):
            raise ValueError('fit: positions must hold one global position per row')
        span = torch.tensor([float(pos.max()) + 1.0 if n else 0.0], device=x.device, dtype=torch.float64)
        if R > 1:                                            # the largest position over the replicas: a sum of one-hot slots
            slots = torch.zeros(R, device=x.device, dtype=torch.float64)
            slots[replica_id(strategy)] = span[0]
            span = _all_reduce(slots, strategy).max().view(1)
        P = int(span[0])
        pos_t = torch.from_numpy(pos).to(x.device)
        live = weights > 0
        mask = torch.zeros(P, device=x.device, dtype=torch.float64)
        mask[pos_t[live]] = 1.0
        _all_reduce(mask, strategy)
        candidates = torch.nonzero(mask > 0).view(-1).cpu().numpy()
        local = torch.full((P,), -1, device=x.device, dtype=torch.int64)
        local[pos_t[live]] = torch.arange(n, device=x.device)[live]
        for r in range(int(restarts)):
            chosen = torch.from_numpy(start_positions(candidates, K, seed, r)).to(x.device)
            rows = local[chosen]
            buf = torch.zeros(K, D, device=x.device, dtype=torch.float64)
            mine = rows >= 0
            buf[mine] = x[rows[mine]].to(torch.float64)
            _all_reduce(buf, strategy)                       # the other addends are exact zeros: every replica holds the same bits
            starts.append(buf.to(torch.float32))
    records, best = [], None
    for r, c0 in enumerate(starts):
        c, J, iterations, converged, empties, Js, _ = lloyd(x, weights, c0, max_iterations, tolerance, strategy)
        records.append({'inertia': J, 'iterations': iterations, 'converged': converged, 'empty_clusters': empties})
        if best is None or J < best[1]:
            best = (c, J, iterations, converged, empties, r, Js)
    c, J, iterations, converged, empties, r, Js = best
    return KMeansFit(c, J, iterations, converged, empties, r, records, Js)


def assign(x, weights, centroids):
    """(assignments int32 [n], best fp32 [n], out fp64 [3] = {sum w (1 - best), sum w, rows of weight > 0}) of unit rows x under
    `centroids`, slab by slab."""
    n, D = x.shape
    K = centroids.shape[0]
    x = x.contiguous()
    weights = weights.to(torch.float32).contiguous()
    centroids = centroids.contiguous()
    a = torch.full((max(n, 1),), -1, device=x.device, dtype=torch.int32)[:n]
    best = torch.empty(n, device=x.device, dtype=torch.float32)
    total = torch.zeros(3, device=x.device, dtype=torch.float64)
    for o, e in _slabs(n):
        _, _, out = ops.kmeans_assign(x[o:e], centroids, weights[o:e], a[o:e], best[o:e])
        total += out
    return a, best, total


def contingency(assignments, labels, weights, k, num_classes, strategy=None):
    """int64 [k, num_classes]: the rows of weight > 0 counted by (cluster, class) with torch.bincount, all replicas summed."""
    keep = weights > 0
    a, y = assignments[keep].long(), labels[keep].long()
    if a.numel() and (int(a.min()) < 0 or int(a.max()) >= k or int(y.min()) < 0 or int(y.max()) >= num_classes):
        raise ValueError('contingency: assignments must lie in [0, %d) and labels in [0, %d)' % (k, num_classes))
    table = torch.bincount(a * num_classes + y, minlength=k * num_classes).view(k, num_classes)
    if strategy is not None and num_replicas(strategy) > 1:
        t = table.to(torch.float64)                          # counts below 2^53: the sum is exact
        strategy.all_reduce_sum(t)
        table = t.to(torch.int64)
    return table


def _entropy(counts, N):
    c = counts[counts > 0].astype(np.float64)
    return float((c / N * np.log(N / c)).sum())           # the form of the mutual information's terms: identical partitions give exactly 1


def nmi(table):
    """Mutual information over the arithmetic mean of the two entropies; 1 when both partitions are a single block."""
    T = np.asarray(table, np.int64)
    N = float(T.sum())
    if N == 0:
        return 1.0
    a, b = T.sum(1), T.sum(0)
    ha, hb = _entropy(a, N), _entropy(b, N)
    if ha + hb == 0.0:
        return 1.0
    i, j = np.nonzero(T)
    t = T[i, j].astype(np.float64)
    mi = float((t / N * np.log(t * N / (a[i].astype(np.float64) * b[j].astype(np.float64)))).sum())      # integer products: exact
    return mi / (0.5 * (ha + hb))


def ari(table):
    """The adjusted Rand index (Hubert & Arabie); 1 where the index and its expectation coincide at the maximum."""
    T = np.asarray(table, np.int64).astype(np.float64)
    N = T.sum()
    pairs = lambda v: float((v * (v - 1.0) / 2.0).sum())
    total = N * (N - 1.0) / 2.0
    if total == 0:
        return 1.0
    sij, sa, sb = pairs(T), pairs(T.sum(1)), pairs(T.sum(0))
    expected, maximum = sa * sb / total, 0.5 * (sa + sb)
    if maximum == expected:
        return 1.0
    return (sij - expected) / (maximum - expected)


def many_to_one_accuracy(bank_table, eval_table):
    """Every cluster predicts the majority class of its BANK rows (lowest class id on ties); a cluster without bank rows predicts
    nothing: its evaluation rows are misses."""
    B, E = np.asarray(bank_table, np.int64), np.asarray(eval_table, np.int64)
    N = int(E.sum())
    if N == 0:
        return 0.0
    pred = B.argmax(1)                                       # numpy's argmax returns the first maximum
    seen = B.sum(1) > 0
    return float(E[np.arange(E.shape[0]), pred][seen].sum()) / N


def matched_accuracy(eval_table):
    """One-to-one matching of clusters to classes that maximises the hits on `eval_table` (matched on the split it scores); None when
    the table is not square or scipy does not import."""
    E = np.asarray(eval_table, np.int64)
    if E.shape[0] != E.shape[1]:
        return None
    try:
        from scipy.optimize import linear_sum_assignment
    except ImportError:
        return None
    N = int(E.sum())
    if N == 0:
        return 0.0
    rows, cols = linear_sum_assignment(E, maximize=True)
    return float(E[rows, cols].sum()) / N


def scores(bank_table, eval_table):
    """The evaluation scores from the two contingency tables [K, num_classes], in float64 on the host."""
    bank_table = bank_table.cpu().numpy() if torch.is_tensor(bank_table) else np.asarray(bank_table)
    eval_table = eval_table.cpu().numpy() if torch.is_tensor(eval_table) else np.asarray(eval_table)
    out = {'eval/kmeans_nmi': nmi(eval_table), 'eval/kmeans_ari': ari(eval_table),
           'eval/kmeans_top_1_accuracy': many_to_one_accuracy(bank_table, eval_table)}
    m = matched_accuracy(eval_table)
    if m is not None:
        out[MATCHED_KEY] = m
    return out


def perform_kmeans_evaluation(model, bank_data, eval_data, eval_steps, ckpt, strategy, model_dir=None):
    """Restore `ckpt` as knn.perform_knn_evaluation does, encode `bank_data` (this replica's shard of --train_split under EVALUATION
    preprocessing), fit --kmeans_restarts spherical k-means on it, assign the bank and `eval_steps` batches of `eval_data` to the
    winning centroids, score and write kmeans_result.json / kmeans_result_<step>.json (replica 0): the keys of RESULT_KEYS (and
    MATCHED_KEY when K equals the class count) plus `restarts`, one record per restart.  Nothing is chosen on the evaluation split."""
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
    batches = []

    def counted(it):
        for item in it:
            batches.append(item[0].shape[0])
            yield item
    x, labels, weights = extract_features(model, counted(bank_data), normalize=True)
    if hasattr(bank_data, 'close'):
        bank_data.close()
    if not ops.kmeans_dim_ok(x.shape[1]):
        raise ValueError('--kmeans_eval needs an encoder width that is a multiple of 64 in [64, 8192] (got %d)' % x.shape[1])
    if len(set(batches)) != 1:
        raise ValueError('perform_kmeans_evaluation: the bank iterator must give equal batches (got %r)' % sorted(set(batches)))
    queries, num_classes = [], None
    for i in range(eval_steps):
        try:
            xe, lab = next(eval_data)
        except StopIteration:
            break
        num_classes = lab['labels'].shape[1]
        z = ops.l2norm_fwd(model.features(xe))[0]
        w = lab.get('mask')
        w = torch.ones(z.shape[0], device=z.device) if w is None else w
        queries.append((z, lab['labels'].argmax(1), w.to(torch.float32)))
        logging.info('Encoded %d / %d evaluation steps for the k-means evaluation', i + 1, eval_steps)
    if hasattr(eval_data, 'close'):
        eval_data.close()
    if num_classes is None:
        raise ValueError('perform_kmeans_evaluation: the evaluation iterator gave no batch')
    K = int(FLAGS.kmeans_k) or int(num_classes)
    res = fit(x, weights, K, FLAGS.kmeans_seed, FLAGS.kmeans_restarts, FLAGS.kmeans_max_iterations, FLAGS.kmeans_tolerance, strategy,
              positions=shard_positions(x.shape[0], batches[0], strategy))
    bank_assign, _, _ = assign(x, weights, res.centroids)
    bank_table = contingency(bank_assign, labels, weights, K, num_classes, strategy)
    eval_table = torch.zeros(K, num_classes, device=x.device, dtype=torch.int64)
    for q, ql, qw in queries:
        qa, _, _ = assign(q, qw, res.centroids)
        eval_table += contingency(qa, ql, qw, K, num_classes, None)
    if strategy is not None and num_replicas(strategy) > 1:
        t = eval_table.to(torch.float64)
        strategy.all_reduce_sum(t)
        eval_table = t.to(torch.int64)
    result = scores(bank_table, eval_table)
    result.update({'kmeans/inertia': float(res.inertia), 'kmeans/iterations': int(res.iterations), 'kmeans/converged': bool(res.converged),
                   'kmeans/empty_clusters': int(res.empty_clusters), 'kmeans/restart': int(res.restart), 'kmeans/k': K,
                   'global_step': int(global_step)})
    logging.info(result)
    if model_dir and (strategy is None or strategy.rank == 0):
        os.makedirs(model_dir, exist_ok=True)
        for name in ('kmeans_result.json', 'kmeans_result_%d.json' % result['global_step']):
            with open(os.path.join(model_dir, name), 'w') as f:
                json.dump(dict(result, restarts=res.restarts), f)
    return result
