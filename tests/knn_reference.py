"""numpy float64 restatement of the weighted k-NN evaluation (simclr_amd/knn.py, csrc/knn.hip; Wu et al. 2018).

  similarities  s(i, j) = sum_d q[i, d] * bank[j, d]
  top-k         row i = the first k pairs of the total order (similarity descending, bank index ascending): np.lexsort on
                (index, -similarity); a NaN similarity sorts last
  vote          w_r = exp((v_r - v_0) / T), score_c = the w_r of the neighbours of class c added in ascending rank order r
  top-5         classes by (score descending, class id ascending); -1 / 0 past the number of classes
"""
import numpy as np


def similarities(q, bank):
    return np.asarray(q, np.float64) @ np.asarray(bank, np.float64).T


def topk(sim, k):
    """sim [Q, N] -> (val [Q, k] float64, idx [Q, k] int64)."""
    sim = np.asarray(sim, np.float64)
    Q, N = sim.shape
    assert 1 <= k <= N
    ar = np.arange(N)
    idx = np.stack([np.lexsort((ar, -sim[i]))[:k] for i in range(Q)])
    return np.take_along_axis(sim, idx, 1), idx


def class_scores(top_val, top_label, num_classes, temperature):
    """[Q, num_classes] float64 scores, accumulated in rank order."""
    top_val = np.asarray(top_val, np.float64)
    Q, k = top_val.shape
    w = np.exp((top_val - top_val[:, :1]) / float(temperature))
    scores = np.zeros((Q, num_classes), np.float64)
    for r in range(k):
        np.add.at(scores, (np.arange(Q), np.asarray(top_label)[:, r]), w[:, r])
    return scores


def top5(scores):
    """(pred [Q, 5] int64, score [Q, 5] float64) by (score descending, class ascending); -1 / 0 past the number of classes."""
    Q, C = scores.shape
    ar = np.arange(C)
    pred = np.full((Q, 5), -1, np.int64)
    sc = np.zeros((Q, 5), np.float64)
    for i in range(Q):
        o = np.lexsort((ar, -scores[i]))[:5]
        pred[i, :len(o)] = o
        sc[i, :len(o)] = scores[i, o]
    return pred, sc


def vote(top_val, top_label, num_classes, temperature):
    return top5(class_scores(top_val, top_label, num_classes, temperature))


def predict(q, bank, bank_labels, num_classes, k, temperature):
    val, idx = topk(similarities(q, bank), k)
    return vote(val, np.asarray(bank_labels)[idx], num_classes, temperature)


def decided_rows(scores, rel=1e-4):
    """(top-1 decided [Q], top-5 decided [Q]): rows whose float64 margin between the rank-1 and rank-2 score (rank-5 and rank-6)
    exceeds `rel` relative to the larger one -- the rows on which an fp32 vote must give the same classes.  Two classes without any
    neighbour score exactly 0 in every precision and are ordered by class id: that tie is decided too."""
    s = -np.sort(-scores, axis=1)
    C = s.shape[1]
    d1 = np.ones(len(s), bool) if C < 2 else ((s[:, 0] - s[:, 1]) > rel * np.abs(s[:, 0])) | ((s[:, 0] == 0) & (s[:, 1] == 0))
    d5 = np.ones(len(s), bool) if C < 6 else ((s[:, 4] - s[:, 5]) > rel * np.abs(s[:, 4])) | ((s[:, 4] == 0) & (s[:, 5] == 0))
    return d1, d5


def hit_counts(pred5, labels, weights=None):
    """[top-1 hits, top-5 hits, examples], each example counted with its weight."""
    labels = np.asarray(labels).reshape(-1, 1)
    w = np.ones(len(labels)) if weights is None else np.asarray(weights, np.float64)
    hit = np.asarray(pred5) == labels
    return np.array([(hit[:, 0] * w).sum(), (hit.any(1) * w).sum(), w.sum()])
