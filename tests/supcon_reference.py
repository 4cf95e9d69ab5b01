"""Float64 restatement of the supervised contrastive loss (objective.add_supcon_loss / csrc/supcon.hip): Khosla et al. 2020,
Supervised Contrastive Learning, the L_out^sup form, written with explicit formulas.

R replicas; replica r holds h_r [2n, D] = [view-1 rows; view-2 rows] and the labels y_r [n] of its images (both views share a label).
z_r = l2-normalised h_r (hidden_norm) or h_r itself.  z_all [2N, D], N = R n: every replica's view-1 rows, then every replica's view-2
rows (the NT-Xent layout); column j has label y_all[j mod N], y_all = concat_r(y_r).  Local row i of replica r (view v = i // n, sample
s = i % n) is global column self(i) = v N + r n + s.

    A(i) = all 2N columns except self(i)
    P(i) = {p in A(i): label(p) == label(i)}          (the other view of the same image is in it: |P(i)| >= 1)
    l_i  = logsumexp_{a in A(i)}(z_i . z_a / T) - (1 / |P(i)|) sum_{p in P(i)} z_i . z_p / T
    loss_r = (1 / n) sum_{i in r's 2n rows} l_i       (the sum of the two per-view means, as tf2/objective.py:76-87 forms NT-Xent;
                                                       the temperature / base_temperature factor of the paper's code is left out)
    objective of the step = (1 / R) sum_r loss_r
    contrast_acc_r       = share of r's 2n rows with max_{p in P(i)} s_ip >= max_{a in A(i) \\ P(i)} s_ia (no non-positive column: a hit)
    contrast_positives_r = mean of |P(i)| over r's 2n rows

With W_ia = softmax_{A(i)}(s_i)_a - [a in P(i)] / |P(i)| for a in A(i) and W_{i, self(i)} = 0 over ALL 2N global rows i (every row is a
local row of exactly one replica), d(sum_r loss_r) / d z_all = (W + W^T) z_all / (n T), hence
    d objective / d z_all = (W + W^T) z_all / (R n T)
l2 normalisation:    z = h / |h|:  d/dh = (dz - z (z . dz)) / |h|

tests/test_supcon_reference.py pins this file against torch float64 autograd, a hand-derived case and the NT-Xent oracle."""
import numpy as np


def l2_normalize(h):
    nrm = np.sqrt(np.maximum((h * h).sum(axis=1, keepdims=True), 1e-12))
    return h / nrm, nrm


def z_all_of(zs, n):
    return np.concatenate([z[:n] for z in zs] + [z[n:] for z in zs], axis=0)


def replica_rows(r, n, N):
    """Global rows of replica r's [view-1; view-2] block."""
    return np.concatenate([np.arange(r * n, (r + 1) * n), N + np.arange(r * n, (r + 1) * n)])


def supcon_reference(hiddens, labels, hidden_norm=True, temperature=1.0):
    """hiddens: list over replicas of [2n, D] array-likes; labels: list over replicas of [n] integer class ids.
    Returns dict(loss, acc, positives: lists over replicas; grads: list over replicas of d objective / d h_r; pcount [2N]) in float64."""
    hs = [np.asarray(h, dtype=np.float64) for h in hiddens]
    R = len(hs)
    n = hs[0].shape[0] // 2
    N, M = R * n, 2 * R * n
    T = float(temperature)
    y = np.concatenate([np.asarray(l).reshape(-1) for l in labels])
    assert y.shape == (N,), 'one label per image of the global batch'
    if hidden_norm:
        zs, nrms = zip(*[l2_normalize(h) for h in hs])
    else:
        zs, nrms = hs, [None] * R
    z_all = z_all_of(zs, n)
    ycol = np.concatenate([y, y])
    S = z_all @ z_all.T / T
    not_self = ~np.eye(M, dtype=bool)
    pos = (ycol[:, None] == ycol[None, :]) & not_self
    pcount = pos.sum(axis=1)
    assert (pcount >= 1).all()
    Sm = np.where(not_self, S, -np.inf)
    m = Sm.max(axis=1, keepdims=True)
    lse = (m + np.log(np.exp(Sm - m).sum(axis=1, keepdims=True)))[:, 0]
    row = lse - np.where(pos, S, 0.0).sum(axis=1) / pcount
    pmax = np.where(pos, S, -np.inf).max(axis=1)
    omax = np.where(not_self & ~pos, S, -np.inf).max(axis=1)
    hit = pmax >= omax
    W = np.exp(Sm - lse[:, None]) - pos / pcount[:, None]
    g_all = (W + W.T) @ z_all / (R * n * T)
    loss, acc, positives, grads = [], [], [], []
    for r in range(R):
        rows = replica_rows(r, n, N)
        loss.append(float(row[rows].sum() / n))
        acc.append(float(hit[rows].sum() / (2.0 * n)))
        positives.append(float(pcount[rows].sum() / (2.0 * n)))
        dz = g_all[rows]
        if hidden_norm:
            dz = (dz - zs[r] * (zs[r] * dz).sum(axis=1, keepdims=True)) / nrms[r]
        grads.append(dz)
    return dict(loss=loss, acc=acc, positives=positives, grads=grads, pcount=pcount)
