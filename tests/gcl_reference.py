"""Float64 reference of the generalized contrastive loss (objective.generalized_contrastive_loss / csrc/gcl.hip), written with
explicit formulas (the loss of colabs/intriguing_properties/generalized_contrastive_loss.ipynb, restated).

R replicas; replica r holds h_r [2n, D] = [view-1 rows; view-2 rows].  z_r = l2-normalised h_r (hidden_norm) or h_r itself.
z_all [M, D], M = 2N = 2 R n: every replica's view-1 rows, then every replica's view-2 rows (the NT-Xent layout).

    align_r = mean_{n x D}((z1_r - z2_r)^2) / 2
    loss_r  = loss_scaling * (align_r + lambda_weight * dist_r)
    objective of the step = (1 / R) sum_r loss_r

dist = 'logsumexp':  L_i = logsumexp_{j in all M columns}(z_i . z_j / T)   (self column included, nothing masked)
                     dist_r = mean_{i in r's 2n rows}(L_i) - log D           (the log of the hidden WIDTH)
    With P = row-softmax of z_all z_all^T / T:  d(sum_i L_i) / d z_all = (P + P^T) z_all / T, hence
    d objective / d z_all = loss_scaling * lambda_weight / (M T) * (P + P^T) z_all  (+ the alignment part).

dist = 'normal' | 'uniform' (sliced Wasserstein):  P = z_all W, Q = prior W (prior rows l2-normalised when hidden_norm),
    every column sorted ascending over the M rows, EQUAL KEYS ORDERED BY ROW INDEX (numpy.argsort(kind='stable')),
                     dist_r = mean_{D x M}((Q_sorted - P_sorted)^2)          (the same global term on every replica)
    d dist / d P[perm[k, c], c] = 2 (P_sorted[k, c] - Q_sorted[k, c]) / (D M),  d dist / d z_all = (d dist / d P) W^T.

alignment:           d align_r / d z1_r = (z1_r - z2_r) / (n D),  d align_r / d z2_r = -(z1_r - z2_r) / (n D)
l2 normalisation:    z = h / |h|:  d/dh = (dz - z (z . dz)) / |h|

tests/test_gcl_reference.py pins this file against torch float64 autograd, hand-derived cases and the tie rule."""
import numpy as np

DISTS = ('logsumexp', 'normal', 'uniform')


def l2_normalize(h):
    nrm = np.sqrt(np.maximum((h * h).sum(axis=1, keepdims=True), 1e-12))
    return h / nrm, nrm


def stable_argsort_columns(P):
    """perm [M, D]: perm[k, c] = row of the k-th smallest entry of column c, equal keys by row index."""
    return np.argsort(P, axis=0, kind='stable')


def z_all_of(zs, n):
    return np.concatenate([z[:n] for z in zs] + [z[n:] for z in zs], axis=0)


def logsumexp_rows(S):
    m = S.max(axis=1, keepdims=True)
    return (m + np.log(np.exp(S - m).sum(axis=1, keepdims=True)))[:, 0]


def gcl_reference(hiddens, lambda_weight=1.0, temperature=1.0, dist='normal', hidden_norm=True, loss_scaling=1.0, rand_w=None, prior=None,
                  perm=None):
    """hiddens: list over replicas of [2n, D] array-likes.  rand_w [D, D], prior [M, D]: SWD only.  perm [M, D]: sort P's columns
    with THIS permutation instead of the stable argsort (the caller has checked that it sorts them).
    Returns dict(loss, align, dist: lists over replicas; grads: list over replicas of d objective / d h_r; perm; P) in float64."""
    if dist not in DISTS:
        raise ValueError('Unknown prior {}'.format(dist))
    hs = [np.asarray(h, dtype=np.float64) for h in hiddens]
    R = len(hs)
    n, D = hs[0].shape[0] // 2, hs[0].shape[1]
    N, M = R * n, 2 * R * n
    T, lam, ls = float(temperature), float(lambda_weight), float(loss_scaling)
    if hidden_norm:
        zs, nrms = zip(*[l2_normalize(h) for h in hs])
    else:
        zs, nrms = hs, [None] * R
    z_all = z_all_of(zs, n)
    align = [float(((z[:n] - z[n:]) ** 2).mean() / 2.0) for z in zs]
    g_all = np.zeros_like(z_all)                      # d objective / d z_all, distribution term
    P = None
    if dist == 'logsumexp':
        S = z_all @ z_all.T / T
        L = logsumexp_rows(S)
        soft = np.exp(S - L[:, None])
        dists = []
        for r in range(R):
            rows = np.concatenate([np.arange(r * n, (r + 1) * n), N + np.arange(r * n, (r + 1) * n)])
            dists.append(float(L[rows].mean() - np.log(D)))
        g_all = ls * lam / (M * T) * ((soft + soft.T) @ z_all)
    else:
        W = np.asarray(rand_w, dtype=np.float64)
        pr = np.asarray(prior, dtype=np.float64)
        assert W.shape == (D, D) and pr.shape == (M, D)
        if hidden_norm:
            pr = l2_normalize(pr)[0]
        P, Q = z_all @ W, pr @ W
        if perm is None:
            perm = stable_argsort_columns(P)
        perm = np.asarray(perm)
        Ps = np.take_along_axis(P, perm, axis=0)
        Qs = np.sort(Q, axis=0)
        d = float(((Qs - Ps) ** 2).mean())
        dists = [d] * R
        dP = np.zeros_like(P)
        np.put_along_axis(dP, perm, 2.0 * (Ps - Qs) / (D * M), axis=0)
        g_all = ls * lam * (dP @ W.T)
    grads = []
    for r in range(R):
        z = zs[r]
        a = (z[:n] - z[n:]) / (n * D) * (ls / R)
        dz = np.concatenate([g_all[r * n:(r + 1) * n] + a, g_all[N + r * n:N + (r + 1) * n] - a], axis=0)
        if hidden_norm:
            dz = (dz - z * (z * dz).sum(axis=1, keepdims=True)) / nrms[r]
        grads.append(dz)
    loss = [ls * (align[r] + lam * dists[r]) for r in range(R)]
    return dict(loss=loss, align=align, dist=dists, grads=grads, perm=perm, P=P)
