"""Float64 restatement of the Barlow Twins loss (objective.add_barlow_twins_loss / csrc/barlow.hip): Zbontar et al. 2021, Barlow Twins:
Self-Supervised Learning via Redundancy Reduction, written with explicit formulas -- once in the DIRECT form (the D x D
cross-correlation matrix) and once in the GRAM form the kernels run, which never builds that matrix.

R replicas; replica r holds h_r [2n, D] = [view-1 rows; view-2 rows].  h_all [2N, D], N = R n: every replica's view-1 rows, then every
replica's view-2 rows (the NT-Xent layout).  Per view v and column j over the N rows of the GLOBAL batch:
    mu = mean_a h_aj,  var = mean_a (h_aj - mu)^2 (biased),  zhat = (h - mu) / sqrt(var + eps)

direct form:
    C   = zhat1^T zhat2 / N                              [D, D]
    on  = sum_i (1 - C_ii)^2,   off = sum_{i != j} C_ij^2
    L   = loss_scaling * (on + lambda * off)
    M   = dL/dC = loss_scaling * (2 lambda C + diag(-2 (1 - c) - 2 lambda c)),  c = diag(C)
    dL/dzhat1 = zhat2 M^T / N,   dL/dzhat2 = zhat1 M / N
Gram form:
    G1 = zhat1 zhat1^T, G2 = zhat2 zhat2^T [N, N];  sum_ij C_ij^2 = tr(C^T C) = (1 / N^2) sum_ab G1_ab G2_ab
    off = (1 / N^2) sum_ab G1_ab G2_ab - sum_i c_i^2
    replica r owns the rows a in [r n, (r + 1) n) against all N columns and reports
        loss_r = loss_scaling * (on + lambda * (R / N^2 * sum_{a in r, b} G1_ab G2_ab - sum_i c_i^2));   mean_r loss_r = L
    g1_a = dL/dzhat1_a = loss_scaling * (lambda * (2 / N^2) * sum_b G2_ab zhat1_b + d o zhat2_a / N),  d = -2 (1 - c) - 2 lambda c
    (view 2: G1, zhat2_b, zhat1_a)
standardisation backward, per view:  dL/dh_a = (g_a - mean_N(g) - zhat_a o mean_N(g o zhat)) / sqrt(var + eps), means over the GLOBAL batch.

tests/test_barlow_reference.py pins both forms against torch float64 autograd of the direct form and a hand-derived case."""
import numpy as np


def h_all_of(hs, n):
    return np.concatenate([h[:n] for h in hs] + [h[n:] for h in hs], axis=0)


def replica_rows(r, n, N):
    """Global rows of replica r's [view-1; view-2] block."""
    return np.concatenate([np.arange(r * n, (r + 1) * n), N + np.arange(r * n, (r + 1) * n)])


def standardize(h, eps=1e-5):
    """One view [N, D] -> (zhat, rstd [D]) over its rows."""
    h = np.asarray(h, dtype=np.float64)
    mu = h.mean(axis=0)
    var = ((h - mu) ** 2).mean(axis=0)
    rstd = 1.0 / np.sqrt(var + eps)
    return (h - mu) * rstd, rstd


def standardize_bwd(g, zhat, rstd):
    return (g - g.mean(axis=0) - zhat * (g * zhat).mean(axis=0)) * rstd


def _views(hiddens, eps):
    hs = [np.asarray(h, dtype=np.float64) for h in hiddens]
    R, n = len(hs), hs[0].shape[0] // 2
    N = R * n
    h_all = h_all_of(hs, n)
    z1, r1 = standardize(h_all[:N], eps)
    z2, r2 = standardize(h_all[N:], eps)
    return R, n, N, z1, r1, z2, r2


def barlow_direct(hiddens, lambda_weight=0.0051, loss_scaling=1.0, eps=1e-5):
    """The D x D form on the global batch.  Returns dict(loss, on_diag, off_diag, frob = sum_ij C_ij^2, grad_zhat [2N, D],
    grad_all [2N, D] = dL/dh_all) in float64."""
    R, n, N, z1, r1, z2, r2 = _views(hiddens, eps)
    C = z1.T @ z2 / N
    c = np.diag(C)
    on = float(((1.0 - c) ** 2).sum())
    frob = float((C ** 2).sum())
    off = float((C ** 2).sum() - (c ** 2).sum())
    M = loss_scaling * (2.0 * lambda_weight * C + np.diag(-2.0 * (1.0 - c) - 2.0 * lambda_weight * c))
    g1, g2 = z2 @ M.T / N, z1 @ M / N
    grad_all = np.concatenate([standardize_bwd(g1, z1, r1), standardize_bwd(g2, z2, r2)], axis=0)
    return dict(loss=loss_scaling * (on + lambda_weight * off), on_diag=on, off_diag=off, frob=frob,
                grad_zhat=np.concatenate([g1, g2], axis=0), grad_all=grad_all)


def barlow_gram(hiddens, lambda_weight=0.0051, loss_scaling=1.0, eps=1e-5):
    """The Gram form, per replica.  Returns dict(loss, on_diag, off_diag: lists over replicas of the per-replica values; grads: list
    over replicas of dL/dh_r [2n, D]; grads_zhat: the same before the standardisation backward; zhat_all [2N, D]; rstd [2, D];
    gram: list over replicas of [2, n, N]) in float64."""
    R, n, N, z1, r1, z2, r2 = _views(hiddens, eps)
    G1, G2 = z1 @ z1.T, z2 @ z2.T
    c = (z1 * z2).sum(axis=0) / N
    on = float(((1.0 - c) ** 2).sum())
    d = -2.0 * (1.0 - c) - 2.0 * lambda_weight * c
    g1 = np.zeros_like(z1)
    g2 = np.zeros_like(z2)
    loss, offs, gram = [], [], []
    for r in range(R):
        a = slice(r * n, (r + 1) * n)
        off_r = float(R / N ** 2 * (G1[a] * G2[a]).sum() - (c ** 2).sum())
        offs.append(off_r)
        loss.append(loss_scaling * (on + lambda_weight * off_r))
        gram.append(np.stack([G1[a], G2[a]]))
        g1[a] = loss_scaling * (lambda_weight * 2.0 / N ** 2 * G2[a] @ z1 + d * z2[a] / N)
        g2[a] = loss_scaling * (lambda_weight * 2.0 / N ** 2 * G1[a] @ z2 + d * z1[a] / N)
    dh = np.concatenate([standardize_bwd(g1, z1, r1), standardize_bwd(g2, z2, r2)], axis=0)
    gz = np.concatenate([g1, g2], axis=0)
    rows = [replica_rows(r, n, N) for r in range(R)]
    return dict(loss=loss, on_diag=[on] * R, off_diag=offs, grads=[dh[i] for i in rows], grads_zhat=[gz[i] for i in rows],
                zhat_all=np.concatenate([z1, z2], axis=0), rstd=np.stack([r1, r2]), gram=gram)
