"""numpy restatement of the BYOL pieces (Grill et al. 2020, Bootstrap Your Own Latent): the loss with its analytic gradient in float64,
the target network's moving average in float32 (the very three roundings of the kernel) and the tau schedule.

Conventions of simclr_amd.objective.add_byol_loss: q [2b, D] is the online predictor's output, t [2b, D] the target projection, row r of q
pairs with row (r + b) mod 2b of t, normalisation is tf.math.l2_normalize (x / sqrt(max(sum x^2, 1e-12))),
  l_r = sum_j (qhat_rj - that_pj)^2,   loss = (1 / b) sum_r l_r,   cosine = mean_r qhat_r . that_p.
The gradient of tf.maximum goes to its first argument where it is >= the second: a row with sum q^2 < 1e-12 has the CONSTANT norm 1e-6."""
import math

import numpy as np

EPS = 1e-12


def l2_normalize(x):
    x = np.asarray(x, np.float64)
    ss = (x * x).sum(-1, keepdims=True)
    return x / np.sqrt(np.maximum(ss, EPS)), ss


def byol_loss(q, t, grad_scale=1.0):
    """-> dict(loss, cosine, rows [2b] (l_r), grad [2b, D] = grad_scale * dloss/dq), all float64."""
    q, t = np.asarray(q, np.float64), np.asarray(t, np.float64)
    assert q.ndim == 2 and q.shape == t.shape and q.shape[0] % 2 == 0 and q.shape[0] >= 2
    b = q.shape[0] // 2
    qh, ssq = l2_normalize(q)
    th, _ = l2_normalize(t)
    tp = np.roll(th, -b, axis=0)                    # row r reads that of row (r + b) mod 2b
    d = qh - tp
    rows = (d * d).sum(-1)
    g = 2.0 * d                                     # dl_r / dqhat_r
    norm = np.sqrt(np.maximum(ssq, EPS))
    radial = np.where(ssq >= EPS, (qh * g).sum(-1, keepdims=True), 0.0)       # eps branch: the norm does not depend on q
    grad = (g - qh * radial) / norm
    return dict(loss=rows.sum() / b, cosine=(qh * tp).sum(-1).mean(), rows=rows, grad=grad * (grad_scale / b))


def ema_f32(t, o, one_minus_tau):
    """t + omt * (o - t) in float32, every operation rounded on its own -- what simclr_ema_multi_tensor computes, bit for bit."""
    t, o = np.asarray(t, np.float32), np.asarray(o, np.float32)
    omt = np.float32(one_minus_tau)
    d = (o - t).astype(np.float32)
    p = (omt * d).astype(np.float32)
    return (t + p).astype(np.float32)


def tau_schedule(step, total_steps, tau_base):
    """1 - (1 - tau_base) * (cos(pi k / K) + 1) / 2 in double."""
    return 1.0 - (1.0 - float(tau_base)) * (math.cos(math.pi * float(step) / float(total_steps)) + 1.0) / 2.0


def one_minus_tau_f32(step, total_steps, tau_base):
    """What the step hands the kernel: 1 - tau_k formed in double, cast to float32 once."""
    return np.float32(1.0 - tau_schedule(step, total_steps, tau_base))
