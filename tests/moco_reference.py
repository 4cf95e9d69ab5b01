"""numpy restatement of the MoCo v2 pieces (He et al. 2020, Momentum Contrast; Chen et al. 2020, Improved Baselines with Momentum
Contrastive Learning): the loss with its accuracy and analytic gradient in float64, a float32 emulation of the two ways to form a row's
loss (the kernel's and the naive one), the queue's initial rows and its write position.

Conventions of simclr_amd.objective.add_moco_loss: q [2b, D] is the online projection output, t [2b, D] the target network's, row r of q
pairs with row p(r) = (r + b) mod 2b of t, Q [K, D] is the queue, normalisation is tf.math.l2_normalize (x / sqrt(max(sum x^2, 1e-12))),
  s_r+ = qhat_r . that_p / T,   s_rj = qhat_r . Q_j / T,   l_r = logsumexp([s_r+, s_r0 .. s_r,K-1]) - s_r+,   loss = (1 / b) sum_r l_r,
  acc = share of the rows with s_r+ >= max_j s_rj (equality is a hit).
The negatives are the queue rows alone; t and Q get no gradient."""
import numpy as np

EPS = 1e-12


def l2_normalize(x):
    x = np.asarray(x, np.float64)
    ss = (x * x).sum(-1, keepdims=True)
    return x / np.sqrt(np.maximum(ss, EPS)), ss


def moco_logits(qh, th, queue, temperature):
    """Normalised rows -> (s+ [2b], S [2b, K]) in float64."""
    qh, th, queue = np.asarray(qh, np.float64), np.asarray(th, np.float64), np.asarray(queue, np.float64)
    b = qh.shape[0] // 2
    tp = np.roll(th, -b, axis=0)                    # row r reads that of row (r + b) mod 2b
    return (qh * tp).sum(-1) / temperature, qh @ queue.T / temperature, tp


def moco_loss_normalized(qh, th, queue, temperature=1.0, grad_scale=1.0):
    """The loss on rows that are normalised already (what simclr_moco_fwd / _bwd take).
    -> dict(loss, acc, rows [2b] (l_r), grad [2b, D] = grad_scale * dloss/dqhat, neg_mass [2b] = 1 - P_r+), float64."""
    qh = np.asarray(qh, np.float64)
    assert qh.ndim == 2 and qh.shape == np.shape(th) and qh.shape[0] % 2 == 0 and qh.shape[0] >= 2
    b = qh.shape[0] // 2
    sp, S, tp = moco_logits(qh, th, queue, temperature)
    M = np.maximum(sp, S.max(-1))
    neg = np.exp(S - M[:, None]).sum(-1)            # the negatives' sum, apart from the positive term
    pos = np.exp(sp - M)
    total = pos + neg
    rows = np.where(M == sp, np.log1p(neg), (M - sp) + np.log(total))
    P = np.exp(S - M[:, None]) / total[:, None]
    neg_mass = neg / total                          # 1 - P_r+, never one minus a number near one
    grad = (P @ np.asarray(queue, np.float64) - neg_mass[:, None] * tp) * (grad_scale / (b * temperature))
    acc = float((sp >= S.max(-1)).mean())
    return dict(loss=rows.sum() / b, acc=acc, rows=rows, grad=grad, neg_mass=neg_mass)


def moco_loss(q, t, queue, temperature=1.0, grad_scale=1.0):
    """The loss on raw projections -> as moco_loss_normalized, with grad = grad_scale * dloss/dq (through the normalisation; a row with
    sum q^2 < 1e-12 has the constant norm 1e-6, as tf.maximum hands its gradient to the epsilon) and keys = that."""
    qh, ssq = l2_normalize(q)
    th, _ = l2_normalize(t)
    out = moco_loss_normalized(qh, th, queue, temperature, grad_scale)
    g = out['grad']
    out['grad_qhat'] = g
    radial = np.where(ssq >= EPS, (qh * g).sum(-1, keepdims=True), 0.0)
    out['grad'] = (g - qh * radial) / np.sqrt(np.maximum(ssq, EPS))
    out['keys'] = th
    return out


def row_loss_f32(sp, S, stable=True):
    """float32 emulation of a row's loss from float32 logits sp [rows], S [rows, K] (natural-log domain), every operation rounded to
    float32, the sums as one running float32 sum per row (a lane's accumulation).
    stable: the negatives' sum kept apart, l = (M - s+) + log(exp(s+ - M) + sum_neg), log1p(sum_neg) when the positive is the maximum
            -- the kernel's form (which finishes in double: this emulation is its float32 worst case);
    naive:  l = logsumexp(all K + 1 logits) - s+, the subtraction of two numbers of the size of s+."""
    f = np.float32
    sp, S = np.asarray(sp, f), np.asarray(S, f)
    M = np.maximum(sp, S.max(-1)).astype(f)
    neg = np.zeros(sp.shape, f)
    for j in range(S.shape[1]):
        neg = (neg + np.exp((S[:, j] - M).astype(f)).astype(f)).astype(f)
    pos = np.exp((sp - M).astype(f)).astype(f)
    if stable:
        general = ((M - sp).astype(f) + np.log((pos + neg).astype(f)).astype(f)).astype(f)
        return np.where(M == sp, np.log1p(neg).astype(f), general).astype(f)
    lse = (M + np.log((pos + neg).astype(f)).astype(f)).astype(f)
    return (lse - sp).astype(f)


def queue_init(K, D, seed):
    """The queue's initial rows: numpy.random.default_rng([seed]).standard_normal((K, D)), l2-normalised in float64, cast once."""
    x = np.random.default_rng([int(seed)]).standard_normal((int(K), int(D)))
    return (x / np.sqrt(np.maximum((x * x).sum(axis=1, keepdims=True), EPS))).astype(np.float32)


def queue_ptr(step, rows_per_step, K):
    """First queue row the keys of optimizer step `step` are written at."""
    return (int(step) * int(rows_per_step)) % int(K)
