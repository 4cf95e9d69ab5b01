"""Float64 reference of the distillation loss (objective.add_kd_loss / simclr_kd_softmax_xent), written with explicit formulas.

For student logits s and teacher logits t of shape [rows, nclass] and a temperature T:

    p = softmax(t / T),  q = softmax(s / T)                      (row-wise, the row maximum subtracted first)
    loss_row = T^2 * (-sum_c p_c log q_c),  loss = mean_rows(loss_row)
    dlogits[row][c] = d loss / d s[row][c] * gscale = T * (q_c - p_c) * gscale / rows
    agreement = share of rows whose first arg-maxima of s and t coincide

The gradient line follows from d(-sum_c p_c log q_c) / d(s_k / T) = q_k - p_k (sum_c p_c = 1) and d(s_k / T) / d s_k = 1 / T.
tests/test_kd_reference.py pins this file against torch autograd, two hand-derived cases and the tie rule."""
import numpy as np


def _log_softmax(x):
    x = x - x.max(axis=1, keepdims=True)
    return x - np.log(np.exp(x).sum(axis=1, keepdims=True))


def first_argmax(v):
    """Column of the first maximum of every row (numpy.argmax / tf.argmax semantics), spelled out."""
    v = np.asarray(v)
    best = v.max(axis=1, keepdims=True)
    cols = np.broadcast_to(np.arange(v.shape[1]), v.shape)
    return np.where(v == best, cols, v.shape[1]).min(axis=1)


def kd_reference(s, t, temperature, gscale=1.0):
    """s, t: [rows, nclass] array-likes (bias already added).  Returns dict(loss, loss_rows, dlogits, agreement, p, q) in float64."""
    s = np.asarray(s, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64)
    assert s.shape == t.shape and s.ndim == 2
    T = float(temperature)
    assert T > 0
    rows = s.shape[0]
    log_q = _log_softmax(s / T)
    log_p = _log_softmax(t / T)
    p, q = np.exp(log_p), np.exp(log_q)
    loss_rows = T * T * -(p * log_q).sum(axis=1)
    dlogits = T * (q - p) * (float(gscale) / rows)
    agreement = float((first_argmax(s) == first_argmax(t)).mean())
    return dict(loss=float(loss_rows.mean()), loss_rows=loss_rows, dlogits=dlogits, agreement=agreement, p=p, q=q)
