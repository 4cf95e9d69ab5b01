"""Contrastive loss functions -- drop-in mirror of /root/reference/tf2/objective.py.

`add_contrastive_loss(hidden, hidden_norm, temperature, strategy)` keeps the reference
signature and 3-tuple return (tf2/objective.py:35-89) but runs the fused NT-Xent HIP kernels:
l2-normalise -> RCCL all-gather of the hidden block (replacing the scatter + all_reduce of
`tpu_cross_replica_concat`, :92-127) -> tiled similarity + online masked softmax-CE on the
matrix cores.  The [n,N] logits and [n,2N] one-hot labels the reference returns are never
materialised on the hot path: `logits_con` / `labels_con` are lazy handles that also carry the
fused contrast accuracy / entropy (tf2/metrics.py:28-35); call `.dense()` for real tensors.

`generalized_contrastive_loss` is the loss of colabs/intriguing_properties/generalized_contrastive_loss.ipynb (alignment + a
distribution-matching term: decoupled NT-Xent, or sliced Wasserstein against a normal / uniform prior) on the kernels of csrc/gcl.hip.

`add_supcon_loss` is the supervised contrastive loss of Khosla et al. 2020 (NT-Xent with every same-class row of the global batch as a
positive) on the kernels of csrc/supcon.hip.

`add_hard_negative_contrastive_loss` is NT-Xent with the hard-negative re-weighting of Robinson et al. 2021 (beta) and the debiasing
correction of Chuang et al. 2020 (tau_plus) on the kernels of csrc/hcl.hip; at beta = 0 and tau_plus = 0 it is NT-Xent.

`add_nn_contrastive_loss` is NNCLR (after Dwibedi et al. 2021): NT-Xent whose anchors are the rows' nearest neighbours in a support
queue (ops.knn_topk for the search, the kernels of csrc/nnclr.hip for the loss); only the columns carry gradient.

`add_barlow_twins_loss` is the Barlow Twins loss of Zbontar et al. 2021 (redundancy reduction on the cross-correlation of the two views'
batch-standardised hiddens; no negatives) in its Gram form on the kernels of csrc/barlow.hip.

`add_vicreg_loss` is the VICReg loss of Bardes, Ponce, LeCun 2022 (invariance + a hinge on every dimension's standard deviation + the
squared off-diagonal covariance, per view over the global batch; no negatives) in its Gram form on the split-k kernels of csrc/vicreg.hip.

`add_byol_loss` is the BYOL loss of Grill et al. 2020 (squared distance of the l2-normalised online prediction of one view to the
l2-normalised projection a momentum target network gives the other view; no negatives, no collective) on the kernels of csrc/byol.hip.

`add_moco_loss` is the MoCo v2 loss of He et al. 2020 / Chen et al. 2020 (InfoNCE of each online row against the momentum key of its
other view and a queue of keys of earlier steps; no collective) on the kernels of csrc/moco.hip.

`add_dino_loss` is the DINO loss of Caron et al. 2021 (cross-entropy of the student's softmax over K trained prototypes against the
centred, sharpened softmax the momentum teacher gives the other view; no collective) on the kernels of csrc/dino.hip.
`add_dino_local_loss` is its multi-crop share: the local views of the same images against the teacher rows of both global views
(csrc/dino_multicrop.hip for the key side, the loss-agnostic local sweeps of csrc/swav_multicrop.hip for the rest; no collective).

`add_swav_loss` is the SwAV loss of Caron et al. 2020 (cross-entropy of the student's softmax over K trained prototypes against the
Sinkhorn-Knopp code of the other view, the codes equipartitioned over the GLOBAL batch per view; one all-gather of the normalised block,
nothing in the backward) on the kernels of csrc/swav.hip.  `add_swav_local_loss` is its multi-crop share: the local views of the same
images against the codes of both global views (csrc/swav_multicrop.hip; no collective).
"""
import torch

from . import ops
from .flags import FLAGS
from .comm import collectives_on, gather_hidden, num_replicas, replica_id, scatter_hidden_grad
from .resnet import RT

LARGE_NUM = 1e9  # tf2/objective.py:24 (kept for reference; the kernel skips the masked column)


class _Loss:
    """A scalar loss living on the device, with the hand-written backward attached.
    backward() = backward_start() + backward_finish(): between the two the caller may enqueue independent work,
    which then overlaps with the collective the first half launched (the reduce-scatter of the key-side gradient)."""

    def __init__(self, value, backward_fn, start_fn=None, finish_fn=None):
        self.value = value            # 0-d / 1-element float32 device tensor
        self._backward = backward_fn
        self._start, self._finish = start_fn, finish_fn

    def backward(self, grad_scale=1.0):
        return self._backward(grad_scale)

    def backward_start(self, grad_scale=1.0):
        if self._start is not None:
            self._start(grad_scale)
        else:
            self._pending = self._backward(grad_scale)

    def backward_finish(self):
        if self._finish is not None:
            return self._finish()
        return self._pending

    def item(self):
        return float(self.value.item())

    __float__ = item


class LazyLogits:
    """logits_ab handle ([n, N], tf2/objective.py:80,89)."""

    def __init__(self, z_local, z_all, temperature, out, ensure_entropy):
        self._z_local, self._z_all, self._t = z_local, z_all, temperature
        self._out = out
        self._ensure_entropy = ensure_entropy
        n, N = z_local.shape[0] // 2, z_all.shape[0] // 2
        self.shape = (n, N)
        self._kept = None

    @property
    def contrast_acc(self):          # tf2/metrics.py:28-31
        return self._kept[0] if self._kept is not None else self._out[1]

    @property
    def contrast_entropy(self):      # tf2/metrics.py:33-35 (produced by the backward sweep)
        if self._kept is not None:
            return self._kept[1]
        self._ensure_entropy()
        return self._out[2]

    def keep(self, acc, entropy):
        """Re-point the two metrics at copies that outlive the step arena (run.make_single_step)."""
        self._kept = (acc, entropy)

    def dense(self):
        return ops.ntxent_logits_ab(self._z_local, self._z_all, self._t)


class LazyLabels:
    """one_hot(labels_idx, 2N) handle ([n, 2N], tf2/objective.py:67-68,73)."""

    def __init__(self, n, N, rank, device):
        self.n, self.N, self.rank, self.device = n, N, rank, device
        self.shape = (n, 2 * N)

    def dense(self):
        idx = torch.arange(self.n, device=self.device) + self.rank * self.n
        return torch.nn.functional.one_hot(idx, 2 * self.N).float()


def tpu_cross_replica_concat(tensor, strategy=None):
    """Reduce a concatenation of the `tensor` across replicas (tf2/objective.py:92-127).
    The reference builds it from scatter_nd + all_reduce(SUM); over RCCL it is an all_gather."""
    if not collectives_on(strategy):
        return tensor
    return strategy.all_gather_concat(tensor)


def add_contrastive_loss(hidden, hidden_norm=True, temperature=1.0, strategy=None, overlap=None):
    """Compute loss for model (tf2/objective.py:35-89).

    Args:
      hidden: float32 device tensor (bsz, dim) = [view-a rows; view-b rows].
      hidden_norm: whether or not to use normalization on the hidden vector.
      temperature: a `floating` number for temperature scaling.
      strategy: replica context (simclr_amd.comm.Strategy) or None.
      overlap: optional zero-argument callable run while the all-gather of the hidden block is in flight
        (collective A runs on the communicator's side stream; north_star: overlap it with independent work).
    Returns:
      A loss scalar (with .backward / .backward_start / .backward_finish), the logits handle, the labels handle.
    """
    assert hidden.dtype == torch.float32 and hidden.dim() == 2
    hidden = hidden.contiguous()
    if hidden_norm:
        z, inv = ops.l2norm_fwd(hidden)                          # :53-54
    else:
        z, inv = hidden, None
    n = z.shape[0] // 2
    R, rank = num_replicas(strategy), replica_id(strategy)
    pending = gather_hidden(z, strategy, async_op=True)          # :58-61 (collective A), asynchronous
    if overlap is not None:
        overlap()
    z_all = pending()
    # FLAGS.ntxent_matmul='f16x3' (opt-in): the sweeps' fp32 products as three fp16-piece MFMA terms -- l2-normalised rows only;
    # embeddings wider than 256 (the wide NT-Xent kernels) run exact whatever the flag says
    split = (bool(hidden_norm) and getattr(FLAGS, 'ntxent_matmul', 'exact') == 'f16x3'
             and not ops.ntxent_is_wide(hidden.shape[1]))
    out, row_stats, ws = ops.ntxent_fwd(z, z_all, rank, temperature, split=split)
    state = {'done': False, 'dz_local': None, 'slot': None}

    def backward_start(grad_scale=1.0):
        dz_local, dz_all = ops.ntxent_bwd(z, z_all, rank, temperature, row_stats, grad_scale, out, ws, split=split)
        state['done'] = True
        state['dz_local'] = dz_local
        state['slot'] = scatter_hidden_grad(dz_all, strategy, async_op=True)   # transpose of the concat, asynchronous

    def backward_finish():
        dz_local = state['dz_local']
        dz_slot = state['slot']()
        state['dz_local'] = state['slot'] = None
        ops.axpy_f32(1.0, dz_slot, dz_local)
        if hidden_norm:
            return ops.l2norm_bwd(z, inv, dz_local)
        return dz_local

    def backward(grad_scale=1.0):
        backward_start(grad_scale)
        return backward_finish()

    def ensure_entropy():
        if not state['done']:
            ops.ntxent_bwd(z, z_all, rank, temperature, row_stats, 0.0, out, ws, split=split)
            state['done'] = True

    loss = _Loss(out[0:1], backward, backward_start, backward_finish)
    logits_con = LazyLogits(z, z_all, temperature, out, ensure_entropy)
    labels_con = LazyLabels(n, n * R, rank, z.device)
    loss.normalized = z
    return loss, logits_con, labels_con


GCL_DISTS = ('logsumexp', 'normal', 'uniform')
_GCL_STEP = [0]


def set_gcl_step(step):
    """The global step the next generalized_contrastive_loss call draws its projection basis and prior for (run.single_step sets it
    from optimizer.iterations, which a checkpoint restores)."""
    _GCL_STEP[0] = int(step)


def _gcl_seed(seed, step, stream):
    return (int(seed) * 0x9E3779B97F4A7C15 + int(step) * 4 + stream) & 0x7FFFFFFFFFFFFFFF


def gcl_draws(D, M, dist, seed, step, device):
    """(rand_w [D, D], prior [M, D]) of one step: a function of (seed, step) only -- identical on every replica, the same after a resume.
    rand_w: a random orthogonal matrix with torch.nn.init.orthogonal_'s construction (QR of a normal matrix, columns signed by
    diag(R)), made on the host and copied asynchronously; prior: N(0, 1) ('normal') or U(-1, 1) ('uniform') from a device generator.
    Nothing here waits for the device."""
    g = torch.Generator(device='cpu').manual_seed(_gcl_seed(seed, step, 0))
    q, r = torch.linalg.qr(torch.randn(D, D, generator=g))
    q = q * torch.sign(torch.diagonal(r)).unsqueeze(0)
    if torch.device(device).type == 'cuda':
        q = q.contiguous().pin_memory()
    rand_w = q.to(device, non_blocking=True)
    gd = torch.Generator(device=device).manual_seed(_gcl_seed(seed, step, 1))
    if dist == 'normal':
        prior = torch.randn(M, D, generator=gd, device=device, dtype=torch.float32)
    else:
        prior = torch.rand(M, D, generator=gd, device=device, dtype=torch.float32).mul_(2.0).sub_(1.0)
    return rand_w, prior


def generalized_contrastive_loss(hidden1, hidden2, lambda_weight=1.0, temperature=1.0, dist='normal', hidden_norm=True, loss_scaling=1.0,
                                 strategy=None, overlap=None, rand_w=None, prior=None):
    """Generalized contrastive loss (colabs/intriguing_properties/generalized_contrastive_loss.ipynb):
    loss_scaling * (alignment + lambda_weight * distribution matching).

    Args:
      hidden1, hidden2: float32 device tensors [n, D], the two views of the local batch; D in {64, 128, 256}.
      lambda_weight: weight of the distribution-matching term.
      temperature: temperature of the 'logsumexp' term (unused by the SWD priors).
      dist: 'logsumexp' (decoupled NT-Xent over the global batch), 'normal' or 'uniform' (sliced Wasserstein distance between the
        global batch and an N(0, 1) / U(-1, 1) prior, at most 8192 global rows).
      hidden_norm: l2-normalise the hiddens (and the SWD prior) first.
      loss_scaling: factor on the whole loss.
      strategy, overlap: as add_contrastive_loss (the hidden block is gathered asynchronously; overlap() runs meanwhile).
      rand_w [D, D], prior [2N, D]: the SWD projection basis and prior samples; drawn by gcl_draws(FLAGS.gcl_seed, step) when None.
    Returns:
      A loss scalar with .backward / .backward_start / .backward_finish (-> gradient wrt [hidden1; hidden2], [2n, D]) and the device
      scalars .align and .dist_match; SWD losses also carry .perm ([D, 2N] int32, the sorting permutation of every projected dimension).
    """
    if dist not in GCL_DISTS:
        raise ValueError('Unknown prior {}'.format(dist))
    assert hidden1.dtype == torch.float32 and hidden1.dim() == 2 and hidden1.shape == hidden2.shape
    n, D = hidden1.shape
    ops._gcl_check_dim(D)
    hidden = torch.cat([hidden1, hidden2], 0)
    return generalized_loss_of_block(hidden, lambda_weight, temperature, dist, hidden_norm, loss_scaling, strategy, overlap, rand_w, prior)


def generalized_loss_of_block(hidden, lambda_weight=1.0, temperature=1.0, dist='normal', hidden_norm=True, loss_scaling=1.0, strategy=None,
                              overlap=None, rand_w=None, prior=None):
    """generalized_contrastive_loss on the stacked block [hidden1; hidden2] (what the projection head returns)."""
    if dist not in GCL_DISTS:
        raise ValueError('Unknown prior {}'.format(dist))
    hidden = hidden.contiguous()
    D = hidden.shape[1]
    ops._gcl_check_dim(D)
    if hidden_norm:
        z, inv = ops.l2norm_fwd(hidden)
    else:
        z, inv = hidden, None
    n = z.shape[0] // 2
    R, rank = num_replicas(strategy), replica_id(strategy)
    M = 2 * n * R
    if dist != 'logsumexp' and M > ops.SWD_MAX_ROWS:
        raise ValueError('the sliced-Wasserstein sort holds at most %d global rows (2 x global batch) per column, got %d' % (ops.SWD_MAX_ROWS, M))
    pending = gather_hidden(z, strategy, async_op=True)
    if dist != 'logsumexp' and (rand_w is None or prior is None):
        w_d, p_d = gcl_draws(D, M, dist, getattr(FLAGS, 'gcl_seed', 0), _GCL_STEP[0], z.device)
        rand_w = w_d if rand_w is None else rand_w
        prior = p_d if prior is None else prior
    if overlap is not None:
        overlap()
    z_all = pending()
    state = {}

    def finish_local(dz_local):
        if hidden_norm:
            return ops.l2norm_bwd(z, inv, dz_local)
        return dz_local

    if dist == 'logsumexp':
        out, row_stats, ws = ops.gcl_lse_fwd(z, z_all, temperature, lambda_weight, loss_scaling)

        def backward_start(grad_scale=1.0):
            # normalised rows: the self column's radial term is left to the normalisation backward, which removes it exactly
            dz_local, dz_all = ops.gcl_lse_bwd(z, z_all, temperature, row_stats, grad_scale, ws, lambda_weight, loss_scaling,
                                               rank=rank, skip_self=bool(hidden_norm))
            state['dz_local'] = dz_local
            state['slot'] = scatter_hidden_grad(dz_all, strategy, async_op=True)   # transpose of the concat, as NT-Xent's

        def backward_finish():
            dz_local, dz_slot = state.pop('dz_local'), state.pop('slot')()
            ops.axpy_f32(1.0, dz_slot, dz_local)
            return finish_local(dz_local)
        perm = None
    else:
        assert tuple(rand_w.shape) == (D, D) and tuple(prior.shape) == (M, D), 'rand_w must be [D, D] and prior [2N, D]'
        w = rand_w.contiguous()
        wt = w.t().contiguous()
        q = ops.l2norm_fwd(prior.contiguous())[0] if hidden_norm else prior.contiguous()
        pt = ops.gcl_gemm_nt(wt, z_all)                       # [D, M] = (z_all W)^T
        qt = ops.gcl_gemm_nt(wt, q)
        # d mean_{D x M}((Q_sorted - P_sorted)^2) / d P_sorted = 2 (P_sorted - Q_sorted) / (D M)
        dp, col_loss, perm = ops.swd_sort_match(pt, qt, 2.0 / (D * M), want_perm=True)
        out = ops.gcl_swd_out(col_loss, z, M, lambda_weight, loss_scaling)

        def backward_start(grad_scale=1.0):
            g_all = ops.gcl_gemm_nt(dp, w)                    # [M, D] = dP W^T
            # every replica holds the identical global term: its own rows' gradient needs no collective
            state['dz_local'] = ops.gcl_swd_bwd(g_all, z, rank, grad_scale, lambda_weight, loss_scaling)

        def backward_finish():
            return finish_local(state.pop('dz_local'))

    def backward(grad_scale=1.0):
        backward_start(grad_scale)
        return backward_finish()

    loss = _Loss(out[0:1], backward, backward_start, backward_finish)
    loss.align, loss.dist_match = out[1:2], out[2:3]
    loss.perm = perm
    loss.normalized = z
    return loss


_CLASS_ID_CACHE = {}


def _class_ids(labels):
    """int32 class ids of a one-hot (or already integer) label tensor; cached per (storage, version), so a batch whose
    labels are reused (both views, several steps of a resident pool) is converted once."""
    key = (labels.data_ptr(), tuple(labels.shape), labels.dtype, labels._version)
    hit = _CLASS_ID_CACHE.get(key)
    if hit is not None and hit[0]() is labels:
        return hit[1]
    ids = labels.argmax(1) if labels.dim() == 2 else labels
    ids = ids.to(torch.int32).contiguous()
    if len(_CLASS_ID_CACHE) > 64:
        _CLASS_ID_CACHE.clear()
    import weakref
    _CLASS_ID_CACHE[key] = (weakref.ref(labels), ids)
    return ids


def _gather_class_ids(ids, strategy):
    """[n] int32 class ids of this replica -> (wait-and-get function of) the [N] ids of the global batch in replica order, which is
    z_all's sample order.  The collective is asynchronous, like gather_hidden's."""
    if not collectives_on(strategy):
        return lambda: ids
    g, work = strategy.all_gather_concat(ids, async_op=True)

    def finish():
        if work is not None:
            work.wait()
        return g
    return finish


def add_supcon_loss(hidden, labels, hidden_norm=True, temperature=1.0, strategy=None, overlap=None):
    """Supervised contrastive loss (Khosla et al. 2020, Supervised Contrastive Learning, the L_out^sup form) on the kernels of
    csrc/supcon.hip: NT-Xent with every same-class row of the GLOBAL batch as a positive.

    With A(i) = every column of the gathered block but row i's own and P(i) = the columns of A(i) with row i's label,
      loss = (1 / n) sum_{i < 2n} [logsumexp_{a in A(i)}(z_i.z_a / T) - (1 / |P(i)|) sum_{p in P(i)} z_i.z_p / T],
    the sum of the two per-view means, as add_contrastive_loss forms NT-Xent: with all labels of the global batch distinct the loss
    and its gradient are add_contrastive_loss's.  The temperature / base_temperature factor of the paper's code is left out.

    Args:
      hidden: float32 device tensor [2n, D] = [view-a rows; view-b rows], D in {64, 128, 256}.
      labels: one-hot float [n, C] or int class ids [n] of the local batch (both views of an image share its label).
      hidden_norm, temperature, strategy, overlap: as add_contrastive_loss (the hidden block and the class ids are gathered
        asynchronously; overlap() runs meanwhile).
    Returns:
      A loss scalar with .backward / .backward_start / .backward_finish (-> gradient wrt hidden), the device scalars .acc (share of rows
      whose best positive scores at least as high as their best non-positive) and .positives (mean |P(i)|), and .normalized.
    """
    assert hidden.dtype == torch.float32 and hidden.dim() == 2
    hidden = hidden.contiguous()
    n, D = hidden.shape[0] // 2, hidden.shape[1]
    ops._supcon_check_dim(D)
    ids = _class_ids(labels)
    if ids.dim() != 1 or ids.shape[0] != n:
        raise ValueError('add_supcon_loss: %d labels for a local batch of %d (hidden holds both views: [2n, D])' % (ids.shape[0], n))
    if hidden_norm:
        z, inv = ops.l2norm_fwd(hidden)
    else:
        z, inv = hidden, None
    rank = replica_id(strategy)
    pending = gather_hidden(z, strategy, async_op=True)
    pending_ids = _gather_class_ids(ids, strategy)
    if overlap is not None:
        overlap()
    z_all, ids_all = pending(), pending_ids()
    out, row_stats, ws = ops.supcon_fwd(z, z_all, ids_all, rank, temperature)
    state = {}

    def backward_start(grad_scale=1.0):
        dz_local, dz_all = ops.supcon_bwd(z, z_all, ids_all, rank, temperature, row_stats, grad_scale, ws)
        state['dz_local'] = dz_local
        state['slot'] = scatter_hidden_grad(dz_all, strategy, async_op=True)   # transpose of the concat, as NT-Xent's

    def backward_finish():
        dz_local, dz_slot = state.pop('dz_local'), state.pop('slot')()
        ops.axpy_f32(1.0, dz_slot, dz_local)
        if hidden_norm:
            return ops.l2norm_bwd(z, inv, dz_local)
        return dz_local

    def backward(grad_scale=1.0):
        backward_start(grad_scale)
        return backward_finish()

    loss = _Loss(out[0:1], backward, backward_start, backward_finish)
    loss.acc, loss.positives = out[1:2], out[2:3]
    loss.normalized = z
    return loss


class _NtxentScoredLogits(LazyLogits):
    """The LazyLogits of a loss whose own kernels score nothing: contrast_acc / contrast_entropy come from one NT-Xent forward and one
    zero-gradient NT-Xent backward sweep over the same (z_local, z_all, T), launched when the first of the two is read."""

    def __init__(self, z_local, z_all, temperature, rank):
        super().__init__(z_local, z_all, temperature, None, None)
        self._rank = rank

    def _score(self):
        if self._out is None:
            out, row_stats, ws = ops.ntxent_fwd(self._z_local, self._z_all, self._rank, self._t)
            ops.ntxent_bwd(self._z_local, self._z_all, self._rank, self._t, row_stats, 0.0, out, ws)
            self._out = out
        return self._out

    @property
    def contrast_acc(self):
        return self._kept[0] if self._kept is not None else self._score()[1]

    @property
    def contrast_entropy(self):
        return self._kept[1] if self._kept is not None else self._score()[2]


def add_hard_negative_contrastive_loss(hidden, temperature=1.0, beta=0.0, tau_plus=0.0, strategy=None, overlap=None):
    """NT-Xent with hard-negative re-weighting (Robinson et al. 2021: beta) and the debiasing correction (Chuang et al. 2020: tau_plus)
    on the kernels of csrc/hcl.hip.  The formulas are this project's definition of the two corrections, not a parity claim.

    With Neg(i) = the M = 2N - 2 columns of the gathered block that are neither row i's own nor its other view, a = 1 / temperature
    and s = the dot products of the l2-normalised rows,
      p_i = exp(a s_i,pos),  A_i = sum_{Neg(i)} exp((1 + beta) a s_ik),  B_i = sum_{Neg(i)} exp(beta a s_ik),
      G_i = max((M A_i / B_i - tau_plus M p_i) / (1 - tau_plus), M exp(-a)),   l_i = log(p_i + G_i) - a s_i,pos,
      loss = (1 / n) sum_{i < 2n} l_i,
    the sum of the two per-view means, as add_contrastive_loss forms NT-Xent; at beta = 0 and tau_plus = 0 the loss and its gradient
    are add_contrastive_loss's.  The weights exp(beta a s) are differentiated through (no stop-gradient).  The hidden block is always
    l2-normalised: the floor M exp(-a) assumes s >= -1.

    Args:
      hidden: float32 device tensor [2n, D] = [view-a rows; view-b rows], D in {64, 128, 256}; the global batch holds N >= 2 images.
      temperature: > 0.  beta: >= 0, the concentration on hard negatives.  tau_plus: in [0, 1), the class prior of a false negative.
      strategy, overlap: as add_contrastive_loss (the hidden block is gathered asynchronously; overlap() runs meanwhile).
    Returns:
      A loss scalar with .backward / .backward_start / .backward_finish (-> gradient wrt hidden), the device scalar .floor_share (the
      share of the local rows whose G sits on the floor: those rows pull on their positive only) and .normalized; the logits handle
      (contrast_acc / contrast_entropy of the same logits matrix, scored by the NT-Xent kernels when read); the labels handle.
    """
    assert hidden.dtype == torch.float32 and hidden.dim() == 2
    hidden = hidden.contiguous()
    n = hidden.shape[0] // 2
    if hidden.shape[1] not in ops.HCL_DIMS:
        raise ValueError('the hard-negative / debiased NT-Xent supports hidden widths %s (got %d)'
                         % ('/'.join(map(str, ops.HCL_DIMS)), hidden.shape[1]))
    if not temperature > 0 or not ops.hcl_beta_ok(beta) or not ops.hcl_tau_plus_ok(tau_plus):
        raise ValueError('add_hard_negative_contrastive_loss: need temperature > 0, beta >= 0 and finite, tau_plus in [0, 1) '
                         '(got %r, %r, %r)' % (temperature, beta, tau_plus))
    z, inv = ops.l2norm_fwd(hidden)
    R, rank = num_replicas(strategy), replica_id(strategy)
    pending = gather_hidden(z, strategy, async_op=True)
    if overlap is not None:
        overlap()
    z_all = pending()
    out, row_stats, ws = ops.hcl_fwd(z, z_all, rank, temperature, beta, tau_plus)
    state = {}

    def backward_start(grad_scale=1.0):
        dz_local, dz_all = ops.hcl_bwd(z, z_all, rank, temperature, beta, tau_plus, row_stats, grad_scale, ws)
        state['dz_local'] = dz_local
        state['slot'] = scatter_hidden_grad(dz_all, strategy, async_op=True)   # transpose of the concat, as NT-Xent's

    def backward_finish():
        dz_local, dz_slot = state.pop('dz_local'), state.pop('slot')()
        ops.axpy_f32(1.0, dz_slot, dz_local)
        return ops.l2norm_bwd(z, inv, dz_local)

    def backward(grad_scale=1.0):
        backward_start(grad_scale)
        return backward_finish()

    loss = _Loss(out[0:1], backward, backward_start, backward_finish)
    loss.floor_share = out[1:2]
    loss.normalized = z
    return loss, _NtxentScoredLogits(z, z_all, temperature, rank), LazyLabels(n, n * R, rank, z.device)


def add_nn_contrastive_loss(hidden, support, temperature=1.0, strategy=None, overlap=None):
    """NNCLR (after Dwibedi et al. 2021): NT-Xent whose anchor is the row's nearest neighbour in a support queue, on the kernels of
    csrc/nnclr.hip.  This project's definition, written from memory of the paper, not a parity claim.

    With z = l2norm(hidden), z_all the gathered block, S = support and a = 1 / temperature, local row r (view v, global image g):
      j(r) = argmax_k z_r . S_k  (exact fp32, ties to the lowest k, no gradient),   nn_r = S_j(r)  (a constant),
      C(r) = the N columns of the OTHER view,   p(r) = (1 - v) N + g,
      l_r  = logsumexp_{c in C(r)}(a nn_r . z_all[c]) - a nn_r . z_all[p(r)],   loss = (1 / n) sum_{r < 2n} l_r,
    the sum of the two per-view means, as add_contrastive_loss forms NT-Xent (a replica's value is its share; the mean over replicas is
    the loss).  Only the columns carry gradient: the rows of the logits matrix are queue rows.

    Args:
      hidden: float32 device tensor [2n, D] = [view-a rows; view-b rows], D in {64, 128, 256}; the global batch holds N >= 2 images.
      support: float32 device tensor [K, D] of unit rows (model.SupportQueue.value); read, never written.
      temperature: > 0.  strategy, overlap: as add_supcon_loss (the hidden block is gathered asynchronously; the search and overlap()
        run meanwhile).
    Returns:
      A loss scalar with .backward / .backward_start / .backward_finish (-> gradient wrt hidden), the device scalars .acc (share of rows
      whose positive column is the lowest-index maximum of C(r)) and .nn_sim (mean z_r . nn_r), .nn_index (int32 [2n]), .neighbours
      ([2n, D]), .normalized (z) and .gathered (z_all, whose first N rows the caller enqueues after the optimizer step).
    """
    assert hidden.dtype == torch.float32 and hidden.dim() == 2
    hidden = hidden.contiguous()
    D = hidden.shape[1]
    if D not in ops.NNCLR_DIMS:
        raise ValueError('the NNCLR kernels support hidden widths %s (got %d)' % ('/'.join(map(str, ops.NNCLR_DIMS)), D))
    if support.dim() != 2 or support.shape[1] != D or support.dtype != torch.float32 or support.shape[0] < 1:
        raise ValueError('add_nn_contrastive_loss: need a float32 support queue [K, %d] (got %s %s)' % (D, tuple(support.shape), support.dtype))
    if not 0.0 < float(temperature) < float('inf'):
        raise ValueError('add_nn_contrastive_loss: need temperature > 0 and finite (got %r)' % (temperature,))
    z, inv = ops.l2norm_fwd(hidden)
    rank = replica_id(strategy)
    pending = gather_hidden(z, strategy, async_op=True)
    # the search needs the local rows only: it runs while the gather is in flight
    _, top_idx = ops.knn_topk(z, support.contiguous(), 1)
    nn_index = top_idx.reshape(-1)
    neighbours = support.index_select(0, nn_index.long())
    if overlap is not None:
        overlap()
    z_all = pending()
    out, row_stats, ws = ops.nnclr_fwd(neighbours, z, z_all, rank, temperature)
    state = {}

    def backward_start(grad_scale=1.0):
        dz_all = ops.nnclr_bwd(neighbours, z_all, rank, temperature, row_stats, grad_scale, ws)
        state['slot'] = scatter_hidden_grad(dz_all, strategy, async_op=True)   # transpose of the concat, as NT-Xent's

    def backward_finish():
        return ops.l2norm_bwd(z, inv, state.pop('slot')())                       # no row-side term: the neighbours are constants

    def backward(grad_scale=1.0):
        backward_start(grad_scale)
        return backward_finish()

    loss = _Loss(out[0:1], backward, backward_start, backward_finish)
    loss.acc, loss.nn_sim = out[1:2], out[2:3]
    loss.nn_index, loss.neighbours, loss.normalized, loss.gathered = nn_index, neighbours, z, z_all
    return loss


def add_barlow_twins_loss(hidden, lambda_weight=0.0051, loss_scaling=1.0, eps=1e-5, strategy=None, overlap=None):
    """Barlow Twins loss (Zbontar et al. 2021) on the Gram-form kernels of csrc/barlow.hip:
      loss = loss_scaling * (sum_i (1 - C_ii)^2 + lambda_weight * sum_{i != j} C_ij^2),   C = zhat1^T zhat2 / N,
    zhat = every dimension of each view standardised over the GLOBAL batch (biased variance, eps inside the root).  No negatives, no
    temperature and no l2 normalisation.  C [D, D] is never formed: sum_ij C_ij^2 = sum_ab (zhat1_a.zhat1_b)(zhat2_a.zhat2_b) / N^2,
    and a replica sums its own rows a of that against all columns b.

    Args:
      hidden: float32 device tensor [2n, D] = [view-a rows; view-b rows], D a multiple of 64 in [64, 8192].
      lambda_weight: weight of the off-diagonal (redundancy-reduction) term.
      loss_scaling: factor on the whole loss.
      eps: added to the variance of the standardisation.
      strategy, overlap: as add_contrastive_loss (the raw hidden block is gathered asynchronously; overlap() runs meanwhile).
    Returns:
      A loss scalar with .backward / .backward_start / .backward_finish (-> grad_scale * R * dL/dhidden of the local rows, [2n, D]: with
      grad_scale = 1 / R and the summed gradient synchronisation a run optimises L itself), the device scalars .on_diag and .off_diag
      (the raw sums, before lambda_weight and loss_scaling) and .normalized (zhat of the local rows).  The value is this replica's share
      loss_scaling * (on_diag + lambda_weight * (R / N^2 * sum_{a local, b} G1_ab G2_ab - sum_i C_ii^2)): the mean over the replicas is
      the loss, as for add_contrastive_loss.
    """
    assert hidden.dtype == torch.float32 and hidden.dim() == 2
    hidden = hidden.contiguous()
    n, D = hidden.shape[0] // 2, hidden.shape[1]
    ops._bt_check_dim(D)
    if n < 1 or hidden.shape[0] != 2 * n:
        raise ValueError('add_barlow_twins_loss: hidden holds both views, [2n, D] with n >= 1 (got %d rows)' % hidden.shape[0])
    R, rank = num_replicas(strategy), replica_id(strategy)
    pending = gather_hidden(hidden, strategy, async_op=True)
    if overlap is not None:
        overlap()
    h_all = pending()
    # every replica standardises the whole gathered block in one fixed order: statistics and zhat_all are bitwise the same everywhere
    zhat_all, rstd = ops.bt_standardize(h_all, eps)
    out, ws = ops.bt_fwd(zhat_all, n, rank, lambda_weight, loss_scaling)
    state = {}

    def backward_start(grad_scale=1.0):
        g, colsums = ops.bt_bwd(zhat_all, n, rank, lambda_weight, loss_scaling, grad_scale, ws)
        if collectives_on(strategy):
            strategy.all_reduce_sum(colsums)          # the SyncBN statistics route: the means of the standardisation backward are global
        state['g'], state['colsums'] = g, colsums

    def backward_finish():
        return ops.bt_apply(state.pop('g'), zhat_all, rstd, state.pop('colsums'), rank)

    def backward(grad_scale=1.0):
        backward_start(grad_scale)
        return backward_finish()

    loss = _Loss(out[0:1], backward, backward_start, backward_finish)
    loss.on_diag, loss.off_diag = out[1:2], out[2:3]
    N = n * R
    v1 = zhat_all[rank * n:(rank + 1) * n]
    loss.normalized = zhat_all if R == 1 else torch.cat([v1, zhat_all[N + rank * n:N + (rank + 1) * n]], 0)
    return loss


def add_vicreg_loss(hidden, sim_coeff=25.0, std_coeff=25.0, cov_coeff=1.0, eps=1e-4, gamma=1.0, strategy=None, overlap=None):
    """VICReg loss (Bardes, Ponce, LeCun 2022) on the Gram-form kernels of csrc/vicreg.hip:
      loss = sim_coeff * inv + std_coeff * var + cov_coeff * cov,
      inv = mean (h1 - h2)^2,  var = (1/2) sum_v mean_i max(0, gamma - sqrt(Var_i(h_v) + eps)),  cov = sum_v (1/D) sum_{i != j} Cov(h_v)_ij^2,
    variance (unbiased) and covariance over the GLOBAL batch.  No negatives, no temperature and no l2 normalisation.  Cov [D, D] is
    never formed: sum_ij Cov_ij^2 = sum_ab (xc_a.xc_b)^2 / (N-1)^2 on the centred rows xc, and a replica sums its own rows a of that
    against all columns b.

    Args:
      hidden: float32 device tensor [2n, D] = [view-a rows; view-b rows], D a multiple of 64 in [64, 8192]; the global batch N >= 2.
      sim_coeff, std_coeff, cov_coeff: weights of the invariance, variance and covariance terms (finite, >= 0).
      eps: added to the variance under the root.  gamma: target of the standard deviation.
      strategy, overlap: as add_contrastive_loss (the raw hidden block is gathered asynchronously; overlap() runs meanwhile).
    Returns:
      A loss scalar with .backward / .backward_start / .backward_finish (-> grad_scale * R * dL/dhidden of the local rows, [2n, D]: with
      grad_scale = 1 / R and the summed gradient synchronisation a run optimises L itself; backward_start launches, backward_finish
      returns, and there is no collective between them), the device scalars .invariance, .variance and .covariance (the raw terms,
      before the coefficients) and .centered (xc of the local rows).  The value is this replica's share -- inv over its own rows, the
      global var, cov with R / (N-1)^2 * sum_{a local, b} G_ab^2 in place of the full sum: the mean over the replicas is the loss, as
      for add_contrastive_loss.
    """
    assert hidden.dtype == torch.float32 and hidden.dim() == 2
    hidden = hidden.contiguous()
    n, D = hidden.shape[0] // 2, hidden.shape[1]
    ops._vicreg_check_dim(D)
    if n < 1 or hidden.shape[0] != 2 * n:
        raise ValueError('add_vicreg_loss: hidden holds both views, [2n, D] with n >= 1 (got %d rows)' % hidden.shape[0])
    if not all(ops.vicreg_coeff_ok(c) for c in (sim_coeff, std_coeff, cov_coeff)):
        raise ValueError('add_vicreg_loss: sim_coeff, std_coeff and cov_coeff must be finite and >= 0 (got %r, %r, %r)'
                         % (sim_coeff, std_coeff, cov_coeff))
    if not float(eps) >= 0.0:
        raise ValueError('add_vicreg_loss: eps must be >= 0 (got %r)' % (eps,))
    R, rank = num_replicas(strategy), replica_id(strategy)
    if n * R < 2:
        raise ValueError('add_vicreg_loss: the unbiased variance needs a global batch of at least 2 (got %d)' % (n * R))
    pending = gather_hidden(hidden, strategy, async_op=True)
    if overlap is not None:
        overlap()
    h_all = pending()
    # every replica centres the whole gathered block in one fixed order: xc_all and the statistics are bitwise the same everywhere
    xc_all, stats = ops.vicreg_center(h_all, eps)
    out, ws = ops.vicreg_fwd(h_all, xc_all, stats, n, rank, sim_coeff, std_coeff, cov_coeff, gamma)
    state = {}

    def backward_start(grad_scale=1.0):
        state['dh'] = ops.vicreg_bwd(h_all, xc_all, stats, n, rank, sim_coeff, std_coeff, cov_coeff, gamma, grad_scale, ws)

    def backward_finish():
        return state.pop('dh')

    def backward(grad_scale=1.0):
        backward_start(grad_scale)
        return backward_finish()

    loss = _Loss(out[0:1], backward, backward_start, backward_finish)
    loss.invariance, loss.variance, loss.covariance = out[1:2], out[2:3], out[3:4]
    N = n * R
    v1 = xc_all[rank * n:(rank + 1) * n]
    loss.centered = xc_all if R == 1 else torch.cat([v1, xc_all[N + rank * n:N + (rank + 1) * n]], 0)
    return loss


def add_byol_loss(online, target, strategy=None, overlap=None):
    """BYOL loss (Grill et al. 2020, Bootstrap Your Own Latent, eq. 2) on the kernels of csrc/byol.hip:
      loss = (1 / b) sum_{r < 2b} |l2n(online_r) - l2n(target_{(r + b) mod 2b})|^2,
    the prediction of each view against the target projection of the other one, both directions -- the sum of the two per-view means,
    as add_contrastive_loss forms NT-Xent.  l2n is tf.math.l2_normalize (epsilon 1e-12); always applied.  The squared difference is
    summed in double: 2 - 2 cos is never formed, so a nearly converged pair keeps its digits.

    Args:
      online: float32 device tensor [2b, D] = the online predictor's output, [view-a rows; view-b rows]; D a multiple of 64 in [64, 8192].
      target: float32 device tensor [2b, D] = the target network's projection output of the same batch.  It gets no gradient.
      strategy: replica context or None.  The loss needs NO collective: a replica's value is the mean over its own rows, the mean over
        the replicas is the loss, and `backward` is called with 1 / R (SyncBN is the only cross-replica coupling).
      overlap: optional zero-argument callable, run after the forward launch.
    Returns:
      A loss scalar with .backward / .backward_start / .backward_finish (-> grad_scale * dloss/donline, [2b, D]), the device scalar
      .cosine (mean cosine of the paired rows) and .value.
    """
    online, target = online.contiguous(), target.contiguous()
    out, row_stats = ops.byol_fwd(online, target)
    if overlap is not None:
        overlap()

    def backward(grad_scale=1.0):
        return ops.byol_bwd(online, target, row_stats, grad_scale)

    loss = _Loss(out[0:1], backward)
    loss.cosine = out[1:2]
    return loss


def add_moco_loss(online, target, queue, temperature=1.0, strategy=None, overlap=None, keys=None):
    """MoCo v2 loss (He et al. 2020; Chen et al. 2020) on the kernels of csrc/moco.hip: InfoNCE of every online row against its one
    positive momentum key and a queue of keys of earlier steps,
      s_r+ = l2n(online_r) . l2n(target_{(r + b) mod 2b}) / T,   s_rj = l2n(online_r) . queue_j / T,
      loss = (1 / b) sum_{r < 2b} [logsumexp([s_r+, s_r0 .. s_r,K-1]) - s_r+],
    the sum of the two per-view means, as add_contrastive_loss forms NT-Xent.  The negatives are the queue rows alone: the other rows
    of the batch are not.  l2n is tf.math.l2_normalize (epsilon 1e-12); always applied.  The [2b, K] logits are never written.

    Args:
      online: float32 device tensor [2b, D] = the online projection output, [view-a rows; view-b rows]; D in {64, 128, 256}.
      target: float32 device tensor [2b, D] = the target network's projection output of the same batch.  It gets no gradient.
      queue: float32 device tensor [K, D], the (normalised) keys of earlier steps.  It gets no gradient and is READ AGAIN by the
        backward, which recomputes the logits: the caller enqueues this step's keys only after `backward`.
      temperature: T.
      strategy: replica context or None.  The loss needs NO collective: a replica's value is the mean over its own rows, the mean over
        the replicas is the loss, and `backward` is called with 1 / R.
      overlap: optional zero-argument callable, run after the forward launches.
      keys: l2n(target), when the caller formed it already (the step does, to start the gather of the keys before the online forward).
    Returns:
      A loss scalar with .backward / .backward_start / .backward_finish (-> grad_scale * dloss/donline, [2b, D]), the device scalars
      .value and .acc (share of rows whose positive scores at least as high as their best negative), and .keys = l2n(target), the
      [2b, D] rows the step enqueues.
    """
    online, target = online.contiguous(), target.contiguous()
    ops._moco_check(online, target, queue, temperature)
    z, inv = ops.l2norm_fwd(online)
    if keys is None:
        keys, _ = ops.l2norm_fwd(target)
    out, row_stats, ws = ops.moco_fwd(z, keys, queue, temperature)
    if overlap is not None:
        overlap()

    def backward(grad_scale=1.0):
        return ops.l2norm_bwd(z, inv, ops.moco_bwd(z, keys, queue, temperature, row_stats, grad_scale, ws))

    loss = _Loss(out[0:1], backward)
    loss.acc = out[1:2]
    loss.keys = keys
    return loss


def add_dino_loss(online, target, prototypes, target_prototypes, center, student_temp=0.1, teacher_temp=0.04, strategy=None,
                  overlap=None, keys=None, update_prototypes=True):
    """DINO loss (Caron et al. 2021) on the kernels of csrc/dino.hip: with q = l2n(online), k = l2n(target), ws / wt the row-normalised
    prototypes of the online / the target network, c the centre and p(r) = (r + b) mod 2b,
      s_rj = q_r . ws_j / Ts,   t_rj = (k_r . wt_j - c_j) / Tt,   Ps = softmax_j(s_r),   Pt = softmax_j(t_r),
      loss = (1 / 2b) sum_{r < 2b} [logsumexp_j(s_r) - sum_j Pt[p(r), j] s_rj],
    the paper's MEAN over the two cross-view terms (the official code divides by n_loss_terms).  This differs on purpose from the
    (1 / b) sum -- the sum of the two per-view means -- of add_byol_loss and add_moco_loss.  l2n is tf.math.l2_normalize (epsilon
    1e-12); always applied.  None of the four [2b, K] matrices is written.

    Args:
      online: float32 device tensor [2b, D] = the online projection output, [view-a rows; view-b rows]; D in {64, 128, 256}.
      target: float32 device tensor [2b, D] = the target network's projection output of the same batch.  It gets no gradient.
      prototypes: the online model.PrototypeHead.  It is called here (its rows are normalised) and its `backward` receives the
        gradient of the normalised rows: grad_scale * the prototype gradient lands in the variable's gradient slot, where the
        model's backward collects parameter gradients.
      target_prototypes: float32 device tensor [K, D], the target network's row-normalised prototypes (TargetNetwork.prototypes()),
        or a PrototypeHead, which is called.  No gradient.
      center: float32 device tensor [K].  No gradient.  The backward READS IT AGAIN (it recomputes the teacher softmax), and the
        target prototypes too: the caller moves the centre and the target only after `backward`.
      student_temp, teacher_temp: Ts, Tt.
      strategy: replica context or None.  The loss needs NO collective of its own: a replica's value is the mean over its own rows,
        the mean over the replicas is the loss, `backward` is called with 1 / R, a rank's prototype gradient is the share of its own
        rows and the usual gradient synchronisation sums the shares.
      overlap: optional zero-argument callable, run after the forward launches.
      keys: l2n(target), when the caller formed it already (the step does, to start the all-reduce of its mean before the online forward).
      update_prototypes: False while the prototypes are frozen: the key-side sweep is skipped and no gradient is written.
    Returns:
      A loss scalar with .backward / .backward_start / .backward_finish (-> grad_scale * dloss/donline, [2b, D]), the device scalars
      .value and .entropy (mean entropy of the teacher rows in nats: log K = uniform, 0 = one-hot collapse), .keys = l2n(target) and
      .target_prototypes = the [K, D] rows the forward used (what the centre update reads).
    """
    online, target = online.contiguous(), target.contiguous()
    ws = prototypes()
    wt = target_prototypes if torch.is_tensor(target_prototypes) else target_prototypes()
    if not torch.is_tensor(target_prototypes):
        target_prototypes.saved = None
    z, inv = ops.l2norm_fwd(online)
    if keys is None:
        keys, _ = ops.l2norm_fwd(target)
    ops._dino_check(z, keys, ws, wt, center, student_temp, teacher_temp)
    out, row_stats, u, wsp = ops.dino_fwd(z, keys, ws, wt, center, student_temp, teacher_temp)
    if overlap is not None:
        overlap()

    def backward(grad_scale=1.0):
        dq = ops.l2norm_bwd(z, inv, ops.dino_bwd_q(z, ws, u, student_temp, row_stats, grad_scale, wsp))
        if update_prototypes:
            prototypes.backward(ops.dino_bwd_w(z, keys, ws, wt, center, student_temp, teacher_temp, row_stats, grad_scale, wsp))
        else:
            prototypes.saved = None
        return dq

    loss = _Loss(out[0:1], backward)
    loss.entropy = out[1:2]
    loss.keys = keys
    loss.target_prototypes = wt
    # what add_dino_local_loss reads for the local views of the same images
    loss.z, loss.u, loss.row_stats, loss.center = z, u, row_stats, center
    loss.student_temp, loss.teacher_temp = student_temp, teacher_temp
    return loss


def add_dino_local_loss(local_online, global_loss, prototypes, strategy=None, update_prototypes=True):
    """The multi-crop share of the DINO loss (Caron et al. 2021; the official loss with ncrops = 2 + L): every LOCAL view's student
    softmax against the teacher rows of BOTH global views of its image.  With x = l2n(local_online) [L b, D] view-major (row v b + i =
    local view v of image i), V = 2 + L and u_g = sum_j Pt[g, j] ws_j the teacher expectation add_dino_loss kept for global row g,
      value = 1 / (2 (V - 1) b) sum_r [2 logsumexp_j(s_r) - x_r . (u_i + u_{b+i}) / Ts],   s_rj = x_r . ws_j / Ts,  i = r mod b.
    The total loss of the step is global_loss.value / (V - 1) + value: every student view against every global teacher view other
    than itself, over 2 (V - 1) terms.  The teacher sees the global views only and is stop-gradient; the centre and its key mean use
    the global keys only.  No collective runs here.

    The value and the query-side backward are the loss-agnostic ops.swav_local_fwd / swav_local_bwd_x on (x, ws, u, L, Ts); the
    key-side backward is ops.dino_local_bwd_w (csrc/dino_multicrop.hip), which READS AGAIN the keys, the target prototypes and the
    centre add_dino_loss read: the caller moves the centre and the target only after `backward`.

    Args:
      local_online: float32 device tensor [L b, D] = the online projection output of the L local views, view-major.
      global_loss: the handle add_dino_loss returned for the two global views of the same b images (its keys, target_prototypes, u,
        row_stats, center and temperatures).
      prototypes: the online model.PrototypeHead.  It is called here again (the variable has not moved since add_dino_loss: the
        normalised rows are bitwise the same) and its `backward` receives the gradient of the normalised rows, student and teacher
        term together.
      strategy: replica context or None; unused beyond the signature's symmetry: a replica's value is the share of its own rows.
      update_prototypes: False while the prototypes are frozen: both key-side sweeps are skipped and no gradient is written.
    Returns:
      A loss scalar with .value and .backward(grad_scale) (-> grad_scale * dvalue/dlocal_online, [L b, D]).
    """
    x_raw = local_online.contiguous()
    keys, u = global_loss.keys, global_loss.u
    b = keys.shape[0] // 2
    if x_raw.dim() != 2 or x_raw.shape[0] < b or x_raw.shape[0] % b:
        raise ValueError('add_dino_local_loss: the local block holds L views of the %d images of the global loss, [L * %d, D] (got %s)'
                         % (b, b, tuple(x_raw.shape)))
    L = x_raw.shape[0] // b
    if not 1 <= L <= ops.DINO_MAX_LOCAL_CROPS:
        raise ValueError('add_dino_local_loss: the number of local views lies in [1, %d] (got %d)' % (ops.DINO_MAX_LOCAL_CROPS, L))
    ts, tt = global_loss.student_temp, global_loss.teacher_temp
    ws = prototypes()
    x, inv = ops.l2norm_fwd(x_raw)
    # row_stats [L b]: lse_s of the local rows in the base-2 domain, what dino_local_bwd_w's student sweep normalises with
    out, row_stats, wsp = ops.swav_local_fwd(x, ws, u, L, ts)

    def backward(grad_scale=1.0):
        dx = ops.l2norm_bwd(x, inv, ops.swav_local_bwd_x(x, ws, u, L, ts, row_stats, grad_scale, wsp))
        if update_prototypes:
            prototypes.backward(ops.dino_local_bwd_w(x, keys, ws, global_loss.target_prototypes, global_loss.center, L, ts, tt,
                                                     row_stats, global_loss.row_stats, grad_scale))
        else:
            prototypes.saved = None
        return dx

    return _Loss(out[0:1], backward)


def add_swav_loss(online, prototypes, temperature=0.1, epsilon=0.05, sinkhorn_iterations=3, strategy=None, overlap=None,
                  update_prototypes=True):
    """SwAV loss (Caron et al. 2020) on the kernels of csrc/swav.hip: with q = l2n(online), w the row-normalised prototypes,
    p(r) = (r + b) mod 2b, v(r) the view of row r and alpha [2, K] the per-view column potentials of the Sinkhorn-Knopp assignment,
      s_rj = q_r . w_j / T,   t_rj = q_r . w_j / eps + alpha[v(r)][j],   Ps = softmax_j(s_r),   Pt = softmax_j(t_r)  (the CODE of row r),
      loss = (1 / 2b) sum_{r < 2b} [logsumexp_j(s_r) - sum_j Pt[p(r), j] s_rj],
    the paper's mean over the two swapped terms (add_dino_loss's convention, not the (1 / b) sum of add_byol_loss / add_moco_loss).
    The codes are STOP-GRADIENT: alpha and Pt are constants of the backward.  l2n is tf.math.l2_normalize (epsilon 1e-12); always
    applied.  No [2b, K] or [2N, K] matrix is written.

    The Sinkhorn is GLOBAL and PER VIEW, as the official distributed_sinkhorn: the normalised block is all-gathered (detached: the
    backward has no reduce-scatter) and every replica runs the same iteration on the same gathered block in the one fixed order, so alpha
    is bitwise identical on every rank and no further collective is needed (the Barlow Twins idiom).  With a global batch smaller than K
    the iteration stays well defined: every prototype still receives N / K of a view's mass, the codes are simply spread over more
    prototypes than there are rows (the official code uses a feature queue there; not built).

    Args:
      online: float32 device tensor [2b, D] = the online projection output, [view-a rows; view-b rows]; D in {64, 128, 256}.
      prototypes: the model.PrototypeHead.  It is called here (its rows are normalised) and its `backward` receives the gradient of the
        normalised rows: grad_scale * the prototype gradient lands in the variable's gradient slot.
      temperature, epsilon, sinkhorn_iterations: T, eps and I (1 .. 16).
      strategy: replica context or None.  A replica's value is the mean over its own rows, the mean over the replicas is the loss,
        `backward` is called with 1 / R, a rank's prototype gradient is the share of its own rows and the usual gradient synchronisation
        sums the shares.
      overlap: optional zero-argument callable, run after the forward launches.
      update_prototypes: False while the prototypes are frozen: the key-side sweep is skipped and no gradient is written.
    Returns:
      A loss scalar with .backward / .backward_start / .backward_finish (-> grad_scale * dloss/donline, [2b, D]), the device scalars
      .value and .entropy (mean entropy of the codes in nats: log K = uniform, 0 = one-hot) and .alpha [2, K].
    """
    online = online.contiguous()
    w = prototypes()
    z, inv = ops.l2norm_fwd(online)
    ops._swav_check('add_swav_loss', z, w)
    z_all = gather_hidden(z.detach(), strategy)
    alpha = ops.swav_sinkhorn(z_all, w, epsilon, sinkhorn_iterations)
    out, row_stats, u, wsp = ops.swav_fwd(z, w, alpha, temperature, epsilon)
    if overlap is not None:
        overlap()

    def backward(grad_scale=1.0):
        dq = ops.l2norm_bwd(z, inv, ops.swav_bwd_q(z, w, u, temperature, row_stats, grad_scale, wsp))
        if update_prototypes:
            prototypes.backward(ops.swav_bwd_w(z, w, alpha, temperature, epsilon, row_stats, grad_scale, wsp))
        else:
            prototypes.saved = None
        return dq

    loss = _Loss(out[0:1], backward)
    loss.entropy = out[1:2]
    loss.alpha = alpha
    # what add_swav_local_loss reads for the local views of the same images
    loss.z, loss.u, loss.row_stats, loss.epsilon = z, u, row_stats, epsilon
    return loss


def add_swav_local_loss(local_online, global_loss, prototypes, temperature=0.1, strategy=None, update_prototypes=True):
    """The multi-crop share of the SwAV loss (Caron et al. 2020, section 4; the official loss with crops_for_assign = [0, 1]) on the
    kernels of csrc/swav_multicrop.hip: every LOCAL view's softmax over the prototypes against the codes of BOTH global views of its
    image.  With x = l2n(local_online) [L b, D] view-major (row v b + i = local view v of image i), V = 2 + L and u_g = sum_j Pt[g, j] w_j
    the code expectation add_swav_loss kept for global row g,
      value = 1 / (2 (V - 1) b) sum_r [2 logsumexp_j(s_r) - x_r . (u_i + u_{b+i}) / T],   s_rj = x_r . w_j / T,  i = r mod b.
    The total loss of the step is global_loss.value / (V - 1) + value.  The codes are the global views' alone and stop-gradient: the
    local rows take no part in the Sinkhorn, so nothing is gathered here and no collective runs.

    Args:
      local_online: float32 device tensor [L b, D] = the online projection output of the L local views, view-major.
      global_loss: the handle add_swav_loss returned for the two global views of the same b images (its z, u, row_stats, alpha, epsilon).
      prototypes: the model.PrototypeHead.  It is called here again (the variable has not moved since add_swav_loss: the normalised
        rows are bitwise the same) and its `backward` receives the gradient of the normalised rows, student and code term together.
      temperature: T, the one add_swav_loss was given.
      strategy: replica context or None; unused beyond the signature's symmetry: a replica's value is the share of its own rows.
      update_prototypes: False while the prototypes are frozen: both key-side sweeps are skipped and no gradient is written.
    Returns:
      A loss scalar with .value and .backward(grad_scale) (-> grad_scale * dvalue/dlocal_online, [L b, D]).
    """
    x_raw = local_online.contiguous()
    zg, u = global_loss.z, global_loss.u
    b = zg.shape[0] // 2
    if x_raw.dim() != 2 or x_raw.shape[0] < b or x_raw.shape[0] % b:
        raise ValueError('add_swav_local_loss: the local block holds L views of the %d images of the global loss, [L * %d, D] (got %s)'
                         % (b, b, tuple(x_raw.shape)))
    L = x_raw.shape[0] // b
    w = prototypes()
    x, inv = ops.l2norm_fwd(x_raw)
    out, row_stats, wsp = ops.swav_local_fwd(x, w, u, L, temperature)

    def backward(grad_scale=1.0):
        dx = ops.l2norm_bwd(x, inv, ops.swav_local_bwd_x(x, w, u, L, temperature, row_stats, grad_scale, wsp))
        if update_prototypes:
            prototypes.backward(ops.swav_local_bwd_w(x, zg, w, global_loss.alpha, L, temperature, global_loss.epsilon, row_stats,
                                                     global_loss.row_stats, grad_scale, wsp))
        else:
            prototypes.saved = None
        return dx

    return _Loss(out[0:1], backward)


def add_supervised_loss(labels, logits):
    """Compute mean supervised loss over local batch (tf2/objective.py:27-32).

    labels: one-hot float [b or 2b, C] (as in the reference) or int class ids [b or 2b]; when
    it holds b rows and the logits 2b, the labels are reused for both views (tf2/run.py:599-600).
    logits: model.SupLogits.  Returns a loss scalar with .backward() -> dlogits and `.acc`.
    """
    labels = _class_ids(labels)
    out = ops.step_scalars(2, logits.z.device)
    gscale = 1.0 / num_replicas(RT.strategy)                    # loss / R, tf2/run.py:617
    dlogits = ops.bias_softmax_xent(logits.z, logits.bias, labels, logits.num_classes, gscale, out)
    loss = _Loss(out[0:1], lambda grad_scale=None: dlogits)
    loss.acc = out[1:2]
    return loss


def add_kd_loss(student_logits, teacher_logits, temperature):
    """Distillation loss of the self-training stage (tf2/colabs/distillation_self_training.ipynb:803-808):
    temperature^2 * mean over the local batch of CE(softmax(teacher / temperature), student / temperature).

    student_logits, teacher_logits: model.SupLogits of the same rows.  Returns a loss scalar with .backward() -> dlogits (gradient
    wrt the student's logits, in their layout) and `.acc`, the share of rows whose student and teacher arg-maxima agree."""
    if student_logits.num_classes != teacher_logits.num_classes:
        raise ValueError('add_kd_loss: the student has %d classes, the teacher %d'
                         % (student_logits.num_classes, teacher_logits.num_classes))
    out = ops.step_scalars(2, student_logits.z.device)
    gscale = 1.0 / num_replicas(RT.strategy)                    # loss / R, tf2/run.py:617
    dlogits = ops.kd_softmax_xent(student_logits.z, student_logits.bias, teacher_logits.z, teacher_logits.bias,
                                  student_logits.num_classes, temperature, gscale, out)
    loss = _Loss(out[0:1], lambda grad_scale=None: dlogits)
    loss.acc = out[1:2]
    return loss
