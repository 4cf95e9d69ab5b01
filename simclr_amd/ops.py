"""Thin torch-tensor wrappers over the C ABI (include/simclr_hip.h).

PyTorch is plumbing here: it owns device memory and the stream; every function
below only validates shapes and forwards raw device pointers to libsimclr_hip.so.
All tensors must be CUDA (ROCm) tensors, contiguous.
"""
import ctypes
import os
import struct

import torch

from ._lib import DT_BF16, DT_F32, lib

NSLOT = 32  # default slot count of hand-filled statistics buffers (tests); producers ask the library (conv_stats_slots ...)


class KernelProfiler:
    """Live per-launch timing with HIP events on the launch stream (torch's current stream is the
    stream every kernel here is enqueued on).  Used by bench.py for the roofline object."""

    def __init__(self):
        self.records = []   # (family, flops, min bytes, as-implemented bytes, start_event, end_event)

    def launch(self, family, flops, nbytes, impl_bytes, fn):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        self.records.append((family, flops, nbytes, impl_bytes, a, b))
        return r

    def summary(self):
        out = {}
        for fam, fl, by, ib, a, b in self.records:
            d = out.setdefault(fam, dict(launches=0, ms=0.0, flops=0.0, bytes=0.0, impl_bytes=0.0))
            d['launches'] += 1
            d['ms'] += a.elapsed_time(b)
            d['flops'] += fl
            d['bytes'] += by
            d['impl_bytes'] += ib
        return out


PROFILER = None


def _launch(family, flops, nbytes, fn, impl_bytes=None):
    """nbytes: SURVEY 8(d)'s MINIMUM bytes of the op (every operand read once, the result written once);
    impl_bytes: what this implementation moves by design (extra operands of fused epilogues), default = nbytes."""
    if PROFILER is None:
        return fn()
    return PROFILER.launch(family, flops, nbytes, nbytes if impl_bytes is None else impl_bytes, fn)


def dt(t):
    if t.dtype == torch.float32:
        return DT_F32
    if t.dtype == torch.bfloat16:
        return DT_BF16
    raise TypeError('unsupported dtype %s' % t.dtype)


def _p(t):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), 'need contiguous device tensor'
    assert getattr(t, '_ps', None) is None, 'a pre-split tensor reached an operation that reads plain floats'
    return ctypes.c_void_p(t.data_ptr())


# ---- pre-split block format (csrc/common.h): an fp32-typed tensor whose 128-byte blocks hold (hi, lo) 16-bit pieces -----------
# Tensors in that format carry the Python attribute `_ps` ('b16' | 'f16'); only the operations that name it accept them (_pp).
FMT_PS_IN, FMT_PS_OUT, FMT_PS_F16, FMT_PS_IN2, FMT_PS_W = 0x100, 0x200, 0x400, 0x800, 0x100000


def ps_kind(t):
    return getattr(t, '_ps', None) if t is not None else None


def _pp(t):
    """Pointer of a tensor that may be pre-split (the callee is told through the dtype flags)."""
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), 'need contiguous device tensor'
    return ctypes.c_void_p(t.data_ptr())


def _pw(w, fwd):
    """(pointer, dtype flag) of a compute-weight operand: its pre-split copy (WeightPairBatch) with SIMCLR_FMT_PS_W when one exists for the
    terms this call runs with, else the fp32 matrix itself."""
    ps = getattr(w, '_psw', None)
    if ps is not None and ps[1] == (_TERMS[0] if fwd else _TERMS[1]):
        return ctypes.c_void_p(ps[0].data_ptr()), FMT_PS_W
    return _p(w), 0


def ps_backward_enabled():
    """Gradient tensors between a BatchNorm backward and the convolution in front of it in the pre-split format: fp32 storage,
    three bf16 backward terms (FLAGS.f32_matmul in 'bf16x3' | 'bf16x6_3' | 'f16x3_3'), SIMCLR_PS_BWD != 0."""
    import os
    if os.environ.get('SIMCLR_PS_BWD', '1') in ('', '0') or os.environ.get('SIMCLR_F32_PRESPLIT', '1') in ('', '0'):
        return False
    return _TERMS[1] == 3


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------- NT-Xent
def l2norm_fwd(x):
    rows, D = x.shape
    z = torch.empty_like(x)
    inv = torch.empty(rows, device=x.device, dtype=torch.float32)
    _launch('l2norm_fwd', 3.0 * rows * D, 8.0 * rows * D, lambda: lib().l2norm_fwd(_p(x), _p(z), _p(inv), rows, D, _s()))
    return z, inv


def l2norm_bwd(z, inv, dz):
    dx = torch.empty_like(z)
    _launch('l2norm_bwd', 5.0 * z.numel(), 12.0 * z.numel(),
            lambda: lib().l2norm_bwd(_p(z), _p(inv), _p(dz), _p(dx), z.shape[0], z.shape[1], _s()))
    return dx


_NTXENT_DIMS = (64, 128, 256)       # embedding widths the fused kernels are instantiated for


def _ntxent_dim(D):
    """Kernel width for a `proj_out_dim` of D (a free flag in the reference, tf2/run.py:196): the next instantiated width.
    Zero columns change neither the dot products nor the norms, so other widths run zero-padded."""
    for d in _NTXENT_DIMS:
        if D <= d:
            return d
    raise ValueError('NT-Xent kernels support proj_out_dim <= %d (got %d)' % (_NTXENT_DIMS[-1], D))


def _ntxent_pad(z):
    D = z.shape[1]
    Dk = _ntxent_dim(D)
    return z if Dk == D else torch.nn.functional.pad(z, (0, Dk - D))


def ntxent_is_wide(D):
    """Embeddings wider than the register-resident sweeps (proj_out_dim > 256, proj_head_mode='none') run the wide NT-Xent path."""
    return D > _NTXENT_DIMS[-1]


def ntxent_workspace(n, N, D, device):
    if ntxent_is_wide(D):
        return ntxent_wide_workspace(n, N, D, device)
    D = _ntxent_dim(D)
    nbytes = lib().ntxent_workspace_bytes(n, N, D)
    return torch.empty((nbytes + 3) // 4, device=device, dtype=torch.float32)


def ntxent_fwd(z_local, z_all, rank, temperature, ws=None, split=False):
    """split: three fp16-piece MFMA terms per fp32 product in the sweeps (SIMCLR_FMT_TERMS(13) in the D argument) -- for
    l2-normalised rows; default = exact fp32-input MFMA.  D > 256 runs the wide path, which has exact arithmetic only: there
    split is ignored (FLAGS.ntxent_matmul's help says so)."""
    n, D = z_local.shape[0] // 2, z_local.shape[1]
    N = z_all.shape[0] // 2
    assert z_local.dtype == torch.float32 and z_all.dtype == torch.float32
    if ntxent_is_wide(D):
        return ntxent_wide_fwd(z_local, z_all, rank, temperature, ws)
    z_local, z_all = _ntxent_pad(z_local), _ntxent_pad(z_all)
    D = z_local.shape[1]
    if ws is None:
        ws = ntxent_workspace(n, N, D, z_local.device)
    out = step_scalars(4, z_local.device)
    row_stats = torch.empty(2 * n, 2, device=z_local.device, dtype=torch.float32)
    _launch('ntxent_fwd', 8.0 * n * N * D, 4.0 * (2 * n + 2 * N) * D,
            lambda: lib().ntxent_fwd(_p(z_local), _p(z_all), n, N, D | ((14 << 12) if split else 0), rank, float(temperature), _p(out), _p(row_stats),
                                     _p(ws), _s()))
    return out, row_stats, ws


def ntxent_bwd(z_local, z_all, rank, temperature, row_stats, grad_scale, out, ws, split=False):
    n, D0 = z_local.shape[0] // 2, z_local.shape[1]
    N = z_all.shape[0] // 2
    if ntxent_is_wide(D0):
        return ntxent_wide_bwd(z_local, z_all, rank, temperature, row_stats, grad_scale, out, ws)
    z_local, z_all = _ntxent_pad(z_local), _ntxent_pad(z_all)
    D = z_local.shape[1]
    dz_local = torch.empty_like(z_local)
    dz_all = torch.empty_like(z_all)
    # bytes: the fused forward+backward I/O of SURVEY 8(d): read h_local + h_all, write dH_local + dH_all
    _launch('ntxent_bwd', 16.0 * n * N * D, 2.0 * (2 * n + 2 * N) * D * 4,
            lambda: lib().ntxent_bwd(_p(z_local), _p(z_all), n, N, D | ((14 << 12) if split else 0), rank, float(temperature), _p(row_stats),
                                     float(grad_scale), _p(dz_local), _p(dz_all), _p(out), _p(ws), _s()))
    if D != D0:
        dz_local, dz_all = dz_local[:, :D0].contiguous(), dz_all[:, :D0].contiguous()
    return dz_local, dz_all


def ntxent_logits_ab(z_local, z_all, temperature):
    if ntxent_is_wide(z_local.shape[1]):
        return ntxent_wide_logits_ab(z_local, z_all, temperature)
    z_local, z_all = _ntxent_pad(z_local), _ntxent_pad(z_all)
    n, D = z_local.shape[0] // 2, z_local.shape[1]
    N = z_all.shape[0] // 2
    out = torch.empty(n, N, device=z_local.device, dtype=torch.float32)
    lib().ntxent_logits_ab(_p(z_local), _p(z_all), n, N, D, float(temperature), _p(out), _s())
    return out


# Wide NT-Xent (csrc/ntxent.hip, simclr_ntxent_wide_*): any width D as LDS-tiled GEMMs with a k-loop over D, exact fp32-input MFMA.
# ntxent_fwd / _bwd / _logits_ab / _workspace route D > 256 here; the functions are public so that the two paths can be compared at
# D <= 256.  Same return contracts as their register-resident counterparts.
def ntxent_wide_workspace(n, N, D, device):
    nbytes = lib().ntxent_wide_workspace_bytes(n, N, D)
    assert nbytes > 0, 'ntxent_wide_workspace: bad shape n=%d N=%d D=%d' % (n, N, D)
    return torch.empty((nbytes + 3) // 4, device=device, dtype=torch.float32)


def ntxent_wide_fwd(z_local, z_all, rank, temperature, ws=None):
    n, D = z_local.shape[0] // 2, z_local.shape[1]
    N = z_all.shape[0] // 2
    assert z_local.dtype == torch.float32 and z_all.dtype == torch.float32 and z_all.shape[1] == D
    if ws is None:
        ws = ntxent_wide_workspace(n, N, D, z_local.device)
    out = step_scalars(4, z_local.device)
    row_stats = torch.empty(2 * n, 2, device=z_local.device, dtype=torch.float32)
    _launch('ntxent_wide_fwd', 8.0 * n * N * D, 4.0 * (2 * n + 2 * N) * D,
            lambda: lib().ntxent_wide_fwd(_p(z_local), _p(z_all), n, N, D, 0, rank, float(temperature), _p(out), _p(row_stats),
                                          _p(ws), _s()))
    return out, row_stats, ws


def ntxent_wide_bwd(z_local, z_all, rank, temperature, row_stats, grad_scale, out, ws):
    n, D = z_local.shape[0] // 2, z_local.shape[1]
    N = z_all.shape[0] // 2
    dz_local = torch.empty_like(z_local)
    dz_all = torch.empty_like(z_all)
    # flops: S recomputed + dS K + dS^T Q; bytes: read h_local + h_all, write dH_local + dH_all (as ntxent_bwd)
    _launch('ntxent_wide_bwd', 24.0 * n * N * D, 2.0 * (2 * n + 2 * N) * D * 4,
            lambda: lib().ntxent_wide_bwd(_p(z_local), _p(z_all), n, N, D, 0, rank, float(temperature), _p(row_stats),
                                          float(grad_scale), _p(dz_local), _p(dz_all), _p(out), _p(ws), _s()))
    return dz_local, dz_all


def ntxent_wide_logits_ab(z_local, z_all, temperature):
    n, D = z_local.shape[0] // 2, z_local.shape[1]
    N = z_all.shape[0] // 2
    out = torch.empty(n, N, device=z_local.device, dtype=torch.float32)
    lib().ntxent_wide_logits_ab(_p(z_local), _p(z_all), n, N, D, 0, float(temperature), _p(out), _s())
    return out


# ---------------------------------------------------------------- generalized contrastive loss (csrc/gcl.hip)
GCL_DIMS = (64, 128, 256)           # hidden widths the generalized-loss kernels are instantiated for (no padding: log D is in the loss)
SWD_MAX_ROWS = 8192                 # global rows (2N) a column sort holds in LDS


def _gcl_check_dim(D):
    if D not in GCL_DIMS:
        raise ValueError('the generalized contrastive loss supports hidden widths %s (got %d)' % ('/'.join(map(str, GCL_DIMS)), D))


def gcl_lse_workspace(n, N, D, device):
    _gcl_check_dim(D)
    nbytes = lib().gcl_lse_workspace_bytes(n, N, D)
    assert nbytes > 0, 'gcl_lse_workspace: bad shape n=%d N=%d D=%d' % (n, N, D)
    return torch.empty((nbytes + 3) // 4, device=device, dtype=torch.float32)


def gcl_lse_fwd(z_local, z_all, temperature, lambda_weight=1.0, loss_scaling=1.0, ws=None):
    """Decoupled NT-Xent forward.  Returns out = [loss, align, dist_match] (device), row_stats [2n], the workspace."""
    n, D = z_local.shape[0] // 2, z_local.shape[1]
    N = z_all.shape[0] // 2
    assert z_local.dtype == torch.float32 and z_all.dtype == torch.float32 and z_all.shape[1] == D
    _gcl_check_dim(D)
    if ws is None:
        ws = gcl_lse_workspace(n, N, D, z_local.device)
    out = step_scalars(4, z_local.device)
    row_stats = torch.empty(2 * n, device=z_local.device, dtype=torch.float32)
    _launch('gcl_lse_fwd', 8.0 * n * N * D, 4.0 * (2 * n + 2 * N) * D,
            lambda: lib().gcl_lse_fwd(_p(z_local), _p(z_all), n, N, D, float(temperature), float(lambda_weight), float(loss_scaling),
                                      _p(out), _p(row_stats), _p(ws), _s()))
    return out, row_stats, ws


def gcl_lse_bwd(z_local, z_all, temperature, row_stats, grad_scale, ws, lambda_weight=1.0, loss_scaling=1.0, rank=0, skip_self=False):
    """skip_self: leave out the (radial) term of every row's own column -- for l2-normalised rows, whose normalisation backward removes
    it anyway (include/simclr_hip.h)."""
    n, D = z_local.shape[0] // 2, z_local.shape[1]
    N = z_all.shape[0] // 2
    _gcl_check_dim(D)
    dz_local = torch.empty_like(z_local)
    dz_all = torch.empty_like(z_all)
    _launch('gcl_lse_bwd', 16.0 * n * N * D, 2.0 * (2 * n + 2 * N) * D * 4,
            lambda: lib().gcl_lse_bwd(_p(z_local), _p(z_all), n, N, D, float(temperature), float(lambda_weight), float(loss_scaling),
                                      int(rank), int(bool(skip_self)), _p(row_stats), float(grad_scale), _p(dz_local), _p(dz_all), _p(ws), _s()))
    return dz_local, dz_all


def gcl_gemm_nt(A, B):
    """A [M, K] fp32, B [N, K] fp32 -> A B^T [M, N] fp32 (exact f32 MFMA), any M and N, K a multiple of 16."""
    M, K = A.shape
    N = B.shape[0]
    assert A.dtype == torch.float32 and B.dtype == torch.float32 and B.shape[1] == K
    C = torch.empty(M, N, device=A.device, dtype=torch.float32)
    _launch('gcl_gemm_nt', 2.0 * M * N * K, 4.0 * (M * K + N * K + M * N), lambda: lib().gcl_gemm_nt(_p(A), _p(B), _p(C), M, N, K, _s()))
    return C


def swd_sort_match(Pt, Qt, coeff, want_perm=False):
    """Pt, Qt [D, M] fp32 (one row per projected dimension).  Returns dP [M, D] (= coeff * (P_sorted - Q_sorted) scattered back to row
    order), col_loss [D] and, on request, perm [D, M] int32 (the stable sorting permutation of every row of Pt)."""
    D, M = Pt.shape
    assert Pt.dtype == torch.float32 and Qt.dtype == torch.float32 and tuple(Qt.shape) == (D, M)
    if M > SWD_MAX_ROWS:
        raise ValueError('the sliced-Wasserstein sort holds at most %d global rows (2 x global batch) per column, got %d' % (SWD_MAX_ROWS, M))
    dP = torch.empty(M, D, device=Pt.device, dtype=torch.float32)
    col_loss = torch.empty(D, device=Pt.device, dtype=torch.float32)
    perm = torch.empty(D, M, device=Pt.device, dtype=torch.int32) if want_perm else None
    logm = max(1, (M - 1).bit_length())
    _launch('swd_sort_match', 3.0 * D * M * logm * (logm + 1), 4.0 * 3 * D * M,
            lambda: lib().swd_sort_match(_p(Pt), _p(Qt), M, D, float(coeff), _p(dP), _p(col_loss), _p(perm), _s()))
    return dP, col_loss, perm


def gcl_swd_out(col_loss, z_local, M, lambda_weight=1.0, loss_scaling=1.0):
    """out = [loss, align, dist_match] of an SWD loss from the column losses of swd_sort_match."""
    n, D = z_local.shape[0] // 2, z_local.shape[1]
    out = step_scalars(4, z_local.device)
    lib().gcl_swd_out(_p(col_loss), _p(z_local), n, M, D, float(lambda_weight), float(loss_scaling), _p(out), _s())
    return out


def gcl_swd_bwd(g_all, z_local, rank, grad_scale, lambda_weight=1.0, loss_scaling=1.0):
    n, D = z_local.shape[0] // 2, z_local.shape[1]
    N = g_all.shape[0] // 2
    dz_local = torch.empty_like(z_local)
    lib().gcl_swd_bwd(_p(g_all), _p(z_local), n, N, D, rank, float(lambda_weight), float(loss_scaling), float(grad_scale), _p(dz_local), _s())
    return dz_local


# ---------------------------------------------------------------- supervised contrastive loss (csrc/supcon.hip)
SUPCON_DIMS = (64, 128, 256)        # hidden widths the supervised contrastive kernels are instantiated for


def _supcon_check_dim(D):
    if D not in SUPCON_DIMS:
        raise ValueError('the supervised contrastive loss supports hidden widths %s (got %d)' % ('/'.join(map(str, SUPCON_DIMS)), D))


def _supcon_check(z_local, z_all, labels_all):
    n, D = z_local.shape[0] // 2, z_local.shape[1]
    N = z_all.shape[0] // 2
    assert z_local.dtype == torch.float32 and z_all.dtype == torch.float32 and z_all.shape[1] == D
    _supcon_check_dim(D)
    if n < 1 or z_local.shape[0] != 2 * n or N < n or N % n != 0 or z_all.shape[0] != 2 * N:
        raise ValueError('supcon: need z_local [2n, D] with n >= 1 and z_all [2N, D] with N = R*n (got %d and %d rows)'
                         % (z_local.shape[0], z_all.shape[0]))
    if labels_all.dtype != torch.int32 or labels_all.dim() != 1 or labels_all.shape[0] != N:
        raise ValueError('supcon: labels_all must hold the N = %d int32 class ids of the global batch (got %s %s)'
                         % (N, tuple(labels_all.shape), labels_all.dtype))
    return n, N, D


def supcon_workspace(n, N, D, device):
    _supcon_check_dim(D)
    nbytes = lib().supcon_workspace_bytes(n, N, D)
    assert nbytes > 0, 'supcon_workspace: bad shape n=%d N=%d D=%d' % (n, N, D)
    return torch.empty((nbytes + 3) // 4, device=device, dtype=torch.float32)


def supcon_fwd(z_local, z_all, labels_all, rank, temperature, ws=None):
    """Supervised contrastive forward.  labels_all [N] int32: the class ids of the global batch in z_all's sample order.
    Returns out = [loss, contrast_acc, contrast_positives] (device), row_stats [2n, 2], the workspace."""
    n, N, D = _supcon_check(z_local, z_all, labels_all)
    if ws is None:
        ws = supcon_workspace(n, N, D, z_local.device)
    out = step_scalars(4, z_local.device)
    row_stats = torch.empty(2 * n, 2, device=z_local.device, dtype=torch.float32)
    _launch('supcon_fwd', 8.0 * n * N * D, 4.0 * (2 * n + 2 * N) * D,
            lambda: lib().supcon_fwd(_p(z_local), _p(z_all), _p(labels_all), n, N, D, int(rank), float(temperature), _p(out), _p(row_stats),
                                     _p(ws), _s()))
    return out, row_stats, ws


def supcon_bwd(z_local, z_all, labels_all, rank, temperature, row_stats, grad_scale, ws):
    n, N, D = _supcon_check(z_local, z_all, labels_all)
    dz_local = torch.empty_like(z_local)
    dz_all = torch.empty_like(z_all)
    _launch('supcon_bwd', 24.0 * n * N * D, 2.0 * (2 * n + 2 * N) * D * 4,
            lambda: lib().supcon_bwd(_p(z_local), _p(z_all), _p(labels_all), n, N, D, int(rank), float(temperature), _p(row_stats),
                                     float(grad_scale), _p(dz_local), _p(dz_all), _p(ws), _s()))
    return dz_local, dz_all


# ---------------------------------------------------------------- hard-negative and debiased NT-Xent (csrc/hcl.hip)
HCL_DIMS = (64, 128, 256)           # hidden widths the hard-negative / debiased NT-Xent kernels are instantiated for


def hcl_beta_ok(beta):
    return 0.0 <= beta < float('inf')          # (NaN fails the comparison)


def hcl_tau_plus_ok(tau_plus):
    return 0.0 <= tau_plus < 1.0


def _hcl_check(z_local, z_all, beta, tau_plus):
    n, D = z_local.shape[0] // 2, z_local.shape[1]
    N = z_all.shape[0] // 2
    assert z_local.dtype == torch.float32 and z_all.dtype == torch.float32 and z_all.shape[1] == D
    if D not in HCL_DIMS:
        raise ValueError('the hard-negative / debiased NT-Xent supports hidden widths %s (got %d)' % ('/'.join(map(str, HCL_DIMS)), D))
    if n < 1 or z_local.shape[0] != 2 * n or N < 2 or N < n or N % n != 0 or z_all.shape[0] != 2 * N:
        raise ValueError('hcl: need z_local [2n, D] with n >= 1 and z_all [2N, D] with N = R*n >= 2 (got %d and %d rows)'
                         % (z_local.shape[0], z_all.shape[0]))
    if not hcl_beta_ok(beta):
        raise ValueError('hcl: beta must be >= 0 and finite (got %r)' % (beta,))
    if not hcl_tau_plus_ok(tau_plus):
        raise ValueError('hcl: tau_plus must lie in [0, 1) (got %r)' % (tau_plus,))
    return n, N, D


def hcl_workspace(n, N, D, device):
    nbytes = lib().hcl_workspace_bytes(n, N, D)
    assert nbytes > 0, 'hcl_workspace: bad shape n=%d N=%d D=%d' % (n, N, D)
    return torch.empty((nbytes + 3) // 4, device=device, dtype=torch.float32)


def hcl_fwd(z_local, z_all, rank, temperature, beta, tau_plus, ws=None):
    """Hard-negative (beta) and debiased (tau_plus) NT-Xent forward.  Returns out = [loss, share of the local rows on the floor]
    (device), row_stats [2n, 4] = {log2 A, log2 B, negative coefficient, positive coefficient}, the workspace."""
    n, N, D = _hcl_check(z_local, z_all, beta, tau_plus)
    if ws is None:
        ws = hcl_workspace(n, N, D, z_local.device)
    out = step_scalars(4, z_local.device)
    row_stats = torch.empty(2 * n, 4, device=z_local.device, dtype=torch.float32)
    _launch('hcl_fwd', 8.0 * n * N * D, 4.0 * (2 * n + 2 * N) * D,
            lambda: lib().hcl_fwd(_p(z_local), _p(z_all), n, N, D, int(rank), float(temperature), float(beta), float(tau_plus), _p(out),
                                  _p(row_stats), _p(ws), _s()))
    return out, row_stats, ws


def hcl_bwd(z_local, z_all, rank, temperature, beta, tau_plus, row_stats, grad_scale, ws):
    n, N, D = _hcl_check(z_local, z_all, beta, tau_plus)
    assert tuple(row_stats.shape) == (2 * n, 4) and row_stats.dtype == torch.float32
    dz_local = torch.empty_like(z_local)
    dz_all = torch.empty_like(z_all)
    _launch('hcl_bwd', 24.0 * n * N * D, 2.0 * (2 * n + 2 * N) * D * 4,
            lambda: lib().hcl_bwd(_p(z_local), _p(z_all), n, N, D, int(rank), float(temperature), float(beta), float(tau_plus),
                                  _p(row_stats), float(grad_scale), _p(dz_local), _p(dz_all), _p(ws), _s()))
    return dz_local, dz_all


# ---------------------------------------------------------------- NNCLR: nearest-neighbour positives for NT-Xent (csrc/nnclr.hip)
NNCLR_DIMS = (64, 128, 256)         # hidden widths the NNCLR kernels are instantiated for


def _nnclr_check(nn_local, z_all, temperature):
    if (nn_local.dim() != 2 or z_all.dim() != 2 or nn_local.dtype != torch.float32 or z_all.dtype != torch.float32
            or z_all.shape[1] != nn_local.shape[1]):
        raise ValueError('nnclr: need float32 neighbour rows [2n, D] and z_all [2N, D] of one width (got %s %s and %s %s)'
                         % (tuple(nn_local.shape), nn_local.dtype, tuple(z_all.shape), z_all.dtype))
    n, D = nn_local.shape[0] // 2, nn_local.shape[1]
    N = z_all.shape[0] // 2
    if D not in NNCLR_DIMS:
        raise ValueError('the NNCLR kernels support hidden widths %s (got %d)' % ('/'.join(map(str, NNCLR_DIMS)), D))
    if n < 1 or nn_local.shape[0] != 2 * n or N < 2 or N < n or N % n != 0 or z_all.shape[0] != 2 * N:
        raise ValueError('nnclr: need neighbour rows [2n, D] with n >= 1 and z_all [2N, D] with N = R*n >= 2 (got %d and %d rows)'
                         % (nn_local.shape[0], z_all.shape[0]))
    if not 0.0 < float(temperature) < float('inf'):
        raise ValueError('nnclr: temperature must be > 0 and finite (got %r)' % (temperature,))
    if not nn_local.is_contiguous() or not z_all.is_contiguous():
        raise ValueError('nnclr: the neighbour rows and z_all must be contiguous')
    return n, N, D


def nnclr_workspace(n, N, D, device):
    nbytes = lib().nnclr_workspace_bytes(n, N, D)
    if nbytes <= 0:
        raise ValueError('nnclr_workspace: bad shape n=%d N=%d D=%d' % (n, N, D))
    return torch.empty((nbytes + 3) // 4, device=device, dtype=torch.float32)


def nnclr_fwd(nn_local, z_local, z_all, rank, temperature, ws=None):
    """NNCLR forward: the neighbour rows nn_local [2n, D] against the other view's N columns of z_all [2N, D]; z_local [2n, D] is read
    for nn_sim only.  Returns out = [loss share, acc, nn_sim, -] (device), row_stats [2n, 4] = {log2-sum-exp2 as a float, what the float left
    of it, 1 - P_r,p(r), z_r . nn_r}, the workspace."""
    n, N, D = _nnclr_check(nn_local, z_all, temperature)
    if tuple(z_local.shape) != (2 * n, D) or z_local.dtype != torch.float32 or not z_local.is_contiguous():
        raise ValueError('nnclr_fwd: z_local must be the contiguous float32 %s block the neighbours were searched for (got %s %s)'
                         % ((2 * n, D), tuple(z_local.shape), z_local.dtype))
    if not 0 <= int(rank) < N // n:
        raise ValueError('nnclr_fwd: rank %d outside the %d replicas' % (rank, N // n))
    if ws is None:
        ws = nnclr_workspace(n, N, D, nn_local.device)
    if ws.numel() * ws.element_size() < lib().nnclr_workspace_bytes(n, N, D):
        raise ValueError('nnclr_fwd: the workspace is smaller than nnclr_workspace(%d, %d, %d)' % (n, N, D))
    out = step_scalars(4, nn_local.device)
    row_stats = torch.empty(2 * n, 4, device=nn_local.device, dtype=torch.float32)
    _launch('nnclr_fwd', 4.0 * n * N * D, 4.0 * (4 * n + 2 * N) * D,
            lambda: lib().nnclr_fwd(_p(nn_local), _p(z_local), _p(z_all), n, N, D, int(rank), float(temperature), _p(out),
                                    _p(row_stats), _p(ws), _s()))
    return out, row_stats, ws


def nnclr_bwd(nn_local, z_all, rank, temperature, row_stats, grad_scale, ws):
    """NNCLR backward, the key-side sweep: dz_all [2N, D] (the per-replica partial, to be reduce-scattered).  There is no row-side
    gradient: the neighbour rows are constants."""
    n, N, D = _nnclr_check(nn_local, z_all, temperature)
    if tuple(row_stats.shape) != (2 * n, 4) or row_stats.dtype != torch.float32 or not row_stats.is_contiguous():
        raise ValueError('nnclr_bwd: row_stats must be the contiguous float32 %s block of nnclr_fwd (got %s %s)'
                         % ((2 * n, 4), tuple(row_stats.shape), row_stats.dtype))
    if not 0 <= int(rank) < N // n:
        raise ValueError('nnclr_bwd: rank %d outside the %d replicas' % (rank, N // n))
    if ws is None or ws.numel() * ws.element_size() < lib().nnclr_workspace_bytes(n, N, D):
        raise ValueError('nnclr_bwd: the workspace is smaller than nnclr_workspace(%d, %d, %d)' % (n, N, D))
    dz_all = torch.empty_like(z_all)
    _launch('nnclr_bwd', 8.0 * n * N * D, 4.0 * (2 * n + 4 * N) * D,
            lambda: lib().nnclr_bwd(_p(nn_local), _p(z_all), n, N, D, int(rank), float(temperature), _p(row_stats), float(grad_scale),
                                    _p(dz_all), _p(ws), _s()))
    return dz_all


# ---------------------------------------------------------------- Barlow Twins loss (csrc/barlow.hip)
BT_DIM_STEP, BT_MIN_DIM, BT_MAX_DIM = 64, 64, 8192       # hidden widths the Barlow Twins kernels take: multiples of 64 in [64, 8192]
BT_EPS = 1e-5


def bt_dim_ok(D):
    return BT_MIN_DIM <= D <= BT_MAX_DIM and D % BT_DIM_STEP == 0


def _bt_check_dim(D):
    if not bt_dim_ok(D):
        raise ValueError('the Barlow Twins loss supports hidden widths that are multiples of %d in [%d, %d] (got %d)'
                         % (BT_DIM_STEP, BT_MIN_DIM, BT_MAX_DIM, D))


def _bt_check(zhat_all, n, rank):
    if zhat_all.dtype != torch.float32 or zhat_all.dim() != 2:
        raise ValueError('barlow: need a float32 [2N, D] block (got %s %s)' % (tuple(zhat_all.shape), zhat_all.dtype))
    D = zhat_all.shape[1]
    _bt_check_dim(D)
    N = zhat_all.shape[0] // 2
    n, rank = int(n), int(rank)
    if n < 1 or N < n or N % n != 0 or zhat_all.shape[0] != 2 * N:
        raise ValueError('barlow: need zhat_all [2N, D] with N = R*n and n >= 1 (got %d rows for n = %d)' % (zhat_all.shape[0], n))
    if not 0 <= rank < N // n:
        raise ValueError('barlow: rank %d is not one of the R = %d replicas' % (rank, N // n))
    return n, N, D, rank


def bt_workspace(n, N, D, device):
    _bt_check_dim(D)
    nbytes = lib().bt_workspace_bytes(n, N, D)
    if nbytes == 0:
        raise ValueError('barlow: need N = R*n with n >= 1 (got n = %d, N = %d)' % (n, N))
    return torch.empty((nbytes + 7) // 8, device=device, dtype=torch.float64)


def bt_standardize(h_all, eps=BT_EPS):
    """h_all [2N, D] = [view-1 rows; view-2 rows] of the global batch -> (zhat_all [2N, D], rstd [2, D]): every column of each view
    standardised over its N rows (biased variance, eps inside the root)."""
    if h_all.dtype != torch.float32 or h_all.dim() != 2 or h_all.shape[0] < 2 or h_all.shape[0] % 2:
        raise ValueError('bt_standardize: need a float32 [2N, D] block with N >= 1 (got %s %s)' % (tuple(h_all.shape), h_all.dtype))
    N, D = h_all.shape[0] // 2, h_all.shape[1]
    _bt_check_dim(D)
    zhat = torch.empty_like(h_all)
    rstd = torch.empty(2, D, device=h_all.device, dtype=torch.float32)
    _launch('bt_standardize', 10.0 * N * D, 16.0 * N * D,
            lambda: lib().bt_standardize(_p(h_all), N, D, float(eps), _p(zhat), _p(rstd), _s()), impl_bytes=32.0 * N * D)
    return zhat, rstd


def bt_fwd(zhat_all, n, rank, lambda_weight, loss_scaling=1.0, ws=None):
    """Barlow Twins forward on the standardised global block.  Returns out = [loss, on_diag, off_diag] (device; the per-replica values
    of include/simclr_hip.h) and the workspace, which keeps the Gram blocks and c for bt_bwd."""
    n, N, D, rank = _bt_check(zhat_all, n, rank)
    if ws is None:
        ws = bt_workspace(n, N, D, zhat_all.device)
    out = step_scalars(4, zhat_all.device)
    _launch('bt_fwd', 4.0 * n * N * D, 4.0 * (2 * N * D + 2 * n * N),
            lambda: lib().bt_fwd(_p(zhat_all), n, N, D, rank, float(lambda_weight), float(loss_scaling), _p(out), _p(ws), _s()))
    return out, ws


def bt_gram_blocks(ws, n, N, D):
    """The [2, n, N] fp32 view of the Gram blocks bt_fwd left in `ws`: block v, row a, column b = zhat_v[rank*n + a] . zhat_v[b]."""
    off, rows, pitch = lib().bt_gram_offset_bytes(n, N, D), lib().bt_gram_rows(n, N, D), lib().bt_gram_pitch(n, N, D)
    assert rows > 0 and off % 8 == 0, 'bt_gram_blocks: bad shape n=%d N=%d D=%d' % (n, N, D)
    return ws[off // 8:].view(torch.float32)[:2 * rows * pitch].view(2, rows, pitch)[:, :n, :N]


def bt_bwd(zhat_all, n, rank, lambda_weight, loss_scaling, grad_scale, ws):
    """Returns g_local [2n, D] = grad_scale * R * dL/dzhat of the local rows and colsums [2, 2, D] float64 (the column sums of g and
    g o zhat over the local rows: sum them over the replicas before bt_apply)."""
    n, N, D, rank = _bt_check(zhat_all, n, rank)
    g = torch.empty(2 * n, D, device=zhat_all.device, dtype=torch.float32)
    colsums = torch.empty(2, 2, D, device=zhat_all.device, dtype=torch.float64)
    _launch('bt_bwd', 4.0 * n * N * D, 4.0 * (2 * N * D + 2 * n * N + 2 * n * D),
            lambda: lib().bt_bwd(_p(zhat_all), n, N, D, rank, float(lambda_weight), float(loss_scaling), float(grad_scale), _p(ws), _p(g),
                                 _p(colsums), _s()))
    return g, colsums


def bt_apply(g_local, zhat_all, rstd, colsums, rank):
    """The standardisation backward of the local rows: (g - colsums[v, 0] / N - zhat o colsums[v, 1] / N) * rstd[v]."""
    n = g_local.shape[0] // 2
    n, N, D, rank = _bt_check(zhat_all, n, rank)
    if tuple(g_local.shape) != (2 * n, D) or tuple(rstd.shape) != (2, D) or tuple(colsums.shape) != (2, 2, D) or colsums.dtype != torch.float64:
        raise ValueError('bt_apply: need g_local [2n, D], rstd [2, D] and float64 colsums [2, 2, D] (got %s, %s, %s %s)'
                         % (tuple(g_local.shape), tuple(rstd.shape), tuple(colsums.shape), colsums.dtype))
    dh = torch.empty_like(g_local)
    _launch('bt_apply', 10.0 * n * D, 4.0 * 6 * n * D,
            lambda: lib().bt_apply(_p(g_local), _p(zhat_all), _p(rstd), _p(colsums), n, N, D, rank, _p(dh), _s()))
    return dh


# ---------------------------------------------------------------- VICReg loss (csrc/vicreg.hip)
VICREG_DIM_STEP, VICREG_MIN_DIM, VICREG_MAX_DIM = 64, 64, 8192   # hidden widths the VICReg kernels take: multiples of 64 in [64, 8192]
VICREG_EPS, VICREG_GAMMA = 1e-4, 1.0


def vicreg_dim_ok(D):
    return VICREG_MIN_DIM <= D <= VICREG_MAX_DIM and D % VICREG_DIM_STEP == 0


def _vicreg_check_dim(D):
    if not vicreg_dim_ok(D):
        raise ValueError('the VICReg loss supports hidden widths that are multiples of %d in [%d, %d] (got %d)'
                         % (VICREG_DIM_STEP, VICREG_MIN_DIM, VICREG_MAX_DIM, D))


def vicreg_coeff_ok(c):
    """A coefficient of the VICReg loss: finite and >= 0 (NaN fails the comparison)."""
    return 0.0 <= float(c) < float('inf')


def _vicreg_check(h_all, xc_all, stats, n, rank, coeffs):
    if h_all.dtype != torch.float32 or h_all.dim() != 2:
        raise ValueError('vicreg: need a float32 [2N, D] block (got %s %s)' % (tuple(h_all.shape), h_all.dtype))
    D = h_all.shape[1]
    _vicreg_check_dim(D)
    N = h_all.shape[0] // 2
    n, rank = int(n), int(rank)
    if n < 1 or N < 2 or N < n or N % n != 0 or h_all.shape[0] != 2 * N:
        raise ValueError('vicreg: need h_all [2N, D] with N = R*n, n >= 1 and N >= 2 (got %d rows for n = %d)' % (h_all.shape[0], n))
    if not 0 <= rank < N // n:
        raise ValueError('vicreg: rank %d is not one of the R = %d replicas' % (rank, N // n))
    if xc_all.dtype != torch.float32 or xc_all.shape != h_all.shape or stats.dtype != torch.float64 or tuple(stats.shape) != (2, 2, D):
        raise ValueError('vicreg: need xc_all like h_all and float64 stats [2, 2, D] (got %s %s, %s %s)'
                         % (tuple(xc_all.shape), xc_all.dtype, tuple(stats.shape), stats.dtype))
    if not all(vicreg_coeff_ok(c) for c in coeffs):
        raise ValueError('vicreg: sim_coeff, std_coeff and cov_coeff must be finite and >= 0 (got %r)' % (tuple(coeffs),))
    return n, N, D, rank


def vicreg_workspace(n, N, D, device):
    _vicreg_check_dim(D)
    nbytes = lib().vicreg_workspace_bytes(n, N, D)
    if nbytes == 0:
        raise ValueError('vicreg: need N = R*n with n >= 1 and N >= 2 (got n = %d, N = %d)' % (n, N))
    return torch.empty((nbytes + 7) // 8, device=device, dtype=torch.float64)


def vicreg_k_splits(n, N, D):
    """S, the number of k parts of vicreg_fwd's Gram launch at this shape (0 for a refused shape)."""
    return int(lib().vicreg_k_splits(int(n), int(N), int(D)))


def vicreg_center(h_all, eps=VICREG_EPS):
    """h_all [2N, D] = [view-1 rows; view-2 rows] of the global batch -> (xc_all [2N, D], stats [2, 2, D] float64 = {var, std} per view):
    every column of each view centred over its N rows; var is the unbiased variance of the stored xc, std = sqrt(var + eps)."""
    if h_all.dtype != torch.float32 or h_all.dim() != 2 or h_all.shape[0] < 4 or h_all.shape[0] % 2:
        raise ValueError('vicreg_center: need a float32 [2N, D] block with N >= 2 (got %s %s)' % (tuple(h_all.shape), h_all.dtype))
    N, D = h_all.shape[0] // 2, h_all.shape[1]
    _vicreg_check_dim(D)
    if not float(eps) >= 0.0:
        raise ValueError('vicreg_center: eps must be >= 0 (got %r)' % (eps,))
    xc = torch.empty_like(h_all)
    stats = torch.empty(2, 2, D, device=h_all.device, dtype=torch.float64)
    _launch('vicreg_center', 8.0 * N * D, 16.0 * N * D,
            lambda: lib().vicreg_center(_p(h_all), N, D, float(eps), _p(xc), _p(stats), _s()), impl_bytes=24.0 * N * D)
    return xc, stats


def vicreg_fwd(h_all, xc_all, stats, n, rank, sim_coeff=25.0, std_coeff=25.0, cov_coeff=1.0, gamma=VICREG_GAMMA, ws=None):
    """VICReg forward on the centred global block.  Returns out = [loss, inv, var, cov] (device; the per-replica values of
    include/simclr_hip.h) and the workspace, which keeps the Gram blocks for vicreg_bwd."""
    n, N, D, rank = _vicreg_check(h_all, xc_all, stats, n, rank, (sim_coeff, std_coeff, cov_coeff))
    if ws is None:
        ws = vicreg_workspace(n, N, D, h_all.device)
    out = step_scalars(4, h_all.device)
    _launch('vicreg_fwd', 4.0 * n * N * D, 4.0 * (2 * N * D + 2 * n * N + 2 * n * D),
            lambda: lib().vicreg_fwd(_p(h_all), _p(xc_all), _p(stats), n, N, D, rank, float(sim_coeff), float(std_coeff), float(cov_coeff),
                                     float(gamma), _p(out), _p(ws), _s()))
    return out, ws


def vicreg_gram_blocks(ws, n, N, D):
    """The [2, n, N] fp32 view of the Gram blocks vicreg_fwd left in `ws`: block v, row a, column b = xc_v[rank*n + a] . xc_v[b]."""
    off, rows, pitch = lib().vicreg_gram_offset_bytes(n, N, D), lib().vicreg_gram_rows(n, N, D), lib().vicreg_gram_pitch(n, N, D)
    assert rows > 0 and off % 8 == 0, 'vicreg_gram_blocks: bad shape n=%d N=%d D=%d' % (n, N, D)
    return ws[off // 8:].view(torch.float32)[:2 * rows * pitch].view(2, rows, pitch)[:, :n, :N]


def vicreg_bwd(h_all, xc_all, stats, n, rank, sim_coeff, std_coeff, cov_coeff, gamma, grad_scale, ws):
    """Returns dh_local [2n, D] = grad_scale * R * dL/dh of the local rows of both views: one launch, nothing to reduce."""
    n, N, D, rank = _vicreg_check(h_all, xc_all, stats, n, rank, (sim_coeff, std_coeff, cov_coeff))
    dh = torch.empty(2 * n, D, device=h_all.device, dtype=torch.float32)
    _launch('vicreg_bwd', 4.0 * n * N * D, 4.0 * (2 * N * D + 2 * n * N + 6 * n * D),
            lambda: lib().vicreg_bwd(_p(h_all), _p(xc_all), _p(stats), n, N, D, rank, float(sim_coeff), float(std_coeff), float(cov_coeff),
                                     float(gamma), float(grad_scale), _p(ws), _p(dh), _s()))
    return dh


# ---------------------------------------------------------------- representation diagnostics (csrc/repr.hip)
REPR_DIM_STEP, REPR_MIN_DIM, REPR_MAX_DIM = 64, 64, 8192   # widths the diagnostics take: multiples of 64 in [64, 8192]
REPR_MIN_ROWS, REPR_MAX_ROWS = 2, 65536                    # rows per view (the global batch)
REPR_MAX_T = 16.0


def repr_dim_ok(D):
    return REPR_MIN_DIM <= D <= REPR_MAX_DIM and D % REPR_DIM_STEP == 0


def repr_t_ok(t):
    """The scale t of the uniformity: 0 < t <= 16 (NaN fails the comparison)."""
    return 0.0 < float(t) <= REPR_MAX_T


def _repr_check_shape(N, D):
    if not repr_dim_ok(D):
        raise ValueError('repr_stats supports widths that are multiples of %d in [%d, %d] (got %d)'
                         % (REPR_DIM_STEP, REPR_MIN_DIM, REPR_MAX_DIM, D))
    if not REPR_MIN_ROWS <= N <= REPR_MAX_ROWS:
        raise ValueError('repr_stats needs %d <= N <= %d rows per view (got %d)' % (REPR_MIN_ROWS, REPR_MAX_ROWS, N))


def repr_workspace(N, D, device):
    N, D = int(N), int(D)
    _repr_check_shape(N, D)
    nbytes = lib().repr_workspace_bytes(N, D)
    assert nbytes > 0
    return torch.empty((nbytes + 7) // 8, device=device, dtype=torch.float64)


def repr_tile_edge(N, D):
    """Edge (64 or 128) of the Gram tile a workgroup of repr_stats' pairs launch owns at this shape (0 for a refused shape)."""
    return int(lib().repr_tile_edge(int(N), int(D)))


def repr_stats(z_all, t=2.0, ws=None):
    """z_all [2N, D] fp32 = [view-a rows; view-b rows] of the l2-normalised global batch -> fp32 [4] = {align, uniform, std, rank}
    (include/simclr_hip.h).  Reads z_all only; `ws` (repr_workspace) is scratch, a fresh one by default."""
    if not torch.is_tensor(z_all) or z_all.dtype != torch.float32 or z_all.dim() != 2 or z_all.shape[0] % 2:
        raise ValueError('repr_stats: need a float32 [2N, D] block (got %s %s)'
                         % (tuple(getattr(z_all, 'shape', ())), getattr(z_all, 'dtype', type(z_all))))
    N, D = z_all.shape[0] // 2, z_all.shape[1]
    _repr_check_shape(N, D)
    z_all = z_all.contiguous()
    if not repr_t_ok(t):
        raise ValueError('repr_stats: t must lie in (0, %g] (got %r)' % (REPR_MAX_T, t))
    if ws is None:
        ws = repr_workspace(N, D, z_all.device)
    elif ws.numel() * ws.element_size() < lib().repr_workspace_bytes(N, D) or ws.data_ptr() % 16:
        raise ValueError('repr_stats: the workspace holds %d bytes at %#x; N = %d, D = %d needs %d bytes, 16-byte aligned'
                         % (ws.numel() * ws.element_size(), ws.data_ptr(), N, D, lib().repr_workspace_bytes(N, D)))
    out = torch.empty(4, device=z_all.device, dtype=torch.float32)
    _launch('repr_stats', 4.0 * N * N * D, 4.0 * 2 * N * D,
            lambda: lib().repr_stats(_p(z_all), N, D, float(t), _p(ws), _p(out), _s()), impl_bytes=4.0 * 8 * N * D)
    return out


# ---------------------------------------------------------------- cached-feature linear probe (csrc/logreg.hip)
LOGREG_DIM_STEP, LOGREG_MIN_DIM, LOGREG_MAX_DIM = 64, 64, 8192   # feature widths: multiples of 64 in [64, 8192]
LOGREG_MIN_CLASSES, LOGREG_MAX_CLASSES = 2, 4096
LOGREG_MAX_ROWS = 65536                                          # rows per call (a slab of the bank)


def logreg_dim_ok(D):
    return LOGREG_MIN_DIM <= D <= LOGREG_MAX_DIM and D % LOGREG_DIM_STEP == 0


def _logreg_check_shape(n, D, C):
    if not logreg_dim_ok(D):
        raise ValueError('logreg supports feature widths that are multiples of %d in [%d, %d] (got %d)'
                         % (LOGREG_DIM_STEP, LOGREG_MIN_DIM, LOGREG_MAX_DIM, D))
    if not LOGREG_MIN_CLASSES <= C <= LOGREG_MAX_CLASSES:
        raise ValueError('logreg needs %d <= C <= %d classes (got %d)' % (LOGREG_MIN_CLASSES, LOGREG_MAX_CLASSES, C))
    if not 1 <= n <= LOGREG_MAX_ROWS:
        raise ValueError('logreg takes 1 <= n <= %d rows per call (got %d)' % (LOGREG_MAX_ROWS, n))


def logreg_store_pitch(C):
    """Floats per row of the [n, pitch] logit / G buffer: C rounded up to 4."""
    return (int(C) + 3) // 4 * 4


def logreg_workspace(n, D, C, device):
    n, D, C = int(n), int(D), int(C)
    _logreg_check_shape(n, D, C)
    nbytes = lib().logreg_workspace_bytes(n, D, C)
    assert nbytes > 0
    return torch.empty((nbytes + 7) // 8, device=device, dtype=torch.float64)


def logreg_row_splits(n, D, C):
    """Row parts of logreg_bwd's product at this shape (0 for a refused shape)."""
    return int(lib().logreg_row_splits(int(n), int(D), int(C)))


def logreg_tile_edge(n, D, C, backward=False):
    """Edge (64 or 128) of the tile a workgroup of the forward (or backward) product owns at this shape (0 for a refused shape)."""
    return int((lib().logreg_bwd_tile_edge if backward else lib().logreg_tile_edge)(int(n), int(D), int(C)))


def _logreg_f32(name, t, shape):
    if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != tuple(shape):
        raise ValueError('logreg: %s must be a float32 tensor of shape %s (got %s %s)'
                         % (name, tuple(shape), tuple(getattr(t, 'shape', ())), getattr(t, 'dtype', type(t))))
    if not t.is_contiguous() or t.data_ptr() % 16:
        raise ValueError('logreg: %s must be contiguous and 16-byte aligned' % name)


def _logreg_ws(ws, n, D, C, device):
    if ws is None:
        return logreg_workspace(n, D, C, device)
    need = lib().logreg_workspace_bytes(n, D, C)
    if not torch.is_tensor(ws) or ws.numel() * ws.element_size() < need or ws.data_ptr() % 16:
        raise ValueError('logreg: the workspace must hold %d bytes, 16-byte aligned, for n = %d, D = %d, C = %d' % (need, n, D, C))
    return ws


def logreg_fwd(x, w, b, labels, weights, inv_S, mode=0, store=None, lse=None, ws=None, check_labels=True):
    """x [n, D], w [C, D], b [C] fp32, labels [n] int32 in [0, C), weights [n] fp32.  Returns (out, lse, store): out = fp64 [3] =
    {sum_n w_n (lse_n - s_n,y_n), weighted top-1 hits, sum_n w_n}, lse fp64 [n], store [n, pitch] fp32 = None (mode 0), G (mode 1) or the
    raw logits (mode 2); columns >= C of store are never written (include/simclr_hip.h).  check_labels=False skips the range check of
    the labels (one device synchronisation) for a caller that has made it already."""
    if not torch.is_tensor(x) or x.dim() != 2 or not torch.is_tensor(w) or w.dim() != 2:
        raise ValueError('logreg_fwd: need x [n, D] and w [C, D]')
    (n, D), C = x.shape, w.shape[0]
    _logreg_check_shape(n, D, C)
    _logreg_f32('x', x, (n, D)); _logreg_f32('w', w, (C, D)); _logreg_f32('b', b, (C,)); _logreg_f32('weights', weights, (n,))
    if not torch.is_tensor(labels) or labels.dtype != torch.int32 or tuple(labels.shape) != (n,) or not labels.is_contiguous() \
            or labels.data_ptr() % 16:
        raise ValueError('logreg_fwd: labels must be a contiguous, 16-byte aligned int32 tensor of shape (%d,)' % n)
    if mode not in (0, 1, 2):
        raise ValueError('logreg_fwd: mode must be 0 (value), 1 (value and G) or 2 (logits) (got %r)' % (mode,))
    inv_S = float(inv_S)
    if not 0.0 < inv_S < float('inf'):
        raise ValueError('logreg_fwd: inv_S must be a finite number > 0 (got %r)' % (inv_S,))
    if check_labels and (int(labels.min()) < 0 or int(labels.max()) >= C):
        raise ValueError('logreg_fwd: labels must lie in [0, %d) (got %d .. %d)' % (C, int(labels.min()), int(labels.max())))
    pitch = logreg_store_pitch(C)
    if mode == 0:
        store = None
    elif store is None:
        store = torch.empty(n, pitch, device=x.device, dtype=torch.float32)
    else:
        if not torch.is_tensor(store) or store.dtype != torch.float32 or store.numel() < n * pitch or not store.is_contiguous() \
                or store.data_ptr() % 16:
            raise ValueError('logreg_fwd: store must be a contiguous, 16-byte aligned float32 tensor of at least %d x %d elements' % (n, pitch))
        store = store.view(-1)[:n * pitch].view(n, pitch)
    if lse is None:
        lse = torch.empty(n, device=x.device, dtype=torch.float64)
    elif not torch.is_tensor(lse) or lse.dtype != torch.float64 or tuple(lse.shape) != (n,) or not lse.is_contiguous() or lse.data_ptr() % 16:
        raise ValueError('logreg_fwd: lse must be a contiguous, 16-byte aligned float64 tensor of shape (%d,)' % n)
    ws = _logreg_ws(ws, n, D, C, x.device)
    out = torch.empty(3, device=x.device, dtype=torch.float64)
    _launch('logreg_fwd', 2.0 * n * D * C, 4.0 * (n * D + C * D + (n * C if mode else 0)),
            lambda: lib().logreg_fwd(_p(x), _p(w), _p(b), _p(labels), _p(weights), n, D, C, inv_S, int(mode), _p(store), _p(lse), _p(out),
                                     _p(ws), _s()))
    return out, lse, store


def logreg_bwd(g, x, C, dw=None, db=None, accumulate=False, ws=None):
    """g [n, pitch] fp32 = the G of logreg_fwd mode 1, x [n, D] -> dw [C, D] (+)= G^T X, db [C] (+)= colsum(G) (accumulate=True adds to
    the dw / db given)."""
    if not torch.is_tensor(x) or x.dim() != 2:
        raise ValueError('logreg_bwd: need x [n, D]')
    (n, D), C = x.shape, int(C)
    _logreg_check_shape(n, D, C)
    _logreg_f32('x', x, (n, D)); _logreg_f32('g', g, (n, logreg_store_pitch(C)))
    if accumulate and (dw is None or db is None):
        raise ValueError('logreg_bwd: accumulate=True needs dw and db')
    dw = torch.empty(C, D, device=x.device, dtype=torch.float32) if dw is None else dw
    db = torch.empty(C, device=x.device, dtype=torch.float32) if db is None else db
    _logreg_f32('dw', dw, (C, D)); _logreg_f32('db', db, (C,))
    ws = _logreg_ws(ws, n, D, C, x.device)
    _launch('logreg_bwd', 2.0 * n * D * C, 4.0 * (n * D + C * D + n * C),
            lambda: lib().logreg_bwd(_p(g), _p(x), n, D, C, _p(dw), _p(db), 1 if accumulate else 0, _p(ws), _s()))
    return dw, db


# ---------------------------------------------------------------- spherical k-means (csrc/kmeans.hip)
KMEANS_DIM_STEP, KMEANS_MIN_DIM, KMEANS_MAX_DIM = 64, 64, 8192   # feature widths: multiples of 64 in [64, 8192]
KMEANS_MIN_K, KMEANS_MAX_K = 2, 16384
KMEANS_MAX_ROWS = 65536                                          # rows per call (a slab of the bank)


def kmeans_dim_ok(D):
    return KMEANS_MIN_DIM <= D <= KMEANS_MAX_DIM and D % KMEANS_DIM_STEP == 0


def _kmeans_check_shape(n, D, K):
    if not kmeans_dim_ok(D):
        raise ValueError('kmeans supports feature widths that are multiples of %d in [%d, %d] (got %d)'
                         % (KMEANS_DIM_STEP, KMEANS_MIN_DIM, KMEANS_MAX_DIM, D))
    if not KMEANS_MIN_K <= K <= KMEANS_MAX_K:
        raise ValueError('kmeans needs %d <= K <= %d centroids (got %d)' % (KMEANS_MIN_K, KMEANS_MAX_K, K))
    if not 1 <= n <= KMEANS_MAX_ROWS:
        raise ValueError('kmeans takes 1 <= n <= %d rows per call (got %d)' % (KMEANS_MAX_ROWS, n))


def kmeans_workspace(n, D, K, device):
    n, D, K = int(n), int(D), int(K)
    _kmeans_check_shape(n, D, K)
    nbytes = lib().kmeans_workspace_bytes(n, D, K)
    assert nbytes > 0
    return torch.empty((nbytes + 7) // 8, device=device, dtype=torch.float64)


def kmeans_tile_edge(n, D, K):
    """Edge (64 or 128) of the score tile a workgroup of the assignment owns at this shape (0 for a refused shape)."""
    return int(lib().kmeans_tile_edge(int(n), int(D), int(K)))


def _kmeans_t(name, t, shape, dtype):
    if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != tuple(shape):
        raise ValueError('kmeans: %s must be a %s tensor of shape %s (got %s %s)'
                         % (name, str(dtype).replace('torch.', ''), tuple(shape), tuple(getattr(t, 'shape', ())), getattr(t, 'dtype', type(t))))
    if not t.is_contiguous() or t.data_ptr() % 16:
        raise ValueError('kmeans: %s must be contiguous and 16-byte aligned' % name)


def _kmeans_ws(ws, n, D, K, device):
    if ws is None:
        return kmeans_workspace(n, D, K, device)
    need = lib().kmeans_workspace_bytes(n, D, K)
    if not torch.is_tensor(ws) or ws.numel() * ws.element_size() < need or ws.data_ptr() % 16:
        raise ValueError('kmeans: the workspace must hold %d bytes, 16-byte aligned, for n = %d, D = %d, K = %d' % (need, n, D, K))
    return ws


def kmeans_assign(x, c, weights, assign=None, best=None, ws=None):
    """x [n, D] unit rows, c [K, D] unit centroids, weights [n], all fp32.  Returns (assign, best, out): assign int32 [n] = argmax_k
    x_n . c_k (ties to the lowest k), best fp32 [n] = that score, out = fp64 [3] = {sum w (1 - best), sum w, rows of weight > 0 whose
    assignment differs from the value `assign` held on entry}.  Without `assign` the previous assignment is -1 everywhere."""
    if not torch.is_tensor(x) or x.dim() != 2 or not torch.is_tensor(c) or c.dim() != 2:
        raise ValueError('kmeans_assign: need x [n, D] and c [K, D]')
    (n, D), K = x.shape, c.shape[0]
    _kmeans_check_shape(n, D, K)
    _kmeans_t('x', x, (n, D), torch.float32); _kmeans_t('c', c, (K, D), torch.float32); _kmeans_t('weights', weights, (n,), torch.float32)
    if assign is None:
        assign = torch.full((n,), -1, device=x.device, dtype=torch.int32)
    _kmeans_t('assign', assign, (n,), torch.int32)
    best = torch.empty(n, device=x.device, dtype=torch.float32) if best is None else best
    _kmeans_t('best', best, (n,), torch.float32)
    ws = _kmeans_ws(ws, n, D, K, x.device)
    out = torch.empty(3, device=x.device, dtype=torch.float64)
    _launch('kmeans_assign', 2.0 * n * D * K, 4.0 * (n * D + K * D),
            lambda: lib().kmeans_assign(_p(x), _p(c), _p(weights), n, D, K, _p(assign), _p(best), _p(out), _p(ws), _s()))
    return assign, best, out


def kmeans_update(x, weights, assign, K, sums=None, wsum=None, accumulate=False):
    """sums [K, D] fp64 (+)= the weighted rows of x [n, D] summed per cluster of assign int32 [n] (values in [0, K)), wsum [K] fp64 (+)=
    the weights.  The rows are sorted by assignment here (torch.sort, stable) and the kernel adds every segment in that order."""
    if not torch.is_tensor(x) or x.dim() != 2:
        raise ValueError('kmeans_update: need x [n, D]')
    (n, D), K = x.shape, int(K)
    _kmeans_check_shape(n, D, K)
    _kmeans_t('x', x, (n, D), torch.float32); _kmeans_t('weights', weights, (n,), torch.float32)
    _kmeans_t('assign', assign, (n,), torch.int32)
    if accumulate and (sums is None or wsum is None):
        raise ValueError('kmeans_update: accumulate=True needs sums and wsum')
    sums = torch.empty(K, D, device=x.device, dtype=torch.float64) if sums is None else sums
    wsum = torch.empty(K, device=x.device, dtype=torch.float64) if wsum is None else wsum
    _kmeans_t('sums', sums, (K, D), torch.float64); _kmeans_t('wsum', wsum, (K,), torch.float64)
    key, order = torch.sort(assign, stable=True)
    order = order.to(torch.int32)
    # offsets[k] = the first sorted position whose assignment is >= k; a value outside [0, K) lands in no segment
    offsets = torch.searchsorted(key, torch.arange(K + 1, device=x.device, dtype=torch.int32)).to(torch.int32)
    _launch('kmeans_update', 2.0 * n * D, 4.0 * n * D + 8.0 * K * D,
            lambda: lib().kmeans_update(_p(x), _p(weights), _p(order), _p(offsets), n, D, K, _p(sums), _p(wsum), 1 if accumulate else 0, _s()))
    return sums, wsum


def kmeans_finish(sums, wsum, c_prev, c_new=None, ws=None):
    """c_new [K, D] fp32 = the rows of sums [K, D] fp64 normalised in double and rounded; a cluster with wsum <= 0 or |sums_k|^2 <= 1e-24
    keeps c_prev_k.  Returns (c_new, out): out = fp64 [2] = {kept clusters, max_k (1 - c_new_k . c_prev_k)}."""
    if not torch.is_tensor(sums) or sums.dim() != 2:
        raise ValueError('kmeans_finish: need sums [K, D]')
    K, D = sums.shape
    _kmeans_check_shape(1, D, K)
    _kmeans_t('sums', sums, (K, D), torch.float64); _kmeans_t('wsum', wsum, (K,), torch.float64)
    _kmeans_t('c_prev', c_prev, (K, D), torch.float32)
    c_new = torch.empty(K, D, device=sums.device, dtype=torch.float32) if c_new is None else c_new
    _kmeans_t('c_new', c_new, (K, D), torch.float32)
    if c_new.data_ptr() == c_prev.data_ptr():
        raise ValueError('kmeans_finish: c_new may not alias c_prev')
    ws = _kmeans_ws(ws, 1, D, K, sums.device)
    out = torch.empty(2, device=sums.device, dtype=torch.float64)
    _launch('kmeans_finish', 3.0 * K * D, 16.0 * K * D,
            lambda: lib().kmeans_finish(_p(sums), _p(wsum), _p(c_prev), K, D, _p(c_new), _p(out), _p(ws), _s()))
    return c_new, out


# ---------------------------------------------------------------- eigen-spectrum evaluation (csrc/spectrum.hip)
SPECTRUM_DIM_STEP, SPECTRUM_MIN_DIM, SPECTRUM_MAX_DIM = 64, 64, 8192   # feature widths: multiples of 64 in [64, 8192]
SPECTRUM_MAX_ROWS = 65536                                              # rows per call (a slab of the bank)


def spectrum_dim_ok(D):
    return SPECTRUM_MIN_DIM <= D <= SPECTRUM_MAX_DIM and D % SPECTRUM_DIM_STEP == 0


def _spectrum_check_shape(n, D):
    if not spectrum_dim_ok(D):
        raise ValueError('spectrum supports feature widths that are multiples of %d in [%d, %d] (got %d)'
                         % (SPECTRUM_DIM_STEP, SPECTRUM_MIN_DIM, SPECTRUM_MAX_DIM, D))
    if not 1 <= n <= SPECTRUM_MAX_ROWS:
        raise ValueError('spectrum takes 1 <= n <= %d rows per call (got %d)' % (SPECTRUM_MAX_ROWS, n))


def spectrum_workspace(n, D, device, colsum_only=False):
    """A workspace for both entry points at this shape (the centred slab and the fp32 row parts of spectrum_cov); colsum_only=True:
    the few kilobytes spectrum_colsum alone needs."""
    n, D = int(n), int(D)
    _spectrum_check_shape(n, D)
    nbytes = (lib().spectrum_colsum_workspace_bytes if colsum_only else lib().spectrum_workspace_bytes)(n, D)
    assert nbytes > 0
    return torch.empty((nbytes + 7) // 8, device=device, dtype=torch.float64)


def spectrum_tile_edge(n, D):
    """Edge (64 or 128) of the covariance tile a workgroup owns at this shape (0 for a refused shape)."""
    return int(lib().spectrum_tile_edge(int(n), int(D)))


def spectrum_row_parts(n, D):
    """Row parts of spectrum_cov's product at this shape (0 for a refused shape)."""
    return int(lib().spectrum_row_parts(int(n), int(D)))


def _spectrum_t(name, t, shape, dtype):
    if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != tuple(shape):
        raise ValueError('spectrum: %s must be a %s tensor of shape %s (got %s %s)'
                         % (name, str(dtype).replace('torch.', ''), tuple(shape), tuple(getattr(t, 'shape', ())), getattr(t, 'dtype', type(t))))
    if not t.is_contiguous() or t.data_ptr() % 16:
        raise ValueError('spectrum: %s must be contiguous and 16-byte aligned' % name)


def _spectrum_ws(ws, n, D, device, colsum_only=False):
    if ws is None:
        return spectrum_workspace(n, D, device, colsum_only)
    need = (lib().spectrum_colsum_workspace_bytes if colsum_only else lib().spectrum_workspace_bytes)(n, D)
    if not torch.is_tensor(ws) or ws.numel() * ws.element_size() < need or ws.data_ptr() % 16:
        raise ValueError('spectrum: the workspace must hold %d bytes, 16-byte aligned, for n = %d, D = %d' % (need, n, D))
    return ws


def spectrum_colsum(x, weights, sums=None, accumulate=False, ws=None):
    """x [n, D] fp32, weights [n] fp32 -> sums fp64 [D + 1] (+)= {column sums of the rows of weight > 0, their number}.  The rows are
    selected, not multiplied: a row of weight <= 0 (or NaN) is not read.  Its workspace is the head of spectrum_cov's: any workspace of
    spectrum_workspace(n, D) serves, and without one only simclr_spectrum_colsum_workspace_bytes are allocated."""
    if not torch.is_tensor(x) or x.dim() != 2:
        raise ValueError('spectrum_colsum: need x [n, D]')
    n, D = x.shape
    _spectrum_check_shape(n, D)
    _spectrum_t('x', x, (n, D), torch.float32); _spectrum_t('weights', weights, (n,), torch.float32)
    if accumulate and sums is None:
        raise ValueError('spectrum_colsum: accumulate=True needs sums')
    sums = torch.empty(D + 1, device=x.device, dtype=torch.float64) if sums is None else sums
    _spectrum_t('sums', sums, (D + 1,), torch.float64)
    ws = _spectrum_ws(ws, n, D, x.device, colsum_only=True)
    _launch('spectrum_colsum', 1.0 * n * D, 4.0 * n * D,
            lambda: lib().spectrum_colsum(_p(x), _p(weights), n, D, _p(sums), 1 if accumulate else 0, _p(ws), _s()))
    return sums


def spectrum_cov(x, weights, mu32, cov=None, accumulate=False, ws=None):
    """cov fp64 [D, D] (+)= sum over the rows of weight > 0 of (x_n - mu32)(x_n - mu32)^T for x [n, D] fp32 and mu32 [D] fp32.  The
    upper tile triangle is computed and mirrored: cov[a, b] and cov[b, a] are the same bits."""
    if not torch.is_tensor(x) or x.dim() != 2:
        raise ValueError('spectrum_cov: need x [n, D]')
    n, D = x.shape
    _spectrum_check_shape(n, D)
    _spectrum_t('x', x, (n, D), torch.float32); _spectrum_t('weights', weights, (n,), torch.float32)
    _spectrum_t('mu32', mu32, (D,), torch.float32)
    if accumulate and cov is None:
        raise ValueError('spectrum_cov: accumulate=True needs cov')
    cov = torch.empty(D, D, device=x.device, dtype=torch.float64) if cov is None else cov
    _spectrum_t('cov', cov, (D, D), torch.float64)
    ws = _spectrum_ws(ws, n, D, x.device)
    _launch('spectrum_cov', 1.0 * n * D * (D + 1), 8.0 * n * D + 8.0 * D * D,
            lambda: lib().spectrum_cov(_p(x), _p(weights), _p(mu32), n, D, _p(cov), 1 if accumulate else 0, _p(ws), _s()))
    return cov


# ---------------------------------------------------------------- BYOL (csrc/byol.hip)
BYOL_DIM_STEP, BYOL_MIN_DIM, BYOL_MAX_DIM = 64, 64, 8192   # loss widths (and predictor hidden widths) the BYOL path takes


def byol_dim_ok(D):
    return BYOL_MIN_DIM <= D <= BYOL_MAX_DIM and D % BYOL_DIM_STEP == 0


def _byol_check(q, t):
    if q.dtype != torch.float32 or t.dtype != torch.float32 or q.dim() != 2 or tuple(q.shape) != tuple(t.shape):
        raise ValueError('byol: need float32 q and t of one shape [2b, D] (got %s %s, %s %s)'
                         % (tuple(q.shape), q.dtype, tuple(t.shape), t.dtype))
    rows, D = q.shape
    if rows < 2 or rows % 2:
        raise ValueError('byol: q and t hold both views, [2b, D] with b >= 1 (got %d rows)' % rows)
    if not byol_dim_ok(D):
        raise ValueError('the BYOL loss supports widths that are multiples of %d in [%d, %d] (got %d)'
                         % (BYOL_DIM_STEP, BYOL_MIN_DIM, BYOL_MAX_DIM, D))
    return rows // 2, D


def byol_fwd(q, t):
    """q [2b, D] (online predictor output), t [2b, D] (target projection) -> (out = [loss, cosine] device fp32, row_stats [2b, 4] float64
    for byol_bwd).  Row r of q pairs with row (r + b) mod 2b of t (include/simclr_hip.h)."""
    b, D = _byol_check(q, t)
    out = step_scalars(2, q.device)
    buf = torch.empty(2 * b * 6, device=q.device, dtype=torch.float64)
    row_stats, row_out = buf[:2 * b * 4], buf[2 * b * 4:]
    _launch('byol_fwd', 8.0 * 2 * b * D, 8.0 * 2 * b * D,
            lambda: lib().byol_fwd(_p(q), _p(t), b, D, _p(out), _p(row_stats), _p(row_out), _s()))
    return out, row_stats.view(2 * b, 4)


def byol_bwd(q, t, row_stats, grad_scale):
    """dq [2b, D] = (grad_scale / b) * d(sum_r l_r) / dq, the eps branch of the normalisation included; t gets no gradient."""
    b, D = _byol_check(q, t)
    if row_stats.dtype != torch.float64 or row_stats.numel() != 2 * b * 4:
        raise ValueError('byol_bwd: row_stats is the float64 [2b, 4] block byol_fwd returned (got %s %s)' % (tuple(row_stats.shape), row_stats.dtype))
    dq = torch.empty_like(q)
    _launch('byol_bwd', 10.0 * 2 * b * D, 12.0 * 2 * b * D,
            lambda: lib().byol_bwd(_p(q), _p(t), b, D, _p(row_stats), float(grad_scale), _p(dq), _s()))
    return dq


class EmaTables:
    """Descriptor and chunk tables of simclr_ema_multi_tensor over (target, online) fp32 tensor pairs, in the layout of
    lars_optimizer.LARSOptimizer._build: built once, rebuilt when a pointer changes.
    run(targets, onlines, one_minus_tau): targets[k] <- targets[k] + one_minus_tau * (onlines[k] - targets[k]) in one launch."""

    def __init__(self):
        self._key = None

    def build(self, targets, onlines):
        chunk = lib().lars_chunk_elems()
        T = len(targets)
        table = torch.zeros(3 * T, dtype=torch.int64)
        chunks = []
        for k, (t, o) in enumerate(zip(targets, onlines)):
            if t.dtype != torch.float32 or o.dtype != torch.float32 or t.numel() != o.numel():
                raise ValueError('ema: tensor %d: need two float32 tensors of one size (got %s %s, %s %s)'
                                 % (k, tuple(t.shape), t.dtype, tuple(o.shape), o.dtype))
            assert t.is_cuda and o.is_cuda and t.is_contiguous() and o.is_contiguous(), 'need contiguous device tensors'
            table[0 * T + k] = t.data_ptr()
            table[1 * T + k] = o.data_ptr()
            table[2 * T + k] = t.numel()
            for off in range(0, t.numel(), chunk):
                chunks.append((k, off))
        dev = targets[0].device
        self.table = table.to(dev)
        self.chunks = torch.tensor(chunks, dtype=torch.int64).view(-1).to(dev)
        self.num = (T, len(chunks))
        self.elems = int(sum(t.numel() for t in targets))
        self._key = tuple((t.data_ptr(), o.data_ptr()) for t, o in zip(targets, onlines))

    def run(self, targets, onlines, one_minus_tau):
        key = tuple((t.data_ptr(), o.data_ptr()) for t, o in zip(targets, onlines))
        if key != self._key:
            self.build(targets, onlines)
        T, nchunks = self.num
        _launch('ema_multi_tensor', 3.0 * self.elems, 12.0 * self.elems,
                lambda: lib().ema_multi_tensor(_p(self.table), T, _p(self.chunks), nchunks, float(one_minus_tau), _s()))


# ---------------------------------------------------------------- MoCo v2 (csrc/moco.hip)
MOCO_DIMS = (64, 128, 256)          # loss widths the MoCo kernels are instantiated for
MOCO_MAX_QUEUE = 1048576            # largest --moco_queue_size


def _moco_check_dim(D):
    if D not in MOCO_DIMS:
        raise ValueError('the MoCo loss supports widths %s (got %d)' % ('/'.join(map(str, MOCO_DIMS)), D))


def _moco_check(q, t, queue, temperature):
    if q.dtype != torch.float32 or t.dtype != torch.float32 or q.dim() != 2 or tuple(q.shape) != tuple(t.shape):
        raise ValueError('moco: need float32 q and t of one shape [2b, D] (got %s %s, %s %s)'
                         % (tuple(q.shape), q.dtype, tuple(t.shape), t.dtype))
    rows, D = q.shape
    if rows < 2 or rows % 2:
        raise ValueError('moco: q and t hold both views, [2b, D] with b >= 1 (got %d rows)' % rows)
    _moco_check_dim(D)
    if queue.dtype != torch.float32 or queue.dim() != 2 or queue.shape[0] < 1 or queue.shape[1] != D:
        raise ValueError('moco: the queue is a float32 [K, %d] block with K >= 1 (got %s %s)' % (D, tuple(queue.shape), queue.dtype))
    if not float(temperature) > 0.0:            # (NaN fails the comparison)
        raise ValueError('moco: temperature must be > 0 (got %r)' % (temperature,))
    return rows, queue.shape[0], D


def moco_key_splits(two_n, K):
    """Number of key splits the forward sweep of moco_fwd uses for two_n query rows against a queue of K rows."""
    splits = lib().moco_key_splits(int(two_n), int(K))
    if splits < 1:
        raise ValueError('moco: need an even two_n >= 2 and K >= 1 (got two_n = %d, K = %d)' % (two_n, K))
    return splits


def moco_workspace(two_n, K, D, device):
    _moco_check_dim(D)
    nbytes = lib().moco_workspace_bytes(two_n, K, D)
    if nbytes == 0:
        raise ValueError('moco: need an even two_n >= 2 and K >= 1 (got two_n = %d, K = %d)' % (two_n, K))
    return torch.empty((nbytes + 7) // 8, device=device, dtype=torch.float64)


def _moco_check_ws(ws, two_n, K, D):
    if ws is None or ws.numel() * ws.element_size() < lib().moco_workspace_bytes(two_n, K, D):
        raise ValueError('moco: the workspace is smaller than moco_workspace(%d, %d, %d)' % (two_n, K, D))


def moco_fwd(q, t, queue, temperature, ws=None):
    """q [2b, D] (normalised online projections), t [2b, D] (normalised momentum keys of the same rows, as the target network returned
    them: row r of q pairs with row (r + b) mod 2b of t inside the kernel), queue [K, D] -> (out = [loss, contrast_acc] device fp32,
    row_stats [2b, 2] for moco_bwd, the workspace both calls share)."""
    two_n, K, D = _moco_check(q, t, queue, temperature)
    if ws is None:
        ws = moco_workspace(two_n, K, D, q.device)
    _moco_check_ws(ws, two_n, K, D)
    out = step_scalars(2, q.device)
    row_stats = torch.empty(two_n, 2, device=q.device, dtype=torch.float32)
    _launch('moco_fwd', 2.0 * two_n * K * D, 4.0 * (2 * two_n + K) * D,
            lambda: lib().moco_fwd(_p(q), _p(t), _p(queue), two_n, K, D, float(temperature), _p(out), _p(row_stats), _p(ws), _s()))
    return out, row_stats, ws


def moco_bwd(q, t, queue, temperature, row_stats, grad_scale, ws):
    """dq [2b, D] = grad_scale * dloss / dq from moco_fwd's row_stats and workspace on the same arguments; t and the queue get no
    gradient."""
    two_n, K, D = _moco_check(q, t, queue, temperature)
    if row_stats.dtype != torch.float32 or tuple(row_stats.shape) != (two_n, 2):
        raise ValueError('moco_bwd: row_stats is the float32 [2b, 2] block moco_fwd returned (got %s %s)' % (tuple(row_stats.shape), row_stats.dtype))
    _moco_check_ws(ws, two_n, K, D)
    dq = torch.empty_like(q)
    _launch('moco_bwd', 4.0 * two_n * K * D, 4.0 * (3 * two_n + K) * D,
            lambda: lib().moco_bwd(_p(q), _p(t), _p(queue), two_n, K, D, float(temperature), _p(row_stats), float(grad_scale), _p(dq),
                                   _p(ws), _s()))
    return dq


# ---------------------------------------------------------------- DINO self-distillation (csrc/dino.hip)
DINO_DIMS = (64, 128, 256)          # loss widths the DINO kernels are instantiated for
DINO_MAX_OUT_DIM = 1048576          # largest --dino_out_dim


def _dino_check_dim(D):
    if D not in DINO_DIMS:
        raise ValueError('the DINO loss supports widths %s (got %d)' % ('/'.join(map(str, DINO_DIMS)), D))


def _dino_check_temp(name, value):
    if not 0.0 < float(value) < float('inf'):            # (NaN fails the comparison)
        raise ValueError('dino: %s must be > 0 and finite (got %r)' % (name, value))


def _dino_check(q, k, ws, wt, center, student_temp, teacher_temp):
    if q.dtype != torch.float32 or k.dtype != torch.float32 or q.dim() != 2 or tuple(q.shape) != tuple(k.shape):
        raise ValueError('dino: need float32 q and k of one shape [2b, D] (got %s %s, %s %s)'
                         % (tuple(q.shape), q.dtype, tuple(k.shape), k.dtype))
    rows, D = q.shape
    if rows < 2 or rows % 2:
        raise ValueError('dino: q and k hold both views, [2b, D] with b >= 1 (got %d rows)' % rows)
    _dino_check_dim(D)
    if (ws.dtype != torch.float32 or wt.dtype != torch.float32 or ws.dim() != 2 or tuple(ws.shape) != tuple(wt.shape)
            or ws.shape[0] < 2 or ws.shape[1] != D):
        raise ValueError('dino: the prototypes are two float32 [K, %d] blocks with K >= 2 (got %s %s, %s %s)'
                         % (D, tuple(ws.shape), ws.dtype, tuple(wt.shape), wt.dtype))
    K = ws.shape[0]
    if center.dtype != torch.float32 or tuple(center.shape) != (K,):
        raise ValueError('dino: the centre is a float32 [%d] vector (got %s %s)' % (K, tuple(center.shape), center.dtype))
    for t in (q, k, ws, wt, center):
        if not t.is_contiguous():
            raise ValueError('dino: every argument is contiguous')
    _dino_check_temp('the student temperature', student_temp)
    _dino_check_temp('the teacher temperature', teacher_temp)
    return rows, K, D


def dino_key_splits(two_n, K):
    """Number of key splits the statistics sweeps of dino_fwd use for two_n rows against K prototypes."""
    splits = lib().dino_key_splits(int(two_n), int(K))
    if splits < 1:
        raise ValueError('dino: need an even two_n >= 2 and K >= 2 (got two_n = %d, K = %d)' % (two_n, K))
    return splits


def dino_row_splits(two_n, K):
    """Number of row splits the key-side sweep of dino_bwd_w uses for two_n rows against K prototypes."""
    splits = lib().dino_row_splits(int(two_n), int(K))
    if splits < 1:
        raise ValueError('dino: need an even two_n >= 2 and K >= 2 (got two_n = %d, K = %d)' % (two_n, K))
    return splits


def dino_workspace(two_n, K, D, device):
    _dino_check_dim(D)
    nbytes = lib().dino_workspace_bytes(two_n, K, D)
    if nbytes == 0:
        raise ValueError('dino: need an even two_n >= 2 and K >= 2 (got two_n = %d, K = %d)' % (two_n, K))
    return torch.empty((nbytes + 7) // 8, device=device, dtype=torch.float64)


def _dino_check_ws(ws, two_n, K, D):
    if ws is None or ws.numel() * ws.element_size() < lib().dino_workspace_bytes(two_n, K, D):
        raise ValueError('dino: the workspace is smaller than dino_workspace(%d, %d, %d)' % (two_n, K, D))


def _dino_check_stats(name, row_stats, two_n):
    if row_stats.dtype != torch.float32 or tuple(row_stats.shape) != (two_n, 2):
        raise ValueError('%s: row_stats is the float32 [2b, 2] block dino_fwd returned (got %s %s)'
                         % (name, tuple(row_stats.shape), row_stats.dtype))


def dino_fwd(q, k, ws, wt, center, student_temp, teacher_temp, workspace=None):
    """q [2b, D] (normalised online projections), k [2b, D] (normalised target projections of the same rows: row r of q pairs with
    row (r + b) mod 2b of k inside the kernels), ws / wt [K, D] (row-normalised online / target prototypes), center [K] ->
    (out = [loss, teacher entropy] device fp32, row_stats [2b, 2], u [2b, D] = Pt . ws, the workspace the three calls share)."""
    two_n, K, D = _dino_check(q, k, ws, wt, center, student_temp, teacher_temp)
    if workspace is None:
        workspace = dino_workspace(two_n, K, D, q.device)
    _dino_check_ws(workspace, two_n, K, D)
    out = step_scalars(2, q.device)
    row_stats = torch.empty(two_n, 2, device=q.device, dtype=torch.float32)
    u = torch.empty_like(q)
    _launch('dino_fwd', 8.0 * two_n * K * D, 4.0 * (3 * two_n + 3 * K) * D,
            lambda: lib().dino_fwd(_p(q), _p(k), _p(ws), _p(wt), _p(center), two_n, K, D, float(student_temp), float(teacher_temp),
                                   _p(out), _p(row_stats), _p(u), _p(workspace), _s()))
    return out, row_stats, u, workspace


def dino_bwd_q(q, ws, u, student_temp, row_stats, grad_scale, workspace):
    """dq [2b, D] = grad_scale * dloss / dq from dino_fwd's row_stats, u and workspace on the same arguments."""
    if (q.dtype != torch.float32 or q.dim() != 2 or q.shape[0] < 2 or q.shape[0] % 2 or u.dtype != torch.float32
            or tuple(u.shape) != tuple(q.shape) or not q.is_contiguous() or not u.is_contiguous()):
        raise ValueError('dino_bwd_q: need contiguous float32 q and u of one shape [2b, D] (got %s %s, %s %s)'
                         % (tuple(q.shape), q.dtype, tuple(u.shape), u.dtype))
    two_n, D = q.shape
    _dino_check_dim(D)
    if ws.dtype != torch.float32 or ws.dim() != 2 or ws.shape[0] < 2 or ws.shape[1] != D or not ws.is_contiguous():
        raise ValueError('dino_bwd_q: the prototypes are a contiguous float32 [K, %d] block with K >= 2 (got %s %s)'
                         % (D, tuple(ws.shape), ws.dtype))
    K = ws.shape[0]
    _dino_check_temp('the student temperature', student_temp)
    _dino_check_stats('dino_bwd_q', row_stats, two_n)
    _dino_check_ws(workspace, two_n, K, D)
    dq = torch.empty_like(q)
    _launch('dino_bwd_q', 4.0 * two_n * K * D, 4.0 * (3 * two_n + K) * D,
            lambda: lib().dino_bwd_q(_p(q), _p(ws), _p(u), two_n, K, D, float(student_temp), _p(row_stats), float(grad_scale), _p(dq),
                                     _p(workspace), _s()))
    return dq


def dino_bwd_w(q, k, ws, wt, center, student_temp, teacher_temp, row_stats, grad_scale, workspace):
    """dws [K, D] = grad_scale * dloss / dws: the key-side sweep.  It recomputes both logits: wt and center are still the ones dino_fwd
    read."""
    two_n, K, D = _dino_check(q, k, ws, wt, center, student_temp, teacher_temp)
    _dino_check_stats('dino_bwd_w', row_stats, two_n)
    _dino_check_ws(workspace, two_n, K, D)
    dws = torch.empty_like(ws)
    _launch('dino_bwd_w', 6.0 * two_n * K * D, 4.0 * (2 * two_n + 3 * K) * D,
            lambda: lib().dino_bwd_w(_p(q), _p(k), _p(ws), _p(wt), _p(center), two_n, K, D, float(student_temp), float(teacher_temp),
                                     _p(row_stats), float(grad_scale), _p(dws), _p(workspace), _s()))
    return dws


def dino_key_mean(k, global_rows):
    """k [2b, D] float32 -> float64 device [D] = (sum of this replica's rows) / global_rows, accumulated in double in a fixed order; summed
    over the replicas it is the global mean the centre update reads."""
    if k.dtype != torch.float32 or k.dim() != 2 or k.shape[0] < 1 or not k.is_contiguous():
        raise ValueError('dino_key_mean: need a contiguous float32 [rows, D] block (got %s %s)' % (tuple(k.shape), k.dtype))
    rows, D = k.shape
    _dino_check_dim(D)
    if int(global_rows) < rows:
        raise ValueError('dino_key_mean: the global batch has at least the %d local rows (got %r)' % (rows, global_rows))
    kbar = torch.empty(D, device=k.device, dtype=torch.float64)
    _launch('dino_key_mean', 1.0 * rows * D, 4.0 * rows * D,
            lambda: lib().dino_key_mean(_p(k), rows, D, 1.0 / float(int(global_rows)), _p(kbar), _s()))
    return kbar


def dino_center(wt, kbar, center, momentum):
    """In place: center <- center + (1 - momentum) (wt . kbar - center); kbar = float64 device [D], the global mean of the normalised
    target projections."""
    if wt.dtype != torch.float32 or wt.dim() != 2 or wt.shape[0] < 2 or not wt.is_contiguous():
        raise ValueError('dino_center: the prototypes are a contiguous float32 [K, D] block with K >= 2 (got %s %s)'
                         % (tuple(wt.shape), wt.dtype))
    K, D = wt.shape
    _dino_check_dim(D)
    if kbar.dtype != torch.float64 or tuple(kbar.shape) != (D,) or not kbar.is_contiguous():
        raise ValueError('dino_center: kbar is a float64 [%d] vector (got %s %s)' % (D, tuple(kbar.shape), kbar.dtype))
    if center.dtype != torch.float32 or tuple(center.shape) != (K,) or not center.is_contiguous():
        raise ValueError('dino_center: the centre is a float32 [%d] vector (got %s %s)' % (K, tuple(center.shape), center.dtype))
    if not 0.0 <= float(momentum) <= 1.0:            # (NaN fails both comparisons)
        raise ValueError('dino_center: the momentum must lie in [0, 1] (got %r)' % (momentum,))
    _launch('dino_center', 2.0 * K * D, 4.0 * K * D,
            lambda: lib().dino_center(_p(wt), _p(kbar), _p(center), K, D, float(momentum), _s()))
    return center


# ---------------------------------------------------------------- SwAV: Sinkhorn codes on prototypes (csrc/swav.hip)
SWAV_DIMS = (64, 128, 256)          # loss widths the SwAV kernels are instantiated for
SWAV_MAX_PROTOTYPES = 1048576       # largest --swav_num_prototypes
SWAV_MAX_ITERS = 16                 # largest --swav_sinkhorn_iterations


def _swav_check_dim(D):
    if D not in SWAV_DIMS:
        raise ValueError('the SwAV loss supports widths %s (got %d)' % ('/'.join(map(str, SWAV_DIMS)), D))


def _swav_check_pos(name, value):
    if not 0.0 < float(value) < float('inf'):            # (NaN fails the comparison)
        raise ValueError('swav: %s must be > 0 and finite (got %r)' % (name, value))


def _swav_check(name, x, w, alpha=None):
    """x [rows, D] (rows even), w [K, D], alpha [2, K] or None -> (rows, K, D)."""
    if x.dtype != torch.float32 or x.dim() != 2 or x.shape[0] < 2 or x.shape[0] % 2 or not x.is_contiguous():
        raise ValueError('%s: need a contiguous float32 block of both views, [2b, D] with b >= 1 (got %s %s)'
                         % (name, tuple(x.shape), x.dtype))
    rows, D = x.shape
    _swav_check_dim(D)
    if (w.dtype != torch.float32 or w.dim() != 2 or not 2 <= w.shape[0] <= SWAV_MAX_PROTOTYPES or w.shape[1] != D
            or not w.is_contiguous()):
        raise ValueError('%s: the prototypes are a contiguous float32 [K, %d] block with K in [2, %d] (got %s %s)'
                         % (name, D, SWAV_MAX_PROTOTYPES, tuple(w.shape), w.dtype))
    K = w.shape[0]
    if alpha is not None and (alpha.dtype != torch.float32 or tuple(alpha.shape) != (2, K) or not alpha.is_contiguous()):
        raise ValueError('%s: alpha is the contiguous float32 [2, %d] block swav_sinkhorn returned (got %s %s)'
                         % (name, K, tuple(alpha.shape), alpha.dtype))
    return rows, K, D


def swav_key_splits(rows, K):
    """Number of key splits the query-side statistics sweeps (swav_fwd, the Sinkhorn's row sweep) use for `rows` rows and K prototypes."""
    splits = lib().swav_key_splits(int(rows), int(K))
    if splits < 1:
        raise ValueError('swav: need an even row count >= 2 and K in [2, %d] (got rows = %d, K = %d)' % (SWAV_MAX_PROTOTYPES, rows, K))
    return splits


def swav_row_splits(rows, K):
    """Number of row splits the key-side sweeps (the Sinkhorn's column sweep, swav_bwd_w) use for `rows` rows and K prototypes."""
    splits = lib().swav_row_splits(int(rows), int(K))
    if splits < 1:
        raise ValueError('swav: need an even row count >= 2 and K in [2, %d] (got rows = %d, K = %d)' % (SWAV_MAX_PROTOTYPES, rows, K))
    return splits


def swav_workspace(rows, K, D, device):
    """Workspace for swav_sinkhorn on `rows` rows, or for swav_fwd / swav_bwd_q / swav_bwd_w on `rows` rows."""
    _swav_check_dim(D)
    nbytes = lib().swav_workspace_bytes(rows, K, D)
    if nbytes == 0:
        raise ValueError('swav: need an even row count >= 2 and K in [2, %d] (got rows = %d, K = %d)' % (SWAV_MAX_PROTOTYPES, rows, K))
    return torch.empty((nbytes + 7) // 8, device=device, dtype=torch.float64)


def _swav_check_ws(ws, rows, K, D):
    if ws is None or ws.numel() * ws.element_size() < lib().swav_workspace_bytes(rows, K, D):
        raise ValueError('swav: the workspace is smaller than swav_workspace(%d, %d, %d)' % (rows, K, D))


def _swav_check_stats(name, row_stats, two_n):
    if row_stats.dtype != torch.float32 or tuple(row_stats.shape) != (two_n, 2):
        raise ValueError('%s: row_stats is the float32 [2b, 2] block swav_fwd returned (got %s %s)'
                         % (name, tuple(row_stats.shape), row_stats.dtype))


def swav_sinkhorn(z_all, w, epsilon=0.05, iters=3, workspace=None):
    """z_all [2N, D] (the gathered normalised batch, view-major), w [K, D] (row-normalised prototypes) -> alpha [2, K] float32, the
    per-view column potentials in nats after `iters` Sinkhorn-Knopp iterations: the code of row g is
    softmax_j(z_g . w_j / epsilon + alpha[view(g)][j])."""
    rows, K, D = _swav_check('swav_sinkhorn', z_all, w)
    _swav_check_pos('epsilon', epsilon)
    if int(iters) != iters or not 1 <= int(iters) <= SWAV_MAX_ITERS:
        raise ValueError('swav_sinkhorn: the iterations lie in [1, %d] (got %r)' % (SWAV_MAX_ITERS, iters))
    if workspace is None:
        workspace = swav_workspace(rows, K, D, z_all.device)
    _swav_check_ws(workspace, rows, K, D)
    alpha = torch.empty(2, K, device=z_all.device, dtype=torch.float32)
    _launch('swav_sinkhorn', (2 * int(iters) - 1) * 2.0 * rows * K * D, 4.0 * (2 * int(iters) - 1) * (rows + K) * D,
            lambda: lib().swav_sinkhorn(_p(z_all), _p(w), rows, K, D, float(epsilon), int(iters), _p(alpha), _p(workspace), _s()))
    return alpha


def swav_fwd(q, w, alpha, temperature, epsilon, workspace=None):
    """q [2b, D] (normalised online projections), w [K, D], alpha [2, K] -> (out = [loss, code entropy] device fp32, row_stats [2b, 2],
    u [2b, D] = Pt . w, the workspace the three calls share)."""
    two_n, K, D = _swav_check('swav_fwd', q, w, alpha)
    _swav_check_pos('the temperature', temperature)
    _swav_check_pos('epsilon', epsilon)
    if workspace is None:
        workspace = swav_workspace(two_n, K, D, q.device)
    _swav_check_ws(workspace, two_n, K, D)
    out = step_scalars(2, q.device)
    row_stats = torch.empty(two_n, 2, device=q.device, dtype=torch.float32)
    u = torch.empty_like(q)
    _launch('swav_fwd', 6.0 * two_n * K * D, 4.0 * (3 * two_n + 2 * K) * D,
            lambda: lib().swav_fwd(_p(q), _p(w), _p(alpha), two_n, K, D, float(temperature), float(epsilon), _p(out), _p(row_stats),
                                   _p(u), _p(workspace), _s()))
    return out, row_stats, u, workspace


def swav_bwd_q(q, w, u, temperature, row_stats, grad_scale, workspace):
    """dq [2b, D] = grad_scale * dloss / dq from swav_fwd's row_stats, u and workspace on the same arguments."""
    two_n, K, D = _swav_check('swav_bwd_q', q, w)
    if u.dtype != torch.float32 or tuple(u.shape) != tuple(q.shape) or not u.is_contiguous():
        raise ValueError('swav_bwd_q: u is the contiguous float32 %s block swav_fwd returned (got %s %s)'
                         % (tuple(q.shape), tuple(u.shape), u.dtype))
    _swav_check_pos('the temperature', temperature)
    _swav_check_stats('swav_bwd_q', row_stats, two_n)
    _swav_check_ws(workspace, two_n, K, D)
    dq = torch.empty_like(q)
    _launch('swav_bwd_q', 4.0 * two_n * K * D, 4.0 * (3 * two_n + K) * D,
            lambda: lib().swav_bwd_q(_p(q), _p(w), _p(u), two_n, K, D, float(temperature), _p(row_stats), float(grad_scale), _p(dq),
                                     _p(workspace), _s()))
    return dq


def swav_bwd_w(q, w, alpha, temperature, epsilon, row_stats, grad_scale, workspace):
    """dw [K, D] = grad_scale * dloss / dw: the key-side sweep.  It recomputes both logits from the alpha swav_fwd read."""
    two_n, K, D = _swav_check('swav_bwd_w', q, w, alpha)
    _swav_check_pos('the temperature', temperature)
    _swav_check_pos('epsilon', epsilon)
    _swav_check_stats('swav_bwd_w', row_stats, two_n)
    _swav_check_ws(workspace, two_n, K, D)
    dw = torch.empty_like(w)
    _launch('swav_bwd_w', 6.0 * two_n * K * D, 4.0 * (2 * two_n + 2 * K) * D,
            lambda: lib().swav_bwd_w(_p(q), _p(w), _p(alpha), two_n, K, D, float(temperature), float(epsilon), _p(row_stats),
                                     float(grad_scale), _p(dw), _p(workspace), _s()))
    return dw


# ---------------------------------------------------------------- SwAV multi-crop: local rows against both global codes (csrc/swav_multicrop.hip)
SWAV_MAX_LOCAL_CROPS = 8            # largest --swav_local_crops


def _swav_local_check(name, x, w, u, L):
    """x [L b, D] (view-major local rows), w [K, D], u [2b, D] (swav_fwd's, of the globals) -> (b, L, K, D)."""
    if int(L) != L or not 1 <= int(L) <= SWAV_MAX_LOCAL_CROPS:
        raise ValueError('%s: the number of local views lies in [1, %d] (got %r)' % (name, SWAV_MAX_LOCAL_CROPS, L))
    L = int(L)
    if x.dtype != torch.float32 or x.dim() != 2 or x.shape[0] < L or x.shape[0] % L or not x.is_contiguous():
        raise ValueError('%s: need a contiguous float32 block of the %d local views, [%d b, D] with b >= 1 (got %s %s)'
                         % (name, L, L, tuple(x.shape), x.dtype))
    b, D = x.shape[0] // L, x.shape[1]
    _swav_check_dim(D)
    if (w.dtype != torch.float32 or w.dim() != 2 or not 2 <= w.shape[0] <= SWAV_MAX_PROTOTYPES or w.shape[1] != D
            or not w.is_contiguous()):
        raise ValueError('%s: the prototypes are a contiguous float32 [K, %d] block with K in [2, %d] (got %s %s)'
                         % (name, D, SWAV_MAX_PROTOTYPES, tuple(w.shape), w.dtype))
    if u.dtype != torch.float32 or tuple(u.shape) != (2 * b, D) or not u.is_contiguous():
        raise ValueError('%s: the global block is the contiguous float32 %s block of swav_fwd on the same images (got %s %s)'
                         % (name, (2 * b, D), tuple(u.shape), u.dtype))
    return b, L, w.shape[0], D


def _swav_local_shape_error(b, L, K):
    return ValueError('swav_local: need b >= 1, L in [1, %d] and K in [2, %d] (got b = %d, L = %d, K = %d)'
                      % (SWAV_MAX_LOCAL_CROPS, SWAV_MAX_PROTOTYPES, b, L, K))


def swav_local_key_splits(b, L, K):
    """Number of key splits of swav_local_fwd's statistics sweep for L views of b images and K prototypes."""
    splits = lib().swav_local_key_splits(int(b), int(L), int(K))
    if splits < 1:
        raise _swav_local_shape_error(b, L, K)
    return splits


def swav_local_row_splits(b, L, K):
    """(row splits of swav_local_bwd_w's student sweep over the L b local rows, of its code sweep over the 2b global rows)."""
    splits = lib().swav_local_row_splits(int(b), int(L), int(K)), lib().swav_local_code_row_splits(int(b), int(L), int(K))
    if min(splits) < 1:
        raise _swav_local_shape_error(b, L, K)
    return splits


def swav_local_workspace(b, L, K, D, device):
    """Workspace for swav_local_fwd / swav_local_bwd_x / swav_local_bwd_w on L views of b images."""
    _swav_check_dim(D)
    nbytes = lib().swav_local_workspace_bytes(int(b), int(L), int(K), D)
    if nbytes == 0:
        raise _swav_local_shape_error(b, L, K)
    return torch.empty((nbytes + 7) // 8, device=device, dtype=torch.float64)


def _swav_local_check_ws(ws, b, L, K, D):
    if ws is None or ws.numel() * ws.element_size() < lib().swav_local_workspace_bytes(b, L, K, D):
        raise ValueError('swav_local: the workspace is smaller than swav_local_workspace(%d, %d, %d, %d)' % (b, L, K, D))


def _swav_local_check_stats(name, row_stats, rows):
    if row_stats.dtype != torch.float32 or tuple(row_stats.shape) != (rows,) or not row_stats.is_contiguous():
        raise ValueError('%s: row_stats is the float32 [L b] block swav_local_fwd returned (got %s %s)'
                         % (name, tuple(row_stats.shape), row_stats.dtype))


def swav_local_fwd(x, w, u, L, temperature, workspace=None):
    """x [L b, D] (normalised local rows, view-major), w [K, D], u [2b, D] (swav_fwd's code expectations of the two global views of the
    same images) -> (out = [the local share of the loss, divided by 2 (L + 1) b] device fp32, row_stats [L b], the workspace the three
    calls share)."""
    b, L, K, D = _swav_local_check('swav_local_fwd', x, w, u, L)
    _swav_check_pos('the temperature', temperature)
    if workspace is None:
        workspace = swav_local_workspace(b, L, K, D, x.device)
    _swav_local_check_ws(workspace, b, L, K, D)
    out = step_scalars(1, x.device)
    row_stats = torch.empty(L * b, device=x.device, dtype=torch.float32)
    _launch('swav_local_fwd', 2.0 * L * b * K * D, 4.0 * (2 * L * b + 2 * b + K) * D,
            lambda: lib().swav_local_fwd(_p(x), _p(w), _p(u), b, L, K, D, float(temperature), _p(out), _p(row_stats), _p(workspace),
                                         _s()))
    return out, row_stats, workspace


def swav_local_bwd_x(x, w, u, L, temperature, row_stats, grad_scale, workspace):
    """dx [L b, D] = grad_scale * d out / dx from swav_local_fwd's row_stats and workspace on the same arguments."""
    b, L, K, D = _swav_local_check('swav_local_bwd_x', x, w, u, L)
    _swav_check_pos('the temperature', temperature)
    _swav_local_check_stats('swav_local_bwd_x', row_stats, L * b)
    _swav_local_check_ws(workspace, b, L, K, D)
    dx = torch.empty_like(x)
    _launch('swav_local_bwd_x', 4.0 * L * b * K * D, 4.0 * (2 * L * b + 2 * b + K) * D,
            lambda: lib().swav_local_bwd_x(_p(x), _p(w), _p(u), b, L, K, D, float(temperature), _p(row_stats), float(grad_scale),
                                           _p(dx), _p(workspace), _s()))
    return dx


def swav_local_bwd_w(x, z, w, alpha, L, temperature, epsilon, row_stats, global_row_stats, grad_scale, workspace):
    """dw [K, D] = grad_scale * d out / dw: the student term over the local rows and the code term over the global rows z [2b, D], whose
    codes are recomputed from alpha [2, K] and the lse_t of swav_fwd's row_stats [2b, 2]."""
    b, L, K, D = _swav_local_check('swav_local_bwd_w', x, w, z, L)
    _swav_check('swav_local_bwd_w', z, w, alpha)
    _swav_check_pos('the temperature', temperature)
    _swav_check_pos('epsilon', epsilon)
    _swav_local_check_stats('swav_local_bwd_w', row_stats, L * b)
    _swav_check_stats('swav_local_bwd_w', global_row_stats, 2 * b)
    if not global_row_stats.is_contiguous():
        raise ValueError('swav_local_bwd_w: the row_stats of swav_fwd must be contiguous')
    _swav_local_check_ws(workspace, b, L, K, D)
    dw = torch.empty_like(w)
    _launch('swav_local_bwd_w', 4.0 * (L * b + 2 * b) * K * D, 4.0 * (L * b + 5 * b + 2 * K) * D,
            lambda: lib().swav_local_bwd_w(_p(x), _p(z), _p(w), _p(alpha), b, L, K, D, float(temperature), float(epsilon),
                                           _p(row_stats), _p(global_row_stats), float(grad_scale), _p(dw), _p(workspace), _s()))
    return dw


# ---------------------------------------------------------------- DINO multi-crop: local rows against both global teacher rows (csrc/dino_multicrop.hip)
# The value and the query-side backward of the local term are swav_local_fwd / swav_local_bwd_x on (x, ws, u, L, Ts) as they stand
# (sum_j Pt[g, j] s_rj = x_r . u_g / Ts); the key-side backward below is DINO's own.
DINO_MAX_LOCAL_CROPS = 8            # largest --dino_local_crops


def _dino_local_shape_error(b, L, K):
    return ValueError('dino_local: need b >= 1, L in [1, %d] and K in [2, %d] (got b = %d, L = %d, K = %d)'
                      % (DINO_MAX_LOCAL_CROPS, DINO_MAX_OUT_DIM, b, L, K))


def dino_local_row_splits(b, L, K):
    """(row splits of dino_local_bwd_w's student sweep over the L b local rows, of its teacher sweep over the 2b global rows)."""
    splits = lib().dino_local_row_splits(int(b), int(L), int(K)), lib().dino_local_teacher_row_splits(int(b), int(L), int(K))
    if min(splits) < 1:
        raise _dino_local_shape_error(b, L, K)
    return splits


def dino_local_workspace(b, L, K, D, device):
    """Workspace of dino_local_bwd_w on L views of b images (its own: swav_local_fwd / swav_local_bwd_x keep theirs)."""
    _dino_check_dim(D)
    nbytes = lib().dino_local_workspace_bytes(int(b), int(L), int(K), D)
    if nbytes == 0:
        raise _dino_local_shape_error(b, L, K)
    return torch.empty((nbytes + 7) // 8, device=device, dtype=torch.float64)


def dino_local_bwd_w(x, k, ws, wt, center, L, student_temp, teacher_temp, local_row_stats, global_row_stats, grad_scale,
                     workspace=None):
    """dws [K, D] = grad_scale * d(local value) / dws: the student term over the local rows x [L b, D] and the teacher term over the
    global keys k [2b, D], whose teacher rows are recomputed from wt, center and the lse_t of dino_fwd's row_stats [2b, 2] -- each
    row's OWN entry.  local_row_stats [L b] is what swav_local_fwd(x, ws, u, L, student_temp) returned: lse_s per local row, base 2."""
    if int(L) != L or not 1 <= int(L) <= DINO_MAX_LOCAL_CROPS:
        raise ValueError('dino_local_bwd_w: the number of local views lies in [1, %d] (got %r)' % (DINO_MAX_LOCAL_CROPS, L))
    L = int(L)
    if x.dtype != torch.float32 or x.dim() != 2 or x.shape[0] < L or x.shape[0] % L or not x.is_contiguous():
        raise ValueError('dino_local_bwd_w: need a contiguous float32 block of the %d local views, [%d b, D] with b >= 1 (got %s %s)'
                         % (L, L, tuple(x.shape), x.dtype))
    b, D = x.shape[0] // L, x.shape[1]
    _dino_check_dim(D)
    if k.dtype != torch.float32 or tuple(k.shape) != (2 * b, D) or not k.is_contiguous():
        raise ValueError('dino_local_bwd_w: the global block is the contiguous float32 %s block of keys dino_fwd read for the same '
                         'images (got %s %s)' % ((2 * b, D), tuple(k.shape), k.dtype))
    _, K, _ = _dino_check(k, k, ws, wt, center, student_temp, teacher_temp)
    if K > DINO_MAX_OUT_DIM:
        raise _dino_local_shape_error(b, L, K)
    _swav_local_check_stats('dino_local_bwd_w', local_row_stats, L * b)
    _dino_check_stats('dino_local_bwd_w', global_row_stats, 2 * b)
    if not global_row_stats.is_contiguous():
        raise ValueError('dino_local_bwd_w: the row_stats of dino_fwd must be contiguous')
    if workspace is None:
        workspace = dino_local_workspace(b, L, K, D, x.device)
    if workspace.numel() * workspace.element_size() < lib().dino_local_workspace_bytes(b, L, K, D):
        raise ValueError('dino_local: the workspace is smaller than dino_local_workspace(%d, %d, %d, %d)' % (b, L, K, D))
    dws = torch.empty_like(ws)
    _launch('dino_local_bwd_w', 4.0 * (L * b + 2 * b) * K * D, 4.0 * (L * b + 3 * b + 3 * K) * D,
            lambda: lib().dino_local_bwd_w(_p(x), _p(k), _p(ws), _p(wt), _p(center), b, L, K, D, float(student_temp),
                                           float(teacher_temp), _p(local_row_stats), _p(global_row_stats), float(grad_scale), _p(dws),
                                           _p(workspace), _s()))
    return dws


# ---------------------------------------------------------------- weighted k-NN evaluation (csrc/knn.hip)
KNN_SLAB = 4096                     # bank rows one workgroup of the top-k kernel reduces to k candidates (simclr_knn_slab_rows)
KNN_MAX_K = 256                     # a query's candidate list is sorted in LDS
KNN_MAX_CLASSES = 32768             # the class scores of a query live in LDS


def knn_topk(q, bank, k):
    """q [Q, D], bank [N, D] fp32 -> (top_val [Q, k] fp32, top_idx [Q, k] int32): per query the first k bank rows of the total order
    "similarity descending, bank index ascending" (exact f32 MFMA, a similarity depends on its two rows only)."""
    if q.dim() != 2 or bank.dim() != 2 or q.shape[1] != bank.shape[1]:
        raise ValueError('knn_topk: need q [Q, D] and bank [N, D] (got %s and %s)' % (tuple(q.shape), tuple(bank.shape)))
    if q.dtype != torch.float32 or bank.dtype != torch.float32:
        raise ValueError('knn_topk: fp32 features only (got %s and %s)' % (q.dtype, bank.dtype))
    (Q, D), N, k = q.shape, bank.shape[0], int(k)
    if not 1 <= k <= KNN_MAX_K:
        raise ValueError('knn_topk: k must be 1..%d (got %d)' % (KNN_MAX_K, k))
    if N < k:
        raise ValueError('knn_topk: the bank has %d rows, fewer than k = %d' % (N, k))
    if N >= 2 ** 31:
        raise ValueError('knn_topk: the bank must have fewer than 2^31 rows (got %d)' % N)
    if D < 16 or D % 16:
        raise ValueError('knn_topk: the feature width must be a multiple of 16 (got %d)' % D)
    if Q < 1:
        raise ValueError('knn_topk: no queries')
    assert lib().knn_slab_rows() == KNN_SLAB, 'libsimclr_hip.so was built with another slab length: rebuild it'
    top_val = torch.empty(Q, k, device=q.device, dtype=torch.float32)
    top_idx = torch.empty(Q, k, device=q.device, dtype=torch.int32)
    ws = _workspace(lib().knn_workspace_bytes(Q, N, D, k), q.device, key='knn')
    _launch('knn_topk', 2.0 * Q * N * D, 4.0 * (Q + N) * D + 8.0 * Q * k,
            lambda: lib().knn_topk(_p(q), _p(bank), Q, N, D, k, _p(top_val), _p(top_idx), _p(ws), _s()))
    return top_val, top_idx


def knn_vote(top_val, top_label, num_classes, temperature):
    """top_val [Q, k] fp32 (descending), top_label [Q, k] int32 -> (pred [Q, 5] int32, score [Q, 5] fp32): the five best classes of the
    weighted vote exp((s - s_max) / temperature), by "score descending, class id ascending"; -1 / 0 past the number of classes."""
    if top_val.dim() != 2 or tuple(top_label.shape) != tuple(top_val.shape):
        raise ValueError('knn_vote: need top_val and top_label of one [Q, k] shape (got %s and %s)' % (tuple(top_val.shape), tuple(top_label.shape)))
    if top_val.dtype != torch.float32 or top_label.dtype != torch.int32:
        raise ValueError('knn_vote: need fp32 similarities and int32 labels (got %s and %s)' % (top_val.dtype, top_label.dtype))
    Q, k = top_val.shape
    num_classes = int(num_classes)
    if not 1 <= k <= KNN_MAX_K or Q < 1:
        raise ValueError('knn_vote: need Q >= 1 and k in 1..%d (got Q=%d k=%d)' % (KNN_MAX_K, Q, k))
    if not 1 <= num_classes <= KNN_MAX_CLASSES:
        raise ValueError('knn_vote: num_classes must be 1..%d (got %d)' % (KNN_MAX_CLASSES, num_classes))
    if not float(temperature) > 0.0:
        raise ValueError('knn_vote: temperature must be > 0 (got %r)' % (temperature,))
    pred = torch.empty(Q, 5, device=top_val.device, dtype=torch.int32)
    score = torch.empty(Q, 5, device=top_val.device, dtype=torch.float32)
    _launch('knn_vote', 2.0 * Q * k, 8.0 * Q * k + 40.0 * Q,
            lambda: lib().knn_vote(_p(top_val), _p(top_label), Q, k, num_classes, float(temperature), _p(pred), _p(score), _s()))
    return pred, score


# ---------------------------------------------------------------- conv / dense
def prep_weights(w_hwio, mode, dtype, khp=0, kwp=0, out=None, cin_p=0, cout_p=0):
    """fp32 HWIO master -> compute copy.  cin_p / cout_p: zero-padded channel dims of the copy."""
    KH, KW, CI, CO = w_hwio.shape
    cip, cop = cin_p or CI, cout_p or CO
    if mode == 2:
        shape = (cop, khp * kwp * 4)
    elif mode == 0:
        shape = (cop, KH * KW * cip)
    else:
        shape = (cip, KH * KW * cop)
    if out is None:
        out = torch.empty(shape, device=w_hwio.device, dtype=dtype)
    lib().prep_weights(_p(w_hwio), _p(out), KH, KW, CI, CO, mode, khp, kwp, cip, cop, dt(out), _s())
    return out


def prep_weights_pair(w_hwio, dtype, cin_p=0, cout_p=0):
    """(w_t [cop, KH*KW*cip], w_d [cip, KH*KW*cop]) -- prep_weights modes 0 and 1 in one launch."""
    KH, KW, CI, CO = w_hwio.shape
    cip, cop = cin_p or CI, cout_p or CO
    w_t = torch.empty(cop, KH * KW * cip, device=w_hwio.device, dtype=dtype)
    w_d = torch.empty(cip, KH * KW * cop, device=w_hwio.device, dtype=dtype)
    lib().prep_weights_pair(_p(w_hwio), _p(w_t), _p(w_d), KH, KW, CI, CO, cip, cop, dt(w_t), _s())
    return w_t, w_d


class WeightPairBatch:
    """Refreshes the (w_t, w_d) compute copies of many convolutions with ONE launch (simclr_prep_weights_pair_multi).
    entries: list of (w_hwio fp32 [KH,KW,CI,CO], cin_p, cout_p); the output buffers are allocated once and keep their
    addresses, so the descriptor table is built once per (dtype, set of master pointers)."""

    def __init__(self, entries, dtype):
        dev = entries[0][0].device
        self.dtype = dtype
        self.key = tuple(w.data_ptr() for w, _, _ in entries)
        self.pairs = []
        chunk = lib().prep_chunk_elems()
        table, chunks = [], []
        for t, (w, cip, cop) in enumerate(entries):
            KH, KW, CI, CO = w.shape
            cip, cop = cip or CI, cop or CO
            assert w.dtype == torch.float32 and w.is_contiguous()
            w_t = torch.empty(cop, KH * KW * cip, device=dev, dtype=dtype)
            w_d = torch.empty(cip, KH * KW * cop, device=dev, dtype=dtype)
            self.pairs.append((w_t, w_d))
            table += [w.data_ptr(), w_t.data_ptr(), w_d.data_ptr(), KH * KW, CI, CO, cip, cop]
            ntile = KH * KW * ((cip + chunk - 1) // chunk) * ((cop + chunk - 1) // chunk)
            chunks += [(t, i) for i in range(ntile)]
        self.table = torch.tensor(table, dtype=torch.int64).to(dev)
        self.chunks = torch.tensor(chunks, dtype=torch.int64).view(-1).to(dev)
        self.nchunks = len(chunks)
        # fp32 storage, three-term modes: the pre-split copies the forward (fp16 pieces of 2^8 w_t) and the data gradient (bf16 pieces of
        # w_d) would otherwise make per launch -- 120 launches of 5 us per ResNet-50 step -- written by ONE launch per refresh
        # (simclr_presplit_weights_multi) and handed to the library with SIMCLR_FMT_PS_W.  SIMCLR_PS_W=0: per-launch copies as before.
        import os
        self.ps = None
        if dtype == torch.float32 and os.environ.get('SIMCLR_PS_W', '1') not in ('', '0'):
            rows_f, rows_b, self.ps_t, self.ps_d = [], [], [], []
            for w_t, w_d in self.pairs:
                ok = w_t.shape[1] % 32 == 0 and w_d.shape[1] % 32 == 0
                pt = torch.empty_like(w_t) if ok else None
                pd = torch.empty_like(w_d) if ok else None
                self.ps_t.append(pt)
                self.ps_d.append(pd)
                if ok:
                    rows_f += [w_t.data_ptr(), pt.data_ptr(), w_t.numel() // 32, 1]
                    rows_b += [w_d.data_ptr(), pd.data_ptr(), w_d.numel() // 32, 0]
            if rows_f:
                self.ps = dict(f=torch.tensor(rows_f, dtype=torch.int64).to(dev), b=torch.tensor(rows_b, dtype=torch.int64).to(dev),
                               n=len(rows_f) // 4, maxb=max(rows_f[2::4] + rows_b[2::4]))

    def matches(self, entries, dtype):
        return dtype == self.dtype and self.key == tuple(w.data_ptr() for w, _, _ in entries)

    def run(self):
        lib().prep_weights_pair_multi(_p(self.table), _p(self.chunks), self.nchunks,
                                      DT_BF16 if self.dtype == torch.bfloat16 else DT_F32, _s())
        if self.ps is not None:
            fwd, bwd = _TERMS[0] == 13, _TERMS[1] == 3
            if fwd:
                lib().presplit_weights_multi(_p(self.ps['f']), self.ps['n'], self.ps['maxb'], _s())
            if bwd:
                lib().presplit_weights_multi(_p(self.ps['b']), self.ps['n'], self.ps['maxb'], _s())
            for (w_t, w_d), pt, pd in zip(self.pairs, self.ps_t, self.ps_d):
                w_t._psw = (pt, 13) if (fwd and pt is not None) else None
                w_d._psw = (pd, 3) if (bwd and pd is not None) else None
        return self.pairs


def conv2d_fwd(x, w_t, KH, KW, stride, pad, OH, OW, stats=None, out=None, store=True):
    """store=False (bf16, stats required): statistics-only pass, nothing is written and None is returned (first half
    of the fused conv + BatchNorm-apply forward, conv2d_fwd_bn_apply)."""
    V, IH, IW, Cin = x.shape
    Cout = w_t.shape[0]
    if not store:
        assert stats is not None and out is None
    elif out is None:
        out = torch.empty(V, OH, OW, Cout, device=x.device, dtype=x.dtype)
    M, K = V * OH * OW, KH * KW * Cin
    esz = x.element_size()
    wp, wf = _pw(w_t, True)
    _launch('conv_igemm_fwd', 2.0 * M * K * Cout, esz * (V * IH * IW * Cin + (M * Cout if store else 0) + K * Cout),
            lambda: lib().conv2d_fwd(_p(x), wp, _p(out), _p(stats), stats.shape[0] if stats is not None else 0, V,
                                     IH, IW, Cin, OH, OW, Cout, KH, KW, stride, pad, dt(x) | _tf() | wf, _s()))
    return out


def bn_pivot_enabled(dtype):
    """Pivoted BatchNorm statistics of the fp32 convolutions (simclr_conv2d_fwd_pivoted); SIMCLR_BN_PIVOT=0: raw moments."""
    return dtype == torch.float32 and os.environ.get('SIMCLR_BN_PIVOT', '1') != '0'


def conv2d_fwd_with_stats(x, w_t, KH, KW, stride, pad, OH, OW, stats):
    """The forward convolution of a conv -> BatchNorm pair (tf2/resnet.py:183-208 followed by :31-78).  Returns (y, stats, sums):
    bf16 (and fp32 with SIMCLR_BN_PIVOT=0): the partial slots as conv2d_fwd fills them, sums None; fp32: the statistics are
    accumulated about a per-channel pivot and come back as this replica's raw fp64 moments `sums` [2, C] (stats None)."""
    if stats is None or not bn_pivot_enabled(x.dtype):
        return conv2d_fwd(x, w_t, KH, KW, stride, pad, OH, OW, stats=stats), stats, None
    V, IH, IW, Cin = x.shape
    Cout = w_t.shape[0]
    out = torch.empty(V, OH, OW, Cout, device=x.device, dtype=x.dtype)
    pivot = torch.empty(Cout, device=x.device, dtype=torch.float32)
    M, K = V * OH * OW, KH * KW * Cin
    wp, wf = _pw(w_t, True)
    _launch('conv_igemm_fwd', 2.0 * M * K * Cout, 4 * (V * IH * IW * Cin + M * Cout + K * Cout),
            lambda: lib().conv2d_fwd_pivoted(_p(x), wp, _p(out), _p(stats), stats.shape[0], _p(pivot), V, IH, IW, Cin, OH, OW,
                                             Cout, KH, KW, stride, pad, dt(x) | _tf() | wf, _s()))
    sums = torch.empty(2, Cout, device=x.device, dtype=torch.float64)
    lib().bn_reduce_slots_pivoted(_p(stats), stats.shape[0], Cout, _p(pivot), float(M), _p(sums), _s())
    return out, None, sums


def conv2d_fwd_bn_apply(x, w_t, KH, KW, stride, pad, OH, OW, scale, shift, res=None, relu=True, want_bits=False,
                        rscale=None, rshift=None):
    """y = act(T(conv(x)) * scale + shift + res) in ONE kernel (bf16; fp32 storage since round 6): what conv2d_fwd + bn_apply
    produce, bit for bit, without the convolution output travelling to memory.  Returns y or (y, relu_bits)."""
    V, IH, IW, Cin = x.shape
    Cout = w_t.shape[0]
    y = torch.empty(V, OH, OW, Cout, device=x.device, dtype=x.dtype)
    M, K = V * OH * OW, KH * KW * Cin
    esz = x.element_size()
    epc = 16 // esz                      # one mask byte per 16-byte chunk of y
    bits = torch.empty(M, Cout // epc, device=x.device, dtype=torch.uint8) if want_bits else None
    # algorithmic bytes = SURVEY 8(d)'s strict count (input + output + weights); the residual read and the mask write of
    # the fused epilogue (bn3's own traffic) are counted under impl_bytes only
    nb = esz * (V * IH * IW * Cin + M * Cout + K * Cout)
    wp, wf = _pw(w_t, True)
    _launch('conv_igemm_fwd', 2.0 * M * K * Cout, nb,
            impl_bytes=nb + (esz * M * Cout if res is not None else 0) + (M * Cout // epc if want_bits else 0),
            fn=lambda: lib().conv2d_fwd_bn_apply(_p(x), wp, _p(y), _p(scale), _p(shift), _p(res), _p(rscale), _p(rshift),
                                              int(relu), _p(bits), V,
                                              IH, IW, Cin, OH, OW, Cout, KH, KW, stride, pad, dt(x) | _tf() | wf, _s()))
    return (y, bits) if want_bits else y


def sparse_dgrad_enabled(dtype):
    """fp32 storage: the data gradient of a stride-2 1x1 projection shortcut stores only the quarter of dx that receives a tap and the
    accumulating data gradient of the block's first convolution reads earlier data there only (simclr_conv2d_dgrad accumulate = 3 / 2):
    no zero fill of, and no read-back from, the other three quarters.  SIMCLR_SPARSE_DGRAD=0: zero fill + full accumulate."""
    return dtype == torch.float32 and os.environ.get('SIMCLR_SPARSE_DGRAD', '1') not in ('', '0')


def _acc_mode(out, accumulate):
    """accumulate argument of the data-gradient entry points: 2 when `out` came from a sparse store (tag `_sparse2`, cleared here)."""
    if not accumulate:
        assert not getattr(out, '_sparse2', False), 'a sparsely stored gradient must be completed by an accumulating data gradient'
        return 0
    if getattr(out, '_sparse2', False):
        out._sparse2 = False
        return 2
    return 1


def conv2d_dgrad(dy, w_d, KH, KW, stride, pad, IH, IW, out=None, accumulate=False, sparse=False):
    """sparse (fp32, stride-2 1x1): only the pixels with even row and column are written, the rest of the result is left
    UNINITIALISED and the tensor is tagged `_sparse2`: its only legal consumer is an accumulating conv2d_dgrad / conv2d_dgrad_bn."""
    V, OH, OW, Cout = dy.shape
    Cin = w_d.shape[0]
    if out is None:
        assert not accumulate
        out = torch.empty(V, IH, IW, Cin, device=dy.device, dtype=dy.dtype)
    if sparse:
        assert not accumulate and stride == 2 and KH == 1 and KW == 1 and pad == 0 and dy.dtype == torch.float32
    M, K = V * IH * IW, KH * KW * Cout
    esz = dy.element_size()
    fmt = FMT_PS_IN if ps_kind(dy) else 0
    assert ps_kind(dy) in (None, 'b16')
    wp, wf = _pw(w_d, False)
    acc = 3 if sparse else _acc_mode(out, accumulate)
    _launch('conv_igemm_dgrad', 2.0 * V * OH * OW * K * Cin, esz * (V * OH * OW * Cout + M * Cin + K * Cin),
            lambda: lib().conv2d_dgrad(_pp(dy), wp, _p(out), acc, V, IH, IW, Cin, OH, OW, Cout,
                                       KH, KW, stride, pad, dt(dy) | fmt | _tb() | wf, _s()))
    if sparse:
        out._sparse2 = True
    return out


def conv2d_dgrad_bn(dy, w_d, KH, KW, pad, IH, IW, bn, out=None, accumulate=False):
    """dgrad + fused BN-backward reduce of the producer BatchNormRelu.  `bn` = dict(x, mask, scale, shift,
    mean, rstd, mode).  Returns (dm, partial[NSLOT,2,Cin])."""
    V, OH, OW, Cout = dy.shape
    Cin = w_d.shape[0]
    if out is None:
        assert not accumulate
        out = torch.empty(V, IH, IW, Cin, device=dy.device, dtype=dy.dtype)
    partial = conv_stats(V * IH * IW, Cin, dy.device)
    K = KH * KW * Cout
    esz = dy.element_size()
    wp, wf = _pw(w_d, False)
    acc = _acc_mode(out, accumulate)
    _launch('conv_igemm_dgrad', 2.0 * V * OH * OW * K * Cin, esz * (V * OH * OW * Cout + V * IH * IW * Cin + K * Cin),
            impl_bytes=esz * (V * OH * OW * Cout + (1 + (bn['mode'] != 4) + (bn['mode'] == 1) + int(accumulate)) * V * IH * IW * Cin + K * Cin),
            fn=lambda: lib().conv2d_dgrad_bn(_pp(dy), wp, _p(out), acc, _p(bn.get('x')), _p(bn.get('mask')),
                                          _p(bn.get('scale')), _p(bn.get('shift')), _p(bn.get('mean')), _p(bn.get('rstd')),
                                          bn['mode'], _p(partial), partial.shape[0], V, IH, IW, Cin, OH, OW, Cout, KH, KW, 1,
                                          pad, dt(dy) | (FMT_PS_IN if ps_kind(dy) else 0) | _tb() | wf, _s()))
    return out, partial


_wgrad_ws = {}


def _workspace(nbytes, device, key='ws'):
    """One scratch buffer per (purpose, device, STREAM): launches on one stream are ordered, so they can share it; a launch
    on the weight-gradient side stream (SIMCLR_WGRAD_STREAM=1) gets its own, so it can never race a main-stream user of the
    same scratch space.  A buffer that has to grow is replaced, the old one stays referenced by the launches
    already queued on its stream (same stream: the allocator orders the reuse)."""
    import os
    # (default: one stream, one buffer -- the configuration the GPU suite runs; the per-stream key only exists with the side stream)
    side = os.environ.get('SIMCLR_WGRAD_STREAM', '0') not in ('', '0')
    k = (key, device, torch.cuda.current_stream(device).cuda_stream) if side else (key, device)
    buf = _wgrad_ws.get(k)
    if buf is None or buf.numel() * 4 < nbytes:
        buf = torch.empty((nbytes + 3) // 4, device=device, dtype=torch.float32)
        _wgrad_ws[k] = buf
    return buf


def conv2d_wgrad(x, dy, KH, KW, stride, pad, Cin=None, pixpitch=None, out=None, accumulate=False):
    V, IH, IW = x.shape[0], x.shape[1], x.shape[2]
    if Cin is None:
        Cin = x.shape[3]
    if pixpitch is None:
        pixpitch = x.shape[3]
    _, OH, OW, Cout = dy.shape
    if out is None:
        assert not accumulate
        out = torch.empty(KH * KW * Cin, Cout, device=x.device, dtype=torch.float32)
    nbytes = lib().conv2d_wgrad_workspace_bytes(V, OH, OW, Cin, Cout, KH, KW, dt(x))
    ws = _workspace(nbytes, x.device)
    M, K = V * OH * OW, KH * KW * Cin
    esz = x.element_size()
    _launch('conv_wgrad', 2.0 * M * K * Cout, esz * (V * IH * IW * pixpitch + M * Cout) + 4 * K * Cout,
            lambda: lib().conv2d_wgrad(_p(x), _pp(dy), _p(out), int(accumulate), _p(ws), V, IH, IW, Cin, pixpitch,
                                       OH, OW, Cout, KH, KW, stride, pad, dt(x) | (FMT_PS_IN if ps_kind(dy) else 0) | _tb(), _s()))
    return out


def stem_geometry(H, W, KH, KW, stride):
    """Packed-input geometry for the stem conv (Conv2dFixedPadding: pad (k-1)//2 before)."""
    pad = (KH - 1) // 2
    OH = (H + (KH - 1) - KH) // stride + 1
    OW = (W + (KW - 1) - KW) // stride + 1
    KWP = 8
    KHP = KH
    HP = (OH - 1) * stride + KHP
    WP = (OW - 1) * stride + KWP
    HP = max(HP, H + pad)
    WP = max(WP, W + pad)
    WP = (WP + 1) // 2 * 2     # 16-byte aligned rows for bf16 (8 B / pixel)
    return dict(pad=pad, OH=OH, OW=OW, KHP=KHP, KWP=KWP, HP=HP, WP=WP)


def pack_views(images, k, geo, dtype, with_presplit=False):
    """with_presplit (fp32): also returns presplit_packed(xp), written in the same pass -> (xp, xq)."""
    b, H, W, C = images.shape
    assert C == 3 * k and images.dtype == torch.float32
    xp = torch.empty(k * b, geo['HP'], geo['WP'], 4, device=images.device, dtype=dtype)
    if with_presplit:
        assert dtype == torch.float32
        xq = torch.empty_like(xp)
        lib().pack_views_ps(_p(images), _p(xp), _p(xq), b, H, W, k, geo['HP'], geo['WP'], geo['pad'], _s())
        return xp, xq
    lib().pack_views(_p(images), _p(xp), b, H, W, k, geo['HP'], geo['WP'], geo['pad'], dt(xp), _s())
    return xp


def stem_conv_fwd(xp, w_s, geo, stride, stats=None):
    V = xp.shape[0]
    Cout = w_s.shape[0]
    y = torch.empty(V, geo['OH'], geo['OW'], Cout, device=xp.device, dtype=xp.dtype)
    M = V * geo['OH'] * geo['OW']
    _launch('stem_conv_fwd', 2.0 * M * 147 * Cout, xp.element_size() * (xp.numel() + M * Cout),
            lambda: lib().stem_conv_fwd(_p(xp), _p(w_s), _p(y), _p(stats), stats.shape[0] if stats is not None else 0, V,
                                        geo['HP'], geo['WP'], geo['OH'], geo['OW'], Cout, geo['KHP'], geo['KWP'],
                                        stride, dt(xp) | _tf(), _s()))
    return y


def stem_wgrad_ps_supported(geo, KH, stride, Cout):
    """Does the pre-split stem weight gradient (simclr_stem_wgrad_ps) cover this stem?  fp32 storage with three bf16 backward terms
    (ps_backward_enabled), the 7x7 / stride-2 stem with 64 output channels; SIMCLR_STEM_WGRAD_PS=0 keeps the multi-tap kernel."""
    import os
    if os.environ.get('SIMCLR_STEM_WGRAD_PS', '1') in ('', '0') or not ps_backward_enabled():
        return False
    return bool(lib().stem_wgrad_ps_supported(KH, geo['KWP'], stride, Cout))


def presplit_packed(xp):
    """The packed views [V, HP, WP, 4] fp32 as (four bf16 hi pieces | four bf16 lo pieces) per pixel: the image operand of
    stem_conv_wgrad when the gradient arrives pre-split."""
    assert xp.dtype == torch.float32 and xp.shape[-1] == 4 and xp.is_contiguous()
    xq = torch.empty_like(xp)
    lib().presplit_packed(_p(xp), _p(xq), xp.numel() // 4, _s())
    return xq


def stem_conv_wgrad(xp, dy, geo, KH, KW, stride, out=None, accumulate=False, xq=None):
    """dW (HWIO [KH,KW,3,Cout] fp32) of the stem from the packed input.  A pre-split dy (bn_bwd_apply(ps_out=True), tagged `_ps`) takes
    simclr_stem_wgrad_ps with xq = presplit_packed(xp) (computed here when the caller has not kept one)."""
    Cout = dy.shape[3]
    kp = geo['KHP'] * geo['KWP'] * 4
    tmp = torch.empty(kp, Cout, device=dy.device, dtype=torch.float32)
    if ps_kind(dy):
        assert ps_kind(dy) == 'b16' and stem_wgrad_ps_supported(geo, KH, stride, Cout), 'pre-split dy without a pre-split stem kernel'
        if xq is None:
            xq = presplit_packed(xp)
        V, OH, OW = dy.shape[0], dy.shape[1], dy.shape[2]
        ws = _workspace(lib().stem_wgrad_ps_workspace_bytes(V, OH, OW, geo['KHP']), dy.device)
        M = V * OH * OW
        _launch('conv_wgrad', 2.0 * M * kp * Cout, 4 * (xp.numel() + M * Cout) + 4 * kp * Cout,
                lambda: lib().stem_wgrad_ps(_p(xq), _pp(dy), _p(tmp), 0, _p(ws), V, geo['HP'], geo['WP'], OH, OW, Cout, geo['KHP'],
                                            geo['KWP'], stride, _s()))
        if out is None:
            out = torch.empty(KH, KW, 3, Cout, device=dy.device, dtype=torch.float32)
        lib().unpack_stem_dw(_p(tmp), _p(out), KH, KW, 3, Cout, geo['KWP'], int(accumulate), _s())
        return out
    # one 'tap' per kernel row: KWP*4 = 32 contiguous elements, pixel pitch 4
    conv2d_wgrad(xp, dy, geo['KHP'], 1, stride, 0, Cin=geo['KWP'] * 4, pixpitch=4, out=tmp)
    if out is None:
        out = torch.empty(KH, KW, 3, Cout, device=dy.device, dtype=torch.float32)
    lib().unpack_stem_dw(_p(tmp), _p(out), KH, KW, 3, Cout, geo['KWP'], int(accumulate), _s())
    return out


# ---------------------------------------------------------------- batch norm
class _StatsArena:
    """All per-layer statistic partials of one step live in one buffer that is zeroed by a single
    memset at the start of the step (instead of ~220 tiny fill kernels)."""

    def __init__(self):
        self.buf = None
        self.ptr = 0
        self.high = 0
        self.missed = 0
        self.want = 0

    def begin_step(self, device, nfloats=64 << 20):
        want = max(nfloats, getattr(self, 'want', 0))
        if self.buf is None or self.buf.device != torch.device(device) or self.buf.numel() < want:
            self.buf = torch.zeros(want, device=device, dtype=torch.float32)
        else:
            self.buf[:max(self.high, 1)].zero_()       # only what the previous step handed out
        self.ptr = 0
        self.high = 0
        self.missed = 0

    def take(self, n, device):
        n_al = (n + 63) // 64 * 64
        if self.buf is None or self.buf.device != torch.device(device) or self.ptr + n_al > self.buf.numel():
            if self.buf is not None and self.ptr < (1 << 60):
                self.missed += n_al                        # arena too small: grow it for the next step
                self.want = self.buf.numel() + 2 * self.missed
            return None
        out = self.buf[self.ptr:self.ptr + n]
        self.ptr += n_al
        self.high = max(self.high, self.ptr)
        return out


_ARENA = _StatsArena()


# (forward terms, backward terms) of simclr_set_f32_matmul; 13 = three split-FP16 terms (11-bit pieces: the accuracy of six bf16
# terms at half the MFMA work; forward only -- gradients span too many binades for fp16 pieces)
F32_MATMUL_TERMS = {'exact': (0, 0), 'bf16x3': (3, 3), 'bf16x6': (6, 6), 'bf16x6_3': (6, 3), 'f16x3_3': (13, 3)}


_TERMS = [0, 0]        # (forward, backward) terms every convolution / dense call of this module passes to the library


def _tf():
    """dtype field of a FORWARD call: this call's matrix arithmetic, SIMCLR_FMT_TERMS(t) = (t + 1) << 12 (csrc/conv.hip terms_of).
    The library's process-wide default (simclr_set_f32_matmul) is never consulted by calls that carry the field: the C ABI is
    re-entrant across threads / streams with different modes."""
    return (_TERMS[0] + 1) << 12


def _tb():
    return (_TERMS[1] + 1) << 12


def set_f32_matmul(mode):
    """Matrix arithmetic of the fp32 convolution / dense kernels (FLAGS.f32_matmul).  The mode is module state of THIS Python layer, sent
    with every call (_tf / _tb); the library's own process-wide default is set too, for callers of the C ABI that pass no field."""
    if mode not in F32_MATMUL_TERMS:
        raise ValueError('f32_matmul must be one of %s, got %r' % (sorted(F32_MATMUL_TERMS), mode))
    fwd, bwd = F32_MATMUL_TERMS[mode]
    _TERMS[0], _TERMS[1] = fwd, bwd
    L = lib()
    if (L.get_f32_matmul(0), L.get_f32_matmul(1)) != (fwd, bwd):
        L.set_f32_matmul(fwd, bwd)


def select_f32_matmul(inference=False):
    """Apply FLAGS.f32_matmul -- for compute_dtype='f32' ONLY: with a bf16 encoder and head_dtype='f32' the fp32
    projection / linear-eval heads exist to keep the loss gradient exact, so they always run the exact fp32-input MFMA.
    inference: a forward through the moving BatchNorm statistics -- 'f16x3_3' falls back to 'bf16x6_3' (fp16 pieces need O(1) operands,
    which only batch statistics guarantee)."""
    from .flags import FLAGS
    mode = getattr(FLAGS, 'f32_matmul', 'exact') if getattr(FLAGS, 'compute_dtype', 'f32') == 'f32' else 'exact'
    if inference and mode == 'f16x3_3':
        mode = 'bf16x6_3'
    set_f32_matmul(mode)


def begin_step(device):
    """Zero the statistics arena and select the fp32 matrix arithmetic; call once at the start of every training step."""
    select_f32_matmul()
    _ARENA.begin_step(device)


def check_split_tail_health():
    """Raise if a workgroup sharing a left-over tile of the persistent convolution grid ever timed out waiting for a partner
    (simclr_conv2d_split_tail_timeouts: sticky device counters; synchronous -- call where the host synchronises anyway)."""
    n = ctypes.c_uint(0)
    lib().conv2d_split_tail_timeouts(ctypes.byref(n))
    if n.value:
        raise RuntimeError('%d split-tail partner(s) of the persistent convolution grid timed out: results of those tiles are wrong '
                           '(SIMCLR_IGEMM_SPLIT=0 disables the split tail)' % n.value)
    return 0


def end_step():
    """Stop handing out arena slices (calls outside a step fall back to fresh zero tensors)."""
    _ARENA.ptr = 1 << 62


def new_stats(C, device, slots=NSLOT):
    """Zeroed partial-statistics buffer [slots, 2, C] (from the per-step arena when inside a step)."""
    t = _ARENA.take(slots * 2 * C, device)
    if t is None:
        return torch.zeros(slots, 2, C, device=device, dtype=torch.float32)
    return t.view(slots, 2, C)


def conv_stats(M, C, device):
    """Statistics buffer for conv2d_fwd / conv2d_dgrad_bn over an [M, C] output with one slot per producing workgroup
    (simclr_conv2d_stats_slots): plain stores instead of float atomics -> run-to-run deterministic BatchNorm."""
    return new_stats(C, device, lib().conv2d_stats_slots(M, C))


def stem_stats(M, C, device):
    return new_stats(C, device, lib().stem_stats_slots(M))


def bn_reduce_slots(partial):
    C = partial.shape[2]
    sums = torch.empty(2, C, device=partial.device, dtype=torch.float64)
    lib().bn_reduce_slots(_p(partial), partial.shape[0], C, _p(sums), _s())
    return sums


def bn_finalize(sums, count, gamma, beta, moving_mean, moving_var, decay, eps=1e-5, partial=None):
    """sums [2,C] fp64 (cross-replica path) or partial [NSLOT,2,C] fp32 (single replica: fused reduce)."""
    src = partial if partial is not None else sums
    C = src.shape[-1]
    dev = src.device
    mean, rstd, scale, shift = (torch.empty(C, device=dev, dtype=torch.float32) for _ in range(4))
    lib().bn_finalize(_p(sums) if partial is None else None, _p(partial), partial.shape[0] if partial is not None else 0,
                      float(count), C, _p(gamma), _p(beta), _p(moving_mean), _p(moving_var),
                      float(decay), float(eps), _p(mean), _p(rstd), _p(scale), _p(shift), _s())
    return mean, rstd, scale, shift


def bn_apply(x, scale, shift, relu, res=None, rscale=None, rshift=None, out=None, want_bits=False):
    """want_bits: also return the ReLU mask (out > 0) as uint8 [rows, C/epc], one byte per 16-byte chunk
    (the operand of conv2d_dgrad_bn mode 3)."""
    C = x.shape[-1]
    rows = x.numel() // C
    if out is None:
        out = torch.empty_like(x)
    bits = torch.empty(rows, C // (16 // x.element_size()), device=x.device, dtype=torch.uint8) if want_bits else None
    lib().bn_apply(_p(x), _p(scale), _p(shift), _p(res), _p(rscale), _p(rshift), _p(out), _p(bits), rows, C,
                   int(relu), dt(x), _s())
    return (out, bits) if want_bits else out


def bn_bwd_reduce(dy, x, mask_src, scale, shift, mean, rstd, mask_mode):
    C = x.shape[-1]
    rows = x.numel() // C
    partial = new_stats(C, x.device, lib().bn_bwd_reduce_slots(rows, C, dt(x)))
    lib().bn_bwd_reduce(_p(dy), _p(x), _p(mask_src), _p(scale), _p(shift), _p(mean), _p(rstd), rows, C,
                        mask_mode, _p(partial), partial.shape[0], dt(x), _s())
    return partial


def bn_bwd_finalize(local_sums, global_sums, count, dgamma, dbeta, accumulate=False, partial=None):
    src = partial if partial is not None else local_sums
    C = src.shape[-1]
    c1 = torch.empty(C, device=src.device, dtype=torch.float32)
    c2 = torch.empty(C, device=src.device, dtype=torch.float32)
    lib().bn_bwd_finalize(_p(local_sums) if partial is None else None, _p(global_sums) if partial is None else None,
                          _p(partial), partial.shape[0] if partial is not None else 0, float(count), C,
                          _p(dgamma), _p(dbeta), int(accumulate), _p(c1), _p(c2), _s())
    return c1, c2


def bn_bwd_apply(dy, x, mask_src, scale, shift, mean, rstd, c1, c2, mask_mode, want_masked=False, out=None, ps_out=False):
    """ps_out (fp32, C % 32 == 0): dx in the pre-split block format with bf16 pieces (tagged `_ps`), for the data-gradient and
    weight-gradient GEMMs of the convolution in front of this BatchNorm."""
    C = x.shape[-1]
    rows = x.numel() // C
    dx = torch.empty_like(x) if out is None else out
    dmasked = torch.empty_like(x) if want_masked else None
    ps_out = bool(ps_out) and x.dtype == torch.float32 and C % 32 == 0
    lib().bn_bwd_apply(_p(dy), _p(x), _p(mask_src), _p(scale), _p(shift), _p(mean), _p(rstd), _p(c1), _p(c2),
                       rows, C, mask_mode, _pp(dx), _p(dmasked), dt(x) | (FMT_PS_OUT if ps_out else 0), _s())
    if ps_out:
        dx._ps = 'b16'
    return dx, dmasked


# ---------------------------------------------------------------- pooling
def same_pad(size, k, s):
    out = -(-size // s)
    total = max((out - 1) * s + k - size, 0)
    return out, total // 2


def bnrelu_maxpool_fwd(x, scale, shift, ksz=3, stride=2, want_arg=True):
    """want_arg=False: no backward pass follows (a frozen stem) -- the tap ids are neither tracked nor stored; arg is None."""
    V, H, W, C = x.shape
    OH, pt = same_pad(H, ksz, stride)
    OW, pl = same_pad(W, ksz, stride)
    y = torch.empty(V, OH, OW, C, device=x.device, dtype=x.dtype)
    arg = torch.empty(V, OH, OW, C, device=x.device, dtype=torch.uint8) if want_arg else None
    lib().bnrelu_maxpool_fwd(_p(x), _p(scale), _p(shift), _p(y), _p(arg), V, H, W, C, OH, OW, ksz, stride,
                             pt, pl, dt(x), _s())
    return y, arg


def maxpool_bwd(dy, arg, H, W, ksz=3, stride=2):
    V, OH, OW, C = dy.shape
    _, pt = same_pad(H, ksz, stride)
    _, pl = same_pad(W, ksz, stride)
    dx = torch.empty(V, H, W, C, device=dy.device, dtype=dy.dtype)
    lib().maxpool_bwd(_p(dy), _p(arg), _p(dx), V, H, W, C, OH, OW, ksz, stride, pt, pl, dt(dy), _s())
    return dx


def global_avgpool_fwd(x, out_dtype=None):
    """reduce_mean over H, W (tf2/resnet.py:693-696).  out_dtype=torch.float32: fp32 means from bf16 activations."""
    V, H, W, C = x.shape
    if out_dtype is None or out_dtype == x.dtype:
        y = torch.empty(V, C, device=x.device, dtype=x.dtype)
        lib().global_avgpool_fwd(_p(x), _p(y), V, H * W, C, dt(x), _s())
        return y
    assert out_dtype == torch.float32
    y = torch.empty(V, C, device=x.device, dtype=torch.float32)
    lib().global_avgpool_fwd_f32(_p(x), _p(y), V, H * W, C, dt(x), _s())
    return y


def global_avgpool_bwd(dy, H, W, mask_src=None):
    V, C = dy.shape
    dx = torch.empty(V, H, W, C, device=dy.device, dtype=dy.dtype)
    lib().global_avgpool_bwd(_p(dy), _p(mask_src), _p(dx), V, H * W, C, dt(dy), _s())
    return dx


def batch_blur(images, filt, selector, solarize=None, threshold=0.5):
    """images f32 [b,H,W,3k]; filt [k,K]; selector [k,b] of 0/1.
    solarize: None (simclr_batch_blur, the launches of a run without solarization), or [k,b] of 0/1 laid out like selector
    (simclr_batch_blur_solarize): after the clip, v >= threshold ? 1 - v : v on the images whose coin is set."""
    b, H, W, C = images.shape
    k, K = filt.shape
    assert C == 3 * k and images.dtype == torch.float32
    tmp = torch.empty_like(images)
    out = torch.empty_like(images)
    if solarize is None:
        lib().batch_blur(_p(images), _p(tmp), _p(out), _p(filt), _p(selector), b, H, W, k, K, _s())
    else:
        assert tuple(solarize.shape) == (k, b) and solarize.dtype == torch.float32 and solarize.is_contiguous()
        lib().batch_blur_solarize(_p(images), _p(tmp), _p(out), _p(filt), _p(selector), _p(solarize), float(threshold),
                                  b, H, W, k, K, _s())
    return out


def avgpool2_fwd(x, stride):
    V, H, W, C = x.shape
    OH, OW = (H, W) if stride == 1 else ((H + 1) // 2, (W + 1) // 2)
    y = torch.empty(V, OH, OW, C, device=x.device, dtype=x.dtype)
    lib().avgpool2_fwd(_p(x), _p(y), V, H, W, C, stride, dt(x), _s())
    return y


def avgpool2_bwd(dy, H, W, stride):
    V, OH, OW, C = dy.shape
    dx = torch.empty(V, H, W, C, device=dy.device, dtype=dy.dtype)
    lib().avgpool2_bwd(_p(dy), _p(dx), V, H, W, C, stride, dt(dy), _s())
    return dx


# ---------------------------------------------------------------- selective kernel unit
def sk_pool_fwd(a, f, gpitch):
    V, H, W, _ = a.shape
    g = torch.zeros(V, gpitch, device=a.device, dtype=a.dtype)
    lib().sk_pool_fwd(_p(a), _p(g), V, H * W, f, gpitch, dt(a), _s())
    return g


def sk_mix_fwd(a, l, f):
    V, H, W, _ = a.shape
    out = torch.empty(V, H, W, f, device=a.device, dtype=a.dtype)
    lib().sk_mix_fwd(_p(a), _p(l), _p(out), V, H * W, f, l.shape[1], dt(a), _s())
    return out


def sk_mix_bwd_logits(a, l, dout, f):
    V, H, W, _ = a.shape
    dl = torch.zeros_like(l)
    lib().sk_mix_bwd_logits(_p(a), _p(l), _p(dout), _p(dl), V, H * W, f, l.shape[1], dt(a), _s())
    return dl


def sk_mix_bwd_streams(l, dout, dg, f):
    V, H, W, _ = dout.shape
    da = torch.empty(V, H, W, 2 * f, device=dout.device, dtype=dout.dtype)
    lib().sk_mix_bwd_streams(_p(l), _p(dout), _p(dg), _p(da), V, H * W, f, l.shape[1], dg.shape[1], dt(dout), _s())
    return da


# ---------------------------------------------------------------- supervised head / misc
def bias_softmax_xent(z, bias, labels, nclass, gscale, out):
    rows, cpad = z.shape
    dlogits = torch.empty_like(z)
    lib().bias_softmax_xent(_p(z), _p(bias), _p(labels), rows, labels.shape[0], nclass, cpad, float(gscale),
                            _p(dlogits), _p(out), dt(z), _s())
    return dlogits


def kd_softmax_xent(zs, bias_s, zt, bias_t, nclass, temperature, gscale, out):
    """Distillation loss of student rows zs [rows, cpad_s] against teacher rows zt [rows, cpad_t] (simclr_kd_softmax_xent): adds the
    loss into out[0] and the teacher agreement into out[1], returns dlogits in the student's layout.  Either bias may be None."""
    rows, cpad_s = zs.shape
    assert zt.dim() == 2 and zt.shape[0] == rows, (tuple(zs.shape), tuple(zt.shape))
    dlogits = torch.empty_like(zs)
    lib().kd_softmax_xent(_p(zs), _p(bias_s), _p(zt), _p(bias_t), rows, nclass, cpad_s, zt.shape[1], float(temperature),
                          float(gscale), _p(dlogits), _p(out), dt(zs), dt(zt), _s())
    return dlogits


def colsum(x, cvalid, out, accumulate=False):
    rows, C = x.shape
    lib().colsum(_p(x), rows, C, cvalid, _p(out), int(accumulate), dt(x), _s())
    return out


def cast(x, dtype, out=None):
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=dtype)
    lib().cast(_p(x), _p(out), x.numel(), dt(x), dt(out), _s())
    return out


def axpy_f32(a, x, y):
    lib().axpy_f32(float(a), _p(x), _p(y), x.numel(), _s())


def step_scalars(n, device):
    """n zeroed fp32 scalars that live until the next begin_step (a slice of the per-step arena: no fill launch); outside
    a step a fresh zero tensor."""
    t = _ARENA.take(n, device)
    return t if t is not None else torch.zeros(n, device=device, dtype=torch.float32)


def accumulate_scalars(srcs, dst=None, scales=None, total=None, total_mask=0, copy=None):
    """dst[i] += scales[i] * srcs[i][0] for up to 16 device scalars in ONE launch; total[0] = sum of the scaled terms
    selected by total_mask; copy[i] = the scaled term (simclr_accumulate_scalars)."""
    assert 1 <= len(srcs) <= 16, 'accumulate_scalars: 1..16 scalars per launch, got %d' % len(srcs)
    import ctypes
    n = len(srcs)
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in srcs])
    sc = (ctypes.c_float * n)(*[float(x) for x in scales]) if scales is not None else None
    lib().accumulate_scalars(ptrs, sc, n, _p(dst), _p(total), int(total_mask), _p(copy), _s())


def l2_loss_f32(x, out):
    lib().l2_loss_f32(_p(x), x.numel(), _p(out), _s())


# ---------------------------------------------------------------- two-view augmentation
def augment_views(src, params, H, W, out=None):
    """src [b, Hs, Ws, 3] float32 in [0,1] or uint8; params [b, views, 16] float32 (simclr_amd.data_util.PARAM_FIELDS).
    Returns [b, H, W, 3*views] float32 in [0,1]."""
    b, Hs, Ws, C = src.shape
    assert C == 3 and params.dtype == torch.float32 and params.shape[0] == b and params.shape[2] == 16
    views = params.shape[1]
    if src.dtype == torch.uint8:
        code = 2
    elif src.dtype == torch.float32:
        code = DT_F32
    else:
        raise TypeError('augment_views: source images must be uint8 or float32, got %s' % src.dtype)
    if out is None:
        out = torch.empty(b, H, W, 3 * views, device=src.device, dtype=torch.float32)
    ws = _workspace(lib().augment_workspace_bytes(b, views, H, W), src.device, key='augment')
    lib().augment_views(_p(src), code, _p(params), _p(ws), _p(out), b, views, Hs, Ws, H, W, _s())
    return out


def check_ragged_table(table, packed_bytes):
    """Host check of a ragged batch's table [b, 3] = (byte offset, height, width): every record must lie inside the packed
    buffer.  Returns the table as a contiguous int64 array; raises ValueError naming the first bad row."""
    import numpy as np
    t = np.ascontiguousarray(np.asarray(table), dtype=np.int64)
    if t.ndim != 2 or t.shape[1] != 3 or t.shape[0] == 0:
        raise ValueError('augment_views_ragged: table must be [b, 3] (byte offset, height, width), got shape %s' % (t.shape,))
    off, h, w = t[:, 0], t[:, 1], t[:, 2]
    bad = (off < 0) | (h <= 0) | (w <= 0) | (h > (1 << 20)) | (w > (1 << 20))
    end = off + 3 * np.where(bad, 0, h) * np.where(bad, 0, w)
    bad |= end > int(packed_bytes)
    if bad.any():
        i = int(np.argmax(bad))
        raise ValueError('augment_views_ragged: table row %d (offset %d, height %d, width %d) does not lie inside the packed '
                         'buffer of %d bytes' % (i, off[i], h[i], w[i], int(packed_bytes)))
    return t


def augment_views_ragged(packed, table, params, H, W, out=None, table_dev=None):
    """packed: device uint8 [nbytes], images HWC back to back; table: HOST int64 [b, 3] = (byte offset, height, width),
    checked here before anything is launched; params [b, views, 16] float32 on the device.  table_dev: the table already
    on the device (the input pipeline ships it in the batch's one copy); otherwise it is uploaded.
    Returns [b, H, W, 3*views] float32 in [0,1], bitwise augment_views' result for the same pixels and draws."""
    if packed.dtype != torch.uint8 or packed.dim() != 1:
        raise TypeError('augment_views_ragged: packed must be a 1-D uint8 tensor')
    t = check_ragged_table(table, packed.numel())
    b = t.shape[0]
    assert params.dtype == torch.float32 and params.shape[0] == b and params.shape[2] == 16
    views = params.shape[1]
    if table_dev is None:
        table_dev = torch.from_numpy(t).to(packed.device, non_blocking=True)
    assert table_dev.dtype == torch.int64 and table_dev.numel() == 3 * b
    if out is None:
        out = torch.empty(b, H, W, 3 * views, device=packed.device, dtype=torch.float32)
    ws = _workspace(lib().augment_workspace_bytes(b, views, H, W), packed.device, key='augment')
    lib().augment_views_ragged(_p(packed), packed.numel(), _p(table_dev), _p(params), _p(ws), _p(out), b, views, H, W, _s())
    return out


# ---------------------------------------------------------------- BatchNorm backward folded into the producing 1x1 conv
def bn_fold_coeffs(scale, mean, rstd, c1, c2):
    C = scale.shape[0]
    a, b, d = (torch.empty(C, device=scale.device, dtype=torch.float32) for _ in range(3))
    lib().bn_fold_coeffs(_p(scale), _p(mean), _p(rstd), _p(c1), _p(c2), _p(a), _p(b), _p(d), C, _s())
    return a, b, d


def bn_fold_pre(w_d, scale, mean, rstd, c1, c2):
    """w_d [K][N] (compute copy, = the conv's dgrad layout) + the BN-backward quantities.  Returns (a, b, d [N],
    wb [K,N] f32 = w*b, wext [K, N+K] (first N columns = w*a, the rest filled by bn_fold_post), e [K] f32 = w d)."""
    K, N = w_d.shape
    dev = w_d.device
    a, b, d = (torch.empty(N, device=dev, dtype=torch.float32) for _ in range(3))
    wb = torch.empty(K, N, device=dev, dtype=torch.float32)
    wext = torch.empty(K, N + K, device=dev, dtype=w_d.dtype)
    e = torch.empty(K, device=dev, dtype=torch.float32)
    lib().bn_fold_pre(_p(w_d), _p(scale), _p(mean), _p(rstd), _p(c1), _p(c2), _p(a), _p(b), _p(d), _p(wb), _p(wext), _p(e),
                      K, N, dt(w_d), _s())
    return a, b, d, wb, wext, e


def bn_fold_post(t1, gw, cs, a, b, d, q, dw, wext, accumulate=False):
    """cs: column sums of h, fp64 [>=K] (bn_reduce_slots output) or fp32 [K] (conv2d_gram).  q = wext = None: the weight gradient
    only (no data gradient follows)."""
    K, N = t1.shape
    assert (q is None) == (wext is None)
    assert (q is None or tuple(q.shape) == (K, K)) and tuple(dw.shape) == (K, N) and cs.is_contiguous()
    c64, c32 = (_p(cs), None) if cs.dtype == torch.float64 else (None, _p(cs))
    lib().bn_fold_post(_p(t1), _p(gw), c64, c32, _p(a), _p(b), _p(d), _p(q), _p(dw), _p(wext), K, N, int(accumulate),
                       dt(wext) if wext is not None else dt(t1), _s())
    return dw


def conv2d_gram(h):
    """h [..., K] activation -> (h^T h [K, K] fp32, colsum(h) [K] fp32), streaming h once (K in {64, 128, 256 bf16})."""
    K = h.shape[-1]
    M = h.numel() // K
    out = torch.empty(K * K + K, device=h.device, dtype=torch.float32)
    ws = _workspace(lib().conv2d_gram_workspace_bytes(M, K, dt(h)), h.device)
    esz = h.element_size()
    _launch('conv_wgrad', 2.0 * M * K * K, esz * M * K + 4 * K * K,
            lambda: lib().conv2d_gram(_p(h), _p(out), _p(ws), M, K, dt(h) | (_tf() if h.dtype == torch.float32 else 0), _s()))
    return out[:K * K].view(K, K), out[K * K:]


def bn_sums_from_gram(gw, w_kn, cs):
    """(sum c, sum c^2) per output channel of c = h W from GW = (h^T h) W [K, N], W [K, N] fp32 and colsum(h) -> fp64 [2, N]."""
    K, N = gw.shape
    assert tuple(w_kn.shape) == (K, N) and gw.dtype == torch.float32 and w_kn.dtype == torch.float32
    sums = torch.empty(2, N, device=gw.device, dtype=torch.float64)
    c64, c32 = (_p(cs), None) if cs.dtype == torch.float64 else (None, _p(cs))
    lib().bn_sums_from_gram(_p(gw), _p(w_kn), c64, c32, K, N, _p(sums), _s())
    return sums


def gram_supported(K, dtype):
    return K in (64, 128) or (K == 256 and dtype == torch.bfloat16)


def small_gemm_nt(A, B):
    """A [M, K] fp32, B [N, K] fp32 -> A B^T [M, N] fp32 (exact f32 MFMA; small matrices)."""
    M, K = A.shape
    N = B.shape[0]
    assert A.dtype == torch.float32 and B.dtype == torch.float32 and B.shape[1] == K
    C = torch.empty(M, N, device=A.device, dtype=torch.float32)
    lib().small_gemm_nt_f32(_p(A), _p(B), _p(C), M, N, K, _s())
    return C


def conv2d_dgrad_bn_ext(dm, h, wext, bias, bn, out=None, accumulate=False):
    """1x1 stride-1 dgrad reading (dm [V,H,W,N], h [V,H,W,K]) with the K-extended weights of bn_fold_pre/post and the bias
    W d, plus the fused BN-backward reduce of the producer BN of h (`bn` as in conv2d_dgrad_bn).  Returns (dm_in, partial)."""
    assert not getattr(out, '_sparse2', False), 'a sparsely stored gradient needs conv2d_dgrad / conv2d_dgrad_bn to complete it'
    V, H, W, N = dm.shape
    K = h.shape[3]
    if out is None:
        assert not accumulate
        out = torch.empty(V, H, W, K, device=dm.device, dtype=dm.dtype)
    partial = conv_stats(V * H * W, K, dm.device)
    esz = dm.element_size()
    M = V * H * W
    _launch('conv_igemm_dgrad', 2.0 * M * N * K, esz * (M * N + M * K + N * K),
            impl_bytes=esz * (M * N + (3 + (bn['mode'] == 1) + int(accumulate)) * M * K + (N + K) * K),
            fn=lambda: lib().conv2d_dgrad_bn_ext(_p(dm), _p(h), _p(wext), _p(bias), _p(out), int(accumulate), _p(bn['x']),
                                                 _p(bn.get('mask')), _p(bn.get('scale')), _p(bn.get('shift')), _p(bn['mean']),
                                                 _p(bn['rstd']), bn['mode'], _p(partial), partial.shape[0], V, H, W, K, N,
                                                 dt(dm) | _tb(), _s()))
    return out, partial


# ---------------------------------------------------------------- stem backward fused with the max-pool backward
def bn_bwd_reduce_pool(dy, arg, x, scale, shift, mean, rstd, ksz=3, stride=2):
    V, H, W, C = x.shape
    _, OH, OW, _ = dy.shape
    _, pt = same_pad(H, ksz, stride)
    _, pl = same_pad(W, ksz, stride)
    partial = new_stats(C, x.device, lib().bn_bwd_pool_slots(V * H * W, C, dt(x)))
    lib().bn_bwd_reduce_pool(_p(dy), _p(arg), _p(x), _p(scale), _p(shift), _p(mean), _p(rstd), V, H, W, C, OH, OW, ksz,
                             stride, pt, pl, _p(partial), partial.shape[0], dt(x), _s())
    return partial


def bn_bwd_apply_pool(dy, arg, x, scale, shift, mean, rstd, c1, c2, ksz=3, stride=2, ps_out=False):
    """ps_out (fp32, C % 32 == 0): dx in the pre-split block format with bf16 pieces (tagged `_ps`), for the stem's weight gradient."""
    V, H, W, C = x.shape
    _, OH, OW, _ = dy.shape
    _, pt = same_pad(H, ksz, stride)
    _, pl = same_pad(W, ksz, stride)
    dx = torch.empty_like(x)
    lib().bn_bwd_apply_pool(_p(dy), _p(arg), _p(x), _p(scale), _p(shift), _p(mean), _p(rstd), _p(c1), _p(c2), _p(dx), V, H,
                            W, C, OH, OW, ksz, stride, pt, pl, dt(x) | (FMT_PS_OUT if ps_out else 0), _s())
    if ps_out:
        dx._ps = 'b16'
    return dx


def bn_fold_s2(t1, w_d, mean, rstd, sums):
    """sums [2, N] fp64 with sums[0] = sum(dm): fills sums[1] = sum(dm * x^) of the BatchNorm behind c = h W from
    t1 = h^T dm [K, N] and the weight copy w_d [K, N] -- no pass over c."""
    K, N = t1.shape
    assert sums.dtype == torch.float64 and tuple(sums.shape) == (2, N) and tuple(w_d.shape) == (K, N)
    lib().bn_fold_s2(_p(t1), _p(w_d), _p(mean), _p(rstd), _p(sums), K, N, dt(w_d), _s())
    return sums


def conv2d_dgrad_ext(dm, h, wext, bias, out=None, accumulate=False):
    """K-extended 1x1 dgrad with a plain epilogue (see conv2d_dgrad_bn_ext): dx [+]= dm (a*W)^T + h Q + W d."""
    assert not getattr(out, '_sparse2', False), 'a sparsely stored gradient needs conv2d_dgrad / conv2d_dgrad_bn to complete it'
    V, H, W, N = dm.shape
    K = h.shape[3]
    if out is None:
        assert not accumulate
        out = torch.empty(V, H, W, K, device=dm.device, dtype=dm.dtype)
    esz = dm.element_size()
    M = V * H * W
    _launch('conv_igemm_dgrad', 2.0 * M * N * K, esz * (M * N + M * K + N * K),
            impl_bytes=esz * (M * N + (2 + int(accumulate)) * M * K + (N + K) * K),
            fn=lambda: lib().conv2d_dgrad_ext(_p(dm), _p(h), _p(wext), _p(bias), _p(out), int(accumulate), V, H, W, K, N,
                                              dt(dm) | _tb(), _s()))
    return out


# ---------------------------------------------------------------- DropBlock (csrc/dropblock.hip, tf2/resnet.py:81-157)
def dropblock_gamma(keep_prob, width, dropblock_size):
    """(k, seed_drop_rate) of tf2/resnet.py:111-114, in Python double as the reference computes it."""
    k = min(dropblock_size, width)
    return k, (1.0 - keep_prob) * width**2 / k**2 / (width - k + 1)**2


def dropblock_keep_thresh(gamma):
    """fp32(1 - gamma), the constant of tf2/resnet.py:130-131 (round to nearest, as tf.cast of the Python double)."""
    return struct.unpack('f', struct.pack('f', 1.0 - gamma))[0]


def dropblock_mask(shape, keep_prob, dropblock_size, key=0, noise=None, device=None):
    """The block pattern of one site for an activation of `shape` [V,H,W,C]: (bits uint8 [V,H,W,C/8], count int64 [2] = ones, size).
    noise: fp32 [V,H,W,C] uniform tensor to read (tests); None: generated in the kernel from `key` (64 bits) and the element index."""
    V, H, W, C = shape
    if H != W:
        raise ValueError('Input tensor with width!=height is not supported.')          # :108-109
    device = noise.device if noise is not None else device
    k, gamma = dropblock_gamma(keep_prob, W, dropblock_size)
    bits = torch.empty(V, H, W, max(C // 8, 1), device=device, dtype=torch.uint8)
    count = torch.empty(2, device=device, dtype=torch.int64)
    key = int(key) & 0xFFFFFFFFFFFFFFFF
    key = key - (1 << 64) if key >= (1 << 63) else key
    lib().dropblock_mask(_p(noise), key, V, H, W, C, int(dropblock_size), dropblock_keep_thresh(gamma), _p(bits), _p(count), _s())
    return bits, count


def dropblock_apply(x, bits, count, out=None):
    """x / percent_ones * pattern (forward; applied to dy, the backward)."""
    C = x.shape[-1]
    rows = x.numel() // C
    y = torch.empty_like(x) if out is None else out
    nbytes = 2.0 * x.numel() * x.element_size() + x.numel() / 8
    _launch('dropblock_apply', 2.0 * x.numel(), nbytes,
            lambda: lib().dropblock_apply(_p(x), _p(bits), _p(count), _p(y), rows, C, dt(x), _s()))
    return y


def dropblock_tail_fwd(a, bits_a, count_a, b, bits_b, count_b, want_bits=True):
    """relu(a / pa * ma + b / pb * mb) -> (out, ReLU bits in bn_apply's format | None)."""
    assert a.shape == b.shape and a.dtype == b.dtype
    C = a.shape[-1]
    rows = a.numel() // C
    out = torch.empty_like(a)
    rb = torch.empty(rows, C // (16 // a.element_size()), device=a.device, dtype=torch.uint8) if want_bits else None
    nbytes = 3.0 * a.numel() * a.element_size() + a.numel() * 3 / 8
    _launch('dropblock_tail_fwd', 6.0 * a.numel(), nbytes,
            lambda: lib().dropblock_tail_fwd(_p(a), _p(bits_a), _p(count_a), _p(b), _p(bits_b), _p(count_b), _p(out), _p(rb), rows, C,
                                             dt(a), _s()))
    return out, rb


def dropblock_tail_bwd(dout, relu_bits, bits_a, count_a, bits_b, count_b):
    """Gradient of dropblock_tail_fwd wrt (a, b)."""
    C = dout.shape[-1]
    rows = dout.numel() // C
    da, db = torch.empty_like(dout), torch.empty_like(dout)
    nbytes = 3.0 * dout.numel() * dout.element_size() + dout.numel() * 3 / 8
    _launch('dropblock_tail_bwd', 4.0 * dout.numel(), nbytes,
            lambda: lib().dropblock_tail_bwd(_p(dout), _p(relu_bits), _p(bits_a), _p(count_a), _p(bits_b), _p(count_b), _p(da), _p(db),
                                             rows, C, dt(dout), _s()))
    return da, db
