"""The batched fp32 epilogue of the fused BatchNorm-backward reduce (csrc/conv.hip, EPS instantiations listed by f32_eps_exists): the
three-term data gradients on a pre-split dy with the mask mode / accumulate flag compiled in request the operands of a fragment row
before the previous row is stored.  Arithmetic and order are those of the generic per-fragment loop, which SIMCLR_F32_EPI_BATCH=0
selects -- so every case runs the same call on the same inputs with the switch at 0 and at 1 and asks for the same BITS (gradient and
per-slot partial sums), checks which instantiation each run took (tile, halo window, EPS), and compares the result with float64.  The
classes that keep the per-fragment loop are in the list too, with EPS = 0 expected under either switch value.

float64 tolerances of the pre-split cases: those of gpu_checks.check_dgrad_bn (2e-5 of max|ref|, doubled when accumulating; sums
1e-4 relative + 1e-3 of the largest per-channel L1 sum), the first doubled for the three bf16-piece terms of the backward GEMMs exactly
as gpu_checks.check_conv does for that arithmetic.  The K-extended case uses check_bn_fold's fp32 gates (2e-4; sums 1e-4 of the L1 sum)."""
import contextlib
import os
import re

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

F32 = torch.float32
SWITCH = 'SIMCLR_F32_EPI_BATCH'


@contextlib.contextmanager
def switch(v):
    old = os.environ.get(SWITCH)
    os.environ[SWITCH] = str(v)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(SWITCH, None)
        else:
            os.environ[SWITCH] = old


@contextlib.contextmanager
def matmul(mode):
    from simclr_amd import ops
    ops.set_f32_matmul(mode)
    try:
        yield
    finally:
        ops.set_f32_matmul('exact')


def last_args():
    """Template arguments of the last conv_igemm_persistent launch, the defaulted tail (EXT ... PSX) filled in: dict by name."""
    from simclr_amd._lib import lib
    rec = lib().conv2d_last_instantiation().decode()
    m = re.search(r'conv_igemm_persistent<([^>]*)>', rec)
    assert m, rec
    a = [s.strip() for s in m.group(1).split(',')]
    names = ['T', 'MODE', 'BM', 'BN', 'NW', 'STAGES', 'STATS', 'BNEPI', 'EXT', 'WIN', 'FAPPLY', 'SPL', 'TAIL', 'PSB', 'FAS', 'EPS', 'PSX']
    dflt = {'EXT': 'false', 'WIN': 'false', 'FAPPLY': 'false', 'SPL': '0', 'TAIL': 'false', 'PSB': 'false', 'FAS': '0', 'EPS': '0', 'PSX': 'false'}
    d = {n: (a[i] if i < len(a) else dflt[n]) for i, n in enumerate(names)}
    d['record'] = rec
    return d


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _assert(res):
    bad = [r for r in res if not r['ok']]
    for r in res:
        print('%-4s %-70s err=%.3e tol=%.3e' % ('ok' if r['ok'] else 'FAIL', r['name'], r['err'], r['tol']))
    assert not bad, bad


def _dgrad_bn_inputs(V, H, N, K, k, mode, acc, seed=0):
    """dy [V,H,H,K] in the pre-split block format, data-gradient weights [k,k,N,K] (dx has N channels), the producer BatchNorm of dx."""
    from simclr_amd import ops
    from tests import gpu_checks as gc
    DEV = gc.DEV
    g = torch.Generator(device=DEV).manual_seed(seed)
    rnd = lambda shape, sc=1.0: torch.randn(shape, device=DEV, generator=g) * sc
    dy = rnd((V, H, H, K))
    w = rnd((k, k, N, K), (k * k * N) ** -0.5)
    bn_x = rnd((V, H, H, N), 1.5) + 0.3
    mask_t = rnd((V, H, H, N))
    prev = rnd((V, H, H, N)) if acc else None
    bn = dict(x=bn_x, mask=None, scale=torch.rand(N, device=DEV, generator=g) - 0.4, shift=0.3 * rnd((N,)),
              mean=0.2 * rnd((N,)), rstd=0.5 + torch.rand(N, device=DEV, generator=g), mode=mode)
    if mode == 1:
        bn['mask'] = mask_t
    elif mode in (3, 4):        # one byte per 4 channels, bit e = element e (the layout simclr_bn_apply writes)
        mb = (mask_t > 0).reshape(-1, N // 4, 4).to(torch.int32)
        bn['mask'] = (mb << torch.arange(4, dtype=torch.int32, device=DEV)).sum(-1).to(torch.uint8)
    if mode == 4:               # sums-only epilogue: no BatchNorm input, no mean / rstd
        bn = dict(mask=bn['mask'], mode=4)
    dy_ps = gc.ps_encode(dy)
    return dict(dy=dy, dy_ps=dy_ps, w=w, w_d=ops.prep_weights(w, 1, F32), bn=bn, bn_x=bn_x, mask_t=mask_t, prev=prev)


def _run_dgrad_bn(inp, H, k, acc, sw):
    from simclr_amd import ops
    with switch(sw):
        out = inp['prev'].clone() if acc else None
        dm, part = ops.conv2d_dgrad_bn(inp['dy_ps'], inp['w_d'], k, k, (k - 1) // 2, H, H, inp['bn'], out=out, accumulate=bool(acc))
        args = last_args()
        sums = ops.bn_reduce_slots(part)
        torch.cuda.synchronize()
    return dm, part, sums, args


def _ref64_dgrad_bn(inp, V, H, N, K, k, mode, acc):
    """float64: dm = (dgrad(value of the pre-split dy) [+ prev]) * mask, sums = (sum dm, sum dm * x^) per channel."""
    from tests import gpu_checks as gc
    dyv = gc.ps_decode(inp['dy_ps'])[0]                          # exactly hi + lo, what the kernel multiplies
    w64 = inp['w'].double().cpu()
    if k == 1:
        da = (dyv.view(-1, K).to(gc.DEV) @ w64[0, 0].t().to(gc.DEV)).cpu().view(V, H, H, N)
    else:
        pad = (k - 1) // 2
        xr = torch.zeros(V, N, H, H, dtype=torch.float64, requires_grad=True)
        yr = F.conv2d(F.pad(xr, (pad, k - 1 - pad, pad, k - 1 - pad)), w64.permute(3, 2, 0, 1))
        yr.backward(dyv.permute(0, 3, 1, 2))
        da = xr.grad.permute(0, 2, 3, 1)
    if acc:
        da = da + inp['prev'].double().cpu()
    bn = inp['bn']
    clear = None
    if mode in (1, 3, 4):
        m = inp['mask_t'].cpu() > 0
    else:
        arg = torch.addcmul(bn['shift'], inp['bn_x'], bn['scale']).cpu()      # fp32 like the kernel (fused or not: `clear` covers it)
        m = arg > 0
        clear = arg.abs() > 1e-3 * (arg.abs().max() + 1e-9)
    dm_ref = torch.where(m, da, torch.zeros(1, dtype=torch.float64))
    s1 = dm_ref.sum((0, 1, 2))
    s2 = l2 = None
    if mode != 4:
        xh = (inp['bn_x'].double().cpu() - bn['mean'].double().cpu()) * bn['rstd'].double().cpu()
        s2 = (dm_ref * xh).sum((0, 1, 2))
        l2 = float((dm_ref * xh).abs().sum((0, 1, 2)).max())
    return dm_ref, clear, s1, s2, float(dm_ref.abs().sum((0, 1, 2)).max()), l2


# (V, H, N = channels of dx, K = channels of dy, k, mask mode, accumulate, expected BN of the tile, expected EPS with the switch on)
# EPS - 1 = 2 * (mode == 4) + accumulate; 0 = the launch keeps the per-fragment loop (csrc/conv.hip f32_eps_exists)
CASES = [
    # mask bits + accumulate, 1x1, 64-wide tile
    (8, 56, 256, 64, 1, 4, 1, 64, 4),       # 196 M-tiles x 4 N-tiles over a 768-workgroup grid: several tiles per workgroup
    (3, 9, 256, 64, 1, 4, 1, 64, 4),        # M = 243: partial last tile, masked rows
    (5, 28, 512, 128, 1, 4, 1, 64, 4),      # K = 128
    # mask bits + accumulate, 1x1, 128 x 128 tile (K = 256)
    (3, 9, 256, 256, 1, 4, 1, 128, 4),
    (11, 56, 256, 256, 1, 4, 1, 128, 4),    # 270 M-tiles x 2 N-tiles over 512 workgroups: several tiles per workgroup
    # mask mode 2, store, 1x1, 128 x 128 tile
    (3, 9, 128, 256, 1, 2, 0, 128, 1),
    (11, 56, 256, 256, 1, 2, 0, 128, 1),    # several tiles per workgroup
    # mask mode 2, store, 1x1, 64-wide gathered tile (the narrow-tile rule takes K <= 128)
    (21, 56, 128, 64, 1, 2, 0, 64, 1),      # 515 M-tiles x 2 N-tiles over 768 workgroups: several tiles per workgroup
    (3, 9, 128, 64, 1, 2, 0, 64, 1),
    # launches that keep the per-fragment loop under either switch value
    (21, 56, 128, 64, 1, 2, 1, 64, 0),      # mode 2 + accumulate (64-wide tile, 515 M-tiles)
    (3, 9, 128, 64, 1, 2, 1, 64, 0),
    (3, 9, 128, 256, 1, 2, 1, 128, 0),      # mode 2 + accumulate
    (3, 9, 256, 256, 1, 4, 0, 128, 0),      # mask-bit store
    (2, 7, 64, 64, 3, 2, 0, 64, 0),         # 3x3 halo window, 64-wide tile, image borders in every tile
    (2, 14, 128, 64, 3, 2, 0, 128, 0),      # 128-wide halo window
    (2, 14, 128, 64, 3, 2, 1, 128, 0),
    (2, 7, 64, 64, 3, 2, 1, 64, 0),         # 64-wide halo window, accumulate
    (2, 7, 64, 64, 3, 4, 1, 64, 0),         # halo window, mask bits
]


@pytest.mark.parametrize('V,H,N,K,k,mode,acc,bn_tile,eps', CASES)
def test_batched_reduce_epilogue_same_bits_as_generic(V, H, N, K, k, mode, acc, bn_tile, eps):
    from tests import gpu_checks as gc
    with matmul('f16x3_3'):
        inp = _dgrad_bn_inputs(V, H, N, K, k, mode, acc)
        dm0, part0, sums0, a0 = _run_dgrad_bn(inp, H, k, acc, 0)
        dm1, part1, sums1, a1 = _run_dgrad_bn(inp, H, k, acc, 1)
    assert eps in (0, 1 + (2 if mode == 4 else 0) + acc)
    assert a0['EPS'] == '0' and a0['PSX'] == 'true', a0['record']
    assert a1['EPS'] == str(eps) and a1['PSX'] == 'true' and a1['BN'] == a0['BN'] == str(bn_tile), a1['record']
    assert a1['WIN'] == a0['WIN'] == ('true' if k == 3 else 'false'), a1['record']
    assert same_bits(dm0, dm1), 'dm: %d elements differ' % int((dm0.view(torch.int32) != dm1.view(torch.int32)).sum())
    dp = part0.view(torch.int32) != part1.view(torch.int32)
    assert not bool(dp.any()), 'partial sums differ: %d of sum(dm), %d of sum(dm * x^), max |diff| %.3e' % (
        int(dp[:, 0].sum()), int(dp[:, 1].sum()), float((part0 - part1).abs().max()))
    # the batched result against float64
    dm_ref, clear, s1, s2, l1, l2 = _ref64_dgrad_bn(inp, V, H, N, K, k, mode, acc)
    got = dm1.double().cpu()
    if clear is not None:       # elements whose fp32 mask argument is within rounding of 0 may legitimately flip
        got = torch.where(clear, got, dm_ref)
    tag = 'V%d %dx%d %d<-%d k%d mode%d acc%d' % (V, H, H, N, K, k, mode, acc)
    res = [gc._res('f32epi_dm ' + tag, got, dm_ref, 2 * gc._tol(F32) * (2 if acc else 1)),
           gc._res('f32epi_sum ' + tag, sums1[0], s1, 1e-4, 1e-3 * l1)]
    if mode != 4:
        res.append(gc._res('f32epi_sumxhat ' + tag, sums1[1], s2, 1e-4, 1e-3 * l2))
    _assert(res)


@pytest.mark.parametrize('V,H,N,K,k,mode,acc', [(3, 8, 256, 64, 1, 1, 1), (3, 8, 256, 64, 1, 3, 1)])
def test_other_mask_modes_keep_the_generic_epilogue(V, H, N, K, k, mode, acc):
    with matmul('f16x3_3'):
        inp = _dgrad_bn_inputs(V, H, N, K, k, mode, acc)
        dm0, part0, _, a0 = _run_dgrad_bn(inp, H, k, acc, 0)
        dm1, part1, _, a1 = _run_dgrad_bn(inp, H, k, acc, 1)
    assert a0['EPS'] == '0' and a1['EPS'] == '0' and a0['record'] == a1['record'], (a0['record'], a1['record'])
    assert same_bits(dm0, dm1) and same_bits(part0, part1)


@pytest.mark.parametrize('V,H,Cin,Cout,k,mode,acc', [(3, 9, 256, 64, 1, 4, 1), (3, 9, 128, 64, 1, 2, 0), (2, 14, 128, 64, 3, 2, 1)])
def test_dgrad_bn_check_with_the_switch_on(V, H, Cin, Cout, k, mode, acc):
    """gpu_checks.check_dgrad_bn as it stands (exact fp32 products, plain dy: the per-fragment loop) is not disturbed by the switch."""
    from tests import gpu_checks as gc
    with switch(1):
        _assert(gc.check_dgrad_bn(V, H, Cin, Cout, k, F32, mode, acc))


@pytest.mark.parametrize('V,H,Cs,Cin,Cmid,mode', [(4, 28, 512, 256, 128, 4), (2, 30, 128, 64, 64, 0)])
def test_sparse_accumulate_keeps_the_generic_epilogue(V, H, Cs, Cin, Cmid, mode):
    """accumulate = 2 / 3 (stride-2 shortcut without zero fill) are not specialised: the check passes with the switch on."""
    from tests import gpu_checks as gc
    with switch(1):
        _assert(gc.check_sparse_dgrad(V, H, Cs, Cin, Cmid, mode, matmul='f16x3_3'))


def test_k_extended_reduce_keeps_the_generic_epilogue(V=4, H=14, K=64, N=256):
    """simclr_conv2d_dgrad_bn_ext (BatchNorm backward folded into the producing 1x1 convolution): dm [V,H,H,N], h [V,H,H,K].  Not
    specialised: the same instantiation and bits under either switch value, and the float64 gates of check_bn_fold with the switch on."""
    from simclr_amd import ops
    from tests import gpu_checks as gc
    DEV = gc.DEV
    g = torch.Generator(device=DEV).manual_seed(0)
    rnd = lambda shape, sc=1.0, sh=0.0: torch.randn(shape, device=DEV, generator=g) * sc + sh
    M = V * H * H
    h = torch.relu(rnd((V, H, H, K), 1.0, 0.4))
    dm = rnd((V, H, H, N))
    w = rnd((K, N), K ** -0.5)
    a = 0.5 + torch.rand(N, device=DEV, generator=g)
    b = 0.05 * rnd((N,))
    d = 0.1 * rnd((N,))
    bn_x = rnd((V, H, H, K), 1.5, 0.3)
    bn = dict(x=bn_x, mask=None, scale=torch.rand(K, device=DEV, generator=g) - 0.4, shift=0.3 * rnd((K,)), mean=0.2 * rnd((K,)),
              rstd=0.5 + torch.rand(K, device=DEV, generator=g), mode=2)
    bmean = 0.3 * rnd((N,))
    c2v = -b / a
    c1v = c2v * bmean - d / a
    a, b, d, wb, wext, e = ops.bn_fold_pre(w, a, bmean, torch.ones(N, device=DEV), c1v, c2v)
    # the sequence of Conv2dFixedPadding.backward_folded (as gpu_checks.check_bn_fold): bn_fold_post completes the K-extended weights
    q = ops.small_gemm_nt(wb, w)
    t1 = ops.conv2d_wgrad(h, dm, 1, 1, 1, 0)
    gm, cs = ops.conv2d_gram(h)
    gw = ops.small_gemm_nt(gm, w.t().contiguous())
    ops.bn_fold_post(t1, gw, cs, a, b, d, q, torch.empty(K, N, device=DEV), wext)
    runs = []
    with matmul('f16x3_3'):
        for sw in (0, 1):
            with switch(sw):
                dmi, part = ops.conv2d_dgrad_bn_ext(dm, h, wext, e, bn)
                runs.append((dmi, part, ops.bn_reduce_slots(part), last_args()))
                torch.cuda.synchronize()
    (dm0, part0, _, a0), (dm1, part1, sums1, a1) = runs
    assert a0['EXT'] == a1['EXT'] == 'true' and a0['EPS'] == a1['EPS'] == '0' and a0['record'] == a1['record'], (a0['record'], a1['record'])
    assert same_bits(dm0, dm1) and same_bits(part0, part1)
    h64, dm64, w64 = h.double().view(M, K), dm.double().view(M, N), w.double()
    dh = a.double() * dm64 + b.double() * (h64 @ w64) + d.double()
    dx = dh @ w64.t()
    arg = torch.addcmul(bn['shift'], bn_x, bn['scale']).view(M, K)
    clear = arg.abs() > 1e-3 * (arg.abs().max() + 1e-9)
    ref = torch.where(arg > 0, dx, torch.zeros((), device=DEV, dtype=torch.float64))
    xh = (bn_x.double().view(M, K) - bn['mean'].double()) * bn['rstd'].double()
    l1 = float((ref.abs().sum(0) + (ref * xh).abs().sum(0)).max())
    got = torch.where(clear, dm1.double().view(M, K), ref)
    _assert([gc._res('f32epi_ext_dm', got, ref, 2e-4), gc._res('f32epi_ext_sum', sums1[0], ref.sum(0), 0, 1e-4 * l1),
             gc._res('f32epi_ext_sumxhat', sums1[1], (ref * xh).sum(0), 0, 1e-4 * l1)])
