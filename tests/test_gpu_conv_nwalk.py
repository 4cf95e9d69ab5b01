"""The N-inner walk of the persistent implicit GEMM (csrc/igemm_nwalk.h, conv_igemm_nwalk): on the short-K 1x1 fused bottleneck tails in
fp32 storage a workgroup owns an M-tile and walks a group of its N-tiles with the activation panel resident in LDS, instead of owning
an N-tile and walking M-tiles (conv_igemm_persistent).  The k-step order and the MFMA order per output element are unchanged, so every
case runs the same call on the same inputs with SIMCLR_IGEMM_NWALK at 0 and at 1 and asks for the same BITS (output and ReLU bit mask),
checks in the instantiation record which walk each run took and how the plan split the work, and compares the result with the unfused
conv -> bn_apply path (bitwise: the gate of test_conv_fused_bn_apply_tail_f32) and with float64.

float64 gate of the output: the reference is relu(c * scale + shift + r) in float64 from the stored fp32 convolution output c (as
gpu_checks.check_conv_fwd_bn_apply takes it from the stored bf16 one), so the only error is the epilogue's own fp32 rounding: two fused
multiply-adds, one addition -- at most 3 half-ulps of the largest intermediate, which the sum of the terms' magnitudes bounds by a
few times max|ref|: 2^-21 max|ref| (8 half-ulps).

The data gradient with the fused BatchNorm-backward reduce has no N-inner instantiation (its per-slot partial sums are pinned bit for
bit by tests/test_gpu_conv_f32_epilogue.py, which an N-inner walk reorders): it is in the fallback list with every other launch that
keeps the M-inner walk under either switch value."""
import contextlib
import os
import re

import pytest
import torch

from tests.test_gpu_conv_f32_epilogue import F32, _dgrad_bn_inputs, _run_dgrad_bn, last_args, matmul, same_bits

pytestmark = pytest.mark.gpu

SWITCH = 'SIMCLR_IGEMM_NWALK'


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


def record():
    from simclr_amd._lib import lib
    return lib().conv2d_last_instantiation().decode()


def field(rec, name):
    m = re.search(r' %s=(\d+)' % name, rec)
    assert m, (name, rec)
    return int(m.group(1))


def _tail_inputs(V, H, K, N, res_bn, k=1, seed=0):
    """x [V,H,H,K], weights K -> N, residual, and the BatchNorm scale / shift from the statistics of the unfused convolution c."""
    from simclr_amd import ops
    from tests import gpu_checks as gc
    DEV = gc.DEV
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(V, H, H, K, device=DEV, generator=g)
    w = torch.randn(k, k, K, N, device=DEV, generator=g) * (k * k * K) ** -0.5
    res = torch.randn(V, H, H, N, device=DEV, generator=g)
    gamma = torch.rand(N, device=DEV, generator=g) + 0.5
    beta = 0.2 * torch.randn(N, device=DEV, generator=g)
    rs = (torch.rand(N, device=DEV, generator=g) + 0.5) if res_bn else None
    rb = (0.3 * torch.randn(N, device=DEV, generator=g)) if res_bn else None
    w_t = ops.prep_weights(w, 0, F32)
    M = V * H * H
    st = ops.conv_stats(M, N, DEV)
    c = ops.conv2d_fwd(x, w_t, k, k, 1, (k - 1) // 2, H, H, stats=st)
    mm, mv = torch.zeros(N, device=DEV), torch.ones(N, device=DEV)
    _, _, scale, shift = ops.bn_finalize(None, M, gamma, beta, mm, mv, 0.9, partial=st)
    return dict(x=x, w_t=w_t, res=res, rs=rs, rb=rb, c=c, scale=scale, shift=shift, k=k)


def _run_tail(inp, H, sw):
    from simclr_amd import ops
    k = inp['k']
    with switch(sw):
        y, bits = ops.conv2d_fwd_bn_apply(inp['x'], inp['w_t'], k, k, 1, (k - 1) // 2, H, H, inp['scale'], inp['shift'], res=inp['res'],
                                          relu=True, want_bits=True, rscale=inp['rs'], rshift=inp['rb'])
        rec = record()
        torch.cuda.synchronize()
    return y, bits, rec


# (V, H, K, N, what the recorded plan must show)
TAILS = [
    (2, 7, 64, 256, 'one_tile'),         # M = 98: less than one full M-tile of the M-inner walk, a ragged second 64-row tile here
    (2, 9, 128, 512, 'ragged'),          # M = 162: ragged last M-tile, K = 128 (four k-blocks), eight N-tiles
    (32, 56, 64, 256, 'three_items'),    # 1568 M-tiles over 768 workgroups: some workgroup walks three M-tiles (x 4 N-tiles each)
    (5, 7, 128, 512, 'groups'),          # 7^2-like: 4 M-tiles, N = 512 split into more than one group
    (10, 56, 64, 256, 'groups_items'),   # 490 M-tiles: N split AND several M-tiles per workgroup
]


@pytest.mark.parametrize('res_bn', [False, True])
@pytest.mark.parametrize('V,H,K,N,plan', TAILS)
def test_fused_tail_same_bits_under_either_walk(V, H, K, N, plan, res_bn):
    from simclr_amd import ops
    with matmul('f16x3_3'):
        inp = _tail_inputs(V, H, K, N, res_bn)
        y0, b0, r0 = _run_tail(inp, H, 0)
        y1, b1, r1 = _run_tail(inp, H, 1)
        y_ref, b_ref = ops.bn_apply(inp['c'], inp['scale'], inp['shift'], True, res=inp['res'], rscale=inp['rs'], rshift=inp['rb'], want_bits=True)
        torch.cuda.synchronize()
    # which walk ran, and the recorded plan
    assert 'conv_igemm_persistent<float, MODE_FWD, 128, 128' in r0 and 'nwalk' not in r0, r0
    assert r1.startswith('(conv_igemm_nwalk<%d, %d>)' % (K // 32, 2 if res_bn else 1)) and ' walk=n_inner ' in r1, r1
    grid, m_tiles, groups, gw = field(r1, 'grid'), field(r1, 'm_tiles'), field(r1, 'n_groups'), field(r1, 'n_group')
    M = V * H * H
    assert m_tiles == (M + 63) // 64 and groups * gw == N and gw % 64 == 0 and grid % (8 * groups) == 0, r1
    items = -(-m_tiles // (grid // groups)) * (gw // 64)          # (M-tile, N-tile) work items of the busiest workgroup
    if plan in ('one_tile', 'ragged'):
        assert M % 64 != 0
    if plan in ('three_items', 'groups_items'):
        assert -(-m_tiles // (grid // groups)) >= 3 and items >= 3, r1
    if plan == 'three_items':
        assert groups == 1, r1
    if plan in ('groups', 'groups_items'):
        assert groups > 1, r1
    # the same bits under either walk, and those of the unfused path
    assert same_bits(y0, y1), 'y: %d elements differ' % int((y0.view(torch.int32) != y1.view(torch.int32)).sum())
    assert torch.equal(b0, b1), 'ReLU bits: %d bytes differ' % int((b0 != b1).sum())
    assert same_bits(y1, y_ref) and torch.equal(b1.reshape(-1), b_ref.reshape(-1))
    # float64 (module docstring)
    rterm = inp['res'].double() * inp['rs'].double() + inp['rb'].double() if res_bn else inp['res'].double()
    ref = (inp['c'].double() * inp['scale'].double() + inp['shift'].double() + rterm).clamp_min(0.0)
    err, sc = float((y1.double() - ref).abs().max()), float(ref.abs().max())
    print('fused tail V%d %dx%d %d->%d resbn%d: err %.3e tol %.3e  %s' % (V, H, H, K, N, res_bn, err, 2.0 ** -21 * sc, r1))
    assert err <= 2.0 ** -21 * sc
    assert torch.equal(b1.reshape(M, N // 4).to(torch.int32),
                       ((y1.reshape(M, N // 4, 4) > 0).to(torch.int32) << torch.arange(4, dtype=torch.int32, device=y1.device)).sum(-1))


@pytest.mark.parametrize('V,H,K,N,k,why', [
    (2, 7, 256, 512, 1, 'IC = 256'),
    (2, 7, 64, 256, 3, '3x3'),
    (2, 7, 64, 96, 1, 'Cout = 96'),
    (2, 7, 64, 128, 1, 'one N-tile of the M-inner walk'),
])
def test_other_fused_tails_keep_the_m_inner_walk(V, H, K, N, k, why):
    with matmul('f16x3_3'):
        inp = _tail_inputs(V, H, K, N, False, k=k)
        y0, b0, r0 = _run_tail(inp, H, 0)
        y1, b1, r1 = _run_tail(inp, H, 1)
    assert r0 == r1 and 'conv_igemm_persistent<' in r0 and 'nwalk' not in r0, (why, r0, r1)
    assert same_bits(y0, y1) and torch.equal(b0, b1)


def test_statistics_forward_keeps_the_m_inner_walk(V=2, H=9, K=64, N=256):
    from simclr_amd import ops
    from tests import gpu_checks as gc
    recs = []
    with matmul('f16x3_3'):
        x = torch.randn(V, H, H, K, device=gc.DEV)
        w_t = ops.prep_weights(torch.randn(1, 1, K, N, device=gc.DEV) * K ** -0.5, 0, F32)
        for sw in (0, 1):
            with switch(sw):
                ops.conv2d_fwd(x, w_t, 1, 1, 1, 0, H, H, stats=ops.conv_stats(V * H * H, N, gc.DEV))
                recs.append(record())
                torch.cuda.synchronize()
    assert recs[0] == recs[1] and 'conv_igemm_persistent<' in recs[0], recs


@pytest.mark.parametrize('V,H,N,K,mode,acc', [(2, 7, 256, 64, 4, 1), (2, 9, 512, 128, 2, 0), (10, 56, 256, 64, 4, 1), (5, 7, 512, 128, 2, 0)])
def test_dgrad_bn_keeps_the_m_inner_walk(V, H, N, K, mode, acc):
    """The fused tail's geometries through the data gradient + BatchNorm-backward reduce on a pre-split dy (mode 2 store, mode 4 +
    accumulate): the same instantiation, gradient bits and per-slot sums under either switch value."""
    with matmul('f16x3_3'):
        inp = _dgrad_bn_inputs(V, H, N, K, 1, mode, acc)
        with switch(0):
            dm0, part0, _, a0 = _run_dgrad_bn(inp, H, 1, acc, 1)
        with switch(1):
            dm1, part1, _, a1 = _run_dgrad_bn(inp, H, 1, acc, 1)
    assert a0['record'] == a1['record'] and a1['PSX'] == 'true' and a1['EPS'] == str(1 + (2 if mode == 4 else 0) + acc), (a0['record'], a1['record'])
    assert same_bits(dm0, dm1) and same_bits(part0, part1)


def test_k_extended_launch_keeps_the_m_inner_walk(V=4, H=14, K=64, N=256):
    """simclr_conv2d_dgrad_bn_ext with the operands of tests/test_gpu_conv_f32_epilogue.py's K-extended case."""
    from simclr_amd import ops
    from tests import gpu_checks as gc
    DEV = gc.DEV
    g = torch.Generator(device=DEV).manual_seed(0)
    rnd = lambda shape, sc=1.0, sh=0.0: torch.randn(shape, device=DEV, generator=g) * sc + sh
    h = torch.relu(rnd((V, H, H, K), 1.0, 0.4))
    dm = rnd((V, H, H, N))
    w = rnd((K, N), K ** -0.5)
    a = 0.5 + torch.rand(N, device=DEV, generator=g)
    b = 0.05 * rnd((N,))
    d = 0.1 * rnd((N,))
    bn = dict(x=rnd((V, H, H, K), 1.5, 0.3), mask=None, scale=torch.rand(K, device=DEV, generator=g) - 0.4, shift=0.3 * rnd((K,)),
              mean=0.2 * rnd((K,)), rstd=0.5 + torch.rand(K, device=DEV, generator=g), mode=2)
    bmean = 0.3 * rnd((N,))
    c2v = -b / a
    a, b, d, wb, wext, e = ops.bn_fold_pre(w, a, bmean, torch.ones(N, device=DEV), c2v * bmean - d / a, c2v)
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
                runs.append((dmi, part, last_args()))
                torch.cuda.synchronize()
    (dm0, part0, a0), (dm1, part1, a1) = runs
    assert a0['EXT'] == a1['EXT'] == 'true' and a0['record'] == a1['record'], (a0['record'], a1['record'])
    assert same_bits(dm0, dm1) and same_bits(part0, part1)
