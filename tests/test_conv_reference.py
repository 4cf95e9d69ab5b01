"""CPU tests that go with tests/test_gpu_conv_lattice.py: the references and the lattice of tests/conv_reference.py pinned without a GPU,
and the kernel family every row of the case table reaches, asserted in a dry run of the library (SIMCLR_DRY_RUN=1: plan_igemm /
plan_wgrad take every decision, nothing is launched), so that a selection rule that later moves a row off its path fails here and not
silently on the GPU."""
import itertools
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from tests import conv_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64

GROUPS = sorted({c.id.split('_')[0] for c in R.CASES})


@pytest.mark.parametrize('group', GROUPS)
def test_conditions_hold_for_every_row(group):
    """conv_reference.reference asserts them: float32 == float64 evaluation (statistics in a random row order too), storage survival
    (bf16, fp16 pieces of 2^8 w, the pre-split block format through gpu_checks.ps_encode / ps_decode), |y|, |dx|, |dm| integers <= 256
    outside the designated rounding rows, order-dependent partial sums below 2^24, and the non-degeneracy floors."""
    rows = [c for c in R.CASES if c.id.split('_')[0] == group]
    assert rows
    for c in rows:
        L, want = R.reference(c)
        assert want['out'].dtype == F64 and bool(torch.isfinite(want['out']).all())
        if c.stats:
            assert 's1' in want and (c.op == 'dgrad_bn' and c.mode == 4) != ('s2' in want)


def test_designated_rounding_rows_round():
    """Their outputs exceed 8 significant bits, the statistics of the exact accumulators differ from those of the rounded outputs, and y
    is the exact value rounded once."""
    acc, rnd = R.CASE_BY_ID['round_acc_tile128'], R.CASE_BY_ID['round_rounded_tile256']
    (La, wa), (Lr, wr) = R.reference(acc), R.reference(rnd)
    for L, w, c in ((La, wa, acc), (Lr, wr, rnd)):
        exact = R.conv_fwd_ref(L['x'], L['w'], c.k, c.s)
        assert torch.equal(w['out'], R.round_to(exact, torch.bfloat16)) and not torch.equal(w['out'], exact)
        assert float(exact.abs().max()) > 256
        s_exact, s_round = R.channel_sums(exact), R.channel_sums(w['out'])
        assert not torch.equal(s_exact[0], s_round[0]) and not torch.equal(s_exact[1], s_round[1])
        pick = s_exact if c.dense == 'acc' else s_round
        assert torch.equal(w['s1'], pick[0]) and torch.equal(w['s2'], pick[1])


SHAPES = [(2, 5, 9, 3, 4, 1, 1), (2, 9, 5, 3, 4, 3, 1), (1, 7, 10, 2, 3, 3, 2), (2, 10, 7, 3, 2, 1, 2), (3, 1, 7, 2, 2, 3, 1), (1, 7, 1, 2, 2, 3, 1),
          (2, 6, 10, 4, 3, 3, 2), (1, 1, 1, 3, 2, 3, 1)]


@pytest.mark.parametrize('V,H,W,Cin,Cout,k,s', SHAPES)
def test_explicit_tap_forward_equals_conv2d(V, H, W, Cin, Cout, k, s):
    """Conv2dFixedPadding: k - 1 explicit zeros ((k - 1) // 2 before), then a VALID F.conv2d."""
    g = torch.Generator().manual_seed(V * 100 + H)
    x = torch.randn(V, H, W, Cin, generator=g, dtype=F64)
    w = torch.randn(k, k, Cin, Cout, generator=g, dtype=F64)
    pad = (k - 1) // 2
    pe = (k - 1) - pad
    y = F.conv2d(F.pad(x.permute(0, 3, 1, 2), (pad, pe, pad, pe)), w.permute(3, 2, 0, 1), stride=s).permute(0, 2, 3, 1)
    got = R.conv_fwd_ref(x, w, k, s)
    assert tuple(got.shape) == (V,) + R.out_hw(H, W, k, s) + (Cout,) == tuple(y.shape)
    assert float((got - y).abs().max()) <= 1e-12 * float(y.abs().max())


@pytest.mark.parametrize('V,H,W,Cin,Cout,k,s', [(2, 5, 5, 3, 4, 3, 1), (2, 7, 10, 3, 2, 3, 2), (3, 4, 6, 2, 5, 1, 1)])
def test_dx_and_dw_equal_autograd_of_the_forward(V, H, W, Cin, Cout, k, s):
    g = torch.Generator().manual_seed(k * 10 + s)
    x = torch.randn(V, H, W, Cin, generator=g, dtype=F64).requires_grad_(True)
    w = torch.randn(k, k, Cin, Cout, generator=g, dtype=F64).requires_grad_(True)
    OH, OW = R.out_hw(H, W, k, s)
    dy = torch.randn(V, OH, OW, Cout, generator=g, dtype=F64)
    R.conv_fwd_ref(x, w, k, s).backward(dy)
    dx = R.conv_dgrad_ref(dy, w.detach(), k, s, H, W)
    dw = R.conv_wgrad_ref(x.detach(), dy, k, s)
    assert float((dx - x.grad).abs().max()) <= 1e-12 * float(x.grad.abs().max())
    assert float((dw - w.grad).abs().max()) <= 1e-12 * float(w.grad.abs().max())


def test_hand_written_1x1_and_3x3_examples():
    # 1x1: two pixels x two input channels -> three output channels
    x = torch.tensor([[1., 2.], [-1., 0.]], dtype=F64).view(1, 1, 2, 2)
    w = torch.tensor([[1., 0., -1.], [2., 1., 0.]], dtype=F64).view(1, 1, 2, 3)
    y = R.conv_fwd_ref(x, w, 1, 1)
    assert y.view(2, 3).tolist() == [[5., 2., -1.], [-1., 0., 1.]]
    dy = torch.tensor([[1., 0., 2.], [0., -1., 1.]], dtype=F64).view(1, 1, 2, 3)
    assert R.conv_dgrad_ref(dy, w, 1, 1, 1, 2).view(2, 2).tolist() == [[-1., 2.], [-1., -1.]]
    assert R.conv_wgrad_ref(x, dy, 1, 1).view(2, 3).tolist() == [[1., 1., 1.], [2., 0., 4.]]
    s1, s2 = R.channel_sums(y)
    assert s1.tolist() == [4., 2., 0.] and s2.tolist() == [26., 4., 2.]
    # 3x3 on a 2 x 3 map, one channel, w = tap index + 1 (row-major): y(oy, ox) = sum over in-bounds taps of x(oy + ty - 1, ox + tx - 1) w(ty, tx)
    x = torch.tensor([[1., 2., 3.], [4., 5., 6.]], dtype=F64).view(1, 2, 3, 1)
    w = torch.arange(1., 10., dtype=F64).view(3, 3, 1, 1)
    # y(0,0) = 1*5 + 2*6 + 4*8 + 5*9 = 94;  y(0,1) = 1*4 + 2*5 + 3*6 + 4*7 + 5*8 + 6*9 = 154;  y(0,2) = 2*4 + 3*5 + 5*7 + 6*8 = 106
    # y(1,0) = 1*2 + 2*3 + 4*5 + 5*6 = 58;  y(1,1) = 1*1 + 2*2 + 3*3 + 4*4 + 5*5 + 6*6 = 91;   y(1,2) = 2*1 + 3*2 + 5*4 + 6*5 = 58
    assert R.conv_fwd_ref(x, w, 3, 1).view(2, 3).tolist() == [[94., 154., 106.], [58., 91., 58.]]
    # stride 2 on the same map: one output row, columns 0 and 2
    assert R.conv_fwd_ref(x, w, 3, 2).view(1, 2).tolist() == [[94., 106.]]
    # dgrad of a single 1 at output pixel (0, 1): the flipped window lands on the map
    dy = torch.zeros(1, 2, 3, 1, dtype=F64)
    dy[0, 0, 1, 0] = 1.0
    assert R.conv_dgrad_ref(dy, w, 3, 1, 2, 3).view(2, 3).tolist() == [[4., 5., 6.], [7., 8., 9.]]
    # dw of the same dy: tap (ty, tx) reads x(0 + ty - 1, 1 + tx - 1)
    assert R.conv_wgrad_ref(x, dy, 3, 1).view(3, 3).tolist() == [[0., 0., 0.], [1., 2., 3.], [4., 5., 6.]]
    # pivot pixel of the pivoted statistics: (0, OH / 2, OW / 2)
    c = R.make_case('pivot_example', 'fwd_pivoted', 'exact', 1, 2, 3, 32, 4, k=3)
    yy = torch.arange(24., dtype=F64).view(1, 2, 3, 4)
    assert R.pivot_of(c, yy).tolist() == yy[0, 1, 1].tolist()
    assert R.pack_bits(torch.tensor([[True, False, False, True, False, False, False, True]]), 4).tolist() == [[9, 8]]


def test_grid_mirrors_and_multi_tile_rows():
    """persistent_grid / wide_grid restate igemm_persistent_grid and the 256-row grid of plan_igemm; the library's own numbers are asserted
    against them where the ABI exposes them (simclr_conv2d_stats_slots = workgroups per N-tile)."""
    from simclr_amd import _lib
    L = _lib.lib()
    for M, N in itertools.product((1, 127, 128, 129, 1025, 8192, 65536, 65537, 98400, 200000), (4, 64, 68, 128, 192, 320, 1024, 8192)):
        BN, nt, pg = R.persistent_grid(M, N)
        assert L.conv2d_stats_slots(M, N) == pg // nt, (M, N)
    assert R.rows_for_tiles(9, 128) == 1025 and R.rows_for_tiles(9, 256) == 2049 and R.rows_for_tiles(769, 64) == 49153
    for M, (V, H, W) in R.ROWS.items():
        assert V * H * W == M and (H != W or M == 1)


def _mutants(c, L, want):
    """(name, changed?) for the three mutations of the issue, applied to the reference: one row dropped from the statistics, IH and IW
    swapped, one mask bit flipped.  A GPU result that equals the unmutated reference differs from every mutant that changed."""
    out = []
    rows_out = want['out'].reshape(-1, want['out'].shape[-1])
    if c.stats and 's1' in want:
        src = R.conv_fwd_ref(L['x'], L['w'], c.k, c.s).reshape(rows_out.shape) if c.dense == 'acc' else rows_out
        r = int(src.abs().sum(1).nonzero()[0])
        keep = torch.ones(src.shape[0], dtype=torch.bool)
        keep[r] = False
        s1, s2 = R.channel_sums(src[keep])
        if c.op == 'dgrad_bn':
            changed = not torch.equal(s1, want['s1'])
        else:
            changed = not torch.equal(s2, want['s2'])
        out.append(('row dropped', changed))
    if c.H != c.W and c.dense is None:
        import copy
        m = copy.copy(c)
        m.H, m.W = c.W, c.H
        m.OH, m.OW = R.out_hw(m.H, m.W, c.k, c.s)
        Lm = dict(L)
        for n in ('x', 'prev', 'bnx', 'msk'):
            if n in Lm and Lm[n].dim() == 4:
                Lm[n] = Lm[n].reshape(c.V, m.H, m.W, -1)
        for n in ('dy', 'res'):
            if n in Lm:
                Lm[n] = Lm[n].reshape(c.V, m.OH, m.OW, -1)
        o = R._main_output(m, Lm)
        same_shape = o.numel() == want['out'].numel()
        if c.op == 'fwd_bn_apply' and same_shape:
            o = R.round_to(R.fwd_bn_apply_ref(m, Lm, o), c.dtype)
        out.append(('IH / IW swapped', (not same_shape) or not torch.equal(o.reshape(-1), want['out'].reshape(-1))))
    if c.op == 'dgrad_bn':
        dx = R.dgrad_of(c, L)
        if c.adds:
            dx = dx + L['prev']
        idx = tuple(dx.nonzero()[0].tolist())
        mask = R.mask_of(c, L).clone()
        mask[idx] = ~mask[idx]
        dm = dx * mask.double()
        out.append(('mask bit flipped', not torch.equal(dm, want['out']) and not torch.equal(dm.reshape(-1, c.Cin).sum(0), want['s1'])))
    return out


@pytest.mark.parametrize('group', GROUPS)
def test_references_notice_the_three_mutations(group):
    """The evidence that the GPU comparisons would notice a subtly wrong kernel: every statistics reference changes when one row is dropped
    and when one mask bit is flipped; every output reference of a 3x3 or strided row changes when IH and IW are swapped.  (A 1x1 stride-1
    convolution reads and writes the same flat rows whichever way H and W are named: there the swap changes nothing, rightly.)"""
    for c in [c for c in R.CASES if c.id.split('_')[0] == group]:
        if c.V * c.H * c.W * max(c.Cin, c.Cout) > 2 ** 21:
            continue
        L, want = R.reference(c, check_ps=False)
        for name, changed in _mutants(c, L, want):
            if name == 'IH / IW swapped' and c.k == 1 and c.s == 1:
                assert not changed, (c.id, name)
            elif name == 'IH / IW swapped' and min(c.H, c.W) == 1 and c.k == 1:
                continue                                   # (a strided 1x1 on a one-pixel-wide map: nothing to tell apart)
            else:
                assert changed, (c.id, name)


_DRY_RUN = r'''
import ctypes, os, sys
from simclr_amd import _lib
from tests import conv_reference as R
L = _lib.lib()
FAKE = ctypes.c_void_p(1 << 20)          # never dereferenced in a dry run
P = {n: FAKE for n in R.POINTERS}
for c in R.CASES:
    for k in [k for k in os.environ if k.startswith('SIMCLR_') and k != 'SIMCLR_DRY_RUN']:
        del os.environ[k]
    os.environ.update(c.env)
    dgrad = c.op in ('dgrad', 'dgrad_bn')
    own = L.conv2d_stats_slots(c.V * (c.H * c.W if dgrad else c.OH * c.OW), c.Cin if dgrad else c.Cout)
    R.launch(L, c, P, nslot=own + 5)
    print('%s\t%s' % (c.id, L.conv2d_last_instantiation().decode()))
print('ok')
'''


def test_every_row_reaches_the_family_it_claims():
    """The whole case table through the library with SIMCLR_DRY_RUN=1, each row under its own SIMCLR_* switches and with fake pointers
    that are never dereferenced: the recorded instantiation names the kernel, the template arguments (BN, WIN, TAIL, EPS, FAS, PSX, ...),
    the split-tail parts / slab count and the tile ownership the row claims, and the families reached contain every family the GPU module
    is required to cover."""
    env = {k: v for k, v in os.environ.items() if not k.startswith('SIMCLR_')}
    env.update(SIMCLR_DRY_RUN='1')
    r = subprocess.run([sys.executable, '-c', _DRY_RUN], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and lines[-1] == 'ok', r.stdout[-2000:] + r.stderr[-2000:]
    recs = dict(l.split('\t', 1) for l in lines[:-1])
    assert set(recs) == set(R.CASE_BY_ID)
    reached = set()
    for c in R.CASES:
        reached |= R.check_record(c, recs[c.id])
    missing = [t for t in R.REQUIRED if t not in reached]
    assert not missing, missing
    # the arithmetics, per family that accepts them
    for ar in R.ARITH:
        ops_ = {c.op for c in R.CASES if c.arith == ar}
        assert {'fwd', 'dgrad', 'dgrad_bn', 'wgrad', 'fwd_bn_apply'} <= ops_, (ar, ops_)
