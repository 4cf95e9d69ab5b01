"""CPU tests that go with tests/test_gpu_stem_gram_lattice.py and with the `ext` / `sparse` rows of tests/test_gpu_conv_lattice.py: the
references and exactness conditions of tests/stem_gram_reference.py without a GPU, the stem forward's instantiation rule pinned, the
recorded weight-gradient / pre-split / Gram launches of every row asserted in a dry run of the library (SIMCLR_DRY_RUN=1), and one
mutation per row group fed to the comparison the GPU checks use (gpu_checks._bitwise): a perturbed reference must fail it."""
import copy
import os
import subprocess
import sys

import pytest
import torch

from tests import conv_reference as R
from tests import stem_gram_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def _lib():
    from simclr_amd import _lib
    return _lib.lib()


STEM_GROUPS = sorted({c.id.split('_')[1] for c in S.STEM_CASES})


@pytest.mark.parametrize('group', STEM_GROUPS)
def test_stem_conditions_hold_for_every_row(group):
    """stem_reference asserts them: float32 == float64 evaluation (statistics in a random row order too), images, weights and gradients
    survive the storage type AND bf16 AND fp16 (the unscaled pieces of the stem's in-register splits), |y| integers <= 256, sums of
    squares and weight-gradient partial sums below 2^24, non-zero shares, a zero ring around a non-zero image."""
    rows = [c for c in S.STEM_CASES if c.id.split('_')[1] == group]
    assert rows
    for c in rows:
        L, want = S.stem_reference(c)
        assert tuple(want['y'].shape) == (c.V, c.OH, c.OW, c.Cout) and tuple(want['xp'].shape) == (c.V, c.HP, c.WP, 4)
        assert bool((want['xp'][..., 3] == 0).all())
        assert float(L['img'].abs().max()) <= 2 and (float(L['img'].min()) < 0 or L['img'].numel() <= 9)      # NOT the [0, 1] of real images


def test_stem_geometry_and_rows():
    from simclr_amd import ops
    for H in (1, 2, 3, 9, 10, 17, 31, 224):
        for W in (1, 7, 15, 253, 513):
            for (k, s) in S.KERNELS + ((7, 1),):
                assert S.stem_geometry(H, W, k, s) == ops.stem_geometry(H, W, k, k, s), (H, W, k, s)
    for table, s in ((S.ROWS_S2, 2), (S.ROWS_S1, 1)):
        for M, (V, H, W) in table.items():
            for k in (3, 7):
                OH, OW = R.out_hw(H, W, k, s)
                assert V * OH * OW == M
    ids = {c.id for c in S.STEM_CASES}
    for (k, s) in S.KERNELS:
        for M in (1, 127, 128, 129, 257):
            for ar in S.STEM_AR:
                assert 'stem_rows%d_k%d_s%d_%s' % (M, k, s, ar) in ids
    assert {c.Cout for c in S.STEM_CASES} >= {4, 32, 64, 68, 96, 128, 192}
    assert {c.OW for c in S.STEM_CASES if c.ps} >= {1, 31, 32, 33, 65} and {c.OH for c in S.STEM_CASES if c.ps} >= {1, 2}
    assert {(c.H, c.W) for c in S.STEM_CASES} >= {(9, 17), (17, 9), (1, 15), (15, 1), (10, 7)}


def test_stem_forward_instantiation_rule():
    """The argument rule of simclr_stem_conv_fwd, restated in stem_inst: KP = KHP * KWP * 4, one padded kernel row = 32 elements; the 7x7
    stem takes the unrolled bf16 kernel and, under three terms, the rolling fp32 kernel; six terms, the exact arithmetic and every 3x3
    stem take the generic loop."""
    want = {('bf16', 7): 'stem_conv_fwd<uint16_t, true, 7>', ('bf16', 3): 'stem_conv_fwd<uint16_t, true>',
            ('exact', 7): 'stem_conv_fwd<float, true>', ('exact', 3): 'stem_conv_fwd<float, true>',
            ('bf16x3', 7): 'stem_conv_fwd<float, true, 14, 3>', ('bf16x3', 3): 'stem_conv_fwd<float, true, 0, 3>',
            ('bf16x6', 7): 'stem_conv_fwd<float, true, 0, 6>', ('bf16x6', 3): 'stem_conv_fwd<float, true, 0, 6>',
            ('bf16x6_3', 7): 'stem_conv_fwd<float, true, 0, 6>', ('bf16x6_3', 3): 'stem_conv_fwd<float, true, 0, 6>',
            ('f16x3_3', 7): 'stem_conv_fwd<float, true, 14, 13>', ('f16x3_3', 3): 'stem_conv_fwd<float, true, 0, 13>'}
    seen = set()
    for c in S.STEM_CASES:
        name, grid = S.stem_inst(c)
        assert name == want[(c.arith, c.k)], c.id
        assert c.KP == (224 if c.k == 7 else 96) and c.geo['KWP'] == 8
        assert grid == (min((c.M + 127) // 128, 2048), (c.Cout + 63) // 64)
        assert _lib().stem_stats_slots(c.M) == grid[0]
        seen.add(name)
    assert seen == set(want.values())
    assert max(S.stem_inst(c)[1][1] for c in S.STEM_CASES) == 3 and max(S.stem_inst(c)[1][0] for c in S.STEM_CASES) >= 3      # grid.y > 1, several M-tiles


def test_hand_written_pack_and_unpack():
    c = S.make_stem('stem_hand', 'exact', 2, 2, 3, 3, 1, 8)
    L = dict(x=torch.arange(1., 37., dtype=F64).view(2, 2, 3, 3))
    xp = S.pack_ref(c, L)
    assert (c.HP, c.WP, c.geo['pad']) == (4, 10, 1)
    assert xp[1, 1, 1].tolist() == [19., 20., 21., 0.] and xp[0, 2, 3].tolist() == [16., 17., 18., 0.]
    assert float(xp[:, 0].abs().sum()) == 0 and float(xp[:, :, 0].abs().sum()) == 0 and float(xp[:, 3].abs().sum()) == 0
    kn = torch.arange(float(c.KP * 8), dtype=F64).view(c.KP, 8)
    dw = S.unpack_ref(c, kn)
    assert dw[1, 2, 1, 5] == kn[(1 * 8 + 2) * 4 + 1, 5]
    L['w'] = torch.arange(float(9 * 3 * 8), dtype=F64).view(3, 3, 3, 8)
    ws = S.stem_weights_ref(c, L)
    assert ws[5, (2 * 8 + 1) * 4 + 2] == L['w'][2, 1, 2, 5] and float(ws.view(8, 3, 8, 4)[:, :, 3:].abs().sum()) == 0
    hi, lo = S.xq_ref(torch.tensor([1.0, 257.0, 1.0 + 2.0 ** -9]))
    assert hi.tolist() == [1.0, 256.0, 1.0] and lo.tolist() == [0.0, 1.0, 2.0 ** -9]


def test_gram_conditions_and_identity():
    """gram_reference asserts: float32 == float64 evaluation of h^T h, the column sums and (h^T h) W; partial sums below 2^24; h survives
    its storage type and bf16; sums == the channel sums of c = h W from conv_fwd_ref.  The reduction chunk comes from the library."""
    lib = _lib()
    for c in S.GRAM_CASES:
        br = S.gram_br(lib, c.K, c.dtype)
        assert br in (16, 32, 64, 128)
        M = S.gram_rows(c, br)
        L, want = S.gram_reference(c, M)
        assert want['sums'].dtype == F64 and bool((want['sums'][1] >= 0).all()) and M >= 1
    ms = {(c.arith, c.K): set() for c in S.GRAM_CASES}
    for c in S.GRAM_CASES:
        ms[(c.arith, c.K)].add(c.m)
    assert set(ms) == {('exact', 64), ('exact', 128), ('bf16x6', 64), ('bf16x6', 128), ('bf16', 64), ('bf16', 128), ('bf16', 256)}
    assert all(v >= {(0, 1), (1, -1), (1, 0), (1, 1), (3, 1)} for v in ms.values())
    for c in S.GEMM_CASES:
        S.gemm_reference(c)
    assert {c.big for c in S.GEMM_CASES} == {True, False}
    assert any(c.M % 32 and c.N % 32 for c in S.GEMM_CASES) and any(c.big and (c.M % 64 or c.N % 64) for c in S.GEMM_CASES)
    assert (1024 // 64) * (1024 // 64) == 256 and any(c.K == 32 for c in S.GEMM_CASES)


def _fails(got, want):
    """The comparison of the GPU checks rejects `got` (a perturbed reference standing in for a wrong kernel)."""
    from tests import gpu_checks as gc
    assert gc._bitwise('unperturbed', want, want)['ok']
    g = torch.as_tensor(got)
    if g.numel() != torch.as_tensor(want).numel():
        return True
    return not gc._bitwise('mutant', g.reshape(torch.as_tensor(want).shape), want)['ok']


def test_mutation_stem():
    """Per stem row: one row dropped from BOTH statistics, H and W swapped (non-square maps), OW off by one in the row decode."""
    for c in S.STEM_CASES:
        L, want = S.stem_reference(c)
        rows = want['y'].reshape(-1, c.Cout)
        r = int(rows.abs().sum(1).nonzero()[0])
        keep = torch.ones(rows.shape[0], dtype=torch.bool)
        keep[r] = False
        s1, s2 = R.channel_sums(rows[keep])
        assert _fails(s1, want['s1']) and _fails(s2, want['s2']), c.id
        if c.H != c.W and min(c.H, c.W) > 1:
            xs = L['x'].reshape(c.V, c.W, c.H, 3)
            assert _fails(R.conv_fwd_ref(xs, L['w'], c.k, c.s), want['y']), c.id
            g = S.stem_geometry(c.W, c.H, c.k, c.s)
            if (g['HP'], g['WP']) != (c.HP, c.WP):
                m = copy.copy(c)
                m.H, m.W, m.geo, m.HP, m.WP = c.W, c.H, g, g['HP'], g['WP']
                assert _fails(S.pack_ref(m, dict(x=xs)), want['xp']), c.id
        if c.OW > 2 and c.M > c.OW:        # rows decoded with OW - 1: every output row after the first reads shifted pixels
            y = want['y'].reshape(-1, c.Cout)
            idx = torch.arange(c.M)
            v, rem = idx // (c.OH * c.OW), idx % (c.OH * c.OW)
            oy, ox = rem // (c.OW - 1), rem % (c.OW - 1)
            src = ((v * c.OH + oy.clamp_max(c.OH - 1)) * c.OW + ox)
            assert _fails(y[src], y), c.id
        dw_dropped = R.conv_wgrad_ref(L['x'], L['dy'] * (torch.arange(c.M).view(c.V, c.OH, c.OW, 1) != r), c.k, c.s)
        assert _fails(dw_dropped, want['dw']) or not bool(L['dy'].reshape(-1, c.Cout)[r].any()), c.id


def test_mutation_gram():
    """One streamed row of h dropped: the Gram matrix, the column sums and both rows of the BatchNorm sums change (by the 1 / M the
    tolerance of the model-sized checks allows)."""
    lib = _lib()
    for c in S.GRAM_CASES:
        M = S.gram_rows(c, S.gram_br(lib, c.K, c.dtype))
        L, want = S.gram_reference(c, M)
        r = int(L['h'].abs().sum(1).nonzero()[-1])
        h = torch.cat([L['h'][:r], L['h'][r + 1:]])
        G = h.t() @ h
        assert _fails(G, want['G']) and _fails(h.sum(0), want['cs']), c.id
        assert _fails(torch.stack([h.sum(0) @ L['w'], ((G @ L['w']) * L['w']).sum(0)]), want['sums']), c.id
        # a wrong column sum in one split: one chunk's worth counted twice
        assert _fails(want['cs'] + L['h'][:1].sum(0) + 1, want['cs']), c.id


def test_mutation_ext_and_sparse():
    """ext: the second operand stream read with the wrong pitch (h shifted by one channel), the bias left out.  sparse: a store that
    zero-fills instead of leaving the sentinel, a sentinel that leaks into the accumulate, the parity taken from the wrong axis."""
    for c in [c for c in R.CASES if c.id.startswith('ext_')]:
        L, want = R.reference(c, check_ps=False)
        Lm = dict(L)
        Lm['dy'] = torch.cat([L['dy'][..., :c.Cout], L['dy'][..., c.Cout:].roll(1, -1)], -1)
        assert _fails(R._main_output(c, Lm), want['out']), c.id
        Lm = dict(L, bias=torch.zeros_like(L['bias']))
        assert _fails(R._main_output(c, Lm), want['out']) or c.op == 'dgrad_bn', c.id
    seen = 0
    for c in [c for c in R.CASES if c.id.startswith('sparse_')]:
        L, want = R.reference(c, check_ps=False)
        ev = R.even_pixels(c)
        if c.H * c.W == 1:
            continue
        seen += 1
        if c.acc == 3:
            assert _fails(torch.where(ev, want['out'], torch.zeros_like(want['out'])), want['out']), c.id
            assert bool((want['out'][~ev.expand_as(want['out'])] >= 12345.0).all())
        else:
            leak = want['out'] + torch.where(ev, 0.0, R.SENTINEL)
            assert _fails(leak, want['out']), c.id
            if c.op == 'dgrad' and c.H > 1 and c.W > 1:
                odd_col = torch.zeros_like(ev)
                odd_col[:, ::2, 1::2] = True          # earlier data looked up at (even row, odd column)
                assert _fails(R.dgrad_of(c, L) + L['prev'].roll(1, 2) * odd_col, want['out']), c.id
    assert seen > 50


_DRY_RUN = r'''
import ctypes, os
from simclr_amd import _lib
from tests import conv_reference as R
from tests import stem_gram_reference as S
L = _lib.lib()
FAKE = ctypes.c_void_p(1 << 20)          # never dereferenced in a dry run
rec = lambda: L.conv2d_last_instantiation().decode()
for c in S.STEM_CASES:
    for k in [k for k in os.environ if k.startswith('SIMCLR_') and k != 'SIMCLR_DRY_RUN']:
        del os.environ[k]
    os.environ.update(c.env)
    g = c.geo
    dt = 1 if c.dtype == S.BF16 else 0
    if c.wgrad_ok:
        L.conv2d_wgrad(FAKE, FAKE, FAKE, 0, FAKE, c.V, c.HP, c.WP, 32, 4, c.OH, c.OW, c.Cout, g['KHP'], 1, c.s, 0, dt | R.terms_field(c.tb), None)
        print('%s\twgrad\t%s' % (c.id, rec()))
    if c.ps_ok:
        L.stem_wgrad_ps(FAKE, FAKE, FAKE, 0, FAKE, c.V, c.HP, c.WP, c.OH, c.OW, c.Cout, g['KHP'], g['KWP'], c.s, None)
        print('%s\tps\t%s' % (c.id, rec()))
for k in [k for k in os.environ if k.startswith('SIMCLR_') and k != 'SIMCLR_DRY_RUN']:
    del os.environ[k]
for c in S.GRAM_CASES:
    br = S.gram_br(L, c.K, c.dtype)
    M = S.gram_rows(c, br)
    dt = 1 if c.dtype == S.BF16 else 0
    L.conv2d_gram(FAKE, FAKE, FAKE, M, c.K, dt | (R.terms_field(c.tf) if dt == 0 else 0), None)
    print('%s\tgram %d %d\t%s' % (c.id, br, M, rec()))
print('ok')
'''


def test_recorded_launches_of_every_row():
    """The weight-gradient, pre-split and Gram launches of every row in a dry run, each under the row's own switches: the record names the
    kernel plan_wgrad / plan_stem_wgrad_ps / plan_gram picks (the multi-tap stem tiles over LDS-DMA or register-staged, the 32-row tile
    for Cout > 64; the ring depth and split shape of the pre-split kernel; the Gram tile, its chunk and its splits)."""
    env = {k: v for k, v in os.environ.items() if not k.startswith('SIMCLR_')}
    env.update(SIMCLR_DRY_RUN='1')
    r = subprocess.run([sys.executable, '-c', _DRY_RUN], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and lines[-1] == 'ok', r.stdout[-2000:] + r.stderr[-2000:]
    got = {}
    for l in lines[:-1]:
        id, kind, rec = l.split('\t', 2)
        got[(id, kind.split()[0])] = (kind, rec)
    kernels = set()
    for c in S.STEM_CASES:
        assert ((c.id, 'wgrad') in got) == c.wgrad_ok and ((c.id, 'ps') in got) == c.ps_ok, c.id
        S.check_stem_records(c, got[(c.id, 'wgrad')][1] if c.wgrad_ok else None, got[(c.id, 'ps')][1] if c.ps_ok else None)
        kernels |= {v[1].split(')')[0] for k_, v in got.items() if k_[0] == c.id}
    for c in S.GRAM_CASES:
        kind, rec = got[(c.id, 'gram')]
        _, br, M = kind.split()
        S.check_gram_record(c, rec, int(br), int(M))
        kernels.add(rec.split(')')[0])
    want = {'(conv_wgrad<uint16_t, 256, 64, true>', '(conv_wgrad<float, 256, 64, true>', '(conv_wgrad<uint16_t, 32, 64>', '(conv_wgrad<float, 32, 64>',
            '(conv_wgrad_dma<uint16_t, 256, 64, 2, 2, 2, 2, false, true>', '(conv_wgrad_dma<float, 256, 64, 2, 2, 4, 2, false, true, 3>',
            '(conv_wgrad_dma<float, 256, 64, 2, 2, 4, 2, false, true, 6>', '(stem_wgrad_ps<7, 2, 2>', '(stem_wgrad_ps<7, 2, 3>',
            '(conv_wgrad_dma<float, 64, 64, 2, 4, 2, 2, true>', '(conv_wgrad_dma<float, 128, 128, 2, 4, 2, 2, true>',
            '(conv_wgrad_dma<float, 64, 64, 2, 4, 2, 2, true, false, 6>', '(conv_wgrad_dma<float, 128, 128, 2, 4, 2, 2, true, false, 6>',
            '(conv_wgrad_dma<uint16_t, 64, 64, 2, 4, 2, 2, true>', '(conv_wgrad_dma<uint16_t, 128, 128, 2, 4, 2, 2, true>',
            '(conv_wgrad_dma<uint16_t, 256, 256, 1, 4, 2, 4, true>'}
    assert kernels == want, (sorted(kernels - want), sorted(want - kernels))
