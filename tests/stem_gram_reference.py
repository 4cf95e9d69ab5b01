"""Integer-lattice rows and float64 references of the stem chain and the Gram chain (csrc/conv.hip, csrc/pool.hip, csrc/bn.hip): the sibling
table of tests/conv_reference.py, whose lattice rules, references and record parser it reuses (the K-extended and the sparse data-gradient
rows are ordinary rows of conv_reference.CASES).

Pure torch on the CPU: shared by tests/gpu_checks.py (check_stem_lattice, check_gram_lattice, check_small_gemm_lattice), by
tests/test_stem_gram_reference.py (conditions, mutations, the dry-run pins) and by tests/test_gpu_stem_gram_lattice.py.

Stem: simclr_pack_views(_ps) -> simclr_prep_weights mode 2 -> simclr_stem_conv_fwd with statistics -> the weight gradient through
simclr_conv2d_wgrad (pixpitch = 4) + simclr_unpack_stem_dw and, where simclr_stem_wgrad_ps_supported, through simclr_presplit_packed +
simclr_stem_wgrad_ps.  Images are integers in [-2, 2]: neither pack_views (a copy with zero fill, csrc/pool.hip) nor the stem kernels
(both operands split in registers, unscaled: split_terms2 / split_terms2_f16) assume [0, 1] anywhere -- the range only matters for the
accuracy of the unscaled fp16 lo pieces, which is not the subject here.  w is in {-1, 0, 1}, thinned by the taps that can land on the
image; dy integers in [-2, 2]; the accumulate operands integers in [-4, 4].  Every operand survives bf16 AND fp16 (asserted), so each
piece of each split is the value itself and the remaining pieces are zero.

Gram: simclr_conv2d_gram (h^T h and the column sums of an integer h in [-2, 2]) -> simclr_small_gemm_nt_f32 ((h^T h) W, W in {-1, 0, 1}
thinned until every partial sum stays below 2^24) -> simclr_bn_sums_from_gram (fp64: colsum(h) W and sum_k GW o W), which must equal the
channel sums of c = h W -- asserted here on the references.

The stem forward writes no launch record, so its instantiation is claimed from the argument rule of simclr_stem_conv_fwd, restated in
stem_inst (KP, KWP, the terms); the weight-gradient, pre-split and Gram launches are recorded (role = wgrad | stem_wgrad_ps | gram) and
their records are pinned in a dry run.  The reduction chunk `br` of a Gram plan is read from the library (gram_br), never written down.
"""
import re
import types
import zlib

import torch

from tests.bn_pool_reference import BF16, F32, F64, assert_exact, assert_survives, row_perm
from tests.conv_reference import ARITH, LIMIT, _ints, channel_sums, conv_fwd_ref, conv_wgrad_ref, out_hw, parse_record

F16 = torch.float16


def _seed(id):
    return zlib.crc32(id.encode()) & 0x7fffffff


def _signs(shape, g):
    sign = torch.randint(0, 2, tuple(shape), generator=g).double() * 2 - 1
    return sign, torch.rand(tuple(shape), generator=g, dtype=F64)


# ===================================================================================================================== stem
def stem_geometry(H, W, k, s):
    """simclr_amd.ops.stem_geometry restated (pinned against it in tests/test_stem_gram_reference.py)."""
    pad = (k - 1) // 2
    OH, OW = out_hw(H, W, k, s)
    HP = max((OH - 1) * s + k, H + pad)
    WP = max((OW - 1) * s + 8, W + pad)
    WP = (WP + 1) // 2 * 2
    return dict(pad=pad, OH=OH, OW=OW, KHP=k, KWP=8, HP=HP, WP=WP)


def make_stem(id, arith, V, H, W, k, s, Cout, env=None, ps=None):
    """One stem row.  V views of H x W pixels: `views` channel triples of V / views images (simclr_pack_views splits them).
    ps: None | 'one' | 'many' = the pre-split weight gradient runs one chunk per split | several with an uneven last split."""
    assert arith in ARITH
    c = types.SimpleNamespace(id=id, arith=arith, V=V, H=H, W=W, k=k, s=s, Cout=Cout, env=dict(env or {}), ps=ps)
    c.dtype, c.tf, c.tb = ARITH[arith]
    c.views = 2 if V % 2 == 0 else (3 if V % 3 == 0 else 1)
    c.b = V // c.views
    c.geo = stem_geometry(H, W, k, s)
    c.OH, c.OW, c.HP, c.WP = c.geo['OH'], c.geo['OW'], c.geo['HP'], c.geo['WP']
    c.M = V * c.OH * c.OW
    c.KP = c.geo['KHP'] * c.geo['KWP'] * 4
    c.epc = 8 if c.dtype == BF16 else 4
    c.fwd_ok = Cout % c.epc == 0                              # simclr_stem_conv_fwd: Cout a multiple of 8 (bf16) / 4 (fp32)
    c.wgrad_ok = Cout % 8 == 0                                # simclr_conv2d_wgrad: Cout a multiple of 8
    c.ps_ok = c.dtype == F32 and c.tb == 3 and k == 7 and s == 2 and Cout == 64      # simclr_stem_wgrad_ps_supported + three backward terms
    assert ps is None or c.ps_ok, id
    return c


def stem_inst(c, stats=True):
    """The instantiation simclr_stem_conv_fwd launches for a row: its argument rule restated.  Returns (text, grid)."""
    row = c.geo['KWP'] * 4
    st = 'true' if stats else 'false'
    if c.dtype == BF16:
        ks = 7 if (row == 32 and c.KP == 7 * 32) else 0
        name = 'stem_conv_fwd<uint16_t, %s, %d>' % (st, ks) if ks else 'stem_conv_fwd<uint16_t, %s>' % st
    else:
        spl = c.tf                                                      # SIMCLR_STEM_SPLIT unset
        roll = c.KP == 14 * 16 and row == 32 and c.V * c.HP * c.WP * 16 < (1 << 32)
        if spl in (3, 13):
            name = 'stem_conv_fwd<float, %s, %d, %d>' % (st, 14 if roll else 0, spl)
        elif spl == 6:
            name = 'stem_conv_fwd<float, %s, 0, 6>' % st
        else:
            name = 'stem_conv_fwd<float, %s>' % st
    return name, (min(-(-c.M // 128), 2048), -(-c.Cout // 64))


def stem_wgrad_kernel(c):
    """The kernel plan_wgrad picks for the stem's weight gradient (x = the packed views, 32 'channels' per kernel row, pixel pitch 4)."""
    T = 'uint16_t' if c.dtype == BF16 else 'float'
    if c.Cout > 64:
        return 'conv_wgrad<%s, 32, 64>' % T
    if c.dtype == BF16 and c.s % 2 == 0:
        return 'conv_wgrad_dma<uint16_t, 256, 64, 2, 2, 2, 2, false, true>'
    if c.dtype == F32 and c.tb != 0:
        return 'conv_wgrad_dma<float, 256, 64, 2, 2, 4, 2, false, true, %d>' % c.tb
    return 'conv_wgrad<%s, 256, 64, true>' % T


def stem_lattice(c):
    g = torch.Generator().manual_seed(_seed(c.id))
    L = dict(img=_ints((c.b, c.H, c.W, 3 * c.views), 2, g))
    L['x'] = torch.cat(torch.split(L['img'], 3, dim=3), 0).contiguous()            # view v = (triple, image): [V, H, W, 3]
    L['dy'] = _ints((c.V, c.OH, c.OW, c.Cout), 2, g)
    L['prev'] = _ints((c.k, c.k, 3, c.Cout), 4, g)                                  # HWIO, what simclr_unpack_stem_dw adds to
    L['prev_kn'] = _ints((c.KP, c.Cout), 4, g)                                      # the padded [KHP KWP 4][Cout] matrix the kernels add to
    sign, u = _signs((c.k, c.k, 3, c.Cout), g)
    dens = min(1.0, 12.0 / (3 * min(c.k, c.H) * min(c.k, c.W)))
    for _ in range(12):
        L['w'] = sign * (u < dens).double()
        y = conv_fwd_ref(L['x'], L['w'], c.k, c.s)
        if float(y.abs().max()) <= 256 and float((y * y).reshape(-1, c.Cout).sum(0).max()) < LIMIT:
            return L
        dens /= 2
    raise AssertionError('no weight density meets the bounds of %s' % c.id)


def pack_ref(c, L):
    """simclr_pack_views: [V][HP][WP][4], the image at (pad, pad), zeros around it and in the 4th channel."""
    xp = torch.zeros(c.V, c.HP, c.WP, 4, dtype=F64)
    p = c.geo['pad']
    xp[:, p:p + c.H, p:p + c.W, :3] = L['x']
    return xp


def stem_weights_ref(c, L):
    """simclr_prep_weights mode 2: [Cout][KHP][KWP][4], zero padded."""
    ws = torch.zeros(c.Cout, c.geo['KHP'], c.geo['KWP'], 4, dtype=F64)
    ws[:, :c.k, :c.k, :3] = L['w'].permute(3, 0, 1, 2)
    return ws.reshape(c.Cout, c.KP)


def unpack_ref(c, kn):
    """simclr_unpack_stem_dw: [KHP KWP 4][Cout] -> HWIO [k][k][3][Cout]"""
    return kn.reshape(c.geo['KHP'], c.geo['KWP'], 4, c.Cout)[:c.k, :c.k, :3].contiguous()


def stem_reference(c):
    """(L, want) of a stem row, after the same conditions conv_reference.reference asserts.  want: xp, ws, y, s1, s2, dw (store), dw_acc (+ prev:
    simclr_unpack_stem_dw's accumulate), dw_kn_acc (+ unpack(prev_kn): the kernels' own accumulate), dw_both."""
    L = stem_lattice(c)
    perm = row_perm(c.M, seed=3)

    def evaluate(dtype, perm=perm):
        y = conv_fwd_ref(L['x'], L['w'], c.k, c.s, dtype)
        s1, s2 = channel_sums(y, perm)
        dw = conv_wgrad_ref(L['x'], L['dy'], c.k, c.s, dtype)
        return dict(y=y, s1=s1, s2=s2, dw=dw, dw_acc=dw + L['prev'].to(dtype), dw_kn_acc=dw + unpack_ref(c, L['prev_kn']).to(dtype))

    want = assert_exact(evaluate, c.id)
    assert_exact(lambda d: evaluate(d, None), c.id + ' (rows in order)')
    want['dw_both'] = want['dw_kn_acc'] + L['prev']
    want['xp'], want['ws'] = pack_ref(c, L), stem_weights_ref(c, L)
    ops_ = {n: L[n] for n in ('img', 'w', 'dy')}
    assert_survives(ops_, c.dtype)
    assert_survives(ops_, BF16)              # the bf16 pieces of the three- and six-term products hold the operand itself ...
    assert_survives(ops_, F16)               # ... and so do the unscaled fp16 pieces (stem: no 2^8 on the weights)
    y = want['y']
    assert float(y.abs().max()) <= 256 and torch.equal(y, y.round()), c.id
    assert float((y * y).reshape(-1, c.Cout).sum(0).max()) < LIMIT, c.id
    xa = want['xp'].abs().reshape(-1, 4).sum(0).max()
    assert float(xa * L['dy'].abs().max()) + 8 < LIMIT, c.id
    nz = float((y != 0).double().mean())
    assert nz >= (0.25 if y.numel() >= 4096 else 0.05), (c.id, nz)
    # (on a map narrower than the kernel only the taps that land on it receive a gradient)
    assert float((want['dw'] != 0).double().mean()) >= (0.05 if min(c.H, c.W) >= c.k else 0.002), c.id
    if c.M > 1 or c.H * c.W > 1:
        inner = want['xp'][:, c.geo['pad']:c.geo['pad'] + c.H, c.geo['pad']:c.geo['pad'] + c.W]
        assert float(want['xp'].abs().sum()) == float(inner.abs().sum()) > 0, c.id          # a zero ring around a non-zero image
    return L, want


def xq_ref(xp32):
    """simclr_presplit_packed / simclr_pack_views_ps of the packed fp32 views: per pixel four bf16 hi pieces, then four bf16 lo pieces."""
    hi = xp32.float().bfloat16().float()
    lo = (xp32.float() - hi).bfloat16().float()
    return hi, lo


STEM_AR = ('bf16', 'exact', 'bf16x3', 'bf16x6', 'bf16x6_3', 'f16x3_3')
# (V, H, W) with V * OH * OW output rows around the 128-row M-tile: stride 2 (OH = (H - 1) // 2 + 1) and stride 1
ROWS_S2 = {1: (1, 1, 1), 127: (1, 1, 253), 128: (4, 3, 31), 129: (3, 2, 85), 257: (1, 1, 513)}
ROWS_S1 = {1: (1, 1, 1), 127: (1, 1, 127), 128: (4, 2, 16), 129: (3, 1, 43), 257: (1, 1, 257)}
KERNELS = ((7, 2), (3, 1), (3, 2))


def build_stem_cases():
    rows = []

    def add(*a, **kw):
        rows.append(make_stem(*a, **kw))

    for (k, s) in KERNELS:
        for M, (V, H, W) in (ROWS_S2 if s == 2 else ROWS_S1).items():
            for ar in STEM_AR:
                add('stem_rows%d_k%d_s%d_%s' % (M, k, s, ar), ar, V, H, W, k, s, 64)
    for (H, W) in ((9, 17), (17, 9), (1, 15), (15, 1)):
        for (k, s) in ((7, 2), (3, 1)):
            for ar in ('bf16', 'exact', 'f16x3_3'):
                add('stem_%dx%d_k%d_s%d_%s' % (H, W, k, s, ar), ar, 4, H, W, k, s, 64)
    for k in (7, 3):
        for ar in ('bf16', 'exact', 'bf16x3', 'f16x3_3'):
            add('stem_10x7_k%d_s2_%s' % (k, ar), ar, 4, 10, 7, k, 2, 64)
    # Cout: the three-conv stem's 32 wm and the one-conv stem's 64 wm (grid.y > 1, a half-empty 64-wide N-tile); fp32 4 and 68 run the
    # forward (the N-tile tail) while simclr_conv2d_wgrad refuses a Cout that is no multiple of 8
    for Cout in (32, 96, 128, 192):
        for ar in ('bf16', 'exact', 'bf16x6', 'f16x3_3'):
            add('stem_cout%d_k7_s2_%s' % (Cout, ar), ar, 3, 9, 17, 7, 2, Cout)
            add('stem_cout%d_k3_s1_%s' % (Cout, ar), ar, 3, 5, 9, 3, 1, Cout)
    for Cout in (4, 68):
        for ar in ('exact', 'bf16x3', 'f16x3_3'):
            add('stem_cout%d_k7_s2_%s' % (Cout, ar), ar, 3, 9, 17, 7, 2, Cout)
            add('stem_cout%d_k3_s2_%s' % (Cout, ar), ar, 3, 10, 7, 3, 2, Cout)
    add('stem_cout68_refused_bf16', 'bf16', 3, 9, 17, 7, 2, 68)
    # simclr_stem_wgrad_ps: OW = 1 / 31 / 32 / 33 / 65 (one 32-column segment, its edges, three segments), OH = 1 and 2
    for OW in (1, 31, 32, 33, 65):
        for i, ar in enumerate(('bf16x3', 'bf16x6_3', 'f16x3_3')):
            add('stem_ps_ow%d_%s' % (OW, ar), ar, 2, 1 if (OW + i) % 2 else 3, 2 * OW - 1, 7, 2, 64, ps='one')
    # several chunks per split with an uneven last one (27 chunks on 8 workgroups: 4, 4, ..., 3); the three-deep ring
    add('stem_ps_blocks8', 'bf16x3', 3, 5, 129, 7, 2, 64, env={'SIMCLR_STEM_WGRAD_BLOCKS': '8'}, ps='many')
    add('stem_ps_blocks8_stages3', 'f16x3_3', 3, 5, 129, 7, 2, 64, env={'SIMCLR_STEM_WGRAD_BLOCKS': '8', 'SIMCLR_STEM_WGRAD_PS_STAGES': '3'}, ps='many')
    add('stem_ps_stages2', 'bf16x6_3', 3, 5, 129, 7, 2, 64, env={'SIMCLR_STEM_WGRAD_PS_STAGES': '2'}, ps='one')
    add('stem_ps_stages3', 'bf16x3', 3, 5, 129, 7, 2, 64, env={'SIMCLR_STEM_WGRAD_PS_STAGES': '3'}, ps='one')
    ids = [c.id for c in rows]
    assert len(set(ids)) == len(ids)
    return rows


def check_stem_records(c, rec_wgrad, rec_ps):
    """The recorded weight-gradient launches of a row: the kernel plan_wgrad names for the packed stem, and the pre-split kernel with the
    ring depth and the split shape the row claims."""
    if rec_wgrad is not None:
        assert rec_wgrad.startswith('(%s)' % stem_wgrad_kernel(c)) and ' role=wgrad ' in rec_wgrad, (c.id, stem_wgrad_kernel(c), rec_wgrad)
    if rec_ps is not None:
        stages = 3 if c.env.get('SIMCLR_STEM_WGRAD_PS_STAGES') == '3' else 2
        assert rec_ps.startswith('(stem_wgrad_ps<7, 2, %d>)' % stages) and ' role=stem_wgrad_ps ' in rec_ps, (c.id, rec_ps)
        f = dict((k_, int(v)) for k_, v in re.findall(r' (\w+)=(\d+)', rec_ps))
        chunks = c.V * c.OH * ((c.OW + 31) // 32)
        assert f['splits'] == -(-chunks // f['chunks_per_split']), (c.id, rec_ps)
        if c.ps == 'one':
            assert f['chunks_per_split'] == 1 and f['splits'] == chunks, (c.id, rec_ps)
        if c.ps == 'many':
            assert f['chunks_per_split'] > 1 and chunks % f['chunks_per_split'] != 0, (c.id, rec_ps)


# ===================================================================================================================== Gram
GRAM_AR = {'bf16': (BF16, 0), 'exact': (F32, 0), 'bf16x6': (F32, 6)}


def make_gram(id, arith, K, m, N=None):
    """One Gram row.  m = (a, b): M = a * br + b rows, br = the reduction chunk of the plan (gram_br); N: columns of W."""
    c = types.SimpleNamespace(id=id, arith=arith, K=K, m=m, N=N or 2 * K)
    c.dtype, c.tf = GRAM_AR[arith]
    c.ranges = 512 if K == 256 else 1024           # plan_gram: the cap on the pixel ranges
    return c


def gram_br(lib, K, dtype):
    """Rows per reduction chunk of plan_gram, read through simclr_conv2d_gram_workspace_bytes: below 8 chunks the plan makes one split per
    chunk, so the workspace holds two slabs from M = br + 1 on."""
    dt = 1 if dtype == BF16 else 0
    slab = (K * K + K) * 4
    for M in range(1, 1025):
        if lib.conv2d_gram_workspace_bytes(M, K, dt) // slab == 2:
            return M - 1
    raise AssertionError('no chunk edge below 1024 rows')


def gram_rows(c, br):
    a, b = c.m
    return a * br + b


def gram_kernel(c):
    T = 'uint16_t' if c.dtype == BF16 else 'float'
    if c.K == 256:
        return 'conv_wgrad_dma<uint16_t, 256, 256, 1, 4, 2, 4, true>'
    return 'conv_wgrad_dma<%s, %d, %d, 2, 4, 2, 2, true%s>' % (T, c.K, c.K, ', false, 6' if c.tf else '')


def check_gram_record(c, rec, br, M):
    kernel, a, f = parse_record(rec)
    assert rec.startswith('(%s)' % gram_kernel(c)) and ' role=gram ' in rec, (c.id, gram_kernel(c), rec)
    esz = 2 if c.dtype == BF16 else 4
    assert f['lds'] == 4 * br * c.K * esz, (c.id, br, rec)                 # the four-deep ring of br-row chunks: br is the library's
    nchunks = -(-M // br)
    assert f['splits'] == -(-nchunks // f['chunks_per_split']) and f['splits'] <= c.ranges, (c.id, rec)
    if c.m[0] >= c.ranges:          # more than one chunk per split, the last split shorter than the others
        assert f['chunks_per_split'] > 1 and nchunks % f['chunks_per_split'] != 0, (c.id, rec)
    else:
        assert f['chunks_per_split'] == 1 and f['splits'] == nchunks, (c.id, rec)


def gram_reference(c, M):
    """(L, want): h [M][K], W [K][N]; want G, cs, GW, sums (float64), after the exactness conditions."""
    g = torch.Generator().manual_seed(_seed(c.id))
    L = dict(h=_ints((M, c.K), 2, g))
    sign, u = _signs((c.K, c.N), g)
    ha = L['h'].abs()
    Ga = ha.t() @ ha
    dens = min(1.0, 12.0 / c.K)
    for _ in range(12):
        L['w'] = sign * (u < dens).double()
        if float((Ga @ L['w'].abs()).max()) < LIMIT:
            break
        dens /= 2
    else:
        raise AssertionError('no weight density meets the bounds of %s' % c.id)

    def evaluate(dtype):
        h, w = L['h'].to(dtype), L['w'].to(dtype)
        G = h.t() @ h
        return dict(G=G, cs=h.sum(0), GW=G @ w)

    want = assert_exact(evaluate, c.id)
    assert float(Ga.max()) < LIMIT and float(ha.sum(0).max()) < LIMIT, c.id
    assert_survives(dict(h=L['h']), c.dtype)
    assert_survives(dict(h=L['h'], w=L['w']), BF16)
    want['sums'] = torch.stack([want['cs'] @ L['w'], (want['GW'] * L['w']).sum(0)])
    # the identity the chain rests on: these are the channel sums of c = h W
    cc = conv_fwd_ref(L['h'].reshape(1, 1, M, c.K), L['w'].reshape(1, 1, c.K, c.N), 1, 1)
    s1, s2 = channel_sums(cc)
    assert torch.equal(want['sums'][0], s1) and torch.equal(want['sums'][1], s2), c.id
    assert float(want['sums'].abs().max()) < 2.0 ** 53
    assert float((L['w'] != 0).double().mean()) >= 0.02 and float((want['GW'] != 0).double().mean()) >= 0.05, c.id
    off = want['G'] - torch.diag(torch.diag(want['G']))
    assert M < 4 or float((off != 0).double().mean()) >= 0.25, c.id
    return L, want


def build_gram_cases():
    rows = []
    for ar, Ks in (('exact', (64, 128)), ('bf16x6', (64, 128)), ('bf16', (64, 128, 256))):
        for K in Ks:
            for (a, b) in ((0, 1), (1, -1), (1, 0), (1, 1), (3, 1)):
                rows.append(make_gram('gram_%s_K%d_%dbr%+d' % (ar, K, a, b), ar, K, (a, b)))
    # more than one chunk per split with an uneven last split: the smallest M above (ranges) chunks
    for ar, K in (('exact', 64), ('bf16x6', 64), ('bf16', 64), ('bf16', 256)):
        rows.append(make_gram('gram_%s_K%d_many' % (ar, K), ar, K, (512 if K == 256 else 1024, 1), N=K))
    return rows


def make_gemm(id, M, N, K):
    return types.SimpleNamespace(id=id, M=M, N=N, K=K, big=(-(-M // 64)) * (-(-N // 64)) >= 256)


def gemm_reference(c):
    g = torch.Generator().manual_seed(_seed(c.id))
    L = dict(a=_ints((c.M, c.K), 2, g))
    sign, u = _signs((c.N, c.K), g)
    L['b'] = sign * (u < min(1.0, 12.0 / c.K)).double()
    want = assert_exact(lambda d: dict(c=L['a'].to(d) @ L['b'].to(d).t()), c.id)
    assert float((L['a'].abs() @ L['b'].abs().t()).max()) < LIMIT
    assert float((want['c'] != 0).double().mean()) >= 0.25, c.id
    return L, want


# both tile branches of simclr_small_gemm_nt_f32 (64-row tiles from 256 tiles on), M and N no multiples of 32 / 64, K = 32 and more
GEMM_CASES = [make_gemm('gemm_%dx%dx%d' % s, *s) for s in
              ((16, 16, 32), (48, 80, 32), (80, 48, 64), (64, 256, 128), (1008, 960, 32), (1024, 1024, 32), (1008, 1040, 32), (976, 1008, 96))]
STEM_CASES = build_stem_cases()
GRAM_CASES = build_gram_cases()
STEM_BY_ID = {c.id: c for c in STEM_CASES}
