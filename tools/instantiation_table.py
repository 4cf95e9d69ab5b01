#!/usr/bin/env python
"""(layer class -> kernel instantiation) table of the forward / data-gradient convolution launches.

    python tools/instantiation_table.py [--views 1024] [--out profiles/r06_instantiations.txt]
    python tools/instantiation_table.py --what wgrad [--out profiles/wgrad_instantiations.txt]

Runs WITHOUT a GPU: with SIMCLR_DRY_RUN=1 the convolution entry points of libsimclr_hip.so take every launch decision
(plan_igemm: tile shape, halo window, wide eight-phase tile, split tail, pre-split weights, compile-time epilogue
specialisations) and record it instead of launching (simclr_conv2d_last_instantiation).  One row per (ResNet-50 1x layer class at
224 px) x (kind of launch a training step issues for it) x (storage / matrix arithmetic).  tests/test_abi.py regenerates the
table and compares it with the committed file, so a change of the selection rules is a visible diff, not a silent one.

--what wgrad: the same for the weight-gradient side -- simclr_conv2d_wgrad per layer class and operand format (bf16; fp32 with every
backward term count; fp32, three terms, pre-split dy), the 7x7 stem as the multi-tap call and as simclr_stem_wgrad_ps, and the Gram
launches of the fused bottleneck tail.  Each record ends with the split-K geometry and the grid of the slab reduction.
"""
import argparse
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

# ResNet-50 1x at 224 px (tf2/resnet.py:385-487, 709-729): (name, H of the INPUT, Cin, Cout, k, stride, count per step)
LAYERS = [
    ('g1 reduce 1x1 64->64 (first block)', 56, 64, 64, 1, 1, 1),
    ('g1 reduce 1x1 256->64', 56, 256, 64, 1, 1, 2),
    ('g1 3x3 64->64', 56, 64, 64, 3, 1, 3),
    ('g1 expand 1x1 64->256', 56, 64, 256, 1, 1, 3),
    ('g1 shortcut 1x1 64->256', 56, 64, 256, 1, 1, 1),
    ('g2 reduce 1x1 256->128 @56', 56, 256, 128, 1, 1, 1),
    ('g2 3x3 s2 128->128 56->28', 56, 128, 128, 3, 2, 1),
    ('g2 shortcut 1x1 s2 256->512', 56, 256, 512, 1, 2, 1),
    ('g2 reduce 1x1 512->128', 28, 512, 128, 1, 1, 3),
    ('g2 3x3 128->128', 28, 128, 128, 3, 1, 3),
    ('g2 expand 1x1 128->512', 28, 128, 512, 1, 1, 4),
    ('g3 reduce 1x1 512->256 @28', 28, 512, 256, 1, 1, 1),
    ('g3 3x3 s2 256->256 28->14', 28, 256, 256, 3, 2, 1),
    ('g3 shortcut 1x1 s2 512->1024', 28, 512, 1024, 1, 2, 1),
    ('g3 reduce 1x1 1024->256', 14, 1024, 256, 1, 1, 5),
    ('g3 3x3 256->256', 14, 256, 256, 3, 1, 5),
    ('g3 expand 1x1 256->1024', 14, 256, 1024, 1, 1, 6),
    ('g4 reduce 1x1 1024->512 @14', 14, 1024, 512, 1, 1, 1),
    ('g4 3x3 s2 512->512 14->7', 14, 512, 512, 3, 2, 1),
    ('g4 shortcut 1x1 s2 1024->2048', 14, 1024, 2048, 1, 2, 1),
    ('g4 reduce 1x1 2048->512', 7, 2048, 512, 1, 1, 2),
    ('g4 3x3 512->512', 7, 512, 512, 3, 1, 2),
    ('g4 expand 1x1 512->2048', 7, 512, 2048, 1, 1, 3),
    ('head dense 2048->2048', 1, 2048, 2048, 1, 1, 2),
    ('head dense 2048->128', 1, 2048, 128, 1, 1, 1),
]
FAKE = ctypes.c_void_p(1 << 20)          # never dereferenced in a dry run
MODES = [('bf16', 1, (0, 0)), ('f32 exact', 0, (0, 0)), ('f32 bf16x6_3', 0, (6, 3)), ('f32 f16x3_3', 0, (13, 3))]


def rows(views):
    os.environ['SIMCLR_DRY_RUN'] = '1'
    from simclr_amd._lib import lib
    L = lib()
    out = []
    last = lambda: L.conv2d_last_instantiation().decode()
    try:
        for mode, dtype, terms in MODES:
            L.set_f32_matmul(*terms)
            for name, H, Cin, Cout, k, s, cnt in LAYERS:
                V = views
                pad = (k - 1) // 2
                OH = (H + (k - 1) - k) // s + 1
                M = V * OH * OH
                nslot = L.conv2d_stats_slots(M, Cout)
                kinds = []
                # forward with BatchNorm statistics in the epilogue (every convolution feeds a BatchNorm, tf2/resnet.py:183-208 + 31-78)
                if dtype == 1:
                    L.conv2d_fwd(FAKE, FAKE, FAKE, FAKE, nslot, V, H, H, Cin, OH, OH, Cout, k, k, s, pad, dtype, None)
                else:
                    L.conv2d_fwd_pivoted(FAKE, FAKE, FAKE, FAKE, nslot, FAKE, V, H, H, Cin, OH, OH, Cout, k, k, s, pad, dtype, None)
                kinds.append(('fwd + statistics', last()))
                if dtype == 1 and 'expand' in name:      # fused bottleneck tail: conv3 + bn3 + shortcut + ReLU + mask bits (bf16)
                    L.conv2d_fwd_bn_apply(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None, None, 1, FAKE, V, H, H, Cin, OH, OH, Cout, k, k, s, pad, dtype, None)
                    kinds.append(('fwd + fused BatchNorm apply / residual / ReLU', last()))
                if dtype == 0 and terms == (13, 3) and 'expand' in name:
                    # the parity mode's fused bottleneck tail: the short-K layers take the N-inner walk (conv_igemm_nwalk, SIMCLR_IGEMM_NWALK);
                    # the first block of a stage applies the projection shortcut's own BatchNorm to the residual
                    for rbn, what in ((None, ''), (FAKE, ', BatchNorm shortcut')):
                        L.conv2d_fwd_bn_apply(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, rbn, rbn, 1, FAKE, V, H, H, Cin, OH, OH, Cout, k, k, s, pad, dtype, None)
                        kinds.append(('fwd + fused BatchNorm apply / residual / ReLU' + what, last()))
                if H > 1 or True:
                    L.conv2d_dgrad(FAKE, FAKE, FAKE, 0, V, H, H, Cin, OH, OH, Cout, k, k, s, pad, dtype, None)
                    kinds.append(('dgrad', last()))
                if s == 1 and H > 1:
                    nsl_in = L.conv2d_stats_slots(V * H * H, Cin)
                    # dgrad + BatchNorm-backward reduce of the producer: mode 2 (mask recomputed from the BatchNorm input), store
                    L.conv2d_dgrad_bn(FAKE, FAKE, FAKE, 0, FAKE, None, FAKE, FAKE, FAKE, FAKE, 2, FAKE, nsl_in, V, H, H, Cin, OH, OH, Cout,
                                      k, k, 1, pad, dtype, None)
                    kinds.append(('dgrad + BN-backward reduce (mode 2)', last()))
                    if 'reduce' in name:                 # conv1 of a block: accumulates into the shortcut gradient, mask bits, sums only
                        L.conv2d_dgrad_bn(FAKE, FAKE, FAKE, 1, None, FAKE, None, None, None, None, 4, FAKE, nsl_in, V, H, H, Cin, OH, OH,
                                          Cout, k, k, 1, pad, dtype, None)
                        kinds.append(('dgrad + accumulate + BN-backward sums (mode 4)', last()))
                    if dtype == 0 and terms == (13, 3) and Cout % 32 == 0:
                        # the parity mode's step: dy arrives pre-split from the BatchNorm backward (fp32 epilogue constants, halo window)
                        L.conv2d_dgrad_bn(FAKE, FAKE, FAKE, 0, FAKE, None, FAKE, FAKE, FAKE, FAKE, 2, FAKE, nsl_in, V, H, H, Cin, OH, OH, Cout,
                                          k, k, 1, pad, dtype | PS_IN, None)
                        kinds.append(('dgrad + BN-backward reduce (mode 2), pre-split dy', last()))
                        if 'reduce' in name:
                            L.conv2d_dgrad_bn(FAKE, FAKE, FAKE, 1, None, FAKE, None, None, None, None, 4, FAKE, nsl_in, V, H, H, Cin, OH, OH,
                                              Cout, k, k, 1, pad, dtype | PS_IN, None)
                            kinds.append(('dgrad + accumulate + BN-backward sums (mode 4), pre-split dy', last()))
                for kind, inst in kinds:
                    out.append((mode, name, cnt, kind, inst))
    finally:
        L.set_f32_matmul(0, 0)
        os.environ.pop('SIMCLR_DRY_RUN', None)
    return out


# weight-gradient operand formats: (name, storage dtype, flags of the dtype argument); SIMCLR_FMT_TERMS(t) = (t + 1) << 12
TERMS = lambda t: (t + 1) << 12
PS_IN = 0x100
WGRAD_MODES = [('bf16', 1, 0), ('f32 exact', 0, TERMS(0)), ('f32 bf16x3', 0, TERMS(3)), ('f32 bf16x6', 0, TERMS(6)),
               ('f32 bf16x3 pre-split dy', 0, TERMS(3) | PS_IN)]
# (name, K, H of the activation, launches per step): the fused bottleneck tail's Gram matrices at the row counts of the 56^2 and 28^2
# blocks (conv3 reads 64 channels in the three 56^2 blocks, 128 in the four 28^2 blocks; x0 = no ResNet-50 1x launch, the rule only)
GRAMS = [('gram 64 @56', 64, 56, 3), ('gram 128 @28', 128, 28, 4), ('gram 64 @28', 64, 28, 0), ('gram 128 @56', 128, 56, 0),
         ('gram 256 @56', 256, 56, 0), ('gram 256 @28', 256, 28, 0)]
GRAM_MODES = [('bf16', 1, 0), ('f32 exact', 0, TERMS(0)), ('f32 split', 0, TERMS(13))]


def stem_geometry(H=224, k=7, s=2):
    """simclr_amd.ops.stem_geometry for the 7x7 / stride-2 stem: packed image HP x WP, 8 taps per packed kernel row."""
    OH = (H + (k - 1) - k) // s + 1
    HP = max((OH - 1) * s + k, H + (k - 1) // 2)
    WP = (max((OH - 1) * s + 8, H + (k - 1) // 2) + 1) // 2 * 2
    return OH, HP, WP


def wgrad_rows(views):
    os.environ['SIMCLR_DRY_RUN'] = '1'
    from simclr_amd._lib import lib, SimclrHipError
    L = lib()
    out = []
    last = lambda: L.conv2d_last_instantiation().decode()
    V = views
    try:
        for mode, dtype, flags in WGRAD_MODES:
            for name, H, Cin, Cout, k, s, cnt in LAYERS:
                pad = (k - 1) // 2
                OH = (H + (k - 1) - k) // s + 1
                L.conv2d_wgrad(FAKE, FAKE, FAKE, 0, FAKE, V, H, H, Cin, Cin, OH, OH, Cout, k, k, s, pad, dtype | flags, None)
                out.append((mode, name, cnt, 'wgrad', last()))
            if not flags & PS_IN:        # the packed stem: one 'tap' per kernel row of 8 x 4 packed elements, pixel pitch 4
                OH, HP, WP = stem_geometry()
                L.conv2d_wgrad(FAKE, FAKE, FAKE, 0, FAKE, V, HP, WP, 32, 4, OH, OH, 64, 7, 1, 2, 0, dtype | flags, None)
                out.append((mode, 'stem 7x7 s2 3->64', 1, 'stem wgrad (multi-tap)', last()))
        OH, HP, WP = stem_geometry()
        L.stem_wgrad_ps(FAKE, FAKE, FAKE, 0, FAKE, V, HP, WP, OH, OH, 64, 7, 8, 2, None)
        out.append(('f32 bf16x3 pre-split dy', 'stem 7x7 s2 3->64', 1, 'stem wgrad (pre-split operands)', last()))
        for mode, dtype, flags in GRAM_MODES:
            for name, K, H, cnt in GRAMS:
                if K == 256 and dtype != 1:
                    continue
                L.conv2d_gram(FAKE, FAKE, FAKE, V * H * H, K, dtype | flags, None)
                out.append((mode, name, cnt, 'gram', last()))
    finally:
        os.environ.pop('SIMCLR_DRY_RUN', None)
    return out


def render_wgrad(views):
    lines = ['# weight-gradient / Gram kernel instantiation per (ResNet-50 1x layer class, operand format) at %d views' % views,
             '# generated by tools/instantiation_table.py --what wgrad (SIMCLR_DRY_RUN=1: decisions only, no device); columns:',
             '# operand format | layer class | launches per step of this class | launch kind | instantiation record', '']
    for mode, name, cnt, kind, inst in wgrad_rows(views):
        lines.append(' | '.join([mode, name, 'x%d' % cnt, kind, inst]))
    return '\n'.join(lines) + '\n'


def render(views):
    lines = ['# forward / data-gradient kernel instantiation per (ResNet-50 1x layer class, launch kind, storage mode) at %d views' % views,
             '# generated by tools/instantiation_table.py (SIMCLR_DRY_RUN=1: decisions only, no device); columns:',
             '# mode | layer class | launches per step of this class | launch kind | instantiation record', '']
    for mode, name, cnt, kind, inst in rows(views):
        lines.append(' | '.join([mode, name, 'x%d' % cnt, kind, inst]))
    return '\n'.join(lines) + '\n'


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--views', type=int, default=1024)
    ap.add_argument('--out', default=None)
    ap.add_argument('--what', choices=['igemm', 'wgrad'], default='igemm', help='forward / data-gradient table (default) or weight-gradient table')
    a = ap.parse_args()
    txt = render_wgrad(a.views) if a.what == 'wgrad' else render(a.views)
    if a.out:
        open(a.out, 'w').write(txt)
        print('wrote %d rows to %s' % (txt.count('\n') - 4, a.out))
    else:
        sys.stdout.write(txt)
