"""Per-layer micro-benchmark of the hot kernels at ResNet-50 1x / 224 px / V views per GPU.

python tools/microbench.py [--views 1024] [--dtype bf16] [--what conv,bn,ntxent,lars,gcl,supcon,hcl,nnclr,barlow,vicreg,byol,moco,dino,swav,swav_multicrop,dino_multicrop,dropblock,knn,repr,logreg,kmeans,spectrum,spectrum_eval]
Prints one line per distinct layer shape: time (us), TFLOP/s, algorithmic GB/s; and a per-step
total weighted by how often the shape occurs.  Timing: HIP events on the launch stream, median of
`--iters` launches after warm-up; inputs are random (never zeros: DVFS).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from simclr_amd import ops  # noqa: E402

# (H, Cin, Cout, k, stride, count) of every conv in ResNet-50 1x after the stem (tf2/resnet.py:385-526)
R50 = [
    (56, 64, 256, 1, 1, 1),    # g1 shortcut
    (56, 64, 64, 1, 1, 1), (56, 256, 64, 1, 1, 2), (56, 64, 64, 3, 1, 3), (56, 64, 256, 1, 1, 3),
    (56, 256, 512, 1, 2, 1),   # g2 shortcut
    (56, 256, 128, 1, 1, 1), (56, 128, 128, 3, 2, 1), (28, 512, 128, 1, 1, 3), (28, 128, 128, 3, 1, 3),
    (28, 128, 512, 1, 1, 4),
    (28, 512, 1024, 1, 2, 1),  # g3 shortcut
    (28, 512, 256, 1, 1, 1), (28, 256, 256, 3, 2, 1), (14, 1024, 256, 1, 1, 5), (14, 256, 256, 3, 1, 5),
    (14, 256, 1024, 1, 1, 6),
    (14, 1024, 2048, 1, 2, 1),  # g4 shortcut
    (14, 1024, 512, 1, 1, 1), (14, 512, 512, 3, 2, 1), (7, 2048, 512, 1, 1, 2), (7, 512, 512, 3, 1, 2),
    (7, 512, 2048, 1, 1, 3),
]


def timeit(fn, iters, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--views', type=int, default=1024)
    ap.add_argument('--dtype', default='bf16')
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--what', default='conv,bn,ntxent,lars')
    ap.add_argument('--out', default='gpurun_out/microbench.json')
    ap.add_argument('--ps', action='store_true', help='--dtype f32 with three backward terms: time dgrad / wgrad on a pre-split gradient operand')
    ap.add_argument('--f32_matmul', default='exact', help="--dtype f32: matrix arithmetic (ops.set_f32_matmul), e.g. bf16x6_3 = the parity mode")
    args = ap.parse_args()
    if args.dtype != 'bf16':
        ops.set_f32_matmul(args.f32_matmul)
    dt = torch.bfloat16 if args.dtype == 'bf16' else torch.float32
    dev = 'cuda'
    V = args.views
    what = args.what.split(',')
    res = []
    tot = dict(fwd=0.0, fwd_nostats=0.0, dgrad=0.0, wgrad=0.0, bn_apply=0.0, bn_bwd=0.0)
    if 'conv' in what:
        print('%-26s %9s %9s %9s %9s | TF/s fwd dgrad wgrad | GB/s fwd' % ('layer', 'fwd_us', 'nostat_us', 'dgrad_us', 'wgrad_us'))
        for (H, Cin, Cout, k, s, cnt) in R50:
            pad = (k - 1) // 2
            OH = (H + (k - 1) - k) // s + 1
            x = torch.randn(V, H, H, Cin, device=dev).to(dt)
            w = (torch.randn(k, k, Cin, Cout, device=dev) * (k * k * Cin) ** -0.5)
            dy = torch.randn(V, OH, OH, Cout, device=dev).to(dt)
            w_t = ops.prep_weights(w, 0, dt); w_d = ops.prep_weights(w, 1, dt)
            y = torch.empty(V, OH, OH, Cout, device=dev, dtype=dt)
            dx = torch.empty(V, H, H, Cin, device=dev, dtype=dt)
            dw = torch.empty(k * k * Cin, Cout, device=dev)
            stats = ops.conv_stats(V * OH * OH, Cout, dev)
            if args.ps and dt == torch.float32 and Cout % 32 == 0 and Cin % 64 == 0:
                # the gradient operand as the BatchNorm backward hands it over in the parity mode: pre-split (hi, lo) bf16 pieces
                one, zero = torch.ones(Cout, device=dev), torch.zeros(Cout, device=dev)
                dy, _ = ops.bn_bwd_apply(dy, dy, None, one, zero, zero, one, zero, zero, 0, ps_out=True)
            t_f = timeit(lambda: ops.conv2d_fwd(x, w_t, k, k, s, pad, OH, OH, stats=stats, out=y), args.iters)
            t_n = timeit(lambda: ops.conv2d_fwd(x, w_t, k, k, s, pad, OH, OH, stats=None, out=y), args.iters)
            t_d = timeit(lambda: ops.conv2d_dgrad(dy, w_d, k, k, s, pad, H, H, out=dx), args.iters)
            t_w = timeit(lambda: ops.conv2d_wgrad(x, dy, k, k, s, pad, out=dw), args.iters)
            t_db = 0.0
            if s == 1:      # dgrad with the fused BatchNorm-backward reduce (mask recomputed from the BN input: mode 2)
                bn = dict(x=x, mask=None, scale=torch.rand(Cin, device=dev) - 0.4, shift=torch.randn(Cin, device=dev) * 0.3,
                          mean=torch.randn(Cin, device=dev) * 0.2, rstd=torch.rand(Cin, device=dev) + 0.5, mode=2)
                t_db = timeit(lambda: ops.conv2d_dgrad_bn(dy, w_d, k, k, pad, H, H, bn, out=dx), args.iters)
            fl = 2.0 * V * OH * OH * k * k * Cin * Cout
            by = x.element_size() * (x.numel() + y.numel())
            name = '%dx%d %d->%d k%d s%d x%d' % (H, H, Cin, Cout, k, s, cnt)
            print('%-26s %9.0f %9.0f %9.0f %9.0f | %6.0f %6.0f %6.0f | %6.0f | dgrad_bn %4.0f' % (
                name, t_f, t_n, t_d, t_w, fl / t_f / 1e6, fl / t_d / 1e6, fl / t_w / 1e6, by / t_f / 1e3, t_db), flush=True)
            res.append(dict(layer=name, fwd_us=t_f, fwd_nostats_us=t_n, dgrad_us=t_d, wgrad_us=t_w, dgrad_bn_us=t_db, flops=fl,
                            bytes=by, count=cnt))
            tot['fwd'] += cnt * t_f; tot['fwd_nostats'] += cnt * t_n; tot['dgrad'] += cnt * t_d; tot['wgrad'] += cnt * t_w
            del x, dy, y, dx
        print('per-step totals (ms): fwd %.2f (no stats %.2f)  dgrad %.2f  wgrad %.2f' % (
            tot['fwd'] / 1e3, tot['fwd_nostats'] / 1e3, tot['dgrad'] / 1e3, tot['wgrad'] / 1e3), flush=True)
    if 'epi' in what:
        # A/B of the fp32 reduce epilogue (--dtype f32 --f32_matmul f16x3_3): SIMCLR_F32_EPI_BATCH = 0 (per-fragment loop) / 1 (operands of
        # a fragment row requested before the previous row is stored), read per launch, so both sides run in this process on the
        # same buffers.  Rows: dgrad + BatchNorm-backward reduce with mask mode 2 (store) and mode 4 + accumulate (conv1 of a block adds
        # to the shortcut gradient); bytes = every tensor pass of the launch once.
        assert dt == torch.float32, '--what epi times the fp32 epilogues'
        print('%-22s %-14s | us 0 / 1 | TB/s 0 / 1' % ('layer', 'launch'))

        def ab(fn):
            ts = []
            for sw in ('0', '1'):
                os.environ['SIMCLR_F32_EPI_BATCH'] = sw
                ts.append(timeit(fn, args.iters))
            os.environ.pop('SIMCLR_F32_EPI_BATCH')
            return ts
        tot_e = {}
        for (H, Cin, Cout, k, s, cnt) in R50:
            if s != 1 or Cout % 32 or Cin % 64:
                continue
            pad = (k - 1) // 2
            M = V * H * H
            w = torch.randn(k, k, Cin, Cout, device=dev) * (k * k * Cin) ** -0.5
            w_d = ops.prep_weights(w, 1, dt)
            dy = torch.randn(V, H, H, Cout, device=dev)
            one, zero = torch.ones(Cout, device=dev), torch.zeros(Cout, device=dev)
            dy, _ = ops.bn_bwd_apply(dy, dy, None, one, zero, zero, one, zero, zero, 0, ps_out=True)
            x = torch.randn(V, H, H, Cin, device=dev)
            dx = torch.randn(V, H, H, Cin, device=dev)
            rows = []
            bn2 = dict(x=x, mask=None, scale=torch.rand(Cin, device=dev) - 0.4, shift=torch.randn(Cin, device=dev) * 0.3,
                       mean=torch.randn(Cin, device=dev) * 0.2, rstd=torch.rand(Cin, device=dev) + 0.5, mode=2)
            rows.append(('dgrad_bn m2', 4.0 * M * (Cout + 2 * Cin), lambda: ops.conv2d_dgrad_bn(dy, w_d, k, k, pad, H, H, bn2, out=dx)))
            if k == 1 and Cin > Cout:
                bn4 = dict(mask=(torch.rand(M, Cin // 4, device=dev) * 16).to(torch.uint8), mode=4)
                rows.append(('dgrad_bn m4+acc', 4.0 * M * (Cout + 2 * Cin) + M * Cin / 4,
                             lambda: ops.conv2d_dgrad_bn(dy, w_d, k, k, pad, H, H, bn4, out=dx, accumulate=True)))
            name = '%dx%d %d->%d k%d x%d' % (H, H, Cin, Cout, k, cnt)
            for kind, nbytes, fn in rows:
                t0, t1 = ab(fn)
                print('%-22s %-14s | %6.0f %6.0f | %5.2f %5.2f' % (name, kind, t0, t1, nbytes / t0 / 1e6, nbytes / t1 / 1e6), flush=True)
                res.append(dict(layer=name, launch=kind, count=cnt, bytes=nbytes, us_switch0=t0, us_switch1=t1))
                e = tot_e.setdefault(kind, [0.0, 0.0])
                e[0] += cnt * t0; e[1] += cnt * t1
            del x, dx, dy, rows
        for kind, (t0, t1) in tot_e.items():
            print('weighted total %-14s: %.2f -> %.2f ms (every layer class x its count; a step launches each kind on a subset)' % (kind, t0 / 1e3, t1 / 1e3))
    if 'nwalk' in what:
        # A/B of the walk of the persistent implicit GEMM on the short-K 1x1 layers with a wide output (--dtype f32 --f32_matmul f16x3_3):
        # SIMCLR_IGEMM_NWALK = 0 (a workgroup owns an N-tile and walks M-tiles) / 1 (a workgroup owns an M-tile and walks its N-tiles,
        # csrc/igemm_nwalk.h), read per launch, so both sides run in this process on the same buffers.  Rows: the 13 launches of a step
        # in the forms the step uses -- the fused bottleneck tail (conv3 + bn3 + shortcut + ReLU + mask bits; FAS 2 = the shortcut has
        # its own BatchNorm: first block of a stage) and conv1's data gradient with the fused BatchNorm-backward reduce on a pre-split dy
        # (mask mode 2 store, mask bits + accumulate) -- each with its narrow-output twin (same M, K and N swapped: same algorithmic
        # bytes and FLOPs).  bytes = every tensor pass of the launch once.  A class without an N-inner instantiation runs the same
        # kernel in both columns: their difference is the noise of the row.
        assert dt == torch.float32, '--what nwalk times the fp32 launches'
        print('%-34s %-16s | us 0 / 1 | TB/s 0 / 1 | kernel with the switch on' % ('layer', 'launch'))
        from simclr_amd._lib import lib as _lib

        def ab_nw(fn):
            ts, rec = [], ''
            for sw in ('0', '1'):
                os.environ['SIMCLR_IGEMM_NWALK'] = sw
                ts.append(timeit(fn, args.iters))
                rec = _lib().conv2d_last_instantiation().decode()
            os.environ.pop('SIMCLR_IGEMM_NWALK')
            return ts[0], ts[1], rec.split(')')[0].lstrip('(')
        tot_n = {}
        # (H, channels of the narrow side, of the wide side, fused tails with a plain / BatchNorm shortcut, conv1 data gradients per step)
        for (H, Cn, Cw, n_fas1, n_fas2, n_dg) in [(56, 64, 256, 2, 1, 2), (56, 128, 256, 0, 0, 1), (28, 128, 512, 3, 1, 3)]:
            M = V * H * H
            for twin in (False, True):
                K, N = (Cw, Cn) if twin else (Cn, Cw)
                x = torch.randn(V, H, H, K, device=dev)
                w = torch.randn(1, 1, K, N, device=dev) * K ** -0.5
                w_t = ops.prep_weights(w, 0, dt)
                resid = torch.randn(V, H, H, N, device=dev)
                scale, shift = torch.rand(N, device=dev) + 0.5, torch.randn(N, device=dev) * 0.2
                rs, rb = torch.rand(N, device=dev) + 0.5, torch.randn(N, device=dev) * 0.3
                rows = []
                nb_tail = 4.0 * M * (K + 2 * N) + M * N / 4
                if n_fas1 or n_fas2:
                    rows.append(('tail FAS1', n_fas1, nb_tail,
                                 lambda: ops.conv2d_fwd_bn_apply(x, w_t, 1, 1, 1, 0, H, H, scale, shift, res=resid, relu=True, want_bits=True)))
                    rows.append(('tail FAS2', n_fas2, nb_tail,
                                 lambda: ops.conv2d_fwd_bn_apply(x, w_t, 1, 1, 1, 0, H, H, scale, shift, res=resid, relu=True, want_bits=True,
                                                                 rscale=rs, rshift=rb)))
                # data gradient of a K <- N convolution's twin: dy has K channels, dx (and the producer BatchNorm's input) N
                w_d = ops.prep_weights(torch.randn(1, 1, N, K, device=dev) * N ** -0.5, 1, dt)
                one, zero = torch.ones(K, device=dev), torch.zeros(K, device=dev)
                dy, _ = ops.bn_bwd_apply(x, x, None, one, zero, zero, one, zero, zero, 0, ps_out=True)
                bn2 = dict(x=resid, mask=None, scale=torch.rand(N, device=dev) - 0.4, shift=torch.randn(N, device=dev) * 0.3,
                           mean=torch.randn(N, device=dev) * 0.2, rstd=torch.rand(N, device=dev) + 0.5, mode=2)
                bn4 = dict(mask=(torch.rand(M, N // 4, device=dev) * 16).to(torch.uint8), mode=4)
                dx = torch.randn(V, H, H, N, device=dev)
                rows.append(('dgrad_bn m2', 0, 4.0 * M * (K + 2 * N), lambda: ops.conv2d_dgrad_bn(dy, w_d, 1, 1, 0, H, H, bn2, out=dx)))
                rows.append(('dgrad_bn m4+acc', n_dg, 4.0 * M * (K + 2 * N) + M * N / 4,
                             lambda: ops.conv2d_dgrad_bn(dy, w_d, 1, 1, 0, H, H, bn4, out=dx, accumulate=True)))
                name = '%dx%d %d->%d%s' % (H, H, K, N, ' (narrow twin)' if twin else '')
                for kind, cnt, nbytes, fn in rows:
                    t0, t1, kern = ab_nw(fn)
                    print('%-34s %-16s | %6.0f %6.0f | %5.2f %5.2f | %s' % (name, kind, t0, t1, nbytes / t0 / 1e6, nbytes / t1 / 1e6, kern), flush=True)
                    res.append(dict(layer=name, launch=kind, twin=twin, count=0 if twin else cnt, bytes=nbytes, us_switch0=t0, us_switch1=t1,
                                    kernel_switch1=kern))
                    if not twin:
                        e = tot_n.setdefault(kind, [0.0, 0.0])
                        e[0] += cnt * t0; e[1] += cnt * t1
                del x, resid, dy, dx, rows, bn2, bn4
        for kind, (t0, t1) in tot_n.items():
            print('per step %-16s: %.2f -> %.2f ms (each target launch x its count in a ResNet-50 step)' % (kind, t0 / 1e3, t1 / 1e3))
    if 'tile' in what:
        # A/B of the forward / dgrad tile: default (128-wide) vs SIMCLR_IGEMM_TILE=256 on every layer whose width allows it
        print('%-26s | fwd+stats 128 / 256 | fwd 128 / 256 | dgrad 128 / 256 | dgrad_bn 128 / 256  (us)' % 'layer')
        tot = [0.0] * 8
        for (H, Cin, Cout, k, s, cnt) in R50:
            if Cout % 256 and Cin % 256:
                continue
            pad = (k - 1) // 2
            OH = (H + (k - 1) - k) // s + 1
            x = torch.randn(V, H, H, Cin, device=dev).to(dt)
            w = (torch.randn(k, k, Cin, Cout, device=dev) * (k * k * Cin) ** -0.5)
            dy = torch.randn(V, OH, OH, Cout, device=dev).to(dt)
            w_t = ops.prep_weights(w, 0, dt); w_d = ops.prep_weights(w, 1, dt)
            y = torch.empty(V, OH, OH, Cout, device=dev, dtype=dt)
            dx = torch.empty(V, H, H, Cin, device=dev, dtype=dt)
            stats = ops.conv_stats(V * OH * OH, Cout, dev)
            bn = dict(x=x, mask=None, scale=torch.rand(Cin, device=dev) - 0.4, shift=torch.randn(Cin, device=dev) * 0.3,
                      mean=torch.randn(Cin, device=dev) * 0.2, rstd=torch.rand(Cin, device=dev) + 0.5, mode=2)
            ts = []
            for tile in ('128', '256'):
                os.environ['SIMCLR_IGEMM_TILE'] = tile
                ts.append(timeit(lambda: ops.conv2d_fwd(x, w_t, k, k, s, pad, OH, OH, stats=stats, out=y), args.iters))
                ts.append(timeit(lambda: ops.conv2d_fwd(x, w_t, k, k, s, pad, OH, OH, stats=None, out=y), args.iters))
                ts.append(timeit(lambda: ops.conv2d_dgrad(dy, w_d, k, k, s, pad, H, H, out=dx), args.iters))
                ts.append(timeit(lambda: ops.conv2d_dgrad_bn(dy, w_d, k, k, pad, H, H, bn, out=dx), args.iters) if s == 1 else 0.0)
            os.environ.pop('SIMCLR_IGEMM_TILE')
            name = '%dx%d %d->%d k%d s%d x%d' % (H, H, Cin, Cout, k, s, cnt)
            print('%-26s | %6.0f %6.0f | %6.0f %6.0f | %6.0f %6.0f | %6.0f %6.0f' % (
                name, ts[0], ts[4], ts[1], ts[5], ts[2], ts[6], ts[3], ts[7]), flush=True)
            res.append(dict(layer='tile ' + name, t128=ts[:4], t256=ts[4:], count=cnt))
            for i in range(8):
                tot[i] += cnt * ts[i]
            del x, dy, y, dx
        print('weighted totals (ms): fwd+stats %.2f / %.2f  fwd %.2f / %.2f  dgrad %.2f / %.2f  dgrad_bn %.2f / %.2f' % (
            tot[0] / 1e3, tot[4] / 1e3, tot[1] / 1e3, tot[5] / 1e3, tot[2] / 1e3, tot[6] / 1e3, tot[3] / 1e3, tot[7] / 1e3), flush=True)
    if 'wide' in what:
        # A/B of the forward / dgrad schedules, us per launch: 128-wide persistent tiles without / with the split tail, the
        # eight-phase 256 x 256 tile (csrc/igemm_wide.h) without / with it.  Columns: fwd+stats, dgrad, dgrad + BN reduce.
        cfgs = [('narrow', dict(SIMCLR_IGEMM_SPLIT='0')), ('narrow+split', {}), ('wide', dict(SIMCLR_IGEMM_WIDE='2', SIMCLR_IGEMM_SPLIT='0')),
                ('wide+split', dict(SIMCLR_IGEMM_WIDE='2'))]
        print('%-26s | %s' % ('layer', ' | '.join('%-22s' % c[0] for c in cfgs)))
        tot = {c[0]: [0.0, 0.0, 0.0] for c in cfgs}
        for (H, Cin, Cout, k, s, cnt) in R50:
            if Cout % 256 and Cin % 256:
                continue
            pad = (k - 1) // 2
            OH = (H + (k - 1) - k) // s + 1
            x = torch.randn(V, H, H, Cin, device=dev).to(dt)
            w = (torch.randn(k, k, Cin, Cout, device=dev) * (k * k * Cin) ** -0.5)
            dy = torch.randn(V, OH, OH, Cout, device=dev).to(dt)
            w_t = ops.prep_weights(w, 0, dt); w_d = ops.prep_weights(w, 1, dt)
            y = torch.empty(V, OH, OH, Cout, device=dev, dtype=dt)
            dx = torch.empty(V, H, H, Cin, device=dev, dtype=dt)
            stats = ops.conv_stats(V * OH * OH, Cout, dev)
            bn = dict(x=x, mask=None, scale=torch.rand(Cin, device=dev) - 0.4, shift=torch.randn(Cin, device=dev) * 0.3,
                      mean=torch.randn(Cin, device=dev) * 0.2, rstd=torch.rand(Cin, device=dev) + 0.5, mode=2)
            row = {}
            for name, env in cfgs:
                for kk, vv in env.items():
                    os.environ[kk] = vv
                ts = [timeit(lambda: ops.conv2d_fwd(x, w_t, k, k, s, pad, OH, OH, stats=stats, out=y), args.iters),
                      timeit(lambda: ops.conv2d_dgrad(dy, w_d, k, k, s, pad, H, H, out=dx), args.iters),
                      timeit(lambda: ops.conv2d_dgrad_bn(dy, w_d, k, k, pad, H, H, bn, out=dx), args.iters) if s == 1 else 0.0]
                for kk in env:
                    os.environ.pop(kk)
                row[name] = ts
                for i in range(3):
                    tot[name][i] += cnt * ts[i]
            name = '%dx%d %d->%d k%d s%d x%d' % (H, H, Cin, Cout, k, s, cnt)
            print('%-26s | %s' % (name, ' | '.join('%6.0f %6.0f %6.0f  ' % tuple(row[c[0]]) for c in cfgs)), flush=True)
            res.append(dict(layer='wide ' + name, count=cnt, **row))
            del x, dy, y, dx
        print('%-26s | %s' % ('weighted totals (ms)', ' | '.join('%6.2f %6.2f %6.2f  ' % tuple(v / 1e3 for v in tot[c[0]]) for c in cfgs)), flush=True)
    if 'comparator' in what:
        # the vendor libraries on the SAME shapes, as a yardstick only (never on the product path):
        # MIOpen through torch.nn.functional.conv2d (bf16, channels_last = NHWC memory) forward / data gradient / weight
        # gradient, and hipBLASLt through torch.matmul for the 1x1 stride-1 layers (the same GEMMs without the conv wrapper).
        import torch.nn.functional as F
        torch.backends.cudnn.benchmark = os.environ.get('SIMCLR_CMP_FIND', '0') == '1'     # default: MIOpen immediate mode (heuristic pick)
        print('%-26s | ours fwd dgrad wgrad | MIOpen fwd dgrad wgrad | hipBLASLt fwd dgrad wgrad | bound us (MFMA / HBM@8)' % 'layer')
        for (H, Cin, Cout, k, s, cnt) in R50:
            pad = (k - 1) // 2
            OH = (H + (k - 1) - k) // s + 1
            x = torch.randn(V, H, H, Cin, device=dev).to(dt)
            w = (torch.randn(k, k, Cin, Cout, device=dev) * (k * k * Cin) ** -0.5)
            dy = torch.randn(V, OH, OH, Cout, device=dev).to(dt)
            w_t = ops.prep_weights(w, 0, dt); w_d = ops.prep_weights(w, 1, dt)
            y = torch.empty(V, OH, OH, Cout, device=dev, dtype=dt)
            dx = torch.empty(V, H, H, Cin, device=dev, dtype=dt)
            dw = torch.empty(k * k * Cin, Cout, device=dev)
            ours = [timeit(lambda: ops.conv2d_fwd(x, w_t, k, k, s, pad, OH, OH, stats=None, out=y), args.iters),
                    timeit(lambda: ops.conv2d_dgrad(dy, w_d, k, k, s, pad, H, H, out=dx), args.iters),
                    timeit(lambda: ops.conv2d_wgrad(x, dy, k, k, s, pad, out=dw), args.iters)]
            xn = x.permute(0, 3, 1, 2)                       # NCHW view of the NHWC tensor = channels_last
            dyn = dy.permute(0, 3, 1, 2)
            wn = w.permute(3, 2, 0, 1).to(dt).contiguous(memory_format=torch.channels_last)
            mi = [float('nan')] * 3
            try:
                mi[0] = timeit(lambda: F.conv2d(xn, wn, None, s, pad), args.iters)
                mi[1] = timeit(lambda: torch.ops.aten.convolution_backward(dyn, xn, wn, None, [s, s], [pad, pad], [1, 1], False, [0, 0], 1, [True, False, False]), args.iters)
                mi[2] = timeit(lambda: torch.ops.aten.convolution_backward(dyn, xn, wn, None, [s, s], [pad, pad], [1, 1], False, [0, 0], 1, [False, True, False]), args.iters)
            except Exception as e:  # noqa: BLE001
                print('   MIOpen failed on this shape:', repr(e)[:200])
            bl = [float('nan')] * 3
            if k == 1 and s == 1:
                A = x.view(-1, Cin); G = dy.view(-1, Cout); W2 = w.view(Cin, Cout).to(dt); W2t = W2.t().contiguous()
                bl = [timeit(lambda: torch.matmul(A, W2), args.iters), timeit(lambda: torch.matmul(G, W2t), args.iters),
                      timeit(lambda: torch.matmul(A.t(), G), args.iters)]
            fl = 2.0 * V * OH * OH * k * k * Cin * Cout
            by = x.element_size() * (x.numel() + y.numel() + w.numel())
            name = '%dx%d %d->%d k%d s%d x%d' % (H, H, Cin, Cout, k, s, cnt)
            print('%-26s | %5.0f %5.0f %5.0f | %5.0f %5.0f %5.0f | %5.0f %5.0f %5.0f | %4.0f / %4.0f' % (
                name, *ours, *mi, *bl, fl / 2.5e9, by / 8e6), flush=True)
            res.append(dict(layer='cmp ' + name, ours=ours, miopen=mi, hipblaslt=bl, flops=fl, bytes=by, count=cnt))
            del x, dy, y, dx, xn, dyn
    if 'bn' in what:
        print('%-22s %9s %9s %9s %9s | GB/s apply resid bwd_red bwd_app' % ('tensor', 'apply_us', 'resid_us', 'bwdred_us', 'bwdapp_us'))
        shapes = [(56, 64, 7), (56, 256, 4), (28, 128, 8), (28, 512, 5), (14, 256, 12), (14, 1024, 7), (7, 512, 6), (7, 2048, 4)]
        for (H, C, cnt) in shapes:
            x = torch.randn(V, H, H, C, device=dev).to(dt)
            r = torch.randn(V, H, H, C, device=dev).to(dt)
            dy = torch.randn(V, H, H, C, device=dev).to(dt)
            y = torch.empty_like(x); dx = torch.empty_like(x)
            scale = torch.rand(C, device=dev) + 0.5; shift = torch.randn(C, device=dev) * 0.1
            mean = torch.randn(C, device=dev) * 0.1; rstd = torch.rand(C, device=dev) + 0.5
            c1 = torch.randn(C, device=dev) * 0.01; c2 = torch.randn(C, device=dev) * 0.01
            t_a = timeit(lambda: ops.bn_apply(x, scale, shift, True, out=y), args.iters)
            t_r = timeit(lambda: ops.bn_apply(x, scale, shift, True, res=r, out=y), args.iters)
            t_br = timeit(lambda: ops.bn_bwd_reduce(dy, x, y, scale, shift, mean, rstd, 1), args.iters)
            t_ba = timeit(lambda: ops.bn_bwd_apply(dy, x, y, scale, shift, mean, rstd, c1, c2, 1, out=dx), args.iters)
            nb = x.numel() * x.element_size()
            print('%-22s %9.0f %9.0f %9.0f %9.0f | %6.0f %6.0f %6.0f %6.0f' % (
                '%dx%d C%d x%d' % (H, H, C, cnt), t_a, t_r, t_br, t_ba, 2 * nb / t_a / 1e3, 3 * nb / t_r / 1e3,
                3 * nb / t_br / 1e3, 4 * nb / t_ba / 1e3), flush=True)
            res.append(dict(layer='bn %dx%d C%d' % (H, H, C), apply_us=t_a, resid_us=t_r, bwdred_us=t_br, bwdapp_us=t_ba, bytes=nb, count=cnt))
            del x, r, dy, y, dx
    if 'ntxent' in what:
        for (n, N) in [(512, 512), (512, 4096), (256, 2048), (4096, 4096)]:
            D = 128
            zl = torch.nn.functional.normalize(torch.randn(2 * n, D, device=dev), dim=1)
            za = torch.nn.functional.normalize(torch.randn(2 * N, D, device=dev), dim=1)
            za[:n] = zl[:n]; za[N:N + n] = zl[n:]
            ws = ops.ntxent_workspace(n, N, D, dev)
            fl = 24.0 * n * N * D
            by = 2.0 * (2 * n + 2 * N) * D * 4
            for split in (False, True):        # exact fp32-input MFMA sweeps | the opt-in split-fp16 sweeps (FLAGS.ntxent_matmul='f16x3')
                out, rs, _ = ops.ntxent_fwd(zl, za, 0, 0.1, ws, split=split)
                t_f = timeit(lambda: ops.ntxent_fwd(zl, za, 0, 0.1, ws, split=split), args.iters)
                t_b = timeit(lambda: ops.ntxent_bwd(zl, za, 0, 0.1, rs, 1.0, out, ws, split=split), args.iters)
                print('ntxent n=%d N=%d %s: fwd %.0f us bwd %.0f us | fused fwd+bwd %.1f TF/s (24nND), algorithmic %.1f GB/s' % (
                    n, N, 'f16x3' if split else 'exact', t_f, t_b, fl / (t_f + t_b) / 1e6, by / (t_f + t_b) / 1e3), flush=True)
                res.append(dict(layer='ntxent n%d N%d%s' % (n, N, ' f16x3' if split else ''), fwd_us=t_f, bwd_us=t_b, flops=fl, bytes=by))
        # the wide path (D > 256: proj_out_dim > 256, proj_head_mode=none), exact fp32-input MFMA; matrix FLOPs: forward S = 8nND,
        # backward S again + dS K + dS^T Q = 24nND
        for (n, N, D) in [(512, 512, 2048), (512, 4096, 2048), (512, 4096, 512), (128, 1024, 8192)]:
            zl = torch.nn.functional.normalize(torch.randn(2 * n, D, device=dev), dim=1)
            za = torch.nn.functional.normalize(torch.randn(2 * N, D, device=dev), dim=1)
            za[:n] = zl[:n]; za[N:N + n] = zl[n:]
            ws = ops.ntxent_workspace(n, N, D, dev)
            out, rs, _ = ops.ntxent_fwd(zl, za, 0, 0.1, ws)
            t_f = timeit(lambda: ops.ntxent_fwd(zl, za, 0, 0.1, ws), args.iters)
            t_b = timeit(lambda: ops.ntxent_bwd(zl, za, 0, 0.1, rs, 1.0, out, ws), args.iters)
            ff, fb = 8.0 * n * N * D, 24.0 * n * N * D
            print('ntxent wide n=%d N=%d D=%d: fwd %.0f us (%.1f TF/s) bwd %.0f us (%.1f TF/s)' % (
                n, N, D, t_f, ff / t_f / 1e6, t_b, fb / t_b / 1e6), flush=True)
            res.append(dict(layer='ntxent wide n%d N%d D%d' % (n, N, D), fwd_us=t_f, bwd_us=t_b, fwd_flops=ff, bwd_flops=fb))
            del zl, za, ws, out, rs
    if 'gcl' in what:
        # generalized contrastive loss (csrc/gcl.hip) at the NT-Xent table's shapes, beside NT-Xent's exact sweeps: the decoupled sweep, and
        # the SWD launches (two projections + sort-and-match + reduce | back-projection + combine) where 2N <= 8192 rows fit a column sort
        for (n, N) in [(512, 512), (512, 4096), (256, 2048), (4096, 4096)]:
            D = 128
            zl = torch.nn.functional.normalize(torch.randn(2 * n, D, device=dev), dim=1)
            za = torch.nn.functional.normalize(torch.randn(2 * N, D, device=dev), dim=1)
            za[:n] = zl[:n]; za[N:N + n] = zl[n:]
            ws = ops.ntxent_workspace(n, N, D, dev)
            out, rs, _ = ops.ntxent_fwd(zl, za, 0, 0.1, ws)
            row = dict(layer='gcl n%d N%d' % (n, N),
                       ntxent_fwd_us=timeit(lambda: ops.ntxent_fwd(zl, za, 0, 0.1, ws), args.iters),
                       ntxent_bwd_us=timeit(lambda: ops.ntxent_bwd(zl, za, 0, 0.1, rs, 1.0, out, ws), args.iters))
            gws = ops.gcl_lse_workspace(n, N, D, dev)
            _, grs, _ = ops.gcl_lse_fwd(zl, za, 0.1, ws=gws)
            row['lse_fwd_us'] = timeit(lambda: ops.gcl_lse_fwd(zl, za, 0.1, ws=gws), args.iters)
            row['lse_bwd_us'] = timeit(lambda: ops.gcl_lse_bwd(zl, za, 0.1, grs, 1.0, gws, skip_self=True), args.iters)
            M = 2 * N
            if M <= ops.SWD_MAX_ROWS:
                w = torch.linalg.qr(torch.randn(D, D))[0].contiguous().to(dev)
                wt = w.t().contiguous()
                prior = torch.nn.functional.normalize(torch.randn(M, D, device=dev), dim=1)

                def swd_fwd():
                    pt, qt = ops.gcl_gemm_nt(wt, za), ops.gcl_gemm_nt(wt, prior)
                    dp, cl, _ = ops.swd_sort_match(pt, qt, 2.0 / (D * M))
                    ops.gcl_swd_out(cl, zl, M)
                    return pt, qt, dp
                pt, qt, dp = swd_fwd()
                row['swd_fwd_us'] = timeit(swd_fwd, args.iters)
                row['swd_sort_us'] = timeit(lambda: ops.swd_sort_match(pt, qt, 2.0 / (D * M)), args.iters)
                row['swd_bwd_us'] = timeit(lambda: ops.gcl_swd_bwd(ops.gcl_gemm_nt(dp, w), zl, 0, 1.0), args.iters)
            print('gcl n=%d N=%d: ' % (n, N) + ' '.join('%s %.0f' % (k[:-3], v) for k, v in row.items() if k != 'layer') + ' (us)', flush=True)
            res.append(row)
            del zl, za, ws, gws
    if 'supcon' in what:
        # supervised contrastive loss (csrc/supcon.hip) beside the closest existing sweeps at the same shapes in the same run: the decoupled
        # sweep of csrc/gcl.hip and NT-Xent's exact sweeps.  Matrix FLOPs: forward S = 8nND, backward S again + dS K + dS^T Q = 24nND.
        # Labels: 100 classes drawn at random (about 2N / 100 positives per row).
        for (n, N) in [(512, 512), (512, 4096)]:
            D = 128
            zl = torch.nn.functional.normalize(torch.randn(2 * n, D, device=dev), dim=1)
            za = torch.nn.functional.normalize(torch.randn(2 * N, D, device=dev), dim=1)
            za[:n] = zl[:n]; za[N:N + n] = zl[n:]
            labels = torch.randint(0, 100, (N,), device=dev, dtype=torch.int32)
            ff, fb = 8.0 * n * N * D, 24.0 * n * N * D
            ws = ops.ntxent_workspace(n, N, D, dev)
            out, rs, _ = ops.ntxent_fwd(zl, za, 0, 0.1, ws)
            gws = ops.gcl_lse_workspace(n, N, D, dev)
            _, grs, _ = ops.gcl_lse_fwd(zl, za, 0.1, ws=gws)
            sws = ops.supcon_workspace(n, N, D, dev)
            _, srs, _ = ops.supcon_fwd(zl, za, labels, 0, 0.1, ws=sws)
            row = dict(layer='supcon n%d N%d D%d' % (n, N, D), fwd_flops=ff, bwd_flops=fb,
                       supcon_fwd_us=timeit(lambda: ops.supcon_fwd(zl, za, labels, 0, 0.1, ws=sws), args.iters),
                       supcon_bwd_us=timeit(lambda: ops.supcon_bwd(zl, za, labels, 0, 0.1, srs, 1.0, sws), args.iters),
                       gcl_lse_fwd_us=timeit(lambda: ops.gcl_lse_fwd(zl, za, 0.1, ws=gws), args.iters),
                       gcl_lse_bwd_us=timeit(lambda: ops.gcl_lse_bwd(zl, za, 0.1, grs, 1.0, gws, skip_self=True), args.iters),
                       ntxent_fwd_us=timeit(lambda: ops.ntxent_fwd(zl, za, 0, 0.1, ws), args.iters),
                       ntxent_bwd_us=timeit(lambda: ops.ntxent_bwd(zl, za, 0, 0.1, rs, 1.0, out, ws), args.iters))
            for k in ('supcon', 'gcl_lse', 'ntxent'):
                row[k + '_fwd_tfs'] = ff / row[k + '_fwd_us'] / 1e6
                row[k + '_bwd_tfs'] = fb / row[k + '_bwd_us'] / 1e6
            row['supcon_over_gcl_lse_fwd'] = row['supcon_fwd_us'] / row['gcl_lse_fwd_us']
            row['supcon_over_gcl_lse_bwd'] = row['supcon_bwd_us'] / row['gcl_lse_bwd_us']
            print('supcon n=%d N=%d D=%d: ' % (n, N, D) + ' | '.join(
                '%s fwd %.0f us (%.1f TF/s) bwd %.0f us (%.1f TF/s)' % (k, row[k + '_fwd_us'], row[k + '_fwd_tfs'], row[k + '_bwd_us'], row[k + '_bwd_tfs'])
                for k in ('supcon', 'gcl_lse', 'ntxent')) + ' | supcon / gcl_lse fwd %.2f bwd %.2f' % (
                    row['supcon_over_gcl_lse_fwd'], row['supcon_over_gcl_lse_bwd']), flush=True)
            res.append(row)
            del zl, za, ws, gws, sws
    if 'hcl' in what:
        # hard-negative / debiased NT-Xent (csrc/hcl.hip) beside the supervised contrastive sweeps and NT-Xent at the same shapes in the
        # same run: the median of --iters launches with [min, max].  beta = 0.5, tau_plus = 0.1 (both online pairs, both exp2 per element)
        # and beta = 0 (the second pair skipped).  Matrix FLOPs as supcon's: 8nND forward, 24nND backward.
        def spread(fn):
            ts = sorted(timeit(fn, 1, warm=0) for _ in range(args.iters))
            return dict(median=ts[len(ts) // 2], min=ts[0], max=ts[-1])
        for (n, N) in [(512, 512), (512, 4096)]:
            D = 128
            zl = torch.nn.functional.normalize(torch.randn(2 * n, D, device=dev), dim=1)
            za = torch.nn.functional.normalize(torch.randn(2 * N, D, device=dev), dim=1)
            za[:n] = zl[:n]; za[N:N + n] = zl[n:]
            labels = torch.randint(0, 100, (N,), device=dev, dtype=torch.int32)
            ws = ops.ntxent_workspace(n, N, D, dev)
            out, rs, _ = ops.ntxent_fwd(zl, za, 0, 0.1, ws)
            sws = ops.supcon_workspace(n, N, D, dev)
            _, srs, _ = ops.supcon_fwd(zl, za, labels, 0, 0.1, ws=sws)
            hws = ops.hcl_workspace(n, N, D, dev)
            _, hrs, _ = ops.hcl_fwd(zl, za, 0, 0.1, 0.5, 0.1, ws=hws)
            _, hrs0, _ = ops.hcl_fwd(zl, za, 0, 0.1, 0.0, 0.1, ws=hws)
            for fn in (lambda: ops.hcl_fwd(zl, za, 0, 0.1, 0.5, 0.1, ws=hws), lambda: ops.hcl_bwd(zl, za, 0, 0.1, 0.5, 0.1, hrs, 1.0, hws)):
                timeit(fn, 2)                                 # warm-up of every launch before the first timed one
            row = dict(layer='hcl n%d N%d D%d' % (n, N, D), fwd_flops=8.0 * n * N * D, bwd_flops=24.0 * n * N * D, iters=args.iters,
                       hcl_fwd_us=spread(lambda: ops.hcl_fwd(zl, za, 0, 0.1, 0.5, 0.1, ws=hws)),
                       hcl_bwd_us=spread(lambda: ops.hcl_bwd(zl, za, 0, 0.1, 0.5, 0.1, hrs, 1.0, hws)),
                       hcl_beta0_fwd_us=spread(lambda: ops.hcl_fwd(zl, za, 0, 0.1, 0.0, 0.1, ws=hws)),
                       hcl_beta0_bwd_us=spread(lambda: ops.hcl_bwd(zl, za, 0, 0.1, 0.0, 0.1, hrs0, 1.0, hws)),
                       supcon_fwd_us=spread(lambda: ops.supcon_fwd(zl, za, labels, 0, 0.1, ws=sws)),
                       supcon_bwd_us=spread(lambda: ops.supcon_bwd(zl, za, labels, 0, 0.1, srs, 1.0, sws)),
                       ntxent_fwd_us=spread(lambda: ops.ntxent_fwd(zl, za, 0, 0.1, ws)),
                       ntxent_bwd_us=spread(lambda: ops.ntxent_bwd(zl, za, 0, 0.1, rs, 1.0, out, ws)))
            print('hcl n=%d N=%d D=%d: ' % (n, N, D) + ' | '.join(
                '%s %.0f [%.0f, %.0f] us' % (k[:-3], v['median'], v['min'], v['max']) for k, v in row.items() if k.endswith('_us')), flush=True)
            res.append(row)
            del zl, za, ws, sws, hws
    if 'nnclr' in what:
        # NNCLR (csrc/nnclr.hip) beside NT-Xent and the supervised contrastive sweeps at the same (n, N, D) in the same run, and the new
        # cost of the step, the exact top-1 search of the 2n local rows in a K = 65536 queue (ops.knn_topk): the median of --iters
        # launches with [min, max].  Matrix FLOPs: 4nND forward (N candidate columns a row, not 2N), 8nND backward (the key side only).
        def spread(fn):
            ts = sorted(timeit(fn, 1, warm=0) for _ in range(args.iters))
            return dict(median=ts[len(ts) // 2], min=ts[0], max=ts[-1])
        K = 65536
        for (n, N) in [(512, 512), (512, 4096)]:
            D = 128
            zl = torch.nn.functional.normalize(torch.randn(2 * n, D, device=dev), dim=1)
            za = torch.nn.functional.normalize(torch.randn(2 * N, D, device=dev), dim=1)
            za[:n] = zl[:n]; za[N:N + n] = zl[n:]
            queue = torch.nn.functional.normalize(torch.randn(K, D, device=dev), dim=1)
            labels = torch.randint(0, 100, (N,), device=dev, dtype=torch.int32)
            ws = ops.ntxent_workspace(n, N, D, dev)
            out, rs, _ = ops.ntxent_fwd(zl, za, 0, 0.1, ws)
            sws = ops.supcon_workspace(n, N, D, dev)
            _, srs, _ = ops.supcon_fwd(zl, za, labels, 0, 0.1, ws=sws)
            _, idx = ops.knn_topk(zl, queue, 1)
            nn = queue.index_select(0, idx.reshape(-1).long())
            nws = ops.nnclr_workspace(n, N, D, dev)
            _, nrs, _ = ops.nnclr_fwd(nn, zl, za, 0, 0.1, ws=nws)
            for fn in (lambda: ops.nnclr_fwd(nn, zl, za, 0, 0.1, ws=nws), lambda: ops.nnclr_bwd(nn, za, 0, 0.1, nrs, 1.0, nws),
                       lambda: ops.knn_topk(zl, queue, 1)):
                timeit(fn, 2)                                 # warm-up of every launch before the first timed one
            row = dict(layer='nnclr n%d N%d D%d K%d' % (n, N, D, K), fwd_flops=4.0 * n * N * D, bwd_flops=8.0 * n * N * D,
                       search_flops=4.0 * n * K * D, iters=args.iters,
                       nnclr_fwd_us=spread(lambda: ops.nnclr_fwd(nn, zl, za, 0, 0.1, ws=nws)),
                       nnclr_bwd_us=spread(lambda: ops.nnclr_bwd(nn, za, 0, 0.1, nrs, 1.0, nws)),
                       nnclr_search_us=spread(lambda: ops.knn_topk(zl, queue, 1)),
                       nnclr_gather_us=spread(lambda: queue.index_select(0, idx.reshape(-1).long())),
                       supcon_fwd_us=spread(lambda: ops.supcon_fwd(zl, za, labels, 0, 0.1, ws=sws)),
                       supcon_bwd_us=spread(lambda: ops.supcon_bwd(zl, za, labels, 0, 0.1, srs, 1.0, sws)),
                       ntxent_fwd_us=spread(lambda: ops.ntxent_fwd(zl, za, 0, 0.1, ws)),
                       ntxent_bwd_us=spread(lambda: ops.ntxent_bwd(zl, za, 0, 0.1, rs, 1.0, out, ws)))
            print('nnclr n=%d N=%d D=%d K=%d: ' % (n, N, D, K) + ' | '.join(
                '%s %.0f [%.0f, %.0f] us' % (k[:-3], v['median'], v['min'], v['max']) for k, v in row.items() if k.endswith('_us')), flush=True)
            res.append(row)
            del zl, za, ws, sws, nws, queue
    if 'barlow' in what:
        # Barlow Twins loss (csrc/barlow.hip) beside NT-Xent at the same (n, N, D) in the same run: the register-resident sweeps at
        # D = 128, the wide kernels above 256 -- the same exact fp32-input MFMA.  Matrix FLOPs: the two Gram blocks 2 x 2nND = 4nND forward,
        # the two [n, N] x [N, D] products 4nND backward; NT-Xent 8nND / 24nND.  The forward also writes the [2, n, N] blocks.
        for (n, N, D) in [(512, 512, 128), (512, 4096, 128), (512, 4096, 2048), (512, 512, 8192)]:
            h = torch.randn(2 * N, D, device=dev) + 1.0
            zl = torch.nn.functional.normalize(torch.randn(2 * n, D, device=dev), dim=1)
            za = torch.nn.functional.normalize(torch.randn(2 * N, D, device=dev), dim=1)
            za[:n] = zl[:n]; za[N:N + n] = zl[n:]
            ws = ops.ntxent_workspace(n, N, D, dev)
            out, rs, _ = ops.ntxent_fwd(zl, za, 0, 0.1, ws)
            bws = ops.bt_workspace(n, N, D, dev)
            zhat, rstd = ops.bt_standardize(h)
            ops.bt_fwd(zhat, n, 0, 0.0051, ws=bws)
            g, cs = ops.bt_bwd(zhat, n, 0, 0.0051, 1.0, 1.0, bws)
            nt = 'ntxent_wide' if ops.ntxent_is_wide(D) else 'ntxent'
            row = dict(layer='barlow n%d N%d D%d' % (n, N, D), ntxent_kernels=nt, bt_flops=4.0 * n * N * D, ntxent_fwd_flops=8.0 * n * N * D,
                       ntxent_bwd_flops=24.0 * n * N * D, bt_workspace_bytes=bws.numel() * 8,
                       bt_standardize_us=timeit(lambda: ops.bt_standardize(h), args.iters),
                       bt_fwd_us=timeit(lambda: ops.bt_fwd(zhat, n, 0, 0.0051, ws=bws), args.iters),
                       bt_bwd_us=timeit(lambda: ops.bt_bwd(zhat, n, 0, 0.0051, 1.0, 1.0, bws), args.iters),
                       bt_apply_us=timeit(lambda: ops.bt_apply(g, zhat, rstd, cs, 0), args.iters),
                       ntxent_fwd_us=timeit(lambda: ops.ntxent_fwd(zl, za, 0, 0.1, ws), args.iters),
                       ntxent_bwd_us=timeit(lambda: ops.ntxent_bwd(zl, za, 0, 0.1, rs, 1.0, out, ws), args.iters))
            row['bt_standardize_gbs'] = 32.0 * N * D / row['bt_standardize_us'] / 1e3       # three reads and one write of [2N, D]
            row['bt_fwd_tfs'] = row['bt_flops'] / row['bt_fwd_us'] / 1e6
            row['bt_bwd_tfs'] = row['bt_flops'] / row['bt_bwd_us'] / 1e6
            row['ntxent_fwd_tfs'] = row['ntxent_fwd_flops'] / row['ntxent_fwd_us'] / 1e6
            row['ntxent_bwd_tfs'] = row['ntxent_bwd_flops'] / row['ntxent_bwd_us'] / 1e6
            row['bt_over_ntxent_fwd'] = row['bt_fwd_us'] / row['ntxent_fwd_us']
            row['bt_over_ntxent_bwd'] = row['bt_bwd_us'] / row['ntxent_bwd_us']
            print('barlow n=%d N=%d D=%d: standardize %.0f us (%.0f GB/s) fwd %.0f us (%.1f TF/s) bwd %.0f us (%.1f TF/s) apply %.0f us | %s fwd '
                  '%.0f us (%.1f TF/s) bwd %.0f us (%.1f TF/s) | barlow / ntxent fwd %.2f bwd %.2f'
                  % (n, N, D, row['bt_standardize_us'], row['bt_standardize_gbs'], row['bt_fwd_us'], row['bt_fwd_tfs'], row['bt_bwd_us'],
                     row['bt_bwd_tfs'], row['bt_apply_us'], nt, row['ntxent_fwd_us'], row['ntxent_fwd_tfs'], row['ntxent_bwd_us'],
                     row['ntxent_bwd_tfs'], row['bt_over_ntxent_fwd'], row['bt_over_ntxent_bwd']), flush=True)
            res.append(row)
            del h, zl, za, ws, bws, zhat, rstd, g, cs
    if 'vicreg' in what:
        # VICReg loss (csrc/vicreg.hip) beside the Barlow Twins launches at the same (n, N, D) in the same run: both forwards form two
        # [n, N] Gram blocks over D (4nND matrix FLOPs), both backwards two [n, N] x [N, D] products (4nND).  VICReg's forward carries one
        # view per workgroup and splits the k range where the grid is small (S parts, then a merge launch); its backward is one launch,
        # Barlow's is bt_bwd + bt_apply around an all-reduce.  Median of --iters launches, and their spread (max - min).
        def spread(fn):
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            ts = []
            for _ in range(args.iters):
                a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
                a.record(); fn(); b.record()
                torch.cuda.synchronize()
                ts.append(a.elapsed_time(b) * 1e3)
            ts.sort()
            return ts[len(ts) // 2], ts[-1] - ts[0]
        from simclr_amd._lib import lib
        for (n, N, D) in [(512, 512, 128), (512, 4096, 2048), (512, 512, 8192), (256, 2048, 8192)]:
            h = torch.randn(2 * N, D, device=dev) + 1.0
            bws = ops.bt_workspace(n, N, D, dev)
            zhat, rstd = ops.bt_standardize(h)
            ops.bt_fwd(zhat, n, 0, 0.0051, ws=bws)
            g, cs = ops.bt_bwd(zhat, n, 0, 0.0051, 1.0, 1.0, bws)
            vws = ops.vicreg_workspace(n, N, D, dev)
            xc, st = ops.vicreg_center(h)
            ops.vicreg_fwd(h, xc, st, n, 0, ws=vws)
            row = dict(layer='vicreg n%d N%d D%d' % (n, N, D), flops=4.0 * n * N * D, k_splits=ops.vicreg_k_splits(n, N, D),
                       vicreg_fwd_workgroups=int(lib().vicreg_fwd_workgroups(n, N, D)), vicreg_workspace_bytes=vws.numel() * 8,
                       bt_workspace_bytes=bws.numel() * 8, iters=args.iters)
            for name, fn in (('vicreg_center', lambda: ops.vicreg_center(h)), ('vicreg_fwd', lambda: ops.vicreg_fwd(h, xc, st, n, 0, ws=vws)),
                             ('vicreg_bwd', lambda: ops.vicreg_bwd(h, xc, st, n, 0, 25.0, 25.0, 1.0, 1.0, 1.0, vws)),
                             ('bt_standardize', lambda: ops.bt_standardize(h)), ('bt_fwd', lambda: ops.bt_fwd(zhat, n, 0, 0.0051, ws=bws)),
                             ('bt_bwd', lambda: ops.bt_bwd(zhat, n, 0, 0.0051, 1.0, 1.0, bws)),
                             ('bt_apply', lambda: ops.bt_apply(g, zhat, rstd, cs, 0))):
                row[name + '_us'], row[name + '_spread_us'] = spread(fn)
            for name in ('vicreg_fwd', 'vicreg_bwd', 'bt_fwd', 'bt_bwd'):
                row[name + '_tfs'] = row['flops'] / row[name + '_us'] / 1e6
            row['vicreg_over_bt_fwd'] = row['vicreg_fwd_us'] / row['bt_fwd_us']
            row['vicreg_total_us'] = row['vicreg_center_us'] + row['vicreg_fwd_us'] + row['vicreg_bwd_us']
            row['bt_total_us'] = row['bt_standardize_us'] + row['bt_fwd_us'] + row['bt_bwd_us'] + row['bt_apply_us']
            print('vicreg n=%d N=%d D=%d S=%d (%d workgroups): centre %.0f us fwd %.0f us (%.1f TF/s) bwd %.0f us (%.1f TF/s) | barlow standardize '
                  '%.0f us fwd %.0f us (%.1f TF/s, spread %.0f us) bwd %.0f us (%.1f TF/s) apply %.0f us | vicreg / barlow fwd %.2f'
                  % (n, N, D, row['k_splits'], row['vicreg_fwd_workgroups'], row['vicreg_center_us'], row['vicreg_fwd_us'], row['vicreg_fwd_tfs'],
                     row['vicreg_bwd_us'], row['vicreg_bwd_tfs'], row['bt_standardize_us'], row['bt_fwd_us'], row['bt_fwd_tfs'],
                     row['bt_fwd_spread_us'], row['bt_bwd_us'], row['bt_bwd_tfs'], row['bt_apply_us'], row['vicreg_over_bt_fwd']), flush=True)
            res.append(row)
            del h, bws, zhat, rstd, g, cs, vws, xc, st
    if 'repr' in what:
        # Representation diagnostics (csrc/repr.hip): the four launches of ops.repr_stats at the global batch N, beside simclr_vicreg_fwd at
        # n = N in the same run -- both form two [N, N] Gram matrices over D (4 N^2 D matrix FLOPs); VICReg's stores its blocks and may
        # split k, this one reduces each tile through g^2 and exp2 in its epilogue and writes two doubles per workgroup.
        # Median of --iters launches with [min, max].
        def med(fn):
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            ts = []
            for _ in range(args.iters):
                a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
                a.record(); fn(); b.record()
                torch.cuda.synchronize()
                ts.append(a.elapsed_time(b) * 1e3)
            ts.sort()
            return ts[len(ts) // 2], [ts[0], ts[-1]]
        for (N, D) in [(4096, 128), (4096, 2048), (512, 8192)]:
            h = torch.randn(2 * N, D, device=dev)
            z, _ = ops.l2norm_fwd(h)
            rws = ops.repr_workspace(N, D, dev)
            vws = ops.vicreg_workspace(N, N, D, dev)
            xc, st = ops.vicreg_center(z)
            row = dict(layer='repr N%d D%d' % (N, D), flops=4.0 * N * N * D, iters=args.iters, repr_workspace_bytes=rws.numel() * 8,
                       vicreg_k_splits=ops.vicreg_k_splits(N, N, D))
            for name, fn in (('repr_stats', lambda: ops.repr_stats(z, 2.0, rws)), ('vicreg_center', lambda: ops.vicreg_center(z)),
                             ('vicreg_fwd', lambda: ops.vicreg_fwd(z, xc, st, N, 0, ws=vws)), ('l2norm_fwd', lambda: ops.l2norm_fwd(h))):
                row[name + '_us'], row[name + '_min_max_us'] = med(fn)
            row['repr_tfs'] = row['flops'] / row['repr_stats_us'] / 1e6
            row['vicreg_fwd_tfs'] = row['flops'] / row['vicreg_fwd_us'] / 1e6
            row['repr_over_vicreg_center_plus_fwd'] = row['repr_stats_us'] / (row['vicreg_center_us'] + row['vicreg_fwd_us'])
            print('repr N=%d D=%d: repr_stats %.0f us [%.0f, %.0f] (%.1f TF/s) | vicreg centre %.0f us + fwd %.0f us [%.0f, %.0f] (%.1f TF/s, '
                  'S=%d) | l2norm %.0f us | repr / (vicreg centre + fwd) %.2f'
                  % (N, D, row['repr_stats_us'], *row['repr_stats_min_max_us'], row['repr_tfs'], row['vicreg_center_us'], row['vicreg_fwd_us'],
                     *row['vicreg_fwd_min_max_us'], row['vicreg_fwd_tfs'], row['vicreg_k_splits'], row['l2norm_fwd_us'],
                     row['repr_over_vicreg_center_plus_fwd']), flush=True)
            res.append(row)
            del h, z, rws, vws, xc, st
    if 'logreg' in what:
        # Cached-feature linear probe (csrc/logreg.hip): the value-only forward (mode 0), the forward that also stores G (mode 1) and the
        # backward G^T X on one slab, in TF/s of 2 n D C per product -- beside the exact-fp32 MFMA figures of the MI355X guide: 155 TF/s
        # peak, 122 TF/s for an untuned 4096^3 GEMM.  Median of --iters launches with [min, max].
        def med(fn):
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            ts = []
            for _ in range(args.iters):
                a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
                a.record(); fn(); b.record()
                torch.cuda.synchronize()
                ts.append(a.elapsed_time(b) * 1e3)
            ts.sort()
            return ts[len(ts) // 2], [ts[0], ts[-1]]
        for (n, D, C) in [(65536, 2048, 1000), (65536, 8192, 1000), (65536, 2048, 10)]:
            x = torch.randn(n, D, device=dev)
            W, b = torch.randn(C, D, device=dev) / D ** 0.5, 0.1 * torch.randn(C, device=dev)
            labels = torch.randint(0, C, (n,), device=dev, dtype=torch.int32)
            weights = torch.ones(n, device=dev)
            ws = ops.logreg_workspace(n, D, C, dev)
            store = torch.empty(n, ops.logreg_store_pitch(C), device=dev)
            lse = torch.empty(n, device=dev, dtype=torch.float64)
            dW, db = torch.empty(C, D, device=dev), torch.empty(C, device=dev)
            row = dict(layer='logreg n%d D%d C%d' % (n, D, C), flops=2.0 * n * D * C, iters=args.iters, workspace_bytes=ws.numel() * 8,
                       fwd_tile_edge=ops.logreg_tile_edge(n, D, C), bwd_tile_edge=ops.logreg_tile_edge(n, D, C, backward=True),
                       row_splits=ops.logreg_row_splits(n, D, C))
            fwd = lambda mode: ops.logreg_fwd(x, W, b, labels, weights, 1.0 / n, mode, store, lse, ws, check_labels=False)
            fwd(1)
            for name, fn in (('fwd_mode0', lambda: fwd(0)), ('fwd_mode1', lambda: fwd(1)),
                             ('bwd', lambda: ops.logreg_bwd(store, x, C, dW, db, ws=ws))):
                if name == 'bwd':
                    fwd(1)                                   # store holds G again
                row[name + '_us'], row[name + '_min_max_us'] = med(fn)
                row[name + '_tfs'] = row['flops'] / row[name + '_us'] / 1e6
            print('logreg n=%d D=%d C=%d (tiles %d / %d, %d row parts): fwd value %.0f us [%.0f, %.0f] (%.1f TF/s) | fwd + G %.0f us '
                  '[%.0f, %.0f] (%.1f TF/s) | bwd %.0f us [%.0f, %.0f] (%.1f TF/s)'
                  % (n, D, C, row['fwd_tile_edge'], row['bwd_tile_edge'], row['row_splits'], row['fwd_mode0_us'], *row['fwd_mode0_min_max_us'],
                     row['fwd_mode0_tfs'], row['fwd_mode1_us'], *row['fwd_mode1_min_max_us'], row['fwd_mode1_tfs'], row['bwd_us'],
                     *row['bwd_min_max_us'], row['bwd_tfs']), flush=True)
            res.append(row)
            del x, W, b, labels, weights, ws, store, lse, dW, db
    if 'kmeans' in what:
        # Spherical k-means (csrc/kmeans.hip) on one slab.  The assignment in TF/s of 2 n D K beside, at the same shape in the same run,
        # the value-only forward of the linear probe (ops.logreg_fwd mode 0: the same tile and the same matrix work; its C is capped at
        # 4096) and the top-1 search ops.knn_topk(x, c, 1).  The update (the sort of the wrapper included, and the kernel alone) beside a
        # plain device copy of the slab: it reads n D floats once.  Median of --iters launches with [min, max].
        def med(fn):
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            ts = []
            for _ in range(args.iters):
                a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
                a.record(); fn(); b.record()
                torch.cuda.synchronize()
                ts.append(a.elapsed_time(b) * 1e3)
            ts.sort()
            return ts[len(ts) // 2], [ts[0], ts[-1]]
        from simclr_amd._lib import lib as _klib
        for (n, D, K) in [(65536, 2048, 1000), (65536, 2048, 10000), (65536, 128, 3000)]:
            x = torch.nn.functional.normalize(torch.randn(n, D, device=dev), dim=1)
            c = torch.nn.functional.normalize(torch.randn(K, D, device=dev), dim=1)
            weights = torch.ones(n, device=dev)
            ws = ops.kmeans_workspace(n, D, K, dev)
            assign = torch.full((n,), -1, device=dev, dtype=torch.int32)
            best = torch.empty(n, device=dev)
            sums, wsum = torch.empty(K, D, device=dev, dtype=torch.float64), torch.empty(K, device=dev, dtype=torch.float64)
            row = dict(layer='kmeans n%d D%d K%d' % (n, D, K), flops=2.0 * n * D * K, iters=args.iters, workspace_bytes=ws.numel() * 8,
                       tile_edge=ops.kmeans_tile_edge(n, D, K))
            row['assign_us'], row['assign_min_max_us'] = med(lambda: ops.kmeans_assign(x, c, weights, assign, best, ws))
            row['assign_tfs'] = row['flops'] / row['assign_us'] / 1e6
            C = min(K, ops.LOGREG_MAX_CLASSES)
            lws = ops.logreg_workspace(n, D, C, dev)
            lse = torch.empty(n, device=dev, dtype=torch.float64)
            bias = torch.zeros(C, device=dev)
            labels = torch.zeros(n, device=dev, dtype=torch.int32)
            cc = c[:C].contiguous()
            row['logreg_classes'] = C
            row['logreg_fwd0_us'], row['logreg_fwd0_min_max_us'] = med(
                lambda: ops.logreg_fwd(x, cc, bias, labels, weights, 1.0 / n, 0, None, lse, lws, check_labels=False))
            row['logreg_fwd0_tfs'] = 2.0 * n * D * C / row['logreg_fwd0_us'] / 1e6
            row['knn_top1_us'], row['knn_top1_min_max_us'] = med(lambda: ops.knn_topk(x, c, 1))
            row['knn_top1_tfs'] = row['flops'] / row['knn_top1_us'] / 1e6
            row['update_us'], row['update_min_max_us'] = med(lambda: ops.kmeans_update(x, weights, assign, K, sums, wsum))
            key, order = torch.sort(assign, stable=True)
            order = order.to(torch.int32)
            offsets = torch.searchsorted(key, torch.arange(K + 1, device=dev, dtype=torch.int32)).to(torch.int32)
            pp = lambda t: t.data_ptr()
            row['update_kernel_us'], row['update_kernel_min_max_us'] = med(
                lambda: _klib().kmeans_update(pp(x), pp(weights), pp(order), pp(offsets), n, D, K, pp(sums), pp(wsum), 0,
                                              torch.cuda.current_stream().cuda_stream))
            y = torch.empty_like(x)
            row['copy_us'], row['copy_min_max_us'] = med(lambda: y.copy_(x))
            row['update_kernel_read_gbs'] = 4.0 * n * D / row['update_kernel_us'] / 1e3
            row['copy_read_gbs'] = 4.0 * n * D / row['copy_us'] / 1e3
            cn = torch.empty_like(c)
            row['finish_us'], row['finish_min_max_us'] = med(lambda: ops.kmeans_finish(sums, wsum, c, cn, ws))
            print('kmeans n=%d D=%d K=%d (tile %d): assign %.0f us [%.0f, %.0f] (%.1f TF/s) | logreg fwd value C=%d %.0f us [%.0f, %.0f] '
                  '(%.1f TF/s) | knn top-1 %.0f us [%.0f, %.0f] (%.1f TF/s) | update %.0f us [%.0f, %.0f], kernel alone %.0f us [%.0f, %.0f] '
                  '(%.0f GB/s read) | copy %.0f us [%.0f, %.0f] (%.0f GB/s read) | finish %.0f us'
                  % (n, D, K, row['tile_edge'], row['assign_us'], *row['assign_min_max_us'], row['assign_tfs'], C, row['logreg_fwd0_us'],
                     *row['logreg_fwd0_min_max_us'], row['logreg_fwd0_tfs'], row['knn_top1_us'], *row['knn_top1_min_max_us'],
                     row['knn_top1_tfs'], row['update_us'], *row['update_min_max_us'], row['update_kernel_us'],
                     *row['update_kernel_min_max_us'], row['update_kernel_read_gbs'], row['copy_us'], *row['copy_min_max_us'],
                     row['copy_read_gbs'], row['finish_us']), flush=True)
            res.append(row)
            del x, c, weights, ws, assign, best, sums, wsum, lws, lse, bias, labels, cc, key, order, offsets, y, cn
    if 'spectrum' in what:
        # Eigen-spectrum evaluation (csrc/spectrum.hip) on one slab.  The covariance (centring launch, upper-triangle product, double
        # finish) in TF/s of the n D (D + 1) operations of the triangle beside, at the same shape in the same run, ops.logreg_bwd at
        # C = min(D, 4096): the full [C, D] product of the same orientation (k = the row) in fp32.  The column sums beside a plain device
        # copy of the slab: they read n D floats once.  Median of --iters launches with [min, max].
        def med(fn):
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            ts = []
            for _ in range(args.iters):
                a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
                a.record(); fn(); b.record()
                torch.cuda.synchronize()
                ts.append(a.elapsed_time(b) * 1e3)
            ts.sort()
            return ts[len(ts) // 2], [ts[0], ts[-1]]
        for (n, D) in [(65536, 2048), (65536, 8192), (65536, 128)]:
            x = torch.relu(torch.randn(n, D, device=dev) + 0.5)
            weights = torch.ones(n, device=dev)
            ws = ops.spectrum_workspace(n, D, dev)
            sums = ops.spectrum_colsum(x, weights, ws=ws)
            mu32 = (sums[:D] / n).float()
            cov = torch.empty(D, D, device=dev, dtype=torch.float64)
            e, parts = ops.spectrum_tile_edge(n, D), ops.spectrum_row_parts(n, D)
            row = dict(layer='spectrum n%d D%d' % (n, D), flops=1.0 * n * D * (D + 1), iters=args.iters, workspace_bytes=ws.numel() * 8,
                       tile_edge=e, row_parts=parts, tile_pairs=(D // e) * (D // e + 1) // 2)
            row['cov_us'], row['cov_min_max_us'] = med(lambda: ops.spectrum_cov(x, weights, mu32, cov, ws=ws))
            row['cov_tfs'] = row['flops'] / row['cov_us'] / 1e6
            row['colsum_us'], row['colsum_min_max_us'] = med(lambda: ops.spectrum_colsum(x, weights, sums, ws=ws))
            row['colsum_read_gbs'] = 4.0 * n * D / row['colsum_us'] / 1e3
            del ws
            C = min(D, ops.LOGREG_MAX_CLASSES)
            pitch = ops.logreg_store_pitch(C)
            g = torch.randn(n, pitch, device=dev)
            dW, db = torch.empty(C, D, device=dev), torch.empty(C, device=dev)
            lws = ops.logreg_workspace(n, D, C, dev)
            row['logreg_classes'] = C
            row['logreg_bwd_us'], row['logreg_bwd_min_max_us'] = med(lambda: ops.logreg_bwd(g, x, C, dW, db, ws=lws))
            row['logreg_bwd_tfs'] = 2.0 * n * D * C / row['logreg_bwd_us'] / 1e6
            row['cov_over_logreg_bwd'] = row['cov_us'] / row['logreg_bwd_us']
            del g, dW, db, lws
            y = torch.empty_like(x)
            row['copy_us'], row['copy_min_max_us'] = med(lambda: y.copy_(x))
            row['copy_read_gbs'] = 4.0 * n * D / row['copy_us'] / 1e3
            print('spectrum n=%d D=%d (tile %d, %d pairs x %d row parts): cov %.0f us [%.0f, %.0f] (%.1f TF/s of the triangle) | logreg_bwd '
                  'C=%d %.0f us [%.0f, %.0f] (%.1f TF/s) | cov / logreg_bwd %.3f | colsum %.0f us [%.0f, %.0f] (%.0f GB/s read) | copy '
                  '%.0f us [%.0f, %.0f] (%.0f GB/s read)'
                  % (n, D, e, row['tile_pairs'], parts, row['cov_us'], *row['cov_min_max_us'], row['cov_tfs'], C, row['logreg_bwd_us'],
                     *row['logreg_bwd_min_max_us'], row['logreg_bwd_tfs'], row['cov_over_logreg_bwd'], row['colsum_us'],
                     *row['colsum_min_max_us'], row['colsum_read_gbs'], row['copy_us'], *row['copy_min_max_us'], row['copy_read_gbs']),
                  flush=True)
            res.append(row)
            del x, weights, sums, mu32, cov, y
    if 'spectrum_eval' in what:
        # One whole evaluation on random features at the size of the ImageNet training split, single replica (no all-reduce): the two
        # passes of spectrum.covariance over the cached slabs, the host eigvalsh at D = 2048, and eigvalsh alone at D = 8192.
        import time
        import numpy as np
        from simclr_amd import spectrum
        n, D = 1281167, 2048
        x = torch.empty(n, D, device=dev)
        for o in range(0, n, 65536):
            x[o:o + 65536] = torch.relu(torch.randn(min(65536, n - o), D, device=dev) + 0.5)
        weights = torch.ones(n, device=dev)
        row = dict(layer='spectrum eval n%d D%d' % (n, D), slabs=len(spectrum._slabs(n)))

        def passes():
            ws = ops.spectrum_workspace(65536, D, dev)
            sums = torch.zeros(D + 1, device=dev, dtype=torch.float64)
            cov = torch.zeros(D, D, device=dev, dtype=torch.float64)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i, (o, e) in enumerate(spectrum._slabs(n)):
                ops.spectrum_colsum(x[o:e], weights[o:e], sums, accumulate=i > 0, ws=ws)
            mu32 = (sums[:D] / float(sums[D])).float()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for i, (o, e) in enumerate(spectrum._slabs(n)):
                ops.spectrum_cov(x[o:e], weights[o:e], mu32, cov, accumulate=i > 0, ws=ws)
            torch.cuda.synchronize()
            return t1 - t0, time.perf_counter() - t1
        passes()
        runs = sorted(passes() for _ in range(3))
        row['colsum_pass_s'], row['cov_pass_s'] = runs[1]
        row['passes_min_max_s'] = [list(runs[0]), list(runs[-1])]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        C, S, _ = spectrum.covariance(x, weights)
        torch.cuda.synchronize()
        row['covariance_s'] = time.perf_counter() - t0
        t0 = time.perf_counter()
        lam = spectrum.eigenvalues(C)
        row['eigvalsh_s'] = time.perf_counter() - t0
        t0 = time.perf_counter()
        s = spectrum.scores(lam)
        row['scores_s'] = time.perf_counter() - t0
        row['rows'], row['rankme'], row['participation_ratio'] = int(S), s['eval/spectrum_rankme'], s['eval/spectrum_participation_ratio']
        del x, weights, C
        A = np.random.RandomState(0).randn(8192, 8192)
        A = A @ A.T / 8192
        t0 = time.perf_counter()
        np.linalg.eigvalsh(A)
        row['eigvalsh_8192_s'] = time.perf_counter() - t0
        print('spectrum eval n=%d D=%d (%d slabs): column-sum pass %.3f s | covariance pass %.3f s | spectrum.covariance %.3f s | eigvalsh '
              '%.3f s | scores %.4f s | eigvalsh at D = 8192 %.1f s' % (n, D, row['slabs'], row['colsum_pass_s'], row['cov_pass_s'],
                                                                         row['covariance_s'], row['eigvalsh_s'], row['scores_s'],
                                                                         row['eigvalsh_8192_s']), flush=True)
        res.append(row)
    if 'byol' in what:
        # BYOL (csrc/byol.hip).  The moving average of the target network over ResNet-50's variable list (the list of the 'lars' entry
        # below) in GB/s of 12 bytes per element (target read + write, online read), beside simclr_lars_multi_tensor on the same list in
        # the same run -- LARS moves at least 20 bytes per element (w, g, v read, w, v written) plus its norm pass.  Then the loss
        # kernels in GB/s of the bytes each must move: forward q and t once (8 B / element), backward q, t and dq (12 B / element).
        from simclr_amd.lars_optimizer import LARSOptimizer, Variable
        sizes = []
        for (H, Cin, Cout, k, s, cnt) in R50:
            sizes += [(k * k * Cin * Cout,)] * cnt + [(Cout,), (Cout,)] * cnt
        sizes += [(7 * 7 * 3 * 64,), (2048 * 2048,), (2048 * 2048,), (2048 * 128,), (2048 * 1000,), (1000,)]
        vs = []
        for i, shp in enumerate(sizes):
            v = Variable('conv2d_%d/kernel:0' % i if shp[0] > 4096 else 'batch_normalization_%d/gamma:0' % i,
                         torch.randn(shp, device=dev) * 0.05)
            v.grad = torch.randn(shp, device=dev) * 1e-3
            vs.append(v)
        targets = [torch.randn(shp, device=dev) * 0.05 for shp in sizes]
        onlines = [v.value for v in vs]
        nel = sum(s[0] for s in sizes)
        tables = ops.EmaTables()
        t_ema = timeit(lambda: tables.run(targets, onlines, 0.004), args.iters)
        opt = LARSOptimizer(0.1, weight_decay=1e-6, exclude_from_weight_decay=['batch_normalization', 'bias', 'head_supervised'])
        gv = [(v.grad, v) for v in vs]
        t_lars = timeit(lambda: opt.apply_gradients(gv), args.iters)
        row = dict(layer='byol ema', tensors=len(vs), elems=nel, ema_us=t_ema, ema_gbs=12.0 * nel / t_ema / 1e3, lars_us=t_lars,
                   lars_gbs_of_20_bytes=20.0 * nel / t_lars / 1e3, ema_over_lars=t_ema / t_lars)
        print('byol ema %d tensors %.1f M elems: %.0f us (%.0f GB/s of 12 B/elem) | lars %.0f us (%.0f GB/s of 20 B/elem) | ema / lars %.2f'
              % (len(vs), nel / 1e6, t_ema, row['ema_gbs'], t_lars, row['lars_gbs_of_20_bytes'], row['ema_over_lars']), flush=True)
        res.append(row)
        del vs, targets, onlines, gv, opt
        for (rows, D) in [(1024, 256), (1024, 4096), (8192, 256)]:
            q = torch.randn(rows, D, device=dev)
            t = torch.randn(rows, D, device=dev)
            _, rs = ops.byol_fwd(q, t)
            t_f = timeit(lambda: ops.byol_fwd(q, t), args.iters)
            t_b = timeit(lambda: ops.byol_bwd(q, t, rs, 1.0), args.iters)
            row = dict(layer='byol loss rows%d D%d' % (rows, D), fwd_us=t_f, fwd_gbs=8.0 * rows * D / t_f / 1e3, bwd_us=t_b,
                       bwd_gbs=12.0 * rows * D / t_b / 1e3)
            print('byol loss 2b=%d D=%d: fwd %.1f us (%.0f GB/s of 8 B/elem, two launches) bwd %.1f us (%.0f GB/s of 12 B/elem)'
                  % (rows, D, t_f, row['fwd_gbs'], t_b, row['bwd_gbs']), flush=True)
            res.append(row)
            del q, t, rs
    if 'moco' in what:
        # MoCo v2 (csrc/moco.hip): the one-sided sweep of 2n query rows against a queue of K keys, beside the supervised contrastive and the
        # decoupled sweeps at (n, N, D) = (512, 4096, 128) -- the same 1024 x 8192 logits -- and NT-Xent at (512, 512, 128) (what the step
        # trades for it), all in the same run.  Matrix FLOPs of moco: forward S = 2 (2n) K D, backward S again + P Q = 4 (2n) K D.
        n, N, D = 512, 4096, 128
        zl = torch.nn.functional.normalize(torch.randn(2 * n, D, device=dev), dim=1)
        za = torch.nn.functional.normalize(torch.randn(2 * N, D, device=dev), dim=1)
        za[:n] = zl[:n]; za[N:N + n] = zl[n:]
        labels = torch.randint(0, 100, (N,), device=dev, dtype=torch.int32)
        gws = ops.gcl_lse_workspace(n, N, D, dev)
        _, grs, _ = ops.gcl_lse_fwd(zl, za, 0.1, ws=gws)
        sws = ops.supcon_workspace(n, N, D, dev)
        _, srs, _ = ops.supcon_fwd(zl, za, labels, 0, 0.1, ws=sws)
        ff, fb = 8.0 * n * N * D, 24.0 * n * N * D
        ref = dict(layer='moco reference sweeps n%d N%d D%d' % (n, N, D), fwd_flops=ff, bwd_flops=fb,
                   supcon_fwd_us=timeit(lambda: ops.supcon_fwd(zl, za, labels, 0, 0.1, ws=sws), args.iters),
                   supcon_bwd_us=timeit(lambda: ops.supcon_bwd(zl, za, labels, 0, 0.1, srs, 1.0, sws), args.iters),
                   gcl_lse_fwd_us=timeit(lambda: ops.gcl_lse_fwd(zl, za, 0.1, ws=gws), args.iters),
                   gcl_lse_bwd_us=timeit(lambda: ops.gcl_lse_bwd(zl, za, 0.1, grs, 1.0, gws, skip_self=True), args.iters))
        zs = za[:2 * n].contiguous()
        zs[:n] = zl[:n]; zs[n:] = zl[n:]
        nws = ops.ntxent_workspace(n, n, D, dev)
        nout, nrs, _ = ops.ntxent_fwd(zl, zs, 0, 0.1, nws)
        ref['ntxent_n512_N512_fwd_us'] = timeit(lambda: ops.ntxent_fwd(zl, zs, 0, 0.1, nws), args.iters)
        ref['ntxent_n512_N512_bwd_us'] = timeit(lambda: ops.ntxent_bwd(zl, zs, 0, 0.1, nrs, 1.0, nout, nws), args.iters)
        for k in ('supcon', 'gcl_lse'):
            ref[k + '_fwd_tfs'] = ff / ref[k + '_fwd_us'] / 1e6
            ref[k + '_bwd_tfs'] = fb / ref[k + '_bwd_us'] / 1e6
        print('moco reference sweeps n=%d N=%d D=%d: ' % (n, N, D) + ' | '.join(
            '%s fwd %.0f us (%.1f TF/s) bwd %.0f us (%.1f TF/s)' % (k, ref[k + '_fwd_us'], ref[k + '_fwd_tfs'], ref[k + '_bwd_us'], ref[k + '_bwd_tfs'])
            for k in ('supcon', 'gcl_lse')) + ' | ntxent n=512 N=512 fwd %.0f us bwd %.0f us' % (
                ref['ntxent_n512_N512_fwd_us'], ref['ntxent_n512_N512_bwd_us']), flush=True)
        res.append(ref)
        del za, gws, sws, nws
        for (two_n, K, D) in [(1024, 8192, 128), (1024, 65536, 128), (1024, 65536, 256)]:
            q = torch.nn.functional.normalize(torch.randn(two_n, D, device=dev), dim=1)
            t = torch.nn.functional.normalize(q.roll(two_n // 2, 0) + 0.5 * torch.randn(two_n, D, device=dev), dim=1)
            queue = torch.nn.functional.normalize(torch.randn(K, D, device=dev), dim=1)
            mws = ops.moco_workspace(two_n, K, D, dev)
            _, mrs, _ = ops.moco_fwd(q, t, queue, 0.2, ws=mws)
            ff, fb = 2.0 * two_n * K * D, 4.0 * two_n * K * D
            row = dict(layer='moco 2n%d K%d D%d' % (two_n, K, D), fwd_flops=ff, bwd_flops=fb, key_splits=ops.moco_key_splits(two_n, K),
                       moco_fwd_us=timeit(lambda: ops.moco_fwd(q, t, queue, 0.2, ws=mws), args.iters),
                       moco_bwd_us=timeit(lambda: ops.moco_bwd(q, t, queue, 0.2, mrs, 1.0, mws), args.iters))
            row['moco_fwd_tfs'] = ff / row['moco_fwd_us'] / 1e6
            row['moco_bwd_tfs'] = fb / row['moco_bwd_us'] / 1e6
            if (two_n, K, D) == (1024, 8192, 128):
                row['moco_over_supcon_fwd'] = row['moco_fwd_us'] / ref['supcon_fwd_us']
                row['moco_over_supcon_bwd'] = row['moco_bwd_us'] / ref['supcon_bwd_us']
            print('moco 2n=%d K=%d D=%d: fwd %.0f us (%.1f TF/s) bwd %.0f us (%.1f TF/s)' % (
                two_n, K, D, row['moco_fwd_us'], row['moco_fwd_tfs'], row['moco_bwd_us'], row['moco_bwd_tfs'])
                + (' | moco / supcon fwd %.2f bwd %.2f' % (row['moco_over_supcon_fwd'], row['moco_over_supcon_bwd'])
                   if 'moco_over_supcon_fwd' in row else ''), flush=True)
            res.append(row)
            del q, t, queue, mws
    if 'dino' in what:
        # DINO (csrc/dino.hip): the two statistics sweeps, the teacher expectation sweep and the finalize (forward), the query-side and
        # the key-side sweep (backward), beside moco fwd / bwd at the same (2n, K, D) in the same run.  Matrix FLOPs: forward S_t + S_s +
        # S_t again + Pt ws = 8 (2n) K D against moco's 2; backward (S_s + Ps ws) + (S_s + S_t + (Ps - Pt)^T q) = 4 + 6 = 10 against 4.
        for (two_n, K, D) in [(1024, 8192, 128), (1024, 65536, 128), (1024, 65536, 256)]:
            q = torch.nn.functional.normalize(torch.randn(two_n, D, device=dev), dim=1)
            k = torch.nn.functional.normalize(q.roll(two_n // 2, 0) + 0.5 * torch.randn(two_n, D, device=dev), dim=1)
            wsn = torch.nn.functional.normalize(torch.randn(K, D, device=dev), dim=1)
            wtn = torch.nn.functional.normalize(wsn + 0.1 * torch.randn(K, D, device=dev), dim=1)
            cen = 0.05 * torch.randn(K, device=dev)
            dws = ops.dino_workspace(two_n, K, D, dev)
            _, drs, du, _ = ops.dino_fwd(q, k, wsn, wtn, cen, 0.1, 0.04, workspace=dws)
            mws = ops.moco_workspace(two_n, K, D, dev)
            _, mrs, _ = ops.moco_fwd(q, k, wsn, 0.2, ws=mws)
            unit = 2.0 * two_n * K * D
            row = dict(layer='dino 2n%d K%d D%d' % (two_n, K, D), fwd_flops=4 * unit, bwd_q_flops=2 * unit, bwd_w_flops=3 * unit,
                       key_splits=ops.dino_key_splits(two_n, K), row_splits=ops.dino_row_splits(two_n, K),
                       dino_fwd_us=timeit(lambda: ops.dino_fwd(q, k, wsn, wtn, cen, 0.1, 0.04, workspace=dws), args.iters),
                       dino_bwd_q_us=timeit(lambda: ops.dino_bwd_q(q, wsn, du, 0.1, drs, 1.0, dws), args.iters),
                       dino_bwd_w_us=timeit(lambda: ops.dino_bwd_w(q, k, wsn, wtn, cen, 0.1, 0.04, drs, 1.0, dws), args.iters),
                       moco_fwd_us=timeit(lambda: ops.moco_fwd(q, k, wsn, 0.2, ws=mws), args.iters),
                       moco_bwd_us=timeit(lambda: ops.moco_bwd(q, k, wsn, 0.2, mrs, 1.0, mws), args.iters))
            row['dino_bwd_us'] = row['dino_bwd_q_us'] + row['dino_bwd_w_us']
            row['dino_fwd_tfs'] = 4 * unit / row['dino_fwd_us'] / 1e6
            row['dino_bwd_tfs'] = 5 * unit / row['dino_bwd_us'] / 1e6
            row['moco_fwd_tfs'] = unit / row['moco_fwd_us'] / 1e6
            row['moco_bwd_tfs'] = 2 * unit / row['moco_bwd_us'] / 1e6
            row['dino_over_moco_fwd'] = row['dino_fwd_us'] / row['moco_fwd_us']       # expected from the matrix work: about 4
            row['dino_over_moco_bwd'] = row['dino_bwd_us'] / row['moco_bwd_us']       # expected: about 2.5
            print('dino 2n=%d K=%d D=%d: fwd %.0f us (%.1f TF/s) bwd_q %.0f us bwd_w %.0f us (bwd %.1f TF/s) | moco fwd %.0f us '
                  '(%.1f TF/s) bwd %.0f us (%.1f TF/s) | dino / moco fwd %.2f bwd %.2f' % (
                      two_n, K, D, row['dino_fwd_us'], row['dino_fwd_tfs'], row['dino_bwd_q_us'], row['dino_bwd_w_us'], row['dino_bwd_tfs'],
                      row['moco_fwd_us'], row['moco_fwd_tfs'], row['moco_bwd_us'], row['moco_bwd_tfs'], row['dino_over_moco_fwd'],
                      row['dino_over_moco_bwd']), flush=True)
            res.append(row)
            del q, k, wsn, wtn, cen, dws, mws
    if 'swav' in what:
        # SwAV (csrc/swav.hip): the Sinkhorn (I = 3: three column sweeps, two row sweeps), the forward (one statistics sweep for both
        # scales + the code expectation sweep), the query-side and the key-side sweep, beside dino fwd / bwd at the same (2b, K, D) in the
        # same run.  Matrix FLOPs in units of 2 (2b) K D: swav fwd 1 + 2 = 3 against dino's 4 (expected ratio 6 / 8), bwd 2 + 3 = 5
        # against 5 (about equal), Sinkhorn (2 I - 1) on rows_all rows.
        iters_s = 3
        for (two_n, K, D) in [(1024, 3000, 128), (1024, 65536, 128), (1024, 65536, 256)]:
            q = torch.nn.functional.normalize(torch.randn(two_n, D, device=dev), dim=1)
            k = torch.nn.functional.normalize(q.roll(two_n // 2, 0) + 0.5 * torch.randn(two_n, D, device=dev), dim=1)
            wsn = torch.nn.functional.normalize(torch.randn(K, D, device=dev), dim=1)
            cen = 0.05 * torch.randn(K, device=dev)
            sws = ops.swav_workspace(two_n, K, D, dev)
            alpha = ops.swav_sinkhorn(q, wsn, 0.05, iters_s, workspace=sws)
            lws = ops.swav_workspace(two_n, K, D, dev)
            _, srs, su, _ = ops.swav_fwd(q, wsn, alpha, 0.1, 0.05, workspace=lws)
            dws = ops.dino_workspace(two_n, K, D, dev)
            _, drs, du, _ = ops.dino_fwd(q, k, wsn, wsn, cen, 0.1, 0.04, workspace=dws)
            unit = 2.0 * two_n * K * D
            row = dict(layer='swav 2b%d K%d D%d' % (two_n, K, D), sinkhorn_iterations=iters_s, fwd_flops=3 * unit, bwd_q_flops=2 * unit,
                       bwd_w_flops=3 * unit, sinkhorn_flops=(2 * iters_s - 1) * unit,
                       key_splits=ops.swav_key_splits(two_n, K), row_splits=ops.swav_row_splits(two_n, K),
                       swav_sinkhorn_us=timeit(lambda: ops.swav_sinkhorn(q, wsn, 0.05, iters_s, workspace=sws), args.iters),
                       swav_fwd_us=timeit(lambda: ops.swav_fwd(q, wsn, alpha, 0.1, 0.05, workspace=lws), args.iters),
                       swav_bwd_q_us=timeit(lambda: ops.swav_bwd_q(q, wsn, su, 0.1, srs, 1.0, lws), args.iters),
                       swav_bwd_w_us=timeit(lambda: ops.swav_bwd_w(q, wsn, alpha, 0.1, 0.05, srs, 1.0, lws), args.iters),
                       dino_fwd_us=timeit(lambda: ops.dino_fwd(q, k, wsn, wsn, cen, 0.1, 0.04, workspace=dws), args.iters),
                       dino_bwd_q_us=timeit(lambda: ops.dino_bwd_q(q, wsn, du, 0.1, drs, 1.0, dws), args.iters),
                       dino_bwd_w_us=timeit(lambda: ops.dino_bwd_w(q, k, wsn, wsn, cen, 0.1, 0.04, drs, 1.0, dws), args.iters))
            row['swav_bwd_us'] = row['swav_bwd_q_us'] + row['swav_bwd_w_us']
            row['dino_bwd_us'] = row['dino_bwd_q_us'] + row['dino_bwd_w_us']
            row['swav_sinkhorn_tfs'] = row['sinkhorn_flops'] / row['swav_sinkhorn_us'] / 1e6
            row['swav_fwd_tfs'] = 3 * unit / row['swav_fwd_us'] / 1e6
            row['swav_bwd_tfs'] = 5 * unit / row['swav_bwd_us'] / 1e6
            row['swav_over_dino_fwd'] = row['swav_fwd_us'] / row['dino_fwd_us']       # expected from the matrix work: about 6 / 8
            row['swav_over_dino_bwd'] = row['swav_bwd_us'] / row['dino_bwd_us']       # expected: about 1
            print('swav 2b=%d K=%d D=%d: sinkhorn %.0f us (%.1f TF/s) fwd %.0f us (%.1f TF/s) bwd_q %.0f us bwd_w %.0f us (bwd %.1f TF/s) '
                  '| dino fwd %.0f us bwd %.0f us | swav / dino fwd %.2f bwd %.2f' % (
                      two_n, K, D, row['swav_sinkhorn_us'], row['swav_sinkhorn_tfs'], row['swav_fwd_us'], row['swav_fwd_tfs'],
                      row['swav_bwd_q_us'], row['swav_bwd_w_us'], row['swav_bwd_tfs'], row['dino_fwd_us'], row['dino_bwd_us'],
                      row['swav_over_dino_fwd'], row['swav_over_dino_bwd']), flush=True)
            res.append(row)
            del q, k, wsn, cen, sws, lws, dws
        # the Sinkhorn on a gathered batch: rows_all = 8192 (estimate: (2 I - 1) * 2 * rows_all * K * D = 31 GFLOP at K = 3000, D = 128)
        for (rows_all, K, D) in [(8192, 3000, 128), (8192, 65536, 128)]:
            z = torch.nn.functional.normalize(torch.randn(rows_all, D, device=dev), dim=1)
            wsn = torch.nn.functional.normalize(torch.randn(K, D, device=dev), dim=1)
            sws = ops.swav_workspace(rows_all, K, D, dev)
            flops = (2 * iters_s - 1) * 2.0 * rows_all * K * D
            t = timeit(lambda: ops.swav_sinkhorn(z, wsn, 0.05, iters_s, workspace=sws), args.iters)
            row = dict(layer='swav_sinkhorn rows%d K%d D%d' % (rows_all, K, D), sinkhorn_iterations=iters_s, sinkhorn_flops=flops,
                       key_splits=ops.swav_key_splits(rows_all, K), row_splits=ops.swav_row_splits(rows_all, K), swav_sinkhorn_us=t,
                       swav_sinkhorn_tfs=flops / t / 1e6)
            print('swav sinkhorn rows_all=%d K=%d D=%d I=%d: %.0f us (%.1f TF/s)' % (rows_all, K, D, iters_s, t, row['swav_sinkhorn_tfs']),
                  flush=True)
            res.append(row)
            del z, wsn, sws
    if 'swav_multicrop' in what:
        # SwAV multi-crop (csrc/swav_multicrop.hip): the three local-view calls at L views of b images, beside swav fwd / bwd on the 2b
        # global rows of the same images in the same run.  Matrix FLOPs: local_fwd 2 (L b) K D (one statistics sweep) against swav_fwd's
        # 6 (2b) K D (expected time ratio L / 6 at equal rates), local_bwd_x 4 (L b) K D, local_bwd_w 4 (L b + 2b) K D.
        for (b, L, K, D) in [(512, 6, 3000, 128), (512, 6, 65536, 128)]:
            q = torch.nn.functional.normalize(torch.randn(2 * b, D, device=dev), dim=1)
            x = torch.nn.functional.normalize(q[:b].repeat(L, 1) + 0.7 * torch.randn(L * b, D, device=dev) / D ** 0.5, dim=1)
            wsn = torch.nn.functional.normalize(torch.randn(K, D, device=dev), dim=1)
            sws = ops.swav_workspace(2 * b, K, D, dev)
            alpha = ops.swav_sinkhorn(q, wsn, 0.05, 3, workspace=sws)
            lws = ops.swav_workspace(2 * b, K, D, dev)
            _, srs, su, _ = ops.swav_fwd(q, wsn, alpha, 0.1, 0.05, workspace=lws)
            mws = ops.swav_local_workspace(b, L, K, D, dev)
            _, mrs, _ = ops.swav_local_fwd(x, wsn, su, L, 0.1, workspace=mws)
            unit = 2.0 * K * D
            row = dict(layer='swav_multicrop b%d L%d K%d D%d' % (b, L, K, D), local_fwd_flops=unit * L * b, swav_fwd_flops=3 * unit * 2 * b,
                       local_bwd_x_flops=2 * unit * L * b, local_bwd_w_flops=2 * unit * (L * b + 2 * b),
                       key_splits=ops.swav_local_key_splits(b, L, K), row_splits=list(ops.swav_local_row_splits(b, L, K)),
                       local_fwd_us=timeit(lambda: ops.swav_local_fwd(x, wsn, su, L, 0.1, workspace=mws), args.iters),
                       local_bwd_x_us=timeit(lambda: ops.swav_local_bwd_x(x, wsn, su, L, 0.1, mrs, 1.0, mws), args.iters),
                       local_bwd_w_us=timeit(lambda: ops.swav_local_bwd_w(x, q, wsn, alpha, L, 0.1, 0.05, mrs, srs, 1.0, mws), args.iters),
                       swav_fwd_us=timeit(lambda: ops.swav_fwd(q, wsn, alpha, 0.1, 0.05, workspace=lws), args.iters),
                       swav_bwd_q_us=timeit(lambda: ops.swav_bwd_q(q, wsn, su, 0.1, srs, 1.0, lws), args.iters),
                       swav_bwd_w_us=timeit(lambda: ops.swav_bwd_w(q, wsn, alpha, 0.1, 0.05, srs, 1.0, lws), args.iters))
            row['local_fwd_tfs'] = row['local_fwd_flops'] / row['local_fwd_us'] / 1e6
            row['local_bwd_x_tfs'] = row['local_bwd_x_flops'] / row['local_bwd_x_us'] / 1e6
            row['local_bwd_w_tfs'] = row['local_bwd_w_flops'] / row['local_bwd_w_us'] / 1e6
            row['local_over_swav_fwd'] = row['local_fwd_us'] / row['swav_fwd_us']
            row['local_over_swav_fwd_expected'] = row['local_fwd_flops'] / row['swav_fwd_flops']          # L / 6
            print('swav_multicrop b=%d L=%d K=%d D=%d: local fwd %.0f us (%.1f TF/s) bwd_x %.0f us (%.1f TF/s) bwd_w %.0f us (%.1f TF/s) | '
                  'swav fwd %.0f us bwd_q %.0f us bwd_w %.0f us | local / swav fwd %.2f (matrix work: %.2f)' % (
                      b, L, K, D, row['local_fwd_us'], row['local_fwd_tfs'], row['local_bwd_x_us'], row['local_bwd_x_tfs'],
                      row['local_bwd_w_us'], row['local_bwd_w_tfs'], row['swav_fwd_us'], row['swav_bwd_q_us'], row['swav_bwd_w_us'],
                      row['local_over_swav_fwd'], row['local_over_swav_fwd_expected']), flush=True)
            res.append(row)
            del q, x, wsn, sws, lws, mws
    if 'dino_multicrop' in what:
        # DINO multi-crop (csrc/dino_multicrop.hip): dino_local_bwd_w at L views of b images, beside swav_local_bwd_w at the same shape
        # and dino_bwd_w on the 2b global rows, in the same run.  Each figure is the median of 5 timeit() calls with their min / max as
        # the spread.  Matrix FLOPs: 4 (L b + 2 b) K D in both local key-side calls -- expected dino_local / swav_local about 1.
        def med5(fn):
            ts = sorted(timeit(fn, args.iters) for _ in range(5))
            return dict(us=ts[2], min_us=ts[0], max_us=ts[4])
        for (b, L, K, D) in [(512, 6, 8192, 128), (512, 6, 65536, 128), (512, 6, 65536, 256)]:
            q = torch.nn.functional.normalize(torch.randn(2 * b, D, device=dev), dim=1)
            k = torch.nn.functional.normalize(q + 0.5 * torch.randn(2 * b, D, device=dev) / D ** 0.5, dim=1)
            x = torch.nn.functional.normalize(q[:b].repeat(L, 1) + 0.7 * torch.randn(L * b, D, device=dev) / D ** 0.5, dim=1)
            wsn = torch.nn.functional.normalize(torch.randn(K, D, device=dev), dim=1)
            wtn = torch.nn.functional.normalize(wsn + 0.1 * torch.randn(K, D, device=dev) / D ** 0.5, dim=1)
            cen = 0.05 * torch.randn(K, device=dev)
            dws = ops.dino_workspace(2 * b, K, D, dev)
            _, drs, du, _ = ops.dino_fwd(q, k, wsn, wtn, cen, 0.1, 0.04, workspace=dws)
            sws = ops.swav_workspace(2 * b, K, D, dev)
            alpha = ops.swav_sinkhorn(q, wsn, 0.05, 3, workspace=sws)
            _, srs, su, _ = ops.swav_fwd(q, wsn, alpha, 0.1, 0.05, workspace=sws)
            mws = ops.swav_local_workspace(b, L, K, D, dev)
            _, mrs, _ = ops.swav_local_fwd(x, wsn, du, L, 0.1, workspace=mws)
            lws = ops.dino_local_workspace(b, L, K, D, dev)
            flops = 4.0 * (L * b + 2 * b) * K * D
            t_d = med5(lambda: ops.dino_local_bwd_w(x, k, wsn, wtn, cen, L, 0.1, 0.04, mrs, drs, 1.0, lws))
            t_s = med5(lambda: ops.swav_local_bwd_w(x, q, wsn, alpha, L, 0.1, 0.05, mrs, srs, 1.0, mws))
            t_g = med5(lambda: ops.dino_bwd_w(q, k, wsn, wtn, cen, 0.1, 0.04, drs, 1.0, dws))
            t_f = med5(lambda: ops.swav_local_fwd(x, wsn, du, L, 0.1, workspace=mws))
            t_x = med5(lambda: ops.swav_local_bwd_x(x, wsn, du, L, 0.1, mrs, 1.0, mws))
            row = dict(layer='dino_multicrop b%d L%d K%d D%d' % (b, L, K, D), local_bwd_w_flops=flops,
                       row_splits=list(ops.dino_local_row_splits(b, L, K)), dino_local_bwd_w=t_d, swav_local_bwd_w=t_s, dino_bwd_w=t_g,
                       local_fwd=t_f, local_bwd_x=t_x, dino_local_bwd_w_tfs=flops / t_d['us'] / 1e6,
                       dino_local_over_swav_local=t_d['us'] / t_s['us'], dino_local_over_swav_local_expected=1.0,
                       local_loss_launches_us=t_f['us'] + t_x['us'] + t_d['us'])
            print('dino_multicrop b=%d L=%d K=%d D=%d: dino_local_bwd_w %.0f us [%.0f, %.0f] (%.1f TF/s) | swav_local_bwd_w %.0f us [%.0f, %.0f] '
                  '| dino_bwd_w %.0f us [%.0f, %.0f] | local fwd %.0f us bwd_x %.0f us | dino_local / swav_local %.3f (matrix work: 1)' % (
                      b, L, K, D, t_d['us'], t_d['min_us'], t_d['max_us'], row['dino_local_bwd_w_tfs'], t_s['us'], t_s['min_us'], t_s['max_us'],
                      t_g['us'], t_g['min_us'], t_g['max_us'], t_f['us'], t_x['us'], row['dino_local_over_swav_local']), flush=True)
            res.append(row)
            del q, k, x, wsn, wtn, cen, dws, sws, mws, lws
    if 'knn' in what:
        # weighted k-NN evaluation (csrc/knn.hip): the fused similarity GEMM + streaming top-k and the vote at one ImageNet eval batch
        # against a 10 % bank, the full bank and a projection-width bank, beside simclr_ntxent_wide_logits_ab at the same (Q, N, D) --
        # the same exact-f32 GEMM, which WRITES the dense [Q, N] matrix (for the full bank: on a 131072-row slice, scaled by N / 131072)
        for (Q, N, D, k) in [(256, 131072, 2048, 200), (256, 1281167, 2048, 200), (256, 131072, 128, 200)]:
            q = torch.nn.functional.normalize(torch.randn(Q, D, device=dev), dim=1)
            bank = torch.randn(N, D, device=dev)
            for lo in range(0, N, 65536):
                bank[lo:lo + 65536] = torch.nn.functional.normalize(bank[lo:lo + 65536], dim=1)
            labels = torch.randint(0, 1000, (N,), device=dev, dtype=torch.int32)
            tv, ti = ops.knn_topk(q, bank, k)
            tl = labels[ti.long()].contiguous()
            t_k = timeit(lambda: ops.knn_topk(q, bank, k), args.iters)
            t_v = timeit(lambda: ops.knn_vote(tv, tl, 1000, 0.07), args.iters)
            Ns = min(N, 131072)
            z_local = torch.cat([q, q])                                    # logits_ab reads z_local[:n] and z_all[N:]
            z_all = torch.cat([bank[:1].expand(Ns, D), bank[:Ns]]).contiguous()
            t_g = timeit(lambda: ops.ntxent_wide_logits_ab(z_local, z_all, 1.0), args.iters) * (N / Ns)
            fl = 2.0 * Q * N * D
            row = dict(layer='knn Q%d N%d D%d k%d' % (Q, N, D, k), topk_us=t_k, topk_tfs=fl / t_k / 1e6, vote_us=t_v,
                       logits_ab_us=t_g, logits_ab_tfs=fl / t_g / 1e6, logits_ab_scaled_from_rows=Ns, topk_over_logits_ab=t_k / t_g,
                       workspace_bytes=Q * k * 8 * -(-N // ops.KNN_SLAB))
            print('knn Q=%d N=%d D=%d k=%d: topk %.0f us (%.1f TF/s) vote %.0f us | dense logits_ab %.0f us (%.1f TF/s%s) | topk / dense %.2f'
                  % (Q, N, D, k, t_k, row['topk_tfs'], t_v, t_g, row['logits_ab_tfs'], '' if Ns == N else ', scaled from %d rows' % Ns,
                     row['topk_over_logits_ab']), flush=True)
            res.append(row)
            del q, bank, z_all, z_local, tv, ti, tl
    if 'dropblock' in what:
        # the four DropBlock kernels (csrc/dropblock.hip) at the sites of block groups 3 and 4, in fp32 and bf16 storage, as GB/s of
        # the bytes each must move (tensors once, bit tensors once; the mask kernel reads nothing and writes one bit per element),
        # beside simclr_bn_apply on the same tensor
        for (H, C) in [(14, 1024), (14, 256), (7, 2048)]:
            for sdt in (torch.float32, torch.bfloat16):
                x = torch.randn(V, H, H, C, device=dev).to(sdt)
                r = torch.randn(V, H, H, C, device=dev).to(sdt)
                y = torch.empty_like(x)
                scale = torch.rand(C, device=dev) + 0.5; shift = torch.randn(C, device=dev) * 0.1
                nb = x.numel() * x.element_size()
                mb = x.numel() / 8
                ba, ca = ops.dropblock_mask(tuple(x.shape), 0.9, 7, key=1, device=dev)
                bb, cb = ops.dropblock_mask(tuple(x.shape), 0.9, 7, key=2, device=dev)
                _, rb = ops.dropblock_tail_fwd(x, ba, ca, r, bb, cb)
                t_bn = timeit(lambda: ops.bn_apply(x, scale, shift, True, out=y), args.iters)
                t_m = timeit(lambda: ops.dropblock_mask(tuple(x.shape), 0.9, 7, key=1, device=dev), args.iters)
                t_a = timeit(lambda: ops.dropblock_apply(x, ba, ca, out=y), args.iters)
                t_tf = timeit(lambda: ops.dropblock_tail_fwd(x, ba, ca, r, bb, cb), args.iters)
                t_tb = timeit(lambda: ops.dropblock_tail_bwd(x, rb, ba, ca, bb, cb), args.iters)
                row = dict(layer='dropblock %dx%d C%d %s' % (H, H, C, 'f32' if sdt == torch.float32 else 'bf16'), tensor_bytes=nb,
                           bn_apply_us=t_bn, bn_apply_gbs=2 * nb / t_bn / 1e3, mask_us=t_m, mask_gbs=mb / t_m / 1e3,
                           apply_us=t_a, apply_gbs=(2 * nb + mb) / t_a / 1e3,
                           tail_fwd_us=t_tf, tail_fwd_gbs=(3 * nb + 2 * mb + rb.numel()) / t_tf / 1e3,
                           tail_bwd_us=t_tb, tail_bwd_gbs=(3 * nb + 2 * mb + rb.numel()) / t_tb / 1e3)
                print(row['layer'] + ': ' + ' '.join('%s %.0f' % (k, v) for k, v in row.items() if k not in ('layer', 'tensor_bytes')), flush=True)
                res.append(row)
                del x, r, y, ba, bb, rb
    if 'lars' in what:
        from simclr_amd.lars_optimizer import LARSOptimizer, Variable
        sizes = []
        for (H, Cin, Cout, k, s, cnt) in R50:
            sizes += [(k * k * Cin * Cout,)] * cnt + [(Cout,), (Cout,)] * cnt
        sizes += [(7 * 7 * 3 * 64,), (2048 * 2048,), (2048 * 2048,), (2048 * 128,), (2048 * 1000,), (1000,)]
        vs = []
        for i, shp in enumerate(sizes):
            v = Variable('conv2d_%d/kernel:0' % i if shp[0] > 4096 else 'batch_normalization_%d/gamma:0' % i,
                         torch.randn(shp, device=dev) * 0.05)
            v.grad = torch.randn(shp, device=dev) * 1e-3
            vs.append(v)
        opt = LARSOptimizer(0.1, weight_decay=1e-6, exclude_from_weight_decay=['batch_normalization', 'bias', 'head_supervised'])
        gv = [(v.grad, v) for v in vs]
        t = timeit(lambda: opt.apply_gradients(gv), args.iters)
        nel = sum(s[0] for s in sizes)
        print('lars %d tensors %.1f M elems: %.0f us, %.0f GB/s (7 x 4 B/elem two-pass)' % (len(vs), nel / 1e6, t, 28.0 * nel / t / 1e3), flush=True)
        res.append(dict(layer='lars', us=t, elems=nel))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
