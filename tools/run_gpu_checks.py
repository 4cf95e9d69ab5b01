"""First-contact GPU diagnostics: run every kernel parity check, print all errors, dump JSON.

Usage (on the GPU box): python tools/run_gpu_checks.py [--quick]
Writes gpurun_out/gpu_checks.json.  Exit code 0 even on failures (this is a report, the
gate is `pytest -m gpu`).
"""
import json
import os
import sys
import time
import traceback

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from tests import gpu_checks as gc  # noqa: E402

BF, F32 = torch.bfloat16, torch.float32


def main():
    results = []

    def run(fn, *a, **k):
        t = time.time()
        try:
            r = fn(*a, **k)
            torch.cuda.synchronize()
            for d in r:
                d['sec'] = round(time.time() - t, 2)
                results.append(d)
                print('%-4s %-70s err=%.3e tol=%.3e scale=%.3e nbad=%d/%d' % (
                    'ok' if d['ok'] else 'FAIL', d['name'], d['err'], d['tol'], d['scale'], d['nbad'], d['numel']),
                    flush=True)
        except Exception as e:  # noqa
            traceback.print_exc()
            results.append(dict(name='%s%r' % (fn.__name__, a), ok=False, err=-1, exc=repr(e)))
            print('EXC  %s%r: %r' % (fn.__name__, a, e), flush=True)

    print(torch.cuda.get_device_name(0), flush=True)
    run(gc.check_probes)
    try:
        m = gc.probe_ds_read_tr16()
        print('ds_read_tr16 lanes 0..19:\n', m[:20].tolist(), flush=True)
        os.makedirs('gpurun_out', exist_ok=True)
        json.dump(m.tolist(), open('gpurun_out/ds_read_tr16_map.json', 'w'))
    except Exception:
        traceback.print_exc()
    run(gc.check_ntxent_closed_forms)
    for n, R, D, rank in [(64, 1, 128, 0), (96, 1, 64, 0), (32, 4, 128, 2), (512, 1, 128, 0), (64, 2, 256, 1)]:
        run(gc.check_ntxent, n, R, D=D, rank=rank)
    run(gc.check_ntxent, 64, 1, hidden_norm=False, temperature=1.0)
    run(gc.check_lars)
    run(gc.check_lars, classic=False, nesterov=True)
    run(gc.check_lars, classic=True, nesterov=True)
    for dt in (F32, BF):
        for (V, H, Cin, Cout, k, s) in [(2, 8, 64, 64, 1, 1), (3, 14, 64, 128, 3, 1), (2, 15, 128, 64, 3, 2),
                                        (2, 16, 64, 256, 1, 2), (3, 9, 128, 192, 3, 1), (130, 1, 128, 64, 1, 1),
                                        (2, 12, 256, 128, 3, 2)]:
            run(gc.check_conv, V, H, H, Cin, Cout, k, s, dt)
        for (V, H, Cin, Cout, k, mode, acc) in [(3, 9, 128, 64, 1, 2, 0), (2, 14, 64, 128, 3, 2, 0), (3, 8, 256, 64, 1, 1, 1), (2, 7, 64, 64, 3, 1, 0)]:
            run(gc.check_dgrad_bn, V, H, Cin, Cout, k, dt, mode, acc)
        run(gc.check_stem, 4, 32, 7, 2, 64, dt)
        run(gc.check_stem, 4, 16, 3, 1, 64, dt)
        run(gc.check_stem, 2, 224, 7, 2, 64, dt)
        for relu, resid in [(True, None), (False, None), (True, 'identity'), (True, 'bn')]:
            run(gc.check_bn, (6, 7, 5), 64, dt, relu, resid)
        run(gc.check_bn, (37,), 2048, dt, False, None)
        run(gc.check_bn, (500,), 128, dt, True, None)
        run(gc.check_pool, 2, 16, 64, dt)
        run(gc.check_pool, 2, 15, 64, dt)
        run(gc.check_sup_head, 64, 1000, 1008, dt)
        run(gc.check_sup_head, 16, 10, 16, dt)
    # the selective-kernel unit and the small head kernels (tests/test_gpu_sk_and_small_kernels.py)
    for dt in (F32, BF):
        for (V, H, W, f, lp, gp) in [(4, 7, 7, 512, None, None), (2, 56, 56, 64, None, None), (3, 4, 4, 72, 192, 128), (130, 3, 3, 64, None, None)]:
            run(gc.check_sk_kernels, V, H, W, f, lp, gp, dt)
        run(gc.check_sk_kernels, 3, 4, 4, 72, 192, 128, dt, logits='equal')
        run(gc.check_sk_kernels, 3, 4, 4, 72, 192, 128, dt, logits='saturated')
        run(gc.check_avgpool_bwd_mask, 4, 7, 2048, dt)
        for mode in ('normal', 'zero', 'tie_cross', 'tie_same', 'large'):
            run(gc.check_xent, 63, 63, 1000, 1008, dt, mode=mode)
            run(gc.check_xent, 10, 5, 1000, 1008, dt, gscale=0.5, mode=mode)
        for rows in (1, 15, 17, 1000):
            run(gc.check_colsum, rows, 1008, 1000, dt)
    run(gc.check_sk_kernels, 3, 5, 5, 4, 64, 64, F32)
    for mm in ('exact', 'f16x3_3'):
        run(gc.check_sk_layer, 3, 14, 64, 64, 2, f32_matmul=mm, seed=4)
        run(gc.check_sk_layer, 4, 7, 64, 64, 1, f32_matmul=mm, seed=11)
    run(gc.check_avgpool_f32_from_bf16, 4, 7, 2048)
    run(gc.check_avgpool_f32_from_bf16, 2, 56, 64)
    run(gc.check_cast_classes)
    for n in (1, 257, (1 << 20) + 3):
        run(gc.check_cast_sizes, n)
        run(gc.check_axpy, n)
    for n in (1, 1025, 2048000):
        run(gc.check_l2_loss, n)
    for n in (1, 5, 16):
        run(gc.check_accumulate_scalars, n)
    run(gc.check_empty_launches)
    # BatchNorm and stem max-pool kernels on exact lattices, tolerance 0 (tests/test_gpu_bn_and_stem_pool.py)
    for dt, widths in ((F32, (4, 96, 192, 1024, 6144)), (BF, (8, 96, 384, 2048, 6144))):
        for C in widths:
            for rows in (3, 515):
                run(gc.check_bn_stream_lattice, rows, C, dt)
        run(gc.check_bn_bwd_reduce_slot_counts, 515, 192 if dt == F32 else 384, dt)
        for (K, N) in [(5, 300), (64, 40)]:
            run(gc.check_bn_fold_lattice, K, N, dt)
        for (V, H, W, C) in [(2, 6, 10, 64), (3, 7, 5, 128), (1, 9, 16, 192), (2, 1, 1, 64), (1, 2, 3, 256), (2, 15, 15, 64)]:
            run(gc.check_stem_pool_lattice, V, H, W, C, dt)
        for (V, H, W, C, k, s) in [(2, 7, 9, 64, 2, 2), (2, 7, 9, 64, 3, 1), (2, 7, 9, 64, 5, 3), (2, 7, 9, 192, 3, 1), (2, 9, 9, 1024, 5, 3)]:
            run(gc.check_stem_pool_lattice, V, H, W, C, dt, ksz=k, stride=s)
        for (H, W, s) in [(7, 4, 2), (5, 8, 2), (7, 4, 1), (4, 7, 1)]:
            run(gc.check_avgpool2, 2, H, 192, s, dt, W=W)
    for nslot, C in [(1, 8), (33, 40), (129, 64), (160, 40), (768, 2048)]:
        run(gc.check_bn_slot_kernels, nslot, C)
    # implicit-GEMM convolutions on exact integer lattices, tolerance 0 (tests/test_gpu_conv_lattice.py); --quick: the small rows only
    from tests import conv_reference as cr
    for c in cr.CASES:
        if '--quick' not in sys.argv or c.V * c.H * c.W * max(c.Cin, c.Cout) <= 2 ** 21:
            run(gc.check_conv_lattice, c)
    # the stem chain and the Gram chain on the same lattices (tests/test_gpu_stem_gram_lattice.py)
    from tests import stem_gram_reference as sg
    for check, cases in ((gc.check_stem_lattice, sg.STEM_CASES), (gc.check_gram_lattice, sg.GRAM_CASES), (gc.check_small_gemm_lattice, sg.GEMM_CASES)):
        for c in cases:
            run(check, c)
    # augmentation and blur kernels stage by stage (tests/test_gpu_augment.py)
    for views in (1, 2, 3):
        run(gc.check_augment_identity, 15, 17, views)
    for (H, W) in [(15, 17), (16, 16), (16, 17), (24, 40)]:
        run(gc.check_augment_colour, H, W)
    run(gc.check_augment_exact_colour)
    for (H, W) in [(16, 32), (32, 16), (24, 40), (40, 24)]:
        for kind in ('u8', 'f32'):
            run(gc.check_augment_resize, H, W, kind)
    run(gc.check_augment_ragged, 40, 24)
    run(gc.check_augment_ragged_clamps, 24, 40)
    for (H, W, hh) in [(40, 3, 40), (3, 40, 3), (3, 40, 40), (45, 20, 45), (7, 9, 7)]:
        run(gc.check_blur_cases, H, W, hh)
    nfail = sum(1 for r in results if not r['ok'])
    print('TOTAL %d checks, %d failed' % (len(results), nfail), flush=True)
    os.makedirs('gpurun_out', exist_ok=True)
    json.dump(results, open('gpurun_out/gpu_checks.json', 'w'), indent=1)


if __name__ == '__main__':
    main()
