"""Time the VICReg step (run.make_single_step under --contrastive_loss=vicreg) next to the Barlow Twins step at the same flags,
ResNet-50 1x at 224 px on two-view synthetic batches, alternating in ONE process and in `rounds` rounds:
    python tools/vicreg_step_time.py [--batch 512] [--width 8192] [--steps 10] [--warmup 3] [--rounds 2] [--f32_matmul f16x3_3]
                                     [--out FILE]
      (a) the barlow step,
      (b) the vicreg step: the same model, add_vicreg_loss in place of add_barlow_twins_loss.
Then the loss kernels alone at the step's shape (n, n, width), median of 5: vicreg centre + fwd + bwd and bt standardize + fwd + bwd +
apply, the launches (b) trades.  Prints (and writes to --out) one JSON object: the per-round times, their means, the allowance
(a) + (vicreg kernels - barlow kernels) + the spread of (a) between the rounds, and the difference (b) - allowance, whichever way it
falls."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def _timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def _median_us(fn, iters=5, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--depth', type=int, default=50)
    ap.add_argument('--width', type=int, default=8192)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--f32_matmul', default='f16x3_3')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    from simclr_amd import model as model_lib
    from simclr_amd import ops
    from simclr_amd.flags import FLAGS
    from simclr_amd.resnet import RT
    from simclr_amd.run import make_single_step, synthetic_batches
    ncls = 10 if args.size <= 32 else 1000
    FLAGS.reset()
    FLAGS.update(resnet_depth=args.depth, image_size=args.size, train_batch_size=args.batch, use_blur=False, compute_dtype='f32',
                 f32_matmul=args.f32_matmul, train_mode='pretrain', proj_out_dim=args.width, contrastive_loss='barlow')
    RT.reset()
    RT.device = torch.device('cuda', torch.cuda.current_device())
    barlow = model_lib.Model(ncls)
    step_barlow = make_single_step(barlow, model_lib.build_optimizer(0.1), None)
    with FLAGS.override(contrastive_loss='vicreg'), RT.fresh_names():
        vicreg = model_lib.Model(ncls)
    data = synthetic_batches(args.batch, args.size, ncls, RT.device, views=2)
    last = {}
    box = {}

    def run_barlow():
        last['barlow'] = step_barlow(*next(data))

    def run_vicreg():
        with FLAGS.override(contrastive_loss='vicreg'):
            if 'step' not in box:
                box['step'] = make_single_step(vicreg, model_lib.build_optimizer(0.1), None)
            last['vicreg'] = box['step'](*next(data))
    rounds = []
    for r in range(args.rounds):
        w = args.warmup if r == 0 else 1
        rounds.append(dict(barlow_ms=_timed(run_barlow, args.steps, w), vicreg_ms=_timed(run_vicreg, args.steps, w)))
    # the loss kernels alone, at the step's shape
    n, D, dev = args.batch, args.width, RT.device
    ops.set_f32_matmul('exact')
    h = torch.randn(2 * n, D, device=dev) + 1.0
    bws = ops.bt_workspace(n, n, D, dev)
    zhat, rstd = ops.bt_standardize(h)
    ops.bt_fwd(zhat, n, 0, 0.0051, ws=bws)
    g, cs = ops.bt_bwd(zhat, n, 0, 0.0051, 1.0, 1.0, bws)
    bt_us = (_median_us(lambda: ops.bt_standardize(h)), _median_us(lambda: ops.bt_fwd(zhat, n, 0, 0.0051, ws=bws)),
             _median_us(lambda: ops.bt_bwd(zhat, n, 0, 0.0051, 1.0, 1.0, bws)), _median_us(lambda: ops.bt_apply(g, zhat, rstd, cs, 0)))
    vws = ops.vicreg_workspace(n, n, D, dev)
    xc, st = ops.vicreg_center(h)
    ops.vicreg_fwd(h, xc, st, n, 0, ws=vws)
    vr_us = (_median_us(lambda: ops.vicreg_center(h)), _median_us(lambda: ops.vicreg_fwd(h, xc, st, n, 0, ws=vws)),
             _median_us(lambda: ops.vicreg_bwd(h, xc, st, n, 0, 25.0, 25.0, 1.0, 1.0, 1.0, vws)))
    kernels_ms = (sum(vr_us) - sum(bt_us)) / 1e3

    mean = {k: sum(r[k] for r in rounds) / len(rounds) for k in rounds[0]}
    spread = max(r['barlow_ms'] for r in rounds) - min(r['barlow_ms'] for r in rounds)
    allowance = mean['barlow_ms'] + kernels_ms + spread
    con = last['vicreg']['con_loss']
    res = dict(batch=args.batch, image_size=args.size, resnet_depth=args.depth, f32_matmul=args.f32_matmul, loss_width=D,
               k_splits=ops.vicreg_k_splits(n, n, D), steps=args.steps, rounds=[{k: round(v, 3) for k, v in r.items()} for r in rounds],
               barlow_ms=round(mean['barlow_ms'], 3), vicreg_ms=round(mean['vicreg_ms'], 3),
               vicreg_center_us=round(vr_us[0], 1), vicreg_fwd_us=round(vr_us[1], 1), vicreg_bwd_us=round(vr_us[2], 1),
               bt_standardize_us=round(bt_us[0], 1), bt_fwd_us=round(bt_us[1], 1), bt_bwd_us=round(bt_us[2], 1), bt_apply_us=round(bt_us[3], 1),
               loss_kernels_difference_ms=round(kernels_ms, 3), barlow_round_spread_ms=round(spread, 3), allowance_ms=round(allowance, 3),
               vicreg_minus_allowance_ms=round(mean['vicreg_ms'] - allowance, 3),
               barlow_loss=float(last['barlow']['con_loss'].value), vicreg_loss=float(con.value), vicreg_inv=float(con.invariance),
               vicreg_var=float(con.variance), vicreg_cov=float(con.covariance))
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
