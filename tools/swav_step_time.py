"""Time the SwAV step (run.make_single_step under --contrastive_loss=swav) next to the NT-Xent step, ResNet-50 1x at 224 px on
two-view synthetic batches, alternating in ONE process and in `rounds` rounds:
    python tools/swav_step_time.py [--batch 512] [--prototypes 3000] [--width 128] [--steps 10] [--warmup 3] [--rounds 2]
                                   [--f32_matmul f16x3_3] [--out FILE]
      (a) the NT-Xent pretraining step,
      (b) the swav step = (a) with add_swav_loss onto the prototypes in place of NT-Xent: the prototype normalisation, the Sinkhorn on
          the batch, the loss sweeps and the prototype gradient.
Then the loss kernels alone, median of 5: swav sinkhorn + fwd + bwd_q + bwd_w at (2n, K, D) and NT-Xent fwd + bwd at (n, n, D), the
sweeps (b) trades.  Prints (and writes to --out) one JSON object: the per-round times, their means, the allowance (a) + (swav kernels -
NT-Xent kernels) + the spread of (a) between the rounds, and the difference (b) - allowance, whichever way it falls."""
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
    ap.add_argument('--prototypes', type=int, default=3000)
    ap.add_argument('--width', type=int, default=128)
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
                 f32_matmul=args.f32_matmul, train_mode='pretrain', proj_out_dim=args.width, swav_num_prototypes=args.prototypes,
                 swav_freeze_prototypes_epochs=0)
    RT.reset()
    RT.device = torch.device('cuda', torch.cuda.current_device())
    plain = model_lib.Model(ncls)
    step_plain = make_single_step(plain, model_lib.build_optimizer(0.1), None)
    with FLAGS.override(contrastive_loss='swav'), RT.fresh_names():
        online = model_lib.Model(ncls)
    data = synthetic_batches(args.batch, args.size, ncls, RT.device, views=2)
    last = {}
    box = {}

    def run_plain():
        last['plain'] = step_plain(*next(data))

    def run_swav():
        with FLAGS.override(contrastive_loss='swav'):
            if 'step' not in box:
                box['step'] = make_single_step(online, model_lib.build_optimizer(0.1), None, steps_per_epoch=100)
            last['swav'] = box['step'](*next(data))
    rounds = []
    for r in range(args.rounds):
        w = args.warmup if r == 0 else 1
        rounds.append(dict(ntxent_ms=_timed(run_plain, args.steps, w), swav_ms=_timed(run_swav, args.steps, w)))
    # the loss kernels alone, at the step's shapes
    n, D, dev = args.batch, FLAGS.proj_out_dim, RT.device
    ops.set_f32_matmul('exact')
    q = torch.nn.functional.normalize(torch.randn(2 * n, D, device=dev), dim=1)
    K = args.prototypes
    w = torch.nn.functional.normalize(torch.randn(K, D, device=dev), dim=1)
    sws = ops.swav_workspace(2 * n, K, D, dev)
    lws = ops.swav_workspace(2 * n, K, D, dev)
    alpha = ops.swav_sinkhorn(q, w, 0.05, 3, workspace=sws)
    _, srs, su, _ = ops.swav_fwd(q, w, alpha, 0.1, 0.05, workspace=lws)
    swav_us = (_median_us(lambda: ops.swav_sinkhorn(q, w, 0.05, 3, workspace=sws)),
               _median_us(lambda: ops.swav_fwd(q, w, alpha, 0.1, 0.05, workspace=lws)),
               _median_us(lambda: ops.swav_bwd_q(q, w, su, 0.1, srs, 1.0, lws)),
               _median_us(lambda: ops.swav_bwd_w(q, w, alpha, 0.1, 0.05, srs, 1.0, lws)))
    nws = ops.ntxent_workspace(n, n, D, dev)
    nout, nrs, _ = ops.ntxent_fwd(q, q, 0, 0.1, nws)
    ntx_us = (_median_us(lambda: ops.ntxent_fwd(q, q, 0, 0.1, nws)), _median_us(lambda: ops.ntxent_bwd(q, q, 0, 0.1, nrs, 1.0, nout, nws)))
    kernels_ms = (sum(swav_us) - sum(ntx_us)) / 1e3

    mean = {k: sum(r[k] for r in rounds) / len(rounds) for k in rounds[0]}
    spread = max(r['ntxent_ms'] for r in rounds) - min(r['ntxent_ms'] for r in rounds)
    allowance = mean['ntxent_ms'] + kernels_ms + spread
    res = dict(batch=args.batch, image_size=args.size, resnet_depth=args.depth, f32_matmul=args.f32_matmul, swav_num_prototypes=K,
               loss_width=D, steps=args.steps, rounds=[{k: round(v, 3) for k, v in r.items()} for r in rounds],
               ntxent_ms=round(mean['ntxent_ms'], 3), swav_ms=round(mean['swav_ms'], 3), swav_sinkhorn_us=round(swav_us[0], 1),
               swav_fwd_us=round(swav_us[1], 1), swav_bwd_q_us=round(swav_us[2], 1), swav_bwd_w_us=round(swav_us[3], 1),
               ntxent_fwd_us=round(ntx_us[0], 1), ntxent_bwd_us=round(ntx_us[1], 1),
               loss_kernels_difference_ms=round(kernels_ms, 3), ntxent_round_spread_ms=round(spread, 3), allowance_ms=round(allowance, 3),
               swav_minus_allowance_ms=round(mean['swav_ms'] - allowance, 3),
               ntxent_loss=float(last['plain']['con_loss'].value), swav_loss=float(last['swav']['con_loss'].value),
               swav_code_entropy=float(last['swav']['con_loss'].entropy))
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
