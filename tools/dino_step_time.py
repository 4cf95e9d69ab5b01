"""Time the DINO step (run.make_single_step(..., target=...) under --contrastive_loss=dino) next to its two parts, ResNet-50 1x at
224 px on two-view synthetic batches, alternating in ONE process and in `rounds` rounds:
    python tools/dino_step_time.py [--batch 512] [--out_dim 65536] [--width 256] [--steps 10] [--warmup 3] [--rounds 2]
                                   [--f32_matmul f16x3_3] [--out FILE]
      (a) the NT-Xent pretraining step,
      (b) the target network's training-mode forward alone (model.TargetNetwork.__call__: batch statistics, nothing kept),
      (c) the dino step = (b) inside (a), with add_dino_loss onto the prototypes in place of NT-Xent, the two prototype
          normalisations, the moving-average launch and the centre update.
Then the loss kernels alone, median of 5: dino fwd + bwd_q + bwd_w at (2n, K, D) and NT-Xent fwd + bwd at (n, n, D), the sweeps (c)
trades.  Prints (and writes to --out) one JSON object: the per-round times, their means, the allowance (a) + (b) + (dino kernels -
NT-Xent kernels) + the spread of (a) between the rounds, and the difference (c) - allowance, whichever way it falls."""
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
    ap.add_argument('--out_dim', type=int, default=65536)
    ap.add_argument('--width', type=int, default=256)
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
                 f32_matmul=args.f32_matmul, train_mode='pretrain', proj_out_dim=args.width, dino_out_dim=args.out_dim,
                 dino_freeze_last_layer_epochs=0)
    RT.reset()
    RT.device = torch.device('cuda', torch.cuda.current_device())
    plain = model_lib.Model(ncls)
    step_plain = make_single_step(plain, model_lib.build_optimizer(0.1), None)
    total = 1000
    with FLAGS.override(contrastive_loss='dino'), RT.fresh_names():
        online = model_lib.Model(ncls)
        target = model_lib.TargetNetwork(online, total, center=model_lib.DinoCenter(args.out_dim), steps_per_epoch=100)
    data = synthetic_batches(args.batch, args.size, ncls, RT.device, views=2)
    last = {}
    box = {}

    def run_plain():
        last['plain'] = step_plain(*next(data))

    def run_target():
        target(next(data)[0])

    def run_dino():
        with FLAGS.override(contrastive_loss='dino'):
            if 'step' not in box:
                box['step'] = make_single_step(online, model_lib.build_optimizer(0.1), None, target=target)
            last['dino'] = box['step'](*next(data))
    rounds = []
    for r in range(args.rounds):
        w = args.warmup if r == 0 else 1
        rounds.append(dict(ntxent_ms=_timed(run_plain, args.steps, w), target_forward_ms=_timed(run_target, args.steps, w),
                           dino_ms=_timed(run_dino, args.steps, w)))
    # the loss kernels alone, at the step's shapes
    n, D, dev = args.batch, FLAGS.proj_out_dim, RT.device
    ops.set_f32_matmul('exact')
    q = torch.nn.functional.normalize(torch.randn(2 * n, D, device=dev), dim=1)
    k = torch.nn.functional.normalize(q.roll(n, 0) + 0.5 * torch.randn(2 * n, D, device=dev), dim=1)
    K = args.out_dim
    ws = torch.nn.functional.normalize(torch.randn(K, D, device=dev), dim=1)
    wt = torch.nn.functional.normalize(ws + 0.1 * torch.randn(K, D, device=dev), dim=1)
    c = 0.05 * torch.randn(K, device=dev)
    dws = ops.dino_workspace(2 * n, K, D, dev)
    _, drs, du, _ = ops.dino_fwd(q, k, ws, wt, c, 0.1, 0.04, workspace=dws)
    dino_us = (_median_us(lambda: ops.dino_fwd(q, k, ws, wt, c, 0.1, 0.04, workspace=dws)),
               _median_us(lambda: ops.dino_bwd_q(q, ws, du, 0.1, drs, 1.0, dws)),
               _median_us(lambda: ops.dino_bwd_w(q, k, ws, wt, c, 0.1, 0.04, drs, 1.0, dws)))
    nws = ops.ntxent_workspace(n, n, D, dev)
    nout, nrs, _ = ops.ntxent_fwd(q, q, 0, 0.1, nws)
    ntx_us = (_median_us(lambda: ops.ntxent_fwd(q, q, 0, 0.1, nws)), _median_us(lambda: ops.ntxent_bwd(q, q, 0, 0.1, nrs, 1.0, nout, nws)))
    kernels_ms = (sum(dino_us) - sum(ntx_us)) / 1e3

    mean = {k: sum(r[k] for r in rounds) / len(rounds) for k in rounds[0]}
    spread = max(r['ntxent_ms'] for r in rounds) - min(r['ntxent_ms'] for r in rounds)
    allowance = mean['ntxent_ms'] + mean['target_forward_ms'] + kernels_ms + spread
    res = dict(batch=args.batch, image_size=args.size, resnet_depth=args.depth, f32_matmul=args.f32_matmul, dino_out_dim=K,
               loss_width=D, steps=args.steps, rounds=[{k: round(v, 3) for k, v in r.items()} for r in rounds],
               ntxent_ms=round(mean['ntxent_ms'], 3), target_forward_ms=round(mean['target_forward_ms'], 3),
               dino_ms=round(mean['dino_ms'], 3), dino_fwd_us=round(dino_us[0], 1), dino_bwd_q_us=round(dino_us[1], 1),
               dino_bwd_w_us=round(dino_us[2], 1), ntxent_fwd_us=round(ntx_us[0], 1), ntxent_bwd_us=round(ntx_us[1], 1),
               loss_kernels_difference_ms=round(kernels_ms, 3), ntxent_round_spread_ms=round(spread, 3), allowance_ms=round(allowance, 3),
               dino_minus_allowance_ms=round(mean['dino_ms'] - allowance, 3),
               ntxent_loss=float(last['plain']['con_loss'].value), dino_loss=float(last['dino']['con_loss'].value),
               dino_teacher_entropy=float(last['dino']['con_loss'].entropy))
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
