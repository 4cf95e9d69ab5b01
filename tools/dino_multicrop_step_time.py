"""Time the DINO multi-crop step (run.make_single_step under --contrastive_loss=dino --dino_local_crops=L) next to the plain dino step,
ResNet-50 1x at 224 px on synthetic batches, alternating in ONE process and in `rounds` rounds:
    python tools/dino_multicrop_step_time.py [--batch 512] [--local_crops 6] [--local_size 96] [--out_dim 65536] [--width 256]
                                             [--steps 10] [--warmup 3] [--rounds 2] [--f32_matmul f16x3_3] [--out FILE]
      (a) the dino step on the two global views,
      (t) the target network's forward alone (the teacher sees the global views only: its share does not grow with L),
      (b) the multi-crop step = (a) up to its backward, then the L local views through the online encoder a second time,
          add_dino_local_loss against the teacher rows of (a), its backward, the add of the two gradient buffers, one optimizer step.
Then the three local loss calls alone, median of 5, at the step's shapes.  Prints (and writes to --out) one JSON object: the per-round
times, their means, the allowance (a) + ((a) - (t)) * L h^2 / (2 H^2) (the ONLINE share of the step by pixel count) + the local loss
launches + the spread of (a) between the rounds, and the difference (b) - allowance, whichever way it falls."""
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
    ap.add_argument('--local_crops', type=int, default=6)
    ap.add_argument('--local_size', type=int, default=96)
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
    L, K = args.local_crops, args.out_dim
    FLAGS.reset()
    FLAGS.update(resnet_depth=args.depth, image_size=args.size, train_batch_size=args.batch, use_blur=False, compute_dtype='f32',
                 f32_matmul=args.f32_matmul, train_mode='pretrain', proj_out_dim=args.width, dino_out_dim=K,
                 dino_freeze_last_layer_epochs=0, contrastive_loss='dino', dino_local_crop_size=args.local_size)
    RT.reset()
    RT.device = torch.device('cuda', torch.cuda.current_device())
    total = 1000
    plain = model_lib.Model(ncls)
    plain_target = model_lib.TargetNetwork(plain, total, center=model_lib.DinoCenter(K), steps_per_epoch=100)
    step_plain = make_single_step(plain, model_lib.build_optimizer(0.1), None, target=plain_target)
    with RT.fresh_names():
        multi = model_lib.Model(ncls)
        multi_target = model_lib.TargetNetwork(multi, total, center=model_lib.DinoCenter(K), steps_per_epoch=100)
    data = synthetic_batches(args.batch, args.size, ncls, RT.device, views=2, local_crops=L, local_size=args.local_size)
    last = {}
    box = {}

    def run_plain():
        (g, _), labels = next(data)
        last['dino'] = step_plain(g, labels)

    def run_target():
        plain_target(next(data)[0][0])

    def run_multi():
        with FLAGS.override(dino_local_crops=L):
            if 'step' not in box:
                box['step'] = make_single_step(multi, model_lib.build_optimizer(0.1), None, target=multi_target)
            last['multicrop'] = box['step'](*next(data))
    rounds = []
    for r in range(args.rounds):
        w = args.warmup if r == 0 else 1
        rounds.append(dict(dino_ms=_timed(run_plain, args.steps, w), target_forward_ms=_timed(run_target, args.steps, w),
                           multicrop_ms=_timed(run_multi, args.steps, w)))
    # the local loss launches alone, at the step's shapes
    b, D, dev = args.batch, FLAGS.proj_out_dim, RT.device
    ops.set_f32_matmul('exact')
    q = torch.nn.functional.normalize(torch.randn(2 * b, D, device=dev), dim=1)
    k = torch.nn.functional.normalize(q + 0.5 * torch.randn(2 * b, D, device=dev) / D ** 0.5, dim=1)
    x = torch.nn.functional.normalize(torch.randn(L * b, D, device=dev), dim=1)
    ws = torch.nn.functional.normalize(torch.randn(K, D, device=dev), dim=1)
    wt = torch.nn.functional.normalize(ws + 0.1 * torch.randn(K, D, device=dev) / D ** 0.5, dim=1)
    c = 0.05 * torch.randn(K, device=dev)
    _, drs, du, _ = ops.dino_fwd(q, k, ws, wt, c, 0.1, 0.04)
    mws = ops.swav_local_workspace(b, L, K, D, dev)
    _, mrs, _ = ops.swav_local_fwd(x, ws, du, L, 0.1, workspace=mws)
    lws = ops.dino_local_workspace(b, L, K, D, dev)
    local_us = (_median_us(lambda: ops.swav_local_fwd(x, ws, du, L, 0.1, workspace=mws)),
                _median_us(lambda: ops.swav_local_bwd_x(x, ws, du, L, 0.1, mrs, 1.0, mws)),
                _median_us(lambda: ops.dino_local_bwd_w(x, k, ws, wt, c, L, 0.1, 0.04, mrs, drs, 1.0, lws)))
    kernels_ms = sum(local_us) / 1e3

    mean = {n: sum(r[n] for r in rounds) / len(rounds) for n in rounds[0]}
    spread = max(r['dino_ms'] for r in rounds) - min(r['dino_ms'] for r in rounds)
    pixels = L * (args.local_size / args.size) ** 2 / 2.0
    online = mean['dino_ms'] - mean['target_forward_ms']
    allowance = mean['dino_ms'] + online * pixels + kernels_ms + spread
    res = dict(batch=args.batch, image_size=args.size, local_crops=L, local_crop_size=args.local_size, resnet_depth=args.depth,
               f32_matmul=args.f32_matmul, dino_out_dim=K, loss_width=D, steps=args.steps,
               rounds=[{n: round(v, 3) for n, v in r.items()} for r in rounds], dino_ms=round(mean['dino_ms'], 3),
               target_forward_ms=round(mean['target_forward_ms'], 3), online_share_ms=round(online, 3),
               multicrop_ms=round(mean['multicrop_ms'], 3), multicrop_over_dino=round(mean['multicrop_ms'] / mean['dino_ms'], 3),
               pixel_ratio=round(pixels, 4), local_fwd_us=round(local_us[0], 1), local_bwd_x_us=round(local_us[1], 1),
               dino_local_bwd_w_us=round(local_us[2], 1), local_loss_kernels_ms=round(kernels_ms, 3), dino_round_spread_ms=round(spread, 3),
               allowance_ms=round(allowance, 3), multicrop_minus_allowance_ms=round(mean['multicrop_ms'] - allowance, 3),
               dino_loss=float(last['dino']['con_loss'].value), multicrop_loss=float(last['multicrop']['con_loss'].value))
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
