"""Time the BYOL step (run.make_single_step(..., target=...)) next to its two parts, ResNet-50 1x at 224 px on two-view synthetic
batches, alternating in ONE process and in `rounds` rounds:
    python tools/byol_step_time.py [--batch 512] [--steps 10] [--warmup 3] [--rounds 2] [--f32_matmul f16x3_3] [--out FILE]
      (a) the NT-Xent pretraining step,
      (b) the target network's training-mode forward alone (model.TargetNetwork.__call__: batch statistics, nothing kept),
      (c) the BYOL step = (b) inside (a), with the predictor, add_byol_loss in place of NT-Xent and the moving-average launch.
Prints (and writes to --out) one JSON object: the per-round times, their means, the allowance (a) + (b) + the spread of (a) between
the rounds, and the difference (c) - allowance, whichever way it falls."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--depth', type=int, default=50)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--f32_matmul', default='f16x3_3')
    ap.add_argument('--pred_hidden_dim', type=int, default=4096)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    from simclr_amd import model as model_lib
    from simclr_amd.flags import FLAGS
    from simclr_amd.resnet import RT
    from simclr_amd.run import make_single_step, synthetic_batches
    ncls = 10 if args.size <= 32 else 1000
    FLAGS.reset()
    FLAGS.update(resnet_depth=args.depth, image_size=args.size, train_batch_size=args.batch, use_blur=False, compute_dtype='f32',
                 f32_matmul=args.f32_matmul, train_mode='pretrain', byol_pred_hidden_dim=args.pred_hidden_dim)
    RT.reset()
    RT.device = torch.device('cuda', torch.cuda.current_device())
    plain = model_lib.Model(ncls)
    step_plain = make_single_step(plain, model_lib.build_optimizer(0.1), None)
    total = 1000
    with FLAGS.override(contrastive_loss='byol'), RT.fresh_names():
        online = model_lib.Model(ncls)
        target = model_lib.TargetNetwork(online, total)
    data = synthetic_batches(args.batch, args.size, ncls, RT.device, views=2)
    last = {}
    box = {}

    def run_plain():
        last['plain'] = step_plain(*next(data))

    def run_target():
        target(next(data)[0])

    def run_byol():
        with FLAGS.override(contrastive_loss='byol'):
            if 'step' not in box:
                box['step'] = make_single_step(online, model_lib.build_optimizer(0.1), None, target=target)
            last['byol'] = box['step'](*next(data))
    rounds = []
    for r in range(args.rounds):
        w = args.warmup if r == 0 else 1
        rounds.append(dict(ntxent_ms=_timed(run_plain, args.steps, w), target_forward_ms=_timed(run_target, args.steps, w),
                           byol_ms=_timed(run_byol, args.steps, w)))
    mean = {k: sum(r[k] for r in rounds) / len(rounds) for k in rounds[0]}
    spread = max(r['ntxent_ms'] for r in rounds) - min(r['ntxent_ms'] for r in rounds)
    allowance = mean['ntxent_ms'] + mean['target_forward_ms'] + spread
    res = dict(batch=args.batch, image_size=args.size, resnet_depth=args.depth, f32_matmul=args.f32_matmul,
               byol_pred_hidden_dim=args.pred_hidden_dim, steps=args.steps,
               rounds=[{k: round(v, 3) for k, v in r.items()} for r in rounds],
               ntxent_ms=round(mean['ntxent_ms'], 3), target_forward_ms=round(mean['target_forward_ms'], 3), byol_ms=round(mean['byol_ms'], 3),
               ntxent_round_spread_ms=round(spread, 3), allowance_ms=round(allowance, 3),
               byol_minus_allowance_ms=round(mean['byol_ms'] - allowance, 3),
               ntxent_loss=float(last['plain']['con_loss'].value), byol_loss=float(last['byol']['con_loss'].value),
               byol_cosine=float(last['byol']['con_loss'].cosine))
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
