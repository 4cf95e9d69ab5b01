"""Time the BYOL pretraining step under --aug_recipe=byol next to --aug_recipe=simclr (blur on), ResNet-50 1x at 224 px on two-view
synthetic batches, ONE model and ONE process, alternating in `rounds` rounds (after tools/byol_step_time.py):
    python tools/aug_recipe_step_time.py [--batch 512] [--steps 10] [--warmup 3] [--rounds 2] [--blur_ms 1.3] [--out FILE]
The step resolves the plan as it reads it (flags.aug_plan), so the recipe is switched between the timed loops by the flag alone.
Expectation: the simclr step plus 10 % of the blur's share (1.1 blurred views per image instead of 1.0; --blur_ms is the blur's time
per step from DESIGN.md); allowance: that plus the spread of the simclr rounds.  Prints (and writes to --out) one JSON object."""
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
    ap.add_argument('--blur_ms', type=float, default=1.3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    from simclr_amd import model as model_lib
    from simclr_amd.flags import FLAGS
    from simclr_amd.resnet import RT
    from simclr_amd.run import make_single_step, synthetic_batches
    ncls = 10 if args.size <= 32 else 1000
    FLAGS.reset()
    FLAGS.update(resnet_depth=args.depth, image_size=args.size, train_batch_size=args.batch, use_blur=True, compute_dtype='f32',
                 f32_matmul=args.f32_matmul, train_mode='pretrain', byol_pred_hidden_dim=args.pred_hidden_dim, contrastive_loss='byol')
    RT.reset()
    RT.device = torch.device('cuda', torch.cuda.current_device())
    online = model_lib.Model(ncls)
    target = model_lib.TargetNetwork(online, 1000)
    step = make_single_step(online, model_lib.build_optimizer(0.1), None, target=target)
    data = synthetic_batches(args.batch, args.size, ncls, RT.device, views=2)
    last = {}

    def run(recipe):
        def fn():
            with FLAGS.override(aug_recipe=recipe):
                last[recipe] = step(*next(data))
        return fn
    rounds = []
    for r in range(args.rounds):
        w = args.warmup if r == 0 else 1
        rounds.append(dict(simclr_ms=_timed(run('simclr'), args.steps, w), byol_ms=_timed(run('byol'), args.steps, w)))
    mean = {k: sum(r[k] for r in rounds) / len(rounds) for k in rounds[0]}
    spread = max(r['simclr_ms'] for r in rounds) - min(r['simclr_ms'] for r in rounds)
    expected = mean['simclr_ms'] + 0.1 * args.blur_ms
    allowance = expected + spread
    res = dict(batch=args.batch, image_size=args.size, resnet_depth=args.depth, f32_matmul=args.f32_matmul, contrastive_loss='byol',
               use_blur=True, steps=args.steps, rounds=[{k: round(v, 3) for k, v in r.items()} for r in rounds],
               simclr_recipe_ms=round(mean['simclr_ms'], 3), byol_recipe_ms=round(mean['byol_ms'], 3),
               simclr_round_spread_ms=round(spread, 3), blur_ms_per_step_assumed=args.blur_ms, expected_ms=round(expected, 3),
               allowance_ms=round(allowance, 3), byol_minus_allowance_ms=round(mean['byol_ms'] - allowance, 3),
               expectation='byol recipe = simclr recipe + 10 % of the blur (1.1 blurred views per image instead of 1.0), within the '
                           'spread of the simclr rounds',
               confirmed=bool(mean['byol_ms'] <= allowance),
               simclr_loss=float(last['simclr']['con_loss'].value), byol_loss=float(last['byol']['con_loss'].value))
    line = json.dumps(res, indent=1)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
