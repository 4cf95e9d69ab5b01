"""Time the NT-Xent pretraining step with --repr_metrics_steps=1 (every step measured) next to --repr_metrics_steps=0, ResNet-50 1x at
224 px on two-view synthetic batches, ONE process, alternating in `rounds` rounds (after tools/aug_recipe_step_time.py):
    python tools/repr_step_time.py [--batch 512] [--steps 10] [--warmup 3] [--rounds 2] [--out FILE]
The step reads K when it is made and a model serves one step function, so each flag value gets a model and an optimizer of its own
(the same seeded initial weights).
Expectation: the K = 0 step plus the time of the new launches alone (l2norm_fwd + ops.repr_stats at N = batch, D = proj_out_dim, timed
here in the same process); allowance: that plus the spread of the K = 0 rounds.  Prints (and writes to --out) one JSON object."""
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
                 f32_matmul=args.f32_matmul, train_mode='pretrain', contrastive_loss='ntxent')
    RT.reset()
    RT.device = torch.device('cuda', torch.cuda.current_device())
    steps = {}
    for K in (0, 1):
        with FLAGS.override(repr_metrics_steps=K):
            steps[K] = make_single_step(model_lib.Model(ncls), model_lib.build_optimizer(0.1), None)
    data = synthetic_batches(args.batch, args.size, ncls, RT.device, views=2)
    last = {}

    def run(K):
        def fn():
            last[K] = steps[K](*next(data))
        return fn
    rounds = []
    for r in range(args.rounds):
        w = args.warmup if r == 0 else 1
        rounds.append(dict(k0_ms=_timed(run(0), args.steps, w), k1_ms=_timed(run(1), args.steps, w)))
    # the new launches alone, at the step's shape
    D = FLAGS.proj_out_dim
    h = torch.randn(2 * args.batch, D, device=RT.device)

    def launches():
        z, _ = ops.l2norm_fwd(h)
        ops.repr_stats(z, FLAGS.repr_uniform_t)
    launches_ms = _timed(launches, 20, 3)
    mean = {k: sum(r[k] for r in rounds) / len(rounds) for k in rounds[0]}
    spread = max(r['k0_ms'] for r in rounds) - min(r['k0_ms'] for r in rounds)
    expected = mean['k0_ms'] + launches_ms
    allowance = expected + spread
    s = last[1]['repr_stats']
    res = dict(batch=args.batch, image_size=args.size, resnet_depth=args.depth, f32_matmul=args.f32_matmul, contrastive_loss='ntxent',
               proj_out_dim=D, steps=args.steps, rounds=[{k: round(v, 3) for k, v in r.items()} for r in rounds],
               k0_ms=round(mean['k0_ms'], 3), k1_ms=round(mean['k1_ms'], 3), k0_round_spread_ms=round(spread, 3),
               new_launches_ms=round(launches_ms, 4), expected_ms=round(expected, 3), allowance_ms=round(allowance, 3),
               k1_minus_allowance_ms=round(mean['k1_ms'] - allowance, 3),
               expectation='K = 1 step = K = 0 step + the time of the new launches alone, within the spread of the K = 0 rounds',
               confirmed=bool(mean['k1_ms'] <= allowance),
               repr_values=dict(align=float(s.align), uniform=float(s.uniform), std=float(s.std), rank=float(s.rank)))
    line = json.dumps(res, indent=1)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
