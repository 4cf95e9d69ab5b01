"""Time the distillation step (run.make_single_step(..., teacher=...)) next to its two parts, ResNet-50 1x at 224 px on single-view
synthetic batches, alternating in ONE process and in `rounds` rounds:
    python tools/distill_step_time.py [--batch 512] [--steps 10] [--warmup 3] [--rounds 2] [--f32_matmul f16x3_3] [--out FILE]
      (a) the plain train_mode=finetune step (fine_tune_after_block = -1),
      (b) the teacher's inference forward alone (model.Teacher.__call__),
      (c) the distillation step = (b) inside (a), add_kd_loss in place of the supervised loss.
Prints (and writes to --out) one JSON object: the per-round times, their means, the allowance (a) + (b) + the spread of (a) between
the rounds, and by how much (c) overshoots it (0 when it does not).  The teacher is freshly initialised unless --teacher_checkpoint
names a file: the time does not depend on the weights."""
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
    ap.add_argument('--teacher_depth', type=int, default=None)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--f32_matmul', default='f16x3_3')
    ap.add_argument('--temperature', type=float, default=1.0)
    ap.add_argument('--teacher_checkpoint', default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    from simclr_amd import model as model_lib
    from simclr_amd.flags import FLAGS
    from simclr_amd.resnet import RT
    from simclr_amd.run import make_single_step, synthetic_batches
    ncls = 10 if args.size <= 32 else 1000
    FLAGS.reset()
    FLAGS.update(resnet_depth=args.depth, image_size=args.size, train_batch_size=args.batch, use_blur=False, compute_dtype='f32',
                 f32_matmul=args.f32_matmul, train_mode='finetune', fine_tune_after_block=-1, distill_temperature=args.temperature,
                 teacher_resnet_depth=args.teacher_depth)
    RT.reset()
    RT.device = torch.device('cuda', torch.cuda.current_device())
    teacher = model_lib.Teacher(ncls, args.teacher_checkpoint)
    plain = model_lib.Model(ncls)
    with RT.fresh_names():
        student = model_lib.Model(ncls)
    step_plain = make_single_step(plain, model_lib.build_optimizer(0.1), None)
    step_kd = make_single_step(student, model_lib.build_optimizer(0.1), None, teacher=teacher)
    data = synthetic_batches(args.batch, args.size, ncls, RT.device, views=1)
    last = {}

    def run_plain():
        last['plain'] = step_plain(*next(data))

    def run_teacher():
        teacher(next(data)[0])

    def run_kd():
        last['kd'] = step_kd(*next(data))
    rounds = []
    for r in range(args.rounds):
        w = args.warmup if r == 0 else 1
        rounds.append(dict(finetune_ms=_timed(run_plain, args.steps, w), teacher_forward_ms=_timed(run_teacher, args.steps, w),
                           distill_ms=_timed(run_kd, args.steps, w)))
    mean = {k: sum(r[k] for r in rounds) / len(rounds) for k in rounds[0]}
    spread = max(r['finetune_ms'] for r in rounds) - min(r['finetune_ms'] for r in rounds)
    allowance = mean['finetune_ms'] + mean['teacher_forward_ms'] + spread
    res = dict(batch=args.batch, image_size=args.size, resnet_depth=args.depth, teacher_resnet_depth=args.teacher_depth or args.depth,
               f32_matmul=args.f32_matmul, temperature=args.temperature, steps=args.steps, rounds=[{k: round(v, 3) for k, v in r.items()} for r in rounds],
               finetune_ms=round(mean['finetune_ms'], 3), teacher_forward_ms=round(mean['teacher_forward_ms'], 3),
               distill_ms=round(mean['distill_ms'], 3), finetune_round_spread_ms=round(spread, 3), allowance_ms=round(allowance, 3),
               overshoot_ms=round(max(mean['distill_ms'] - allowance, 0.0), 3),
               supervised_loss=float(last['plain']['sup_loss'].value), distill_loss=float(last['kd']['sup_loss'].value),
               distill_agreement=float(last['kd']['sup_loss'].acc))
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
