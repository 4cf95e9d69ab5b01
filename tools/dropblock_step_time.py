"""Time the pretraining step (run.make_single_step) of ResNet-50 1x at 224 px with DropBlock in block groups 3 and 4 against the default
step, alternating in one process:
    python tools/dropblock_step_time.py [--batch 512] [--keep_probs 1,1,0.9,0.9] [--size_db 7] [--rounds 2] [--steps 10] [--warmup 3]
                                        [--f32_matmul f16x3_3] [--out FILE]
Prints one JSON line per (round, variant): ms per step (mean over `steps` after `warmup`); --out collects them in one JSON file.
The DropBlock step gives up three fusions in every block with an active keep probability (the fused conv3 + bn3 + shortcut + ReLU tail,
the folded tail BatchNorm backward, the BatchNorm-backward reduce in the consumer's data gradient): this reports what that costs."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def time_pretrain(keep_probs, size_db, batch, size, steps, warmup, f32_matmul, compute_dtype, depth=50):
    from simclr_amd import model as model_lib
    from simclr_amd.flags import FLAGS
    from simclr_amd.resnet import RT
    from simclr_amd.run import make_single_step, synthetic_batches
    FLAGS.reset()
    FLAGS.update(resnet_depth=depth, image_size=size, train_batch_size=batch, use_blur=False, compute_dtype=compute_dtype,
                 f32_matmul=f32_matmul)
    if keep_probs:
        FLAGS.update(dropblock_keep_probs=keep_probs, dropblock_size=size_db)
    RT.reset()
    RT.device = torch.device('cuda', torch.cuda.current_device())
    model = model_lib.Model(1000)
    step = make_single_step(model, model_lib.build_optimizer(0.1), None)
    data = synthetic_batches(batch, size, 1000, RT.device)
    for _ in range(warmup):
        step(*next(data))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = step(*next(data))
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    res = dict(dropblock_keep_probs=keep_probs or None, dropblock_size=size_db if keep_probs else None, batch=batch, image_size=size,
               compute_dtype=compute_dtype, f32_matmul=f32_matmul, steps=steps, ms_per_step=round(dt * 1e3, 3),
               images_per_sec=round(batch / dt, 1), total_loss=float(out['total_loss'].reshape(-1)[0]))
    del model, step, data, out
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--depth', type=int, default=50)
    ap.add_argument('--keep_probs', default='1,1,0.9,0.9')
    ap.add_argument('--size_db', type=int, default=7)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--compute_dtype', default='f32')
    ap.add_argument('--f32_matmul', default='f16x3_3')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    rows = []
    for rnd in range(args.rounds):
        for keep_probs in ('', args.keep_probs):
            r = time_pretrain(keep_probs, args.size_db, args.batch, args.size, args.steps, args.warmup, args.f32_matmul,
                              args.compute_dtype, args.depth)
            r['round'] = rnd
            rows.append(r)
            print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
