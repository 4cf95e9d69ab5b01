"""Time the pretraining step (run.make_single_step) of ResNet-50 1x at 224 px with plain NT-Xent and with NNCLR (--nn_queue_size: the
search of the local rows in the support queue, the neighbour-row loss, the enqueue), alternating in one process:
    python tools/nnclr_step_time.py [--batch 512] [--queue 65536] [--rounds 2] [--steps 10] [--warmup 3] [--out FILE]
Prints one JSON line per (round, loss): ms per step (mean over `steps` after `warmup`); --out collects them in one JSON file."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def time_pretrain(queue, batch, size, steps, warmup, f32_matmul, depth=50):
    from simclr_amd import model as model_lib
    from simclr_amd.flags import FLAGS
    from simclr_amd.resnet import RT
    from simclr_amd.run import make_single_step, synthetic_batches
    FLAGS.reset()
    FLAGS.update(resnet_depth=depth, image_size=size, train_batch_size=batch, use_blur=False, compute_dtype='f32', f32_matmul=f32_matmul,
                 nn_queue_size=queue)
    RT.reset()
    RT.device = torch.device('cuda', torch.cuda.current_device())
    model = model_lib.Model(1000)
    support = model_lib.SupportQueue(queue, model_lib.projection_width(), FLAGS.nn_queue_seed) if queue else None
    step = make_single_step(model, model_lib.build_optimizer(0.1), None, support=support)
    data = synthetic_batches(batch, size, 1000, RT.device)
    for _ in range(warmup):
        step(*next(data))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = step(*next(data))
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    con = out['con_loss']
    res = dict(loss='ntxent' if not queue else 'ntxent nn_queue_size=%d' % queue, batch=batch, image_size=size, f32_matmul=f32_matmul,
               steps=steps, ms_per_step=round(dt * 1e3, 3), images_per_sec=round(batch / dt, 1),
               contrast_loss=float(con.value.reshape(-1)[0]))
    if hasattr(con, 'nn_sim'):
        res['nn_similarity'] = float(con.nn_sim.reshape(-1)[0])
        res['contrast_acc'] = float(con.acc.reshape(-1)[0])
    del model, step, data, out, con, support
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--depth', type=int, default=50)
    ap.add_argument('--queue', type=int, default=65536)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--f32_matmul', default='f16x3_3')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    rows = []
    for rnd in range(args.rounds):
        for queue in (0, args.queue):
            r = time_pretrain(queue, args.batch, args.size, args.steps, args.warmup, args.f32_matmul, args.depth)
            r['round'] = rnd
            rows.append(r)
            print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
