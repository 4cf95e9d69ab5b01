"""Time the pretraining step (run.make_single_step) of ResNet-50 1x at 224 px on two-view synthetic batches, by projection-head mode:
    python tools/head_mode_step_time.py [--batch 512] [--modes nonlinear,none] [--steps 20] [--warmup 5] [--f32_matmul f16x3_3]
proj_head_mode=none hands the 2048-wide encoder output to the contrastive loss (the wide NT-Xent kernels); the default nonlinear head
hands it 128 columns.  Prints one JSON line per mode: ms per step (mean over `steps` after `warmup`) and images/s."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def time_pretrain(mode, batch, size, steps, warmup, f32_matmul, depth=50):
    from simclr_amd import model as model_lib
    from simclr_amd.flags import FLAGS
    from simclr_amd.resnet import RT
    from simclr_amd.run import make_single_step, synthetic_batches
    FLAGS.reset()
    FLAGS.update(resnet_depth=depth, image_size=size, train_batch_size=batch, use_blur=False, compute_dtype='f32',
                 f32_matmul=f32_matmul, proj_head_mode=mode)
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
    return dict(proj_head_mode=mode, batch=batch, image_size=size, f32_matmul=f32_matmul, steps=steps,
                embedding_width=int(out['con_loss'].normalized.shape[1]), ms_per_step=round(dt * 1e3, 3),
                images_per_sec=round(batch / dt, 1), contrast_loss=float(out['con_loss'].value.reshape(-1)[0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--modes', default='nonlinear,none')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--f32_matmul', default='f16x3_3')
    args = ap.parse_args()
    for mode in args.modes.split(','):
        print(json.dumps(time_pretrain(mode, args.batch, args.size, args.steps, args.warmup, args.f32_matmul)), flush=True)


if __name__ == '__main__':
    main()
