"""Wall time of the cached-feature linear probe (simclr_amd/logreg.py) at ImageNet size:
    python tools/logreg_fit_time.py [--rows 1281167] [--dim 2048] [--classes 1000] [--encode_batches 20] [--batch 512] [--out FILE]
One fit with the default flags on random standardised features with random labels (the products cost what they cost on real features;
the iteration count does not transfer), and the encoding rate of model.features on synthetic 224 px images (ResNet-50, the default
arithmetic), measured on --encode_batches batches and scaled to --rows.  Prints and writes one JSON record."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=1281167)
    ap.add_argument('--dim', type=int, default=2048)
    ap.add_argument('--classes', type=int, default=1000)
    ap.add_argument('--encode_batches', type=int, default=20)
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--out', default=None, help='also write the record to this file')
    args = ap.parse_args()
    from simclr_amd import logreg
    from simclr_amd import model as model_lib
    from simclr_amd.flags import FLAGS
    from simclr_amd.resnet import RT
    FLAGS.reset()
    dev = torch.device('cuda', torch.cuda.current_device())
    rec = dict(rows=args.rows, dim=args.dim, classes=args.classes, l2=float(FLAGS.logreg_l2), max_iterations=FLAGS.logreg_max_iterations,
               tolerance=FLAGS.logreg_tolerance, history=FLAGS.logreg_history)
    if args.encode_batches:
        RT.reset()
        RT.device = dev
        model = model_lib.Model(args.classes)
        model(torch.zeros(2, FLAGS.image_size, FLAGS.image_size, 3, device=dev), training=False)      # builds the variables
        model.release()
        x = torch.rand(args.batch, FLAGS.image_size, FLAGS.image_size, 3, device=dev)
        for _ in range(3):
            model.features(x)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.encode_batches):
            model.features(x)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / args.encode_batches
        rec.update(encode_batch=args.batch, encode_ms_per_batch=round(dt * 1e3, 3), encode_images_per_sec=round(args.batch / dt, 1),
                   encode_seconds_scaled_to_rows=round(dt * args.rows / args.batch, 1))
        del model, x
        RT.reset()
    g = torch.Generator(device=dev).manual_seed(0)
    feats = torch.randn(args.rows, args.dim, device=dev, generator=g)
    labels = torch.randint(0, args.classes, (args.rows,), device=dev, generator=g).to(torch.int32)
    weights = torch.ones(args.rows, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    mu, var = logreg.standardize_stats(feats, weights)
    x = logreg.standardize(feats, mu, var)
    torch.cuda.synchronize()
    rec['standardize_seconds'] = round(time.perf_counter() - t0, 3)
    del feats
    t0 = time.perf_counter()
    fit = logreg.fit(x, labels, weights, args.classes, rec['l2'], rec['max_iterations'], rec['tolerance'], rec['history'])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    rec.update(fit_seconds=round(dt, 3), iterations=fit.iterations, evaluations=fit.evaluations, converged=fit.converged,
               seconds_per_evaluation=round(dt / fit.evaluations, 4), train_loss=fit.loss, grad_norm=fit.grad_norm,
               tflops_per_gradient_evaluation=round(4.0 * args.rows * args.dim * args.classes / 1e12, 3))
    print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
        json.dump(rec, open(args.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
