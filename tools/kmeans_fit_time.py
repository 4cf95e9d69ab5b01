"""Wall time of the k-means clustering evaluation's fit (simclr_amd/kmeans.py) at ImageNet size:
    python tools/kmeans_fit_time.py [--rows 1281167] [--dim 2048] [--k 1000] [--out FILE]
One fit with the default flags on random unit rows (the kernels cost what they cost on real features; the iteration count on random
rows does not transfer to real features), then one assignment pass and one update pass over all slabs timed on their own.  Prints and
writes one JSON record."""
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
    ap.add_argument('--k', type=int, default=1000)
    ap.add_argument('--out', default=None, help='also write the record to this file')
    args = ap.parse_args()
    from simclr_amd import kmeans, ops
    from simclr_amd.flags import FLAGS
    FLAGS.reset()
    dev = torch.device('cuda', torch.cuda.current_device())
    rec = dict(rows=args.rows, dim=args.dim, k=args.k, restarts=FLAGS.kmeans_restarts, max_iterations=FLAGS.kmeans_max_iterations,
               tolerance=FLAGS.kmeans_tolerance, seed=FLAGS.kmeans_seed)
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.empty(args.rows, args.dim, device=dev)
    for o, e in kmeans._slabs(args.rows):
        x[o:e] = torch.nn.functional.normalize(torch.randn(e - o, args.dim, device=dev, generator=g), dim=1)
    weights = torch.ones(args.rows, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fit = kmeans.fit(x, weights, args.k, rec['seed'], rec['restarts'], rec['max_iterations'], rec['tolerance'])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    rec.update(fit_seconds=round(dt, 3), iterations=fit.iterations, converged=fit.converged, inertia=fit.inertia,
               empty_clusters=fit.empty_clusters, seconds_per_iteration=round(dt / fit.iterations, 4),
               tflops_per_assignment_pass=round(2.0 * args.rows * args.dim * args.k / 1e12, 3))
    slabs = kmeans._slabs(args.rows)
    ws = kmeans._workspace(slabs[0][1] - slabs[0][0], slabs[-1][1] - slabs[-1][0], args.dim, args.k, dev)
    assign = torch.full((args.rows,), -1, device=dev, dtype=torch.int32)
    best = torch.empty(args.rows, device=dev)
    sums = torch.zeros(args.k, args.dim, device=dev, dtype=torch.float64)
    wsum = torch.zeros(args.k, device=dev, dtype=torch.float64)

    def assign_pass():
        for o, e in slabs:
            ops.kmeans_assign(x[o:e], fit.centroids, weights[o:e], assign[o:e], best[o:e], ws)

    def update_pass():
        for i, (o, e) in enumerate(slabs):
            ops.kmeans_update(x[o:e], weights[o:e], assign[o:e], args.k, sums, wsum, accumulate=i > 0)

    for name, fn in (('assign', assign_pass), ('update', update_pass)):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        ts.sort()
        rec[name + '_pass_seconds'] = round(ts[1], 4)
        rec[name + '_pass_min_max_seconds'] = [round(ts[0], 4), round(ts[-1], 4)]
    rec['assign_pass_tfs'] = round(rec['tflops_per_assignment_pass'] / rec['assign_pass_seconds'], 1)
    rec['update_pass_read_gbs'] = round(4.0 * args.rows * args.dim / rec['update_pass_seconds'] / 1e9, 1)
    rec['note'] = 'random unit rows: the iteration count does not transfer to real features'
    print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
        json.dump(rec, open(args.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
