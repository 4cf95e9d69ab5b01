"""Time simclr_batch_blur_solarize next to simclr_batch_blur on the same inputs and selectors:
    python tools/aug_recipe_microbench.py [--batch 512] [--size 224] [--views 2] [--reps 5] [--launches 10] [--out FILE]
Three variants -- the old entry, the new entry with every coin 0 and with every coin 1 -- alternate inside each of `reps` repetitions; a
repetition times `launches` back-to-back calls with device events.  Prints (and writes to --out) one JSON object: per variant the median
of the repetitions with [min, max], and whether both new medians lie inside the old entry's own [min, max]."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--views', type=int, default=2)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--launches', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()

    from simclr_amd import _lib, data_util, ops
    L = _lib.lib()
    dev = torch.device('cuda', torch.cuda.current_device())
    g = torch.Generator().manual_seed(0)
    b, H, k = a.batch, a.size, a.views
    x = torch.rand(b, H, H, 3 * k, generator=g).to(dev)
    tmp, out = torch.empty_like(x), torch.empty_like(x)
    filt = data_util.gaussian_filter(H // 10, torch.linspace(1.0, 1.5, k).to(dev)).contiguous()
    K = filt.shape[1]
    sel = (torch.rand(k, b, generator=g) < 0.5).float().to(dev)
    zeros, ones = torch.zeros(k, b, device=dev), torch.ones(k, b, device=dev)
    p = [ops._p(t) for t in (x, tmp, out, filt, sel)]
    variants = {
        'batch_blur': lambda: L.batch_blur(*p, b, H, H, k, K, ops._s()),
        'batch_blur_solarize coins 0': lambda: L.batch_blur_solarize(*p, ops._p(zeros), 0.5, b, H, H, k, K, ops._s()),
        'batch_blur_solarize coins 1': lambda: L.batch_blur_solarize(*p, ops._p(ones), 0.5, b, H, H, k, K, ops._s()),
    }
    times = {n: [] for n in variants}
    for fn in variants.values():                  # warm-up
        fn()
    torch.cuda.synchronize()
    for _ in range(a.reps):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.launches)
    summary = {n: dict(median_ms=round(statistics.median(t), 4), min_ms=round(min(t), 4), max_ms=round(max(t), 4)) for n, t in times.items()}
    old = summary['batch_blur']
    inside = all(old['min_ms'] <= summary[n]['median_ms'] <= old['max_ms'] for n in summary if n != 'batch_blur')
    res = dict(shape=dict(b=b, H=H, W=H, k=k, K=K, selected_share=round(float(sel.mean()), 4)), reps=a.reps, launches_per_rep=a.launches,
               ms_per_call=summary,
               expectation="both new medians inside the old entry's own [min, max]: one compare and one select per element of a "
                           'memory-bound pass',
               new_medians_inside_old_min_max=inside)
    line = json.dumps(res, indent=1)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
