"""Time the input pipeline (simclr_amd/data.py) against the synthetic-input training step, on the GPU:

    python tools/input_pipeline_time.py [--batch 512] [--size 224] [--images 1536] [--steps 8] [--warmup 3] [--rounds 2]
                                        [--out profiles/input_pipeline_time.json]

A dataset of ImageNet-like sizes (sides 200 ... 500) is generated from a seed into a temporary directory and read back
through the page cache.  One ResNet-50 model and one step function (the bench.py headline configuration: fp32 storage,
f32_matmul=f16x3_3, no blur) are fed alternately from `run.synthetic_batches` (resident tensors, no augmentation) and from
`data.build_distributed_dataset`; every time window ends in a device synchronise.  Reported:

* step_ms: per round, synthetic and dataset-fed; `allowed_ms` = the synthetic mean + the stand-alone time of the three
  augmentation kernels for batch x 2 views (device events) + the spread of the synthetic rounds; `excess_ms` is what the
  dataset-fed step takes beyond that (<= 0: the feeding is hidden behind the step).  `dataset_batches_resident`: the same
  step on two dataset batches kept on the device and cycled like the synthetic pool -- the dataset's pixel statistics with
  no feeding and no augmentation, which separates what the data costs from what the feeding costs.
* loader: images/s of the iterator with no model behind it (gather by `--threads` host threads, one copy, augmentation),
  next to the step rates of f16x3_3 and of --compute_dtype=bf16.
* ragged_vs_canvas: bytes copied host-to-device per batch (from shapes) and front-end + colour kernel time of both forms on
  the same images.
"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def generate(data_dir, n, seed=0, lo=200, hi=500):
    """n images with sides U[lo, hi]: a coarse random colour field enlarged 8x plus noise (cheap; the content does not matter
    to the timing, the sizes do)."""
    from tools.make_array_dataset import write_split
    rng = np.random.default_rng(seed)

    class Images:
        def __len__(self):
            return n

        def __getitem__(self, i):
            r = np.random.default_rng([seed, i])
            h, w = int(r.integers(lo, hi + 1)), int(r.integers(lo, hi + 1))
            coarse = r.integers(0, 256, (h // 8 + 1, w // 8 + 1, 3), dtype=np.uint8)
            im = np.repeat(np.repeat(coarse, 8, 0), 8, 1)[:h, :w]
            return (im // 2 + r.integers(0, 128, (h, w, 3), dtype=np.uint8)).astype(np.uint8)
    write_split(data_dir, 'sizes', 'train', Images(), rng.integers(0, 1000, n), 1000)


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def event_ms(fn, n):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def build(batch, size, dtype, dev):
    from simclr_amd import model as model_lib
    from simclr_amd.flags import FLAGS
    from simclr_amd.resnet import RT
    from simclr_amd.run import make_single_step
    FLAGS.update(resnet_depth=50, image_size=size, train_batch_size=batch, compute_dtype=dtype, use_blur=False,
                 learning_rate=0.075, learning_rate_scaling='sqrt', f32_matmul='f16x3_3')
    RT.reset()
    RT.device = dev
    model = model_lib.Model(1000)
    opt = model_lib.build_optimizer(model_lib.WarmUpAndCosineDecay(FLAGS.learning_rate, 1281167))
    opt.iterations = 1000
    return make_single_step(model, opt, None)


def side_measurements(a, split, builder, dev, res):
    """ragged against canvas on the same images, and the loader alone; returns the stand-alone time of the three augmentation
    kernels for one batch (ms)."""
    from simclr_amd import data as data_lib
    from simclr_amd import data_util as du
    # ---- ragged against canvas, same images, same draws (and the stand-alone augmentation time the step is allowed)
    idx = data_lib.train_indices(a.images, 0, 0, a.batch)
    rows = split.index[idx]
    sizes = 3 * rows[:, 1] * rows[:, 2]
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    packed = np.concatenate([np.asarray(split.images[o:o + s]) for o, s in zip(rows[:, 0], sizes)])
    table = np.stack([offs, rows[:, 1], rows[:, 2]], 1).astype(np.int64)
    Hs, Ws = int(rows[:, 1].max()), int(rows[:, 2].max())
    canvas = np.zeros((a.batch, Hs, Ws, 3), np.uint8)
    for i in range(a.batch):
        h, w = rows[i, 1], rows[i, 2]
        canvas[i, :h, :w] = packed[offs[i]:offs[i] + sizes[i]].reshape(h, w, 3)
    params = torch.from_numpy(du.draw_train_params(a.batch, rows[:, 1], rows[:, 2], a.size, a.size, 1.0,
                                                   rng=np.random.default_rng(0))).to(dev)
    d_packed, d_canvas, d_table = torch.from_numpy(packed).to(dev), torch.from_numpy(canvas).to(dev), torch.from_numpy(table).to(dev)
    out_r = du.two_view_batch_ragged(d_packed, table, a.size, a.size, params=params, table_dev=d_table)
    out_c = du.two_view_batch(d_canvas, a.size, a.size, sizes=rows[:, 1:3], params=params)
    same = bool(torch.equal(out_r, out_c))
    rag_ms = event_ms(lambda: du.two_view_batch_ragged(d_packed, table, a.size, a.size, params=params, table_dev=d_table), 10)
    can_ms = event_ms(lambda: du.two_view_batch(d_canvas, a.size, a.size, sizes=rows[:, 1:3], params=params), 10)
    res['ragged_vs_canvas'] = dict(h2d_bytes_ragged=int(packed.nbytes + table.nbytes + params.numel() * 4), h2d_bytes_canvas=int(canvas.nbytes + params.numel() * 4),
                                   canvas_shape=list(canvas.shape), augment_three_kernels_ms_ragged=round(rag_ms, 3),
                                   augment_three_kernels_ms_canvas=round(can_ms, 3), outputs_bitwise_equal=same)
    del d_canvas, canvas, out_c, out_r
    torch.cuda.empty_cache()

    # ---- loader alone
    it = data_lib.build_distributed_dataset(builder, a.batch, True, None)
    for _ in range(2):
        next(it)
    n_load = max(6, a.steps)
    load_ms = timed(lambda: next(it), n_load)
    it.close()
    host = data_lib.DatasetIterator(split, 1000, a.batch, True, device=None, image_size=a.size, train_mode='pretrain')
    next(host)
    t0 = time.perf_counter()
    for _ in range(n_load):
        next(host)
    host_ms = (time.perf_counter() - t0) / n_load * 1e3
    host.close()
    res['loader'] = dict(ms_per_batch=round(load_ms, 2), images_per_s=round(a.batch / load_ms * 1e3, 1),
                         host_only_ms_per_batch=round(host_ms, 2), host_only_images_per_s=round(a.batch / host_ms * 1e3, 1),
                         note='gather by %d host threads from the page cache (memory-mapped), one copy, augmentation; no model' % a.threads)

    return rag_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--images', type=int, default=1536)
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--threads', type=int, default=2)
    ap.add_argument('--data_dir', default=None)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no_bf16', action='store_true')
    ap.add_argument('--feed', choices=['synthetic', 'dataset', 'resident'], default=None,
                    help='time `steps` steps of this feed only and stop (the run to put under rocprofv3 --kernel-trace --stats)')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this is a GPU measurement'
    from simclr_amd import data as data_lib
    from simclr_amd.flags import FLAGS
    from simclr_amd.run import synthetic_batches
    dev = torch.device('cuda', torch.cuda.current_device())
    tmp = None
    if a.data_dir is None:
        tmp = tempfile.TemporaryDirectory()
        a.data_dir = tmp.name
    t0 = time.perf_counter()
    if not os.path.exists(os.path.join(a.data_dir, 'sizes', 'info.json')):
        generate(a.data_dir, a.images)
    gen_s = time.perf_counter() - t0
    FLAGS.reset()
    FLAGS.update(dataset='sizes', data_dir=a.data_dir, input_threads=a.threads, train_split='train', image_size=a.size,
                 train_batch_size=a.batch)
    builder = data_lib.ArrayDatasetBuilder('sizes', a.data_dir)
    split = builder.split('train')
    np.asarray(split.images).sum()                                       # read once: the timed passes come from the page cache
    res = dict(config=dict(batch=a.batch, image_size=a.size, images=a.images, steps=a.steps, warmup=a.warmup, rounds=a.rounds,
                           input_threads=a.threads, prefetch_batches=FLAGS.prefetch_batches, model='ResNet-50 1x, f32 / f16x3_3, no blur',
                           dataset_bytes=int(split.images.shape[0]), dataset_generation_s=round(gen_s, 1)))

    rag_ms = 0.0 if a.feed else side_measurements(a, split, builder, dev, res)

    # ---- the step, fed alternately
    step = build(a.batch, a.size, 'f32', dev)
    syn = synthetic_batches(a.batch, a.size, 1000, dev)
    ds = data_lib.build_distributed_dataset(builder, a.batch, True, None)
    for _ in range(a.warmup):
        step(*next(syn))
    for _ in range(a.warmup):
        step(*next(ds))
    # two dataset batches kept resident and cycled like the synthetic pool: the dataset's pixel statistics without any feeding
    # (some kernels' time depends on the data, e.g. on how sparse the ReLU masks are)
    pool = [(f.clone(), {'labels': l['labels'].clone()}) for f, l in (next(ds), next(ds))]
    cycle = {'i': 0}

    def resident():
        cycle['i'] += 1
        return pool[cycle['i'] % 2]
    for _ in range(a.warmup):
        step(*resident())
    if a.feed:                                                           # one feed only: the run to put under a kernel trace
        src = dict(synthetic=lambda: next(syn), dataset=lambda: next(ds), resident=resident)[a.feed]
        ms = timed(lambda: step(*src()), a.steps)
        ds.close()
        print(json.dumps(dict(feed=a.feed, steps=a.steps, ms_per_step=round(ms, 2))), flush=True)
        return
    rounds = dict(synthetic=[], dataset=[], resident=[])
    for _ in range(a.rounds):
        rounds['synthetic'].append(timed(lambda: step(*next(syn)), a.steps))
        rounds['dataset'].append(timed(lambda: step(*next(ds)), a.steps))
        rounds['resident'].append(timed(lambda: step(*resident()), a.steps))
    ds.close()
    del pool
    s_mean, d_mean = float(np.mean(rounds['synthetic'])), float(np.mean(rounds['dataset']))
    spread = float(max(rounds['synthetic']) - min(rounds['synthetic']))
    allowed = s_mean + rag_ms + spread
    res['step_ms'] = dict(synthetic_rounds=[round(x, 2) for x in rounds['synthetic']], dataset_rounds=[round(x, 2) for x in rounds['dataset']],
                          synthetic_mean=round(s_mean, 2), dataset_mean=round(d_mean, 2), synthetic_spread=round(spread, 2),
                          augment_three_kernels_ms=round(rag_ms, 3), allowed_ms=round(allowed, 2), excess_ms=round(d_mean - allowed, 2),
                          feeding_hidden=bool(d_mean <= allowed),
                          dataset_batches_resident_rounds=[round(x, 2) for x in rounds['resident']],
                          dataset_batches_resident_mean=round(float(np.mean(rounds['resident'])), 2),
                          fed_minus_resident_ms=round(d_mean - float(np.mean(rounds['resident'])), 2))
    res['step_rate'] = dict(f16x3_3_images_per_s=round(a.batch / s_mean * 1e3, 1))
    if not a.no_bf16:
        del step
        torch.cuda.empty_cache()
        step = build(a.batch, a.size, 'bf16', dev)
        for _ in range(a.warmup):
            step(*next(syn))
        b_ms = timed(lambda: step(*next(syn)), a.steps)
        res['step_rate']['bf16_images_per_s'] = round(a.batch / b_ms * 1e3, 1)
        res['step_rate']['bf16_ms'] = round(b_ms, 2)
    lr = res['loader']['images_per_s']
    res['loader']['limits'] = [m for m in ('f16x3_3', 'bf16') if res['step_rate'].get(m + '_images_per_s', 0) > lr]
    FLAGS.reset()
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')
    if tmp is not None:
        tmp.cleanup()


if __name__ == '__main__':
    main()
