"""Data pipeline -- mirror of the reference's tf2/data.py on an on-disk array format.

`<data_dir>/<dataset>/` holds (tools/make_array_dataset.py writes it):

* `info.json`: `{"format": "simclr-arrays-1", "num_classes": K, "splits": {"train": N, "validation": M, ...}}`
* `<split>.index.npy`: int64 `[n, 4]` = (byte offset, height, width, label) per image
* `<split>.images.u8`: raw RGB uint8, HWC, tightly packed, images of any size back to back

`ArrayDatasetBuilder` stands in for the tfds builder (`builder.info.splits[s].num_examples`,
`builder.info.features['label'].num_classes`, tf2/run.py:473-475); `build_distributed_dataset` has the signature of
tf2/data.py:95 and returns an iterator of `(features, {'labels': one_hot})` on the device.

Order of the examples.  The training stream is the concatenation of per-epoch permutations
`perm(data_seed, epoch)` of the split; global batch k takes stream positions [k*B, (k+1)*B), replica r of R takes
[k*B + r*b, k*B + (r+1)*b) with b = B // R (tf2/data.py:45); batches may span an epoch boundary, as
`shuffle().repeat().batch(drop_remainder=True)` does.  The augmentation draws of a batch come from
`np.random.default_rng([data_seed, step, replica])` through data_util.draw_train_params.  The batch of step s therefore
depends on (data_seed, s, r, R, flags) only, never on history: a resumed run continues the uninterrupted run's data.
This is a FULL permutation per epoch, not the reference's bounded shuffle buffer (`shuffle(batch_size * 10 | 50)`), and
the draws come from numpy, not tf.random: parity of order and draws with the reference is distributional (as
data_util.py states for the draws); the arithmetic given the draws is exact.

Eval: global batch k covers split positions [k*E, (k+1)*E), split over replicas the same way; positions past the end
are padded with example 0 and carry weight 0 (`labels['mask']`), so every replica runs the same number of steps and the
weighted metrics count each example once.

Feeding.  `input_threads` host threads gather the records of the next `prefetch_batches` batches into pinned buffers:
one buffer per batch holding its table, labels, weights, parameter table and the packed image bytes -- no padding to a
canvas.  One host-to-device copy per batch runs on a copy stream; an event orders it before the augmentation kernels on
the compute stream, and a buffer is refilled only after the events of its previous use.  No device synchronise is added
to the step.  `--cache_dataset` holds the split in host memory, otherwise the image file is memory-mapped.
"""
import collections
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import data_util, ops
from .flags import FLAGS, aug_plan, local_crop_flags

FORMAT = 'simclr-arrays-1'
LAYOUT = ('<data_dir>/<dataset>/info.json {"format": "%s", "num_classes": K, "splits": {"train": N, ...}}, '
          '<split>.index.npy (int64 [n, 4]: byte offset, height, width, label) and <split>.images.u8 (raw RGB uint8, HWC, '
          'back to back); tools/make_array_dataset.py writes it from arrays or from an image folder' % FORMAT)


class DatasetError(ValueError):
    pass


SplitInfo = collections.namedtuple('SplitInfo', 'num_examples')
LabelInfo = collections.namedtuple('LabelInfo', 'num_classes')
DatasetInfo = collections.namedtuple('DatasetInfo', 'splits features')
Split = collections.namedtuple('Split', 'index images')          # index int64 [n, 4]; images uint8 [nbytes]


class ArrayDatasetBuilder:
    """The builder of tf2/run.py:471-475 for the array format: `info.splits[split].num_examples`,
    `info.features['label'].num_classes`.  Opening validates the files against each other and names the offending file."""

    def __init__(self, name, data_dir):
        if not data_dir:
            raise DatasetError('--dataset=%s needs --data_dir; expected layout: %s' % (name, LAYOUT))
        self.name = name
        self.dir = os.path.join(data_dir, name)
        info_path = os.path.join(self.dir, 'info.json')
        if not os.path.isfile(info_path):
            raise DatasetError('%s not found; expected layout: %s' % (info_path, LAYOUT))
        try:
            with open(info_path) as f:
                info = json.load(f)
        except ValueError as e:
            raise DatasetError('%s is not valid JSON: %s' % (info_path, e))
        if not isinstance(info, dict) or info.get('format') != FORMAT:
            raise DatasetError('%s: "format" must be "%s"' % (info_path, FORMAT))
        k, splits = info.get('num_classes'), info.get('splits')
        if not isinstance(k, int) or k <= 0 or not isinstance(splits, dict) or not splits:
            raise DatasetError('%s: needs a positive integer "num_classes" and a non-empty "splits" object' % info_path)
        self._index = {}
        for split, n in splits.items():
            self._index[split] = self._check_split(split, n, k, info_path)
        self.info = DatasetInfo({s: SplitInfo(int(n)) for s, n in splits.items()}, {'label': LabelInfo(k)})
        self._images = {}

    def _paths(self, split):
        return os.path.join(self.dir, split + '.index.npy'), os.path.join(self.dir, split + '.images.u8')

    def _check_split(self, split, n, num_classes, info_path):
        ipath, dpath = self._paths(split)
        for p in (ipath, dpath):
            if not os.path.isfile(p):
                raise DatasetError('%s not found (split %r of %s)' % (p, split, info_path))
        try:
            idx = np.load(ipath, allow_pickle=False)
        except Exception as e:
            raise DatasetError('%s is not a readable .npy array: %s' % (ipath, e))
        if idx.dtype != np.int64 or idx.ndim != 2 or idx.shape[1] != 4:
            raise DatasetError('%s: expected int64 [n, 4] (byte offset, height, width, label), got %s %s'
                               % (ipath, idx.dtype, idx.shape))
        if not isinstance(n, int) or idx.shape[0] != n or n <= 0:
            raise DatasetError('%s has %d rows but %s says split %r has %r examples' % (ipath, idx.shape[0], info_path, split, n))
        off, h, w, lab = idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]
        if (h <= 0).any() or (w <= 0).any() or (h > 1 << 20).any() or (w > 1 << 20).any():
            raise DatasetError('%s: row %d has a non-positive or oversized height / width'
                               % (ipath, int(np.argmax((h <= 0) | (w <= 0) | (h > 1 << 20) | (w > 1 << 20)))))
        size = os.path.getsize(dpath)
        bad = (off < 0) | (off > size) | (off + 3 * h * w > size)
        if bad.any():
            i = int(np.argmax(bad))
            raise DatasetError('%s: row %d (offset %d, %d x %d) lies outside %s (%d bytes)' % (ipath, i, off[i], h[i], w[i], dpath, size))
        bad = (lab < 0) | (lab >= num_classes)
        if bad.any():
            i = int(np.argmax(bad))
            raise DatasetError('%s: row %d has label %d, but %s says num_classes = %d' % (ipath, i, lab[i], info_path, num_classes))
        return idx

    def split(self, split, cache=False):
        """Split(index, images): images is a read-only memory map of the image file, or (cache=True, --cache_dataset) an
        array in host memory."""
        if split not in self._index:
            raise DatasetError('split %r is not in %s (splits: %s)' % (split, os.path.join(self.dir, 'info.json'),
                                                                     ', '.join(sorted(self._index))))
        key = (split, bool(cache))
        if key not in self._images:
            dpath = self._paths(split)[1]
            self._images[key] = np.fromfile(dpath, dtype=np.uint8) if cache else np.memmap(dpath, dtype=np.uint8, mode='r')
        return Split(self._index[split], self._images[key])


# --------------------------------------------------------------------------- which examples a batch holds (host arithmetic)
def epoch_permutation(data_seed, epoch, n):
    return np.random.default_rng([int(data_seed), int(epoch)]).permutation(n)


def train_indices(n, data_seed, step, global_batch, replica=0, num_replicas=1):
    """Examples of replica `replica`'s share of global training batch `step`: stream positions
    [step*B + r*b, step*B + (r+1)*b) of the concatenated per-epoch permutations."""
    b = global_batch // num_replicas
    lo = step * global_batch + replica * b
    pos = np.arange(lo, lo + b, dtype=np.int64)
    out = np.empty(b, np.int64)
    for e in np.unique(pos // n):
        m = pos // n == e
        out[m] = epoch_permutation(data_seed, e, n)[pos[m] % n]
    return out


def eval_num_steps(m, global_batch):
    return -(-m // global_batch)


def eval_indices(m, step, global_batch, replica=0, num_replicas=1):
    """(indices, weights) of replica `replica`'s share of global eval batch `step`: split positions
    [step*E + r*b, step*E + (r+1)*b); positions past the end are example 0 with weight 0."""
    b = global_batch // num_replicas
    lo = step * global_batch + replica * b
    pos = np.arange(lo, lo + b, dtype=np.int64)
    w = (pos < m).astype(np.float32)
    return np.where(pos < m, pos, 0), w


def _align(x, a=16):
    return (x + a - 1) // a * a


HostBatch = collections.namedtuple('HostBatch', 'step indices labels weights table params nbytes local_params', defaults=(None,))


class DatasetIterator:
    """Iterator over the batches of one replica.  `device=None`: host only -- yields HostBatch records (what the order and
    history tests read); with a device: `(features, {'labels': one_hot})` (+ `'mask'`, the per-sample weights, for eval)."""

    def __init__(self, split, num_classes, global_batch, is_training, replica=0, num_replicas=1, device=None,
                 start_step=0, image_size=None, train_mode=None, color_jitter_strength=None, data_seed=None,
                 input_threads=None, prefetch_batches=None, local_crops=None):
        self.split, self.num_classes = split, num_classes
        self.n = split.index.shape[0]
        self.B, self.R, self.r = int(global_batch), int(num_replicas), int(replica)
        if self.B % self.R or self.B <= 0:
            raise ValueError('batch size %d is not a positive multiple of the %d replicas' % (self.B, self.R))
        self.b = self.B // self.R
        self.is_training = bool(is_training)
        self.size = FLAGS.image_size if image_size is None else image_size
        mode = FLAGS.train_mode if train_mode is None else train_mode
        self.pretrain = self.is_training and mode == 'pretrain'
        # get_preprocess_fn (tf2/data.py:101-115): jitter strength 0 outside pretraining, no test crop for image_size <= 32
        s = FLAGS.color_jitter_strength if color_jitter_strength is None else color_jitter_strength
        self.strength = float(s) if self.pretrain else 0.
        # the jitter components of the augmentation recipe (flags.aug_plan): the global and the local views draw from the same ranges
        self.jitter_components = aug_plan().jitter_components
        self.test_crop = self.size > 32
        self.views = 2 if self.pretrain else 1
        # multi-crop: L local views per image at their own size, area range and generator (pretraining with --contrastive_loss=swav or
        # dino, each under its own four flags: flags.local_crop_flags)
        flag_crops, local_size, lo, hi = local_crop_flags()
        if local_crops is None:
            local_crops = flag_crops if self.pretrain else 0
        self.local_crops = int(local_crops) if self.pretrain else 0
        self.local_size = local_size
        self.local_scale = (lo, hi)
        self.seed = int(FLAGS.data_seed if data_seed is None else data_seed)
        self.threads = max(1, int(FLAGS.input_threads if input_threads is None else input_threads))
        self.depth = max(1, int(FLAGS.prefetch_batches if prefetch_batches is None else prefetch_batches))
        self.device = device
        self.step = int(start_step)
        self.num_steps = None if self.is_training else eval_num_steps(self.n, self.B)
        # section offsets of a staged batch (bytes): table | labels | weights | params | image bytes
        self._o_lab = _align(24 * self.b)
        self._o_w = self._o_lab + _align(8 * self.b)
        self._o_par = self._o_w + _align(4 * self.b)
        # (the local parameters have a section of their own behind the global ones: empty without local crops)
        self._o_lpar = self._o_par + _align(4 * 16 * self.views * self.b)
        self._o_img = self._o_lpar + _align(4 * 16 * self.local_crops * self.b)
        self._pool = ThreadPoolExecutor(self.threads, thread_name_prefix='simclr-input')
        self._slots = [dict(host=None, dev=None, copied=None, consumed=None) for _ in range(self.depth + 1)]
        self._free = collections.deque(range(len(self._slots)))
        self._pending = collections.OrderedDict()          # step -> (future, slot)
        self._copy_stream = torch.cuda.Stream(device) if device is not None else None
        self._next_submit = self.step

    # ---- host side
    def plan(self, step):
        """(indices, weights, params) of this replica's batch `step` -- a function of (data_seed, step, replica, R, flags)."""
        if self.is_training:
            idx = train_indices(self.n, self.seed, step, self.B, self.r, self.R)
            w = np.ones(self.b, np.float32)
            rng = np.random.default_rng([self.seed, int(step), self.r])
            hw = self.split.index[idx, 1:3]
            params = data_util.draw_train_params(self.b, hw[:, 0], hw[:, 1], self.size, self.size, self.strength,
                                                 views=self.views, rng=rng, jitter_components=self.jitter_components)
        else:
            idx, w = eval_indices(self.n, step, self.B, self.r, self.R)
            hw = self.split.index[idx, 1:3]
            params = data_util.eval_params(hw[:, 0], hw[:, 1], self.size, self.size, crop=self.test_crop)
        return idx, w, params

    def local_plan(self, step, idx=None):
        """The parameters [b, L, 16] of the L local views of batch `step`, from a generator of their own -- a function of (data_seed,
        step, replica, 1): the global views of a run with local crops are bitwise those of a run without."""
        if idx is None:
            idx = train_indices(self.n, self.seed, step, self.B, self.r, self.R)
        rng = np.random.default_rng([self.seed, int(step), self.r, 1])
        hw = self.split.index[idx, 1:3]
        return data_util.draw_local_params(self.b, hw[:, 0], hw[:, 1], self.local_size, self.local_crops, self.local_scale[0],
                                           self.local_scale[1], self.strength, rng=rng, jitter_components=self.jitter_components)

    def _host_buffer(self, slot, nbytes):
        buf = slot['host']
        if buf is None or buf.numel() < nbytes:
            cap = _align(int(nbytes * 1.25), 4096)
            buf = torch.empty(cap, dtype=torch.uint8, pin_memory=self.device is not None)
            slot['host'] = buf
        return buf

    def _fill(self, step, slot_id):
        """Worker thread: gather the records of batch `step` into the slot's (pinned) buffer."""
        slot = self._slots[slot_id]
        if slot['copied'] is not None:
            slot['copied'].synchronize()           # the previous copy out of this buffer is done (an event, not the device)
        idx, w, params = self.plan(step)
        rows = self.split.index[idx]
        sizes = 3 * rows[:, 1] * rows[:, 2]
        offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        img_bytes = int(sizes.sum())
        nbytes = self._o_img + img_bytes
        buf = self._host_buffer(slot, nbytes).numpy()
        table = np.stack([offs, rows[:, 1], rows[:, 2]], 1)
        buf[0:24 * self.b].view(np.int64)[:] = table.reshape(-1)
        buf[self._o_lab:self._o_lab + 8 * self.b].view(np.int64)[:] = rows[:, 3]
        buf[self._o_w:self._o_w + 4 * self.b].view(np.float32)[:] = w
        buf[self._o_par:self._o_par + params.size * 4].view(np.float32)[:] = params.reshape(-1)
        local_params = None
        if self.local_crops:
            local_params = self.local_plan(step, idx)
            buf[self._o_lpar:self._o_lpar + local_params.size * 4].view(np.float32)[:] = local_params.reshape(-1)
        images, dst = self.split.images, buf[self._o_img:]
        for o, src, sz in zip(offs, rows[:, 0], sizes):
            dst[o:o + sz] = images[src:src + sz]
        return HostBatch(step, idx, rows[:, 3].copy(), w, table, params, nbytes, local_params)

    def _submit_ahead(self):
        while self._free and self._next_submit < self.step + self.depth + 1 and \
                (self.num_steps is None or self._next_submit < self.num_steps):
            s = self._free.popleft()
            self._pending[self._next_submit] = (self._pool.submit(self._fill, self._next_submit, s), s)
            self._next_submit += 1

    def __iter__(self):
        return self

    def __next__(self):
        if self.num_steps is not None and self.step >= self.num_steps:
            self.close()
            raise StopIteration
        self._submit_ahead()
        fut, slot_id = self._pending.pop(self.step)
        hb = fut.result()
        self.step += 1
        if self.device is None:
            self._free.append(slot_id)
            self._submit_ahead()
            return hb
        out = self._to_device(hb, slot_id)
        self._free.append(slot_id)                 # its refill waits for `copied`, its next copy for `consumed`
        self._submit_ahead()
        return out

    # ---- device side
    def _to_device(self, hb, slot_id):
        slot = self._slots[slot_id]
        dev = self.device
        host = slot['host']
        if slot['dev'] is None or slot['dev'].numel() < host.numel():
            slot['dev'] = torch.empty(host.numel(), dtype=torch.uint8, device=dev)
            slot['copied'], slot['consumed'] = torch.cuda.Event(), torch.cuda.Event()
            # the allocator may hand out memory whose last user is still queued on the compute stream: the copy waits for it
            slot['consumed'].record(torch.cuda.current_stream(dev))
        compute = torch.cuda.current_stream(dev)
        with torch.cuda.stream(self._copy_stream):
            self._copy_stream.wait_event(slot['consumed'])         # the kernels that read this device buffer last are done
            slot['dev'][:hb.nbytes].copy_(host[:hb.nbytes], non_blocking=True)
            slot['copied'].record(self._copy_stream)
        compute.wait_event(slot['copied'])
        d, b = slot['dev'], self.b
        table_dev = d[0:24 * b].view(torch.int64)
        labels = d[self._o_lab:self._o_lab + 8 * b].view(torch.int64)
        params = d[self._o_par:self._o_par + 64 * self.views * b].view(torch.float32).view(b, self.views, 16)
        packed = d[self._o_img:hb.nbytes]
        features = ops.augment_views_ragged(packed, hb.table, params, self.size, self.size, table_dev=table_dev)
        if self.local_crops:
            # one more launch at the local size on the same packed records
            lparams = d[self._o_lpar:self._o_lpar + 64 * self.local_crops * b].view(torch.float32).view(b, self.local_crops, 16)
            features = (features, ops.augment_views_ragged(packed, hb.table, lparams, self.local_size, self.local_size,
                                                           table_dev=table_dev))
        lab = {'labels': torch.nn.functional.one_hot(labels, self.num_classes).float()}
        if not self.is_training:
            lab['mask'] = d[self._o_w:self._o_w + 4 * b].view(torch.float32).clone()
        slot['consumed'].record(compute)
        return features, lab

    def close(self):
        for fut, _ in self._pending.values():
            fut.cancel()
        self._pool.shutdown(wait=True)
        self._pending.clear()

    def __del__(self):
        try:
            self._pool.shutdown(wait=False)
        except Exception:
            pass


def build_distributed_dataset(builder, batch_size, is_training, strategy, topology=None, start_step=0):
    """tf2/data.py:95.  `batch_size` is the GLOBAL batch; this process gets replica `strategy.rank`'s share on its current
    device.  `start_step`: the global step the training stream starts at (a resumed run passes the restored step)."""
    from .comm import num_replicas, replica_id
    del topology                                            # TPU only
    R = num_replicas(strategy)
    r = replica_id(strategy)
    split = builder.split(FLAGS.train_split if is_training else FLAGS.eval_split, cache=FLAGS.cache_dataset)
    device = torch.device('cuda', torch.cuda.current_device())
    return DatasetIterator(split, builder.info.features['label'].num_classes, batch_size, is_training, replica=r,
                           num_replicas=R, device=device, start_step=start_step if is_training else 0)
