"""Seeded datasets in the array format of simclr_amd/data.py, generated into a temporary directory (nothing is committed)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def wave_image(rng, h, w):
    """uint8 [h, w, 3]: smooth waves plus a little noise (as tests/gpu_checks.py::check_augment), so that bicubic overshoot
    and every HSV branch are exercised."""
    yy, xx = np.mgrid[0:h, 0:w]
    a, c = rng.uniform(2.0, 9.0, 2)
    ph = rng.uniform(0, 6.28, 3)
    amp = rng.uniform(0.3, 1.0, 3) * rng.choice([-1.0, 1.0], 3)
    base = rng.uniform(60, 190, 3)
    wave = base + 110 * np.sin(yy[..., None] / a + xx[..., None] / c + ph) * amp
    noise = rng.integers(0, 256, (h, w, 3))
    return np.clip(0.8 * wave + 0.2 * noise, 0, 255).astype(np.uint8)


def mixed_sizes(rng, n, lo=8, hi=72):
    return [(int(rng.integers(lo, hi + 1)), int(rng.integers(lo, hi + 1))) for _ in range(n)]


def make_dataset(data_dir, name='waves', splits=(('train', 103), ('validation', 37)), num_classes=10, seed=0, sizes=None,
                 lo=8, hi=72):
    """Writes the dataset with tools/make_array_dataset.py::write_split.  Returns {split: (list of images, labels)}."""
    from tools.make_array_dataset import write_split
    rng = np.random.default_rng(seed)
    out = {}
    for split, n in splits:
        sz = sizes[split] if sizes and split in sizes else mixed_sizes(rng, n, lo, hi)
        images = [wave_image(rng, h, w) for h, w in sz]
        labels = rng.integers(0, num_classes, n).astype(np.int64)
        labels[:num_classes] = np.arange(num_classes)[:n]            # every class occurs: num_classes is what info.json gets
        write_split(data_dir, name, split, images, labels, num_classes)
        out[split] = (images, labels)
    return out
