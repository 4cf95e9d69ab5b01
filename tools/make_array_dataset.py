"""Write a dataset in the array format simclr_amd/data.py reads (`<out>/<name>/info.json`, `<split>.index.npy`,
`<split>.images.u8`):

    # from arrays: an .npz with `images` [n,H,W,3] uint8 and `labels` [n] (or an images .npy + a labels .npy)
    python tools/make_array_dataset.py --out DATA_DIR --name cifar10 --split train --arrays train.npz
    python tools/make_array_dataset.py --out DATA_DIR --name cifar10 --split validation --images x.npy --labels y.npy
    # from an image folder root/<class>/<file> (needs PIL; grey and RGBA are converted to RGB)
    python tools/make_array_dataset.py --out DATA_DIR --name flowers --split train --folder root [--max_side 500]

Each call writes one split and adds it to info.json; `num_classes` is the largest seen over the splits unless
--num_classes is given.  Decoding happens here, once: the training loop reads raw bytes.
"""
import argparse
import json
import os
import sys

import numpy as np

FORMAT = 'simclr-arrays-1'


def write_split(out_dir, name, split, images, labels, num_classes=None):
    """images: a sequence of uint8 [h, w, 3] arrays (any sizes) or one [n, H, W, 3] array; labels: n integers.
    Writes the two files of `split` and updates info.json.  Returns the dataset directory."""
    d = os.path.join(out_dir, name)
    os.makedirs(d, exist_ok=True)
    labels = np.asarray(labels).reshape(-1)
    if not np.issubdtype(labels.dtype, np.integer):
        raise ValueError('labels must be integers, got %s' % labels.dtype)
    n = len(images)
    if n == 0 or labels.shape[0] != n:
        raise ValueError('%d images but %d labels' % (n, labels.shape[0]))
    if labels.min() < 0:
        raise ValueError('negative label')
    index = np.zeros((n, 4), np.int64)
    off = 0
    with open(os.path.join(d, split + '.images.u8'), 'wb') as f:
        for i in range(n):
            im = np.asarray(images[i])
            if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3 or im.shape[0] == 0 or im.shape[1] == 0:
                raise ValueError('image %d: expected uint8 [h, w, 3], got %s %s' % (i, im.dtype, im.shape))
            f.write(np.ascontiguousarray(im).tobytes())
            index[i] = (off, im.shape[0], im.shape[1], labels[i])
            off += im.size
    np.save(os.path.join(d, split + '.index.npy'), index)
    info_path = os.path.join(d, 'info.json')
    info = {'format': FORMAT, 'num_classes': 0, 'splits': {}}
    if os.path.isfile(info_path):
        with open(info_path) as f:
            info = json.load(f)
        if info.get('format') != FORMAT:
            raise ValueError('%s has another format' % info_path)
    info['splits'][split] = n
    k = int(labels.max()) + 1
    info['num_classes'] = int(num_classes) if num_classes else max(int(info.get('num_classes', 0)), k)
    if info['num_classes'] < k:
        raise ValueError('label %d does not fit num_classes = %d' % (k - 1, info['num_classes']))
    with open(info_path, 'w') as f:
        json.dump(info, f, indent=1, sort_keys=True)
    return d


def load_folder(root, max_side=0):
    """root/<class>/<file> -> (list of uint8 [h,w,3], labels); classes are numbered in sorted order."""
    try:
        from PIL import Image
    except ImportError:
        raise SystemExit('--folder needs PIL (Pillow) to decode image files and it is not importable here; '
                         'decode elsewhere and pass the arrays with --arrays / --images --labels')
    classes = sorted(c for c in os.listdir(root) if os.path.isdir(os.path.join(root, c)))
    if not classes:
        raise SystemExit('%s has no class directories (expected root/<class>/<file>)' % root)
    images, labels = [], []
    for k, c in enumerate(classes):
        for fn in sorted(os.listdir(os.path.join(root, c))):
            path = os.path.join(root, c, fn)
            if not os.path.isfile(path):
                continue
            with Image.open(path) as im:
                im = im.convert('RGB')                       # grey, palette and RGBA alike
                if max_side and max(im.size) > max_side:
                    s = max_side / float(max(im.size))
                    im = im.resize((max(1, round(im.size[0] * s)), max(1, round(im.size[1] * s))), Image.BICUBIC)
                images.append(np.asarray(im, dtype=np.uint8))
            labels.append(k)
    return images, np.asarray(labels, np.int64), classes


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', required=True, help='the --data_dir of training')
    ap.add_argument('--name', required=True, help='the --dataset of training')
    ap.add_argument('--split', required=True, help="'train', 'validation', ...")
    ap.add_argument('--arrays', help='.npz with `images` [n,H,W,3] uint8 and `labels` [n]')
    ap.add_argument('--images', help='.npy [n,H,W,3] uint8 (with --labels)')
    ap.add_argument('--labels', help='.npy [n] integers (with --images)')
    ap.add_argument('--folder', help='image folder root/<class>/<file> (needs PIL)')
    ap.add_argument('--max_side', type=int, default=0, help='--folder: shrink images whose longer side exceeds this')
    ap.add_argument('--num_classes', type=int, default=0)
    a = ap.parse_args(argv)
    if sum(bool(x) for x in (a.arrays, a.images, a.folder)) != 1 or bool(a.images) != bool(a.labels):
        ap.error('give exactly one of --arrays, --images with --labels, --folder')
    if a.folder:
        images, labels, classes = load_folder(a.folder, a.max_side)
        num_classes = a.num_classes or len(classes)
    else:
        if a.arrays:
            z = np.load(a.arrays, allow_pickle=False)
            images, labels = z['images'], z['labels']
        else:
            images, labels = np.load(a.images, allow_pickle=False), np.load(a.labels, allow_pickle=False)
        if images.dtype != np.uint8 or images.ndim != 4 or images.shape[3] != 3:
            ap.error('images must be uint8 [n,H,W,3], got %s %s' % (images.dtype, images.shape))
        num_classes = a.num_classes
    d = write_split(a.out, a.name, a.split, images, labels, num_classes)
    print('wrote split %r (%d images) to %s' % (a.split, len(images), d))


if __name__ == '__main__':
    main(sys.argv[1:])
