"""CPU tests of the input pipeline (simclr_amd/data.py) and of the converter (tools/make_array_dataset.py): format round
trip, order of the training and eval streams, independence of history, file validation, the driver's error message."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from simclr_amd import data as data_lib
from simclr_amd import metrics
from simclr_amd.flags import FLAGS
from tests.data_fixtures import ROOT, make_dataset, wave_image


@pytest.fixture(autouse=True)
def _flags():
    FLAGS.reset()
    yield
    FLAGS.reset()


def _host_iter(split, batch, training, r=0, R=1, **kw):
    kw.setdefault('image_size', 32)
    kw.setdefault('train_mode', 'pretrain')
    return data_lib.DatasetIterator(split, 10, batch, training, replica=r, num_replicas=R, device=None, **kw)


# ------------------------------------------------------------------ 1. converter -> builder round trip
def test_round_trip_from_arrays(tmp_path):
    rng = np.random.default_rng(0)
    images = np.stack([wave_image(rng, 12, 9) for _ in range(7)])
    labels = np.array([0, 3, 1, 2, 4, 4, 0])
    np.savez(tmp_path / 'a.npz', images=images, labels=labels)
    np.save(tmp_path / 'x.npy', images[:3])
    np.save(tmp_path / 'y.npy', labels[:3])
    tool = os.path.join(ROOT, 'tools', 'make_array_dataset.py')
    out = str(tmp_path / 'data')
    subprocess.check_call([sys.executable, tool, '--out', out, '--name', 'd', '--split', 'train', '--arrays', str(tmp_path / 'a.npz')])
    subprocess.check_call([sys.executable, tool, '--out', out, '--name', 'd', '--split', 'validation',
                           '--images', str(tmp_path / 'x.npy'), '--labels', str(tmp_path / 'y.npy')])
    info = json.load(open(os.path.join(out, 'd', 'info.json')))
    assert info == {'format': 'simclr-arrays-1', 'num_classes': 5, 'splits': {'train': 7, 'validation': 3}}
    b = data_lib.ArrayDatasetBuilder('d', out)
    assert b.info.splits['train'].num_examples == 7 and b.info.splits['validation'].num_examples == 3
    assert b.info.features['label'].num_classes == 5
    for cache in (False, True):
        sp = b.split('train', cache=cache)
        assert sp.index.dtype == np.int64 and sp.index.shape == (7, 4)
        assert sp.index[:, 3].tolist() == labels.tolist()
        for i in range(7):
            o, h, w, _ = sp.index[i]
            assert (h, w) == (12, 9)
            assert np.array_equal(np.asarray(sp.images[o:o + 3 * h * w]).reshape(h, w, 3), images[i])
    assert os.path.getsize(os.path.join(out, 'd', 'train.images.u8')) == images.size


def test_round_trip_of_mixed_sizes(tmp_path):
    made = make_dataset(str(tmp_path), splits=(('train', 11),), num_classes=4)
    sp = data_lib.ArrayDatasetBuilder('waves', str(tmp_path)).split('train')
    images, labels = made['train']
    assert sp.index[:, 3].tolist() == labels.tolist()
    for i, im in enumerate(images):
        o, h, w, _ = sp.index[i]
        assert (h, w) == im.shape[:2] and np.array_equal(np.asarray(sp.images[o:o + im.size]).reshape(im.shape), im)


def test_round_trip_from_a_folder(tmp_path):
    Image = pytest.importorskip('PIL.Image')
    rng = np.random.default_rng(1)
    want = {}
    for c, (mode, hw) in {'ant': ('RGB', (10, 14)), 'bee': ('L', (9, 9)), 'cat': ('RGBA', (40, 20))}.items():
        os.makedirs(tmp_path / 'root' / c)
        rgb = wave_image(rng, *hw)
        if mode == 'L':
            im = Image.fromarray(rgb[..., 0], 'L')
            rgb = np.repeat(rgb[..., :1], 3, 2)
        elif mode == 'RGBA':
            im = Image.fromarray(np.concatenate([rgb, np.full(hw + (1,), 255, np.uint8)], 2), 'RGBA')
        else:
            im = Image.fromarray(rgb, 'RGB')
        im.save(tmp_path / 'root' / c / 'one.png')
        want[c] = rgb
    tool = os.path.join(ROOT, 'tools', 'make_array_dataset.py')
    subprocess.check_call([sys.executable, tool, '--out', str(tmp_path / 'o'), '--name', 'f', '--split', 'train',
                           '--folder', str(tmp_path / 'root')])
    b = data_lib.ArrayDatasetBuilder('f', str(tmp_path / 'o'))
    sp = b.split('train')
    assert b.info.features['label'].num_classes == 3 and sp.index[:, 3].tolist() == [0, 1, 2]
    for i, c in enumerate(['ant', 'bee', 'cat']):
        o, h, w, _ = sp.index[i]
        assert np.array_equal(np.asarray(sp.images[o:o + 3 * h * w]).reshape(h, w, 3), want[c])
    subprocess.check_call([sys.executable, tool, '--out', str(tmp_path / 'o'), '--name', 'f', '--split', 'validation',
                           '--folder', str(tmp_path / 'root'), '--max_side', '20'])
    v = data_lib.ArrayDatasetBuilder('f', str(tmp_path / 'o')).split('validation').index
    assert v[:, 1:3].tolist() == [[10, 14], [9, 9], [20, 10]]


def test_folder_without_pil_exits_with_a_clear_message(tmp_path):
    os.makedirs(tmp_path / 'root' / 'a')
    (tmp_path / 'root' / 'a' / 'x.png').write_bytes(b'')
    code = ('import sys; sys.modules["PIL"] = None; sys.argv = ["make_array_dataset.py"]; sys.path.insert(0, %r)\n'
            'from tools import make_array_dataset as m\n'
            'm.main(["--out", %r, "--name", "f", "--split", "train", "--folder", %r])\n'
            % (ROOT, str(tmp_path / 'o'), str(tmp_path / 'root')))
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True)
    assert r.returncode != 0 and 'needs PIL' in r.stderr and 'Traceback' not in r.stderr


# ------------------------------------------------------------------ 2. the training stream
@pytest.mark.parametrize('R', [1, 2, 4])
def test_train_stream_order(tmp_path, R):
    N, B = 103, 16
    make_dataset(str(tmp_path), splits=(('train', N),))
    split = data_lib.ArrayDatasetBuilder('waves', str(tmp_path)).split('train')
    steps = 3 * N // B + 2

    def stream(seed):
        its = [_host_iter(split, B, True, r, R, data_seed=seed) for r in range(R)]
        out = []
        for k in range(steps):
            parts = [next(it) for it in its]
            assert all(p.step == k and p.indices.shape == (B // R,) for p in parts)
            glob = np.concatenate([p.indices for p in parts])
            # the replicas' slices are the documented parts of the global batch (R = 1 run), hence disjoint positions
            assert np.array_equal(glob, data_lib.train_indices(N, seed, k, B))
            out.append(glob)
        for it in its:
            it.close()
        return np.concatenate(out)

    s0 = stream(0)
    for e in range(3):                                                   # every epoch-aligned window is a permutation
        assert sorted(s0[e * N:(e + 1) * N].tolist()) == list(range(N))
    assert np.array_equal(s0, stream(0))                                 # same seed, same order
    assert not np.array_equal(s0[:N], s0[N:2 * N])                       # two epochs differ
    assert not np.array_equal(s0[:N], stream(1)[:N])                     # two seeds differ
    # replicas are disjoint within a global batch wherever the batch lies inside one epoch
    for k in range(steps):
        if (k * B) // N == ((k + 1) * B - 1) // N:
            assert len(set(s0[k * B:(k + 1) * B].tolist())) == B


# ------------------------------------------------------------------ 3. history independence
@pytest.mark.parametrize('mode', ['pretrain', 'finetune'])
def test_batches_do_not_depend_on_history(tmp_path, mode):
    N, B, R = 103, 16, 2
    make_dataset(str(tmp_path), splits=(('train', N),))
    split = data_lib.ArrayDatasetBuilder('waves', str(tmp_path)).split('train')
    fresh = _host_iter(split, B, True, 1, R, train_mode=mode)
    seq = [next(fresh) for _ in range(10)]                               # steps 6 and 12.. cross 103 / 16 = 6.4
    fresh.close()
    assert seq[0].params.shape == (B // R, 2 if mode == 'pretrain' else 1, 16)
    for s in (5, 6, 7):
        it = _host_iter(split, B, True, 1, R, train_mode=mode, start_step=s)
        for k in range(s, s + 3):
            hb = next(it)
            assert hb.step == k
            assert np.array_equal(hb.indices, seq[k].indices) and np.array_equal(hb.params, seq[k].params)
            assert np.array_equal(hb.table, seq[k].table) and np.array_equal(hb.labels, seq[k].labels)
        it.close()
    assert (6 * B) // N != (7 * B - 1) // N, 'step 6 spans the epoch boundary'
    if mode == 'finetune':
        assert not seq[0].params[:, :, 5:].any()                         # jitter strength 0 outside pretraining
    # the boxes lie inside their images
    for hb in seq:
        p, hw = hb.params, split.index[hb.indices, 1:3]
        assert (p[..., 0] >= 0).all() and (p[..., 1] >= 0).all() and (p[..., 2] >= 1).all() and (p[..., 3] >= 1).all()
        assert (p[..., 0] + p[..., 2] <= hw[:, None, 0]).all() and (p[..., 1] + p[..., 3] <= hw[:, None, 1]).all()


def test_staged_bytes_are_the_records(tmp_path):
    """The buffer a worker thread fills holds each image's bytes at the offset its table row names."""
    made = make_dataset(str(tmp_path), splits=(('train', 20),))
    split = data_lib.ArrayDatasetBuilder('waves', str(tmp_path)).split('train', cache=True)
    it = _host_iter(split, 8, True, prefetch_batches=1, input_threads=1)
    hb = it._fill(3, 0)
    buf = it._slots[0]['host'].numpy()[it._o_img:hb.nbytes]
    for j, i in enumerate(hb.indices):
        o, h, w = hb.table[j]
        assert np.array_equal(buf[o:o + 3 * h * w].reshape(h, w, 3), made['train'][0][i])
    assert hb.nbytes == it._o_img + sum(made['train'][0][i].size for i in hb.indices)
    it.close()


# ------------------------------------------------------------------ 4. the eval stream
@pytest.mark.parametrize('R', [1, 2])
def test_eval_stream_covers_every_example_once(tmp_path, R):
    M, E = 37, 16
    made = make_dataset(str(tmp_path), splits=(('validation', M),))
    split = data_lib.ArrayDatasetBuilder('waves', str(tmp_path)).split('validation')
    labels = made['validation'][1]
    its = [_host_iter(split, E, False, r, R) for r in range(R)]
    per = [list(it) for it in its]
    assert [len(p) for p in per] == [3] * R == [data_lib.eval_num_steps(M, E)] * R       # same step count everywhere
    seen = np.zeros(M, int)
    top1, top5 = metrics.Accuracy('a'), metrics.TopKCategoricalAccuracy(5, 'b')
    rng = np.random.default_rng(0)
    logits_all = rng.normal(size=(M, 10)).astype(np.float32)
    for p in per:
        for hb in p:
            assert hb.params.shape == (E // R, 1, 16) and set(np.unique(hb.weights)) <= {0.0, 1.0}
            np.add.at(seen, hb.indices[hb.weights == 1], 1)
            assert (hb.indices[hb.weights == 0] == 0).all()
            lab = torch.nn.functional.one_hot(torch.from_numpy(hb.labels), 10).float()
            lg = torch.from_numpy(logits_all[hb.indices])
            metrics.update_finetune_metrics_eval(top1, top5, lg, lab, torch.from_numpy(hb.weights))
    assert seen.tolist() == [1] * M
    assert sum(int((hb.weights == 0).sum()) for p in per for hb in p) == 3 * E - M
    hits1 = int((logits_all.argmax(1) == labels).sum())
    tv = logits_all[np.arange(M), labels]
    hits5 = int(((logits_all > tv[:, None]).sum(1) < 5).sum())
    assert top1.result() == hits1 / M and top5.result() == hits5 / M
    assert top1.totals().tolist() == [hits1, M]


def test_unweighted_metrics_are_unchanged():
    a = metrics.Accuracy('a')
    a.update_state(torch.tensor([1, 2, 3, 4]), torch.tensor([1, 0, 3, 0]))
    assert a.result() == 0.5 and a._count == 4 and a.totals().tolist() == [2.0, 4.0]


# ------------------------------------------------------------------ 5. validation failures name the file
def test_validation_failures_name_the_file(tmp_path):
    import shutil
    make_dataset(str(tmp_path / 'good'), splits=(('train', 12), ('validation', 5)), num_classes=4)

    def broken(tag, fn):
        d = str(tmp_path / tag)
        shutil.copytree(str(tmp_path / 'good'), d)
        fn(os.path.join(d, 'waves'))
        return d

    def edit_index(split, f):
        def go(d):
            p = os.path.join(d, split + '.index.npy')
            idx = np.load(p)
            np.save(p, f(idx))
        return go

    def edit_info(f):
        def go(d):
            p = os.path.join(d, 'info.json')
            info = json.load(open(p))
            f(info)
            json.dump(info, open(p, 'w'))
        return go

    def past_end(idx):
        idx[-1, 0] += 1
        return idx

    def bad_label(idx):
        idx[2, 3] = 4
        return idx

    cases = [
        ('past_end', edit_index('train', past_end), r'train\.index\.npy.*row 11.*outside.*train\.images\.u8'),
        ('label', edit_index('validation', bad_label), r'validation\.index\.npy.*row 2.*label 4.*num_classes = 4'),
        ('count', edit_info(lambda i: i['splits'].__setitem__('train', 13)), r'train\.index\.npy has 12 rows.*info\.json.*13'),
        ('dtype', edit_index('train', lambda idx: idx.astype(np.int32)), r'train\.index\.npy.*int64 \[n, 4\]'),
        ('format', edit_info(lambda i: i.__setitem__('format', 'other')), r'info\.json.*format'),
        ('no_images', lambda d: os.remove(os.path.join(d, 'validation.images.u8')), r'validation\.images\.u8 not found'),
        ('truncated', lambda d: open(os.path.join(d, 'train.images.u8'), 'r+b').truncate(100), r'train\.index\.npy.*outside.*train\.images\.u8'),
        ('zero_side', edit_index('train', lambda idx: idx * np.array([1, 0, 1, 1])), r'train\.index\.npy.*height / width'),
    ]
    for tag, fn, pattern in cases:
        with pytest.raises(data_lib.DatasetError, match=pattern):
            data_lib.ArrayDatasetBuilder('waves', broken(tag, fn))
    b = data_lib.ArrayDatasetBuilder('waves', str(tmp_path / 'good'))
    with pytest.raises(data_lib.DatasetError, match=r"split 'test' is not in .*info\.json"):
        b.split('test')


# ------------------------------------------------------------------ 6. the driver's message
@pytest.mark.parametrize('args', [[], ['--data_dir=/nonexistent/dir']])
def test_dataset_without_usable_data_dir_fails_before_device_work(args):
    code = ('import sys, torch\n'
            'def boom(*a, **k): raise SystemExit("device work before the data_dir check")\n'
            'torch.cuda.current_device = torch.cuda.set_device = torch.cuda.is_available = boom\n'
            'from simclr_amd import run\n'
            'try:\n'
            '    run.main(["--dataset=x", "--mode=train_then_eval"] + %r)\n'
            'except ValueError as e:\n'
            '    print("ERR", e)\n' % (args,))
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr[-2000:]
    assert 'ERR' in r.stdout and 'info.json' in r.stdout and '<split>.index.npy' in r.stdout
    assert 'tools/make_array_dataset.py' in r.stdout
    assert ('needs --data_dir' in r.stdout) if not args else ('/nonexistent/dir/x/info.json not found' in r.stdout)
