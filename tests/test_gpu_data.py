"""GPU tests of the input pipeline (pytest -m gpu): the ragged augmentation front end against the oracle and against the canvas
kernel, the iterator against the existing canvas API, run.main end to end on a generated dataset, resume, two ranks over gloo.

Measured on an MI355X, the ragged kernel against oracle/augment.py (float64), bounds 5e-3 (max) and 3e-5 (0.9999-quantile):
two views at 32 px from the mixed sizes max 1.5e-6 / p9999 1.2e-6, eval centre crop max 1.8e-7; at 224 px the eval crop max 2.9e-7.
Every test prints its figures before it asserts (run with -s)."""
import ctypes
import glob
import json
import math
import os
import shutil
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests.data_fixtures import make_dataset, wave_image

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _pack(images):
    """(packed uint8 [nbytes], table int64 [b, 3]) of a list of uint8 [h, w, 3] images."""
    table, off = [], 0
    for im in images:
        table.append((off, im.shape[0], im.shape[1]))
        off += im.size
    return np.concatenate([im.reshape(-1) for im in images]), np.asarray(table, np.int64)


def _canvas(images):
    """(canvas uint8 [b, Hmax, Wmax, 3], sizes [b, 2]): every image in the top-left corner of its slot."""
    Hs, Ws = max(im.shape[0] for im in images), max(im.shape[1] for im in images)
    c = np.zeros((len(images), Hs, Ws, 3), np.uint8)
    for i, im in enumerate(images):
        c[i, :im.shape[0], :im.shape[1]] = im
    return c, np.asarray([im.shape[:2] for im in images], np.int64)


def _boxes_inside(params, sizes):
    p = params
    return bool((p[..., 0] >= 0).all() and (p[..., 1] >= 0).all() and (p[..., 2] >= 1).all() and (p[..., 3] >= 1).all()
                and (p[..., 0] + p[..., 2] <= sizes[:, None, 0]).all() and (p[..., 1] + p[..., 3] <= sizes[:, None, 1]).all())


SIZES_32 = [(20, 17), (33, 32), (8, 8), (375, 500), (32, 32), (64, 48)]
SIZES_224 = [(375, 500), (224, 224), (100, 130), (500, 333)]


# ------------------------------------------------------------------ 7. ragged kernel vs the oracle
@pytest.mark.parametrize('sizes,H', [(SIZES_32, 32), (SIZES_224, 224)])
def test_ragged_augmentation_vs_oracle(sizes, H):
    """simclr_augment_views_ragged vs oracle/augment.py given identical draws, at check_augment's tolerances for the canvas
    kernel: max error 5e-3, 0.9999-quantile 3e-5, range [0,1], shape; both views and the eval centre crop."""
    from oracle import augment as oa
    from simclr_amd import data_util as du
    rng = np.random.default_rng(7)
    images = [wave_image(rng, h, w) for h, w in sizes]
    b = len(images)
    packed, table = _pack(images)
    sz = table[:, 1:3]
    params = du.draw_train_params(b, sz[:, 0], sz[:, 1], H, H, 1.0, rng=rng)
    params[0, 0, 5] = 1; params[0, 0, 6:10] = (1, 0, 2, 3); params[0, 0, 14] = 0      # contrast first: mean of the raw crop
    params[1, 1, 5] = 1; params[1, 1, 6:10] = (3, 2, 0, 1); params[1, 1, 14] = 1      # contrast last + grayscale
    params[2, 0, 0:4] = (0, 0, sz[2, 0], sz[2, 1])                                    # a crop equal to the whole image
    assert _boxes_inside(params, sz)
    dev = torch.from_numpy(packed).to(DEV)
    got = du.two_view_batch_ragged(dev, table, H, H, params=params)
    torch.cuda.synchronize()
    ref = oa.two_view_batch(images, params.astype(np.float64), H, H)
    assert ref.min() >= 0.0 and ref.max() <= 1.0
    g = got.double().cpu().numpy()
    err = np.abs(g - ref)
    print('ragged two-view %s -> %d: max %.3e  p9999 %.3e' % (sizes, H, err.max(), np.quantile(err, 0.9999)))
    assert g.shape == (b, H, H, 6) and g.min() >= 0.0 and g.max() <= 1.0
    assert err.max() <= 5e-3 and np.quantile(err, 0.9999) <= 3e-5
    ev = du.preprocess_for_eval_batch_ragged(dev, table, H, H).double().cpu().numpy()
    ev_ref = np.stack([oa.preprocess_for_eval(im, H, H) for im in images])
    e2 = np.abs(ev - ev_ref)
    print('ragged eval centre crop -> %d: max %.3e  p9999 %.3e' % (H, e2.max(), np.quantile(e2, 0.9999)))
    assert ev.shape == (b, H, H, 3) and ev.min() >= 0.0 and ev.max() <= 1.0
    assert e2.max() <= 5e-3 and np.quantile(e2, 0.9999) <= 3e-5


# ------------------------------------------------------------------ 8. ragged == canvas, bitwise
@pytest.mark.parametrize('sizes,H', [(SIZES_32, 32), (SIZES_224, 224)])
def test_ragged_output_is_bitwise_the_canvas_path(sizes, H):
    from simclr_amd import data_util as du
    rng = np.random.default_rng(11)
    images = [wave_image(rng, h, w) for h, w in sizes]
    packed, table = _pack(images)
    canvas, sz = _canvas(images)
    params = du.draw_train_params(len(images), sz[:, 0], sz[:, 1], H, H, 1.0, rng=rng)
    a = du.two_view_batch_ragged(torch.from_numpy(packed).to(DEV), table, H, H, params=params)
    c = du.two_view_batch(torch.from_numpy(canvas).to(DEV), H, H, sizes=sz, params=params)
    assert torch.equal(a, c)
    for crop in (True, False):
        a = du.preprocess_for_eval_batch_ragged(torch.from_numpy(packed).to(DEV), table, H, H, crop=crop)
        c = du.preprocess_for_eval_batch(torch.from_numpy(canvas).to(DEV), H, H, crop=crop, sizes=sz)
        assert torch.equal(a, c)
    p1 = du.draw_train_params(len(images), sz[:, 0], sz[:, 1], H, H, 0.0, views=1, rng=rng)       # the finetune form
    a = du.preprocess_for_train_batch_ragged(torch.from_numpy(packed).to(DEV), table, H, H, params=p1)
    c = du.preprocess_for_train_batch(torch.from_numpy(canvas).to(DEV), H, H, sizes=sz, params=p1)
    assert torch.equal(a, c)


# ------------------------------------------------------------------ 9. bad tables and arguments are refused, nothing is launched
def test_bad_table_and_arguments_are_refused():
    from simclr_amd import _lib, ops
    images = [np.zeros((4, 5, 3), np.uint8), np.zeros((6, 3, 3), np.uint8)]
    packed, table = _pack(images)
    dev = torch.from_numpy(packed).to(DEV)
    params = torch.zeros(2, 1, 16, device=DEV)
    for row, col, val in [(1, 0, table[1, 0] + 1), (1, 1, 7), (0, 0, -1), (0, 2, 0), (1, 0, 1 << 40), (1, 2, 1 << 30)]:
        t = table.copy()
        t[row, col] = val
        with pytest.raises(ValueError, match='table row %d' % row):
            ops.augment_views_ragged(dev, t, params, 8, 8)
    with pytest.raises(ValueError, match=r'\[b, 3\]'):
        ops.augment_views_ragged(dev, table[:, :2], params, 8, 8)
    L = _lib.lib()
    fake = ctypes.c_void_p(1 << 20)                # never dereferenced: every call below fails its argument check
    with pytest.raises(_lib.SimclrHipError, match='null argument'):
        L.augment_views_ragged(None, 100, fake, fake, fake, fake, 2, 1, 8, 8, None)
    with pytest.raises(_lib.SimclrHipError, match='null argument'):
        L.augment_views_ragged(fake, 100, None, fake, fake, fake, 2, 1, 8, 8, None)
    for args in [(0, 2, 1, 8, 8), (-5, 2, 1, 8, 8), (100, 0, 1, 8, 8), (100, 2, 0, 8, 8), (100, 2, 1, 0, 8), (100, 2, 1, 8, -1)]:
        with pytest.raises(_lib.SimclrHipError, match='bad shape'):
            L.augment_views_ragged(fake, args[0], fake, fake, fake, fake, args[1], args[2], args[3], args[4], None)
    assert 'bad shape' in L.last_error()


# ------------------------------------------------------------------ 10. the iterator against the existing API
def _setup(tmp_path, **flags):
    from simclr_amd import data as data_lib
    from simclr_amd.flags import FLAGS
    made = make_dataset(str(tmp_path / 'data'), splits=(('train', 50), ('validation', 37)), num_classes=10, seed=3)
    FLAGS.reset()
    FLAGS.update(dataset='waves', data_dir=str(tmp_path / 'data'), image_size=32, **flags)
    return made, data_lib.ArrayDatasetBuilder('waves', str(tmp_path / 'data'))


@pytest.mark.parametrize('mode,cache', [('pretrain', False), ('finetune', True)])
def test_iterator_equals_the_canvas_api_on_the_documented_batches(tmp_path, mode, cache):
    from simclr_amd import data as data_lib
    from simclr_amd import data_util as du
    from simclr_amd.flags import FLAGS
    made, builder = _setup(tmp_path, train_mode=mode, cache_dataset=cache, data_seed=5)
    B, E, N, M = 16, 16, 50, 37
    views = 2 if mode == 'pretrain' else 1
    images, labels = made['train']
    it = data_lib.build_distributed_dataset(builder, B, True, None)
    for k in range(4):                                                   # step 3 spans the epoch boundary (50 / 16)
        feats, lab = next(it)
        idx = data_lib.train_indices(N, 5, k, B)
        canvas, sz = _canvas([images[i] for i in idx])
        params = du.draw_train_params(B, sz[:, 0], sz[:, 1], 32, 32, FLAGS.color_jitter_strength if views == 2 else 0., views=views,
                                      rng=np.random.default_rng([5, k, 0]))
        want = du.preprocess_for_train_batch(torch.from_numpy(canvas).to(DEV), 32, 32, sizes=sz, views=views, params=params)
        assert feats.shape == (B, 32, 32, 3 * views) and torch.equal(feats, want), k
        assert torch.equal(lab['labels'].cpu(), torch.nn.functional.one_hot(torch.from_numpy(labels[idx]), 10).float())
    it.close()
    images, labels = made['validation']
    ev = list(data_lib.build_distributed_dataset(builder, E, False, None))
    assert len(ev) == 3
    for k, (feats, lab) in enumerate(ev):
        idx, w = data_lib.eval_indices(M, k, E)
        canvas, sz = _canvas([images[i] for i in idx])
        want = du.preprocess_for_eval_batch(torch.from_numpy(canvas).to(DEV), 32, 32, crop=False, sizes=sz)   # no test crop at 32 px
        assert torch.equal(feats, want), k
        assert torch.equal(lab['labels'].cpu(), torch.nn.functional.one_hot(torch.from_numpy(labels[idx]), 10).float())
        assert lab['mask'].cpu().tolist() == w.tolist()
    FLAGS.reset()


def test_iterator_applies_the_test_crop_above_32_px(tmp_path):
    from simclr_amd import data as data_lib
    from simclr_amd import data_util as du
    from simclr_amd.flags import FLAGS
    made, builder = _setup(tmp_path)
    FLAGS.update(image_size=48)
    feats, _ = next(data_lib.build_distributed_dataset(builder, 8, False, None))
    canvas, sz = _canvas(made['validation'][0][:8])
    assert torch.equal(feats, du.preprocess_for_eval_batch(torch.from_numpy(canvas).to(DEV), 48, 48, crop=True, sizes=sz))
    FLAGS.reset()


# ------------------------------------------------------------------ 11. run.main end to end
COMMON = ['--dataset=waves', '--resnet_depth=18', '--image_size=32', '--train_batch_size=16', '--eval_batch_size=16',
          '--use_blur=False', '--compute_dtype=f32', '--f32_matmul=exact']


def test_main_train_then_eval_on_a_generated_dataset(tmp_path):
    from simclr_amd import data as data_lib
    from simclr_amd import data_util as du
    from simclr_amd import model as model_lib
    from simclr_amd import run
    from simclr_amd.checkpoint import Checkpoint
    from simclr_amd.flags import FLAGS
    from simclr_amd.resnet import RT
    M = 37
    made = make_dataset(str(tmp_path / 'data'), splits=(('train', 200), ('validation', M)), num_classes=10, seed=4)
    args = COMMON + ['--data_dir=' + str(tmp_path / 'data'), '--model_dir=' + str(tmp_path / 'm'), '--mode=train_then_eval',
                     '--train_steps=4', '--checkpoint_steps=2']
    FLAGS.reset()
    result = run.main(args)
    assert result is not None and result['global_step'] == 4
    assert all(math.isfinite(v) for v in result.values()), result
    lines = [json.loads(l) for l in open(tmp_path / 'm' / 'summaries.jsonl')]
    assert lines and all(math.isfinite(l['value']) for l in lines)
    # the same padded batches through the canvas API on the restored checkpoint
    FLAGS.reset()
    FLAGS.parse(args)
    RT.reset()
    RT.device = torch.device(DEV)
    model = model_lib.Model(10)
    with torch.no_grad():
        model(torch.zeros(2, 32, 32, 3, device=DEV), training=False)
    Checkpoint(model=model).restore(str(tmp_path / 'm' / 'ckpt-4.pt'), model_only=True).expect_partial()
    images, labels = made['validation']
    hits = 0
    for k in range(data_lib.eval_num_steps(M, 16)):
        idx, w = data_lib.eval_indices(M, k, 16)
        canvas, sz = _canvas([images[i] for i in idx])
        feats = du.preprocess_for_eval_batch(torch.from_numpy(canvas).to(DEV), 32, 32, crop=False, sizes=sz)
        _, sup = model(feats, training=False)
        pred = sup.dense().argmax(1).cpu().numpy()
        hits += int(((pred == labels[idx]) & (w == 1)).sum())
    x = result['eval/label_top_1_accuracy'] * M
    print('top-1 hits: main %.12f, canvas API %d of %d' % (x, hits, M))
    assert abs(x - hits) < 1e-9
    assert 0 <= result['eval/label_top_5_accuracy'] * M <= M and abs(result['eval/label_top_5_accuracy'] * M - round(result['eval/label_top_5_accuracy'] * M)) < 1e-9
    # --mode=eval on the written checkpoints gives the same result
    FLAGS.reset()
    again = run.main(COMMON + ['--data_dir=' + str(tmp_path / 'data'), '--model_dir=' + str(tmp_path / 'm'), '--mode=eval'])
    assert again['eval/label_top_1_accuracy'] == result['eval/label_top_1_accuracy'] and again['global_step'] == 4
    FLAGS.reset()


# ------------------------------------------------------------------ 12. resume continues the uninterrupted run
def test_resumed_run_equals_the_uninterrupted_run_bitwise(tmp_path):
    from simclr_amd import run
    from simclr_amd.flags import FLAGS
    make_dataset(str(tmp_path / 'data'), splits=(('train', 200), ('validation', 37)), num_classes=10, seed=4)
    args = COMMON + ['--data_dir=' + str(tmp_path / 'data'), '--mode=train', '--train_steps=6', '--checkpoint_steps=3']
    a_dir, b_dir = str(tmp_path / 'a'), str(tmp_path / 'b')
    FLAGS.reset()
    run.main(args + ['--model_dir=' + a_dir])
    assert sorted(os.path.basename(p) for p in glob.glob(os.path.join(a_dir, 'ckpt-*.pt'))) == ['ckpt-3.pt', 'ckpt-6.pt']
    os.makedirs(b_dir)
    shutil.copy(os.path.join(a_dir, 'ckpt-3.pt'), b_dir)
    with open(os.path.join(b_dir, 'checkpoint.json'), 'w') as f:
        json.dump({'model_checkpoint_path': 'ckpt-3.pt', 'all_model_checkpoint_paths': ['ckpt-3.pt']}, f)
    FLAGS.reset()
    run.main(args + ['--model_dir=' + b_dir])
    FLAGS.reset()
    a = torch.load(os.path.join(a_dir, 'ckpt-6.pt'), map_location='cpu')
    b = torch.load(os.path.join(b_dir, 'ckpt-6.pt'), map_location='cpu')
    a3 = torch.load(os.path.join(a_dir, 'ckpt-3.pt'), map_location='cpu')
    assert a['global_step'] == b['global_step'] == 6 and b['optimizer']['iterations'] == 6
    assert set(a['model']) == set(b['model']) and set(a['optimizer']['slots']) == set(b['optimizer']['slots']) and a['optimizer']['slots']
    moved = [n for n in a['model'] if not torch.equal(a['model'][n], a3['model'][n])]
    assert len(moved) > 50                                               # steps 4..6 did train
    diff = [n for n in a['model'] if not torch.equal(a['model'][n], b['model'][n])]
    diff += ['slot ' + n for n in a['optimizer']['slots'] if not torch.equal(a['optimizer']['slots'][n], b['optimizer']['slots'][n])]
    assert not diff, diff[:8]


# ------------------------------------------------------------------ 13. two ranks on one GPU over gloo
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, data_dir, model_dir, q):
    try:
        import torch.distributed as dist
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          SIMCLR_DIST_BACKEND='gloo', SIMCLR_SHARE_GPU='1')
        torch.cuda.set_device(0)
        dist.init_process_group('gloo', rank=rank, world_size=world)
        from simclr_amd import comm
        from simclr_amd import data as data_lib
        from simclr_amd import data_util as du
        from simclr_amd import run
        from simclr_amd.flags import FLAGS
        N, M, B, E = 60, 37, 16, 16
        FLAGS.reset()
        FLAGS.update(dataset='waves', data_dir=data_dir, image_size=32, data_seed=2)
        builder = data_lib.ArrayDatasetBuilder('waves', data_dir)
        strategy = comm.Strategy()
        b = B // world
        sp = builder.split('train')                    # the file's own bytes (the converter round trip is a CPU test)
        images = [np.asarray(sp.images[o:o + 3 * h * w]).reshape(h, w, 3) for o, h, w, _ in sp.index]
        it = data_lib.build_distributed_dataset(builder, B, True, strategy)
        for k in range(3):
            feats, lab = next(it)
            idx = data_lib.train_indices(N, 2, k, B)[rank * b:(rank + 1) * b]          # the documented slice of the global batch
            canvas, sz = _canvas([images[i] for i in idx])
            params = du.draw_train_params(b, sz[:, 0], sz[:, 1], 32, 32, 1.0, rng=np.random.default_rng([2, k, rank]))
            want = du.two_view_batch(torch.from_numpy(canvas).cuda(), 32, 32, sizes=sz, params=params)
            assert torch.equal(feats, want), (rank, k)
            assert lab['labels'].argmax(1).cpu().tolist() == sp.index[idx, 3].tolist()
        it.close()
        ev = list(data_lib.build_distributed_dataset(builder, E, False, strategy))
        counted = torch.tensor([float(sum(float(l['mask'].sum()) for _, l in ev)), float(len(ev))], dtype=torch.float64)
        mine = int(counted[0])
        dist.all_reduce(counted)
        res = dict(eval_examples=float(counted[0]), eval_steps_sum=float(counted[1]), mine=mine)
        FLAGS.reset()
        result = run.main(['--dataset=waves', '--data_dir=' + data_dir, '--model_dir=' + model_dir, '--resnet_depth=18', '--image_size=32',
                           '--train_batch_size=16', '--eval_batch_size=16', '--use_blur=False', '--compute_dtype=f32', '--f32_matmul=exact',
                           '--mode=train_then_eval', '--train_steps=3', '--checkpoint_steps=3', '--data_seed=2'])
        res['result'] = result
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, 'ok', res))
    except Exception:  # noqa
        import traceback
        q.put((rank, 'FAIL', traceback.format_exc()))


def test_two_ranks_over_gloo_read_their_slices_and_finish(tmp_path):
    data_dir, model_dir = str(tmp_path / 'data'), str(tmp_path / 'm')
    make_dataset(data_dir, splits=(('train', 60), ('validation', 37)), num_classes=10, seed=6)
    os.environ['SIMCLR_PEER_STATS'] = '0'          # the statistics travel over gloo (the peer-mapped exchange has its own tests)
    try:
        ctx = mp.get_context('spawn')
        q = ctx.Queue()
        port = _free_port()
        procs = [ctx.Process(target=_worker, args=(r, 2, port, data_dir, model_dir, q)) for r in range(2)]
        for p in procs:
            p.start()
        res = [q.get(timeout=600) for _ in procs]
        for p in procs:
            p.join(timeout=60)
    finally:
        os.environ.pop('SIMCLR_PEER_STATS', None)
    assert all(r[1] == 'ok' for r in res), res
    M = 37
    for _, _, m in res:
        assert m['eval_examples'] == M and m['eval_steps_sum'] == 2 * 3, m         # counts all-reduce to M; same steps on both ranks
        r = m['result']
        assert r['global_step'] == 3 and all(math.isfinite(v) for v in r.values()), r
        x = r['eval/label_top_1_accuracy'] * M
        assert abs(x - round(x)) < 1e-9 and 0 <= round(x) <= M, r
    for key in ('eval/label_top_1_accuracy', 'eval/label_top_5_accuracy', 'global_step'):       # all-reduced counts: equal on both ranks
        assert res[0][2]['result'][key] == res[1][2]['result'][key], key
    assert sorted(m['mine'] for _, _, m in res) == [16, 21]                        # 8 + 8 + 5 and 8 + 8 + 0 of the 37
    assert os.path.exists(os.path.join(model_dir, 'ckpt-3.pt')) and os.path.exists(os.path.join(model_dir, 'result.json'))
