"""The float64 restatement tests/swav_multicrop_reference.py pinned from outside: the u / m form against the official crop loop, the
analytic gradients against float64 autograd with the codes detached (and AWAY from autograd without the detach), L = 0 against
tests/swav_reference.py, the hand case of tests/golden/SWAV_MULTICROP_HAND_DERIVED.md, the crop sampler's area range and cover, the
input pipeline's generator of the local views, flags, refusals and metric names, and the error budget of the GPU tests' cases.  No GPU."""
import math

import numpy as np
import pytest

from simclr_amd import data as data_lib
from simclr_amd import data_util
from simclr_amd.flags import FLAGS
from tests import swav_multicrop_reference as mr
from tests import swav_reference as sr


@pytest.fixture(autouse=True)
def _flags():
    FLAGS.reset()
    yield
    FLAGS.reset()


def _case(b, L, K, D, seed=0):
    g = np.random.default_rng(seed)
    unit = lambda x: sr.l2_normalize(x)[0]
    a = g.standard_normal((b, D))
    qh = unit(np.concatenate([a, a + 0.5 * g.standard_normal((b, D))]))
    xh = unit(np.tile(a, (L, 1)) + 0.7 * g.standard_normal((L * b, D)))
    w = unit(g.standard_normal((K, D)))
    alpha, _ = sr.sinkhorn_potentials(qh, w, 0.05, 3)
    return qh, xh, w, alpha


@pytest.mark.parametrize('b,L,K,D', [(1, 1, 2, 4), (3, 2, 7, 8), (5, 6, 16, 8), (4, 8, 5, 16)])
def test_u_m_form_equals_the_official_crop_loop(b, L, K, D):
    qh, xh, w, alpha = _case(b, L, K, D)
    r = mr.multicrop_loss_normalized(qh, xh, w, alpha)
    official = mr.official_loop(qh, xh, w, alpha)
    assert abs(r['loss'] - official) <= 1e-12 * max(1.0, abs(official))
    assert abs(r['global_loss'] + r['local_loss'] - r['loss']) <= 1e-15 * abs(r['loss'])
    # the row form: sum_j Pt[g, j] s_rj = x_r . u_g / T
    s = (xh @ w.T) / 0.1
    i = np.arange(L * b) % b
    direct = 2 * sr.logsumexp(s, 1) - ((r['Pt'][i] + r['Pt'][b + i]) * s).sum(1)
    assert np.abs(direct - r['rows']).max() <= 1e-12 * np.abs(direct).max()


@pytest.mark.parametrize('b,L,K,D', [(3, 2, 7, 8), (5, 6, 16, 8), (2, 1, 3, 4)])
def test_gradients_are_autograd_with_the_codes_detached_and_not_without(b, L, K, D):
    qh, xh, w, _ = _case(b, L, K, D, seed=3)
    alpha, _ = sr.sinkhorn_potentials(qh, w, 0.05, 3)
    r = mr.multicrop_loss_normalized(qh, xh, w, alpha)
    loss, gq, gx, gw = mr.autograd_gradients(qh, xh, w, detach=True)
    assert abs(loss - r['loss']) <= 1e-12 * abs(loss)
    for name, got, ref in (('q', r['grad_q'], gq), ('x', r['grad_x'], gx), ('w', r['grad_w'], gw)):
        assert np.abs(got - ref).max() <= 1e-10 * np.abs(ref).max(), name
    _, gq2, gx2, gw2 = mr.autograd_gradients(qh, xh, w, detach=False)
    # the local rows never enter the Sinkhorn: their gradient is the same; the global rows' and the prototypes' are not
    assert np.abs(r['grad_x'] - gx2).max() <= 1e-10 * np.abs(gx2).max()
    assert np.abs(r['grad_q'] - gq2).max() > 1e-3 * np.abs(gq2).max()
    assert np.abs(r['grad_w'] - gw2).max() > 1e-3 * np.abs(gw2).max()


def test_no_local_views_is_the_swav_loss():
    qh, xh, w, alpha = _case(4, 2, 9, 8, seed=5)
    r = mr.multicrop_loss_normalized(qh, xh[:0], w, alpha)
    g = sr.swav_loss_normalized(qh, w, alpha)
    assert r['loss'] == g['loss'] and np.array_equal(r['grad_q'], g['grad_q']) and np.array_equal(r['grad_w'], g['grad_w'])
    assert mr.official_loop(qh, xh[:0], w, alpha) == pytest.approx(float(g['loss']), rel=1e-13)


def test_hand_case():
    """b = 2, L = 1, K = 2, D = 2 with one-hot-like codes GIVEN as u (tests/golden/SWAV_MULTICROP_HAND_DERIVED.md, "Hand case")."""
    w = np.array([[1.0, 0.0], [0.0, 1.0]])
    # codes: image 0 -> (1, 0) in both views; image 1 -> (1/2, 1/2) in view a, (0, 1) in view b.  u_g = Pt[g] . w = Pt[g]
    u = np.array([[1.0, 0.0], [0.5, 0.5], [1.0, 0.0], [0.0, 1.0]])
    xh = np.array([[1.0, 0.0], [0.0, 1.0]])
    T = 0.5
    r = mr.local_loss_normalized(xh, w, u, b=2, temperature=T)
    lse = math.log(math.exp(2.0) + 1.0)                    # both rows: logits (2, 0) in some order
    rows = [2 * lse - 2 * 2.0, 2 * lse - 1.5 * 2.0]          # x_0 . (u_0 + u_2) = 2,  x_1 . (u_1 + u_3) = 1.5
    assert np.allclose(r['rows'], rows, rtol=0, atol=1e-15)
    assert r['loss'] == pytest.approx(sum(rows) / 8.0, rel=1e-15)             # 2 (V - 1) b = 2 * 2 * 2
    p = math.exp(2.0) / (math.exp(2.0) + 1.0)
    c = 1.0 / (8.0 * T)
    assert np.allclose(r['grad_x'], c * np.array([[2 * p - 2.0, 2 * (1 - p)], [2 * (1 - p) - 0.5, 2 * p - 1.5]]), rtol=0, atol=1e-15)
    # mis-paired by one image the first row reads u_1 + u_3 instead
    s = mr.local_loss_normalized(xh, w, u, b=2, temperature=T, shift=1)
    assert np.allclose(s['rows'], [2 * lse - 0.5 * 2.0, 2 * lse - 0.0], rtol=0, atol=1e-15)


# ---------------------------------------------------------------------------------------------------------------- the sampler
def _reference_boxes(rng, heights, widths, out_h, out_w, max_attempts=100):
    """sample_crop_boxes as it stood before the area range and the cover became arguments (0.08, 1.0 and 0.1 spelled out)."""
    _lrint = lambda x: np.rint(x).astype(np.int64)
    Hh, Ww = np.asarray(heights, np.int64), np.asarray(widths, np.int64)
    m, f32 = Hh.shape[0], np.float32
    ar0 = out_w / out_h
    lo, hi = f32(3. / 4 * ar0), f32(4. / 3. * ar0)
    box = np.stack([np.zeros(m, np.int64), np.zeros(m, np.int64), Hh, Ww], 1)
    todo = np.ones(m, bool)
    min_area = f32(0.08) * Ww.astype(f32) * Hh.astype(f32)
    max_area = f32(1.0) * Ww.astype(f32) * Hh.astype(f32)
    for _ in range(max_attempts):
        if not todo.any():
            break
        ar = (rng.random(m).astype(f32) * (hi - lo) + lo).astype(np.float64)
        h = _lrint(np.sqrt(min_area / ar.astype(f32)))
        max_h = _lrint(np.sqrt(max_area / ar.astype(f32)))
        over = _lrint(max_h * ar) > Ww
        alt = ((Ww + 0.5 - 0.0000001) / ar).astype(np.int64)
        alt = np.where(_lrint(alt * ar) > Ww, alt - 1, alt)
        max_h = np.minimum(np.where(over, alt, max_h), Hh)
        h = np.minimum(h, max_h)
        h = h + np.floor(rng.random(m) * (max_h - h + 1)).astype(np.int64) * (h < max_h)
        w = _lrint(h * ar)
        area = (w * h).astype(np.float64)
        small = area < min_area
        h = np.where(small, h + 1, h); w = np.where(small, _lrint(h * ar), w); area = (w * h).astype(np.float64)
        big = area > max_area
        h = np.where(big, h - 1, h); w = np.where(big, _lrint(h * ar), w); area = (w * h).astype(np.float64)
        ok = ~((area < min_area) | (area > max_area) | (w > Ww) | (h > Hh) | (w <= 0) | (h <= 0))
        y = np.floor(rng.random(m) * np.maximum(Hh - h, 1)).astype(np.int64) * (h < Hh)
        x = np.floor(rng.random(m) * np.maximum(Ww - w, 1)).astype(np.int64) * (w < Ww)
        ok &= (w * h) / (Ww * Hh).astype(np.float64) >= 0.1
        take = todo & ok
        box[take] = np.stack([y, x, h, w], 1)[take]
        todo &= ~ok
    return box


def test_sampler_defaults_reproduce_the_former_boxes_bitwise():
    g = np.random.default_rng(11)
    Hh, Ww = g.integers(8, 500, 4000), g.integers(8, 500, 4000)
    for out_h, out_w in ((224, 224), (32, 32), (96, 128)):
        got = data_util.sample_crop_boxes(np.random.default_rng(5), Hh, Ww, out_h, out_w)
        ref = _reference_boxes(np.random.default_rng(5), Hh, Ww, out_h, out_w)
        assert got.dtype == ref.dtype and np.array_equal(got, ref)
    a = data_util.draw_train_params(64, Hh[:64], Ww[:64], 32, 32, rng=np.random.default_rng(2))
    b = data_util.draw_train_params(64, Hh[:64], Ww[:64], 32, 32, rng=np.random.default_rng(2), area_range=(0.08, 1.0),
                                    min_object_covered=0.1)
    assert a.tobytes() == b.tobytes()


def test_local_draws_cover_their_whole_area_range():
    """375 x 500, 20 000 local draws: every area share lies in [0.05, 0.14] and the smallest is below 0.06 -- with the cover left at the
    sampler's 0.1 the range is silently cut to [0.1, 0.14] (shown beside it)."""
    n = 20000
    p = data_util.draw_local_params(n, 375, 500, 96, 1, 0.05, 0.14, rng=np.random.default_rng(1))
    assert p.shape == (n, 1, 16)
    frac = (p[:, 0, 2].astype(np.float64) * p[:, 0, 3]) / (375 * 500)
    assert frac.min() >= 0.05 and frac.max() <= 0.14 and frac.min() < 0.06, (frac.min(), frac.max())
    assert set(np.unique(p[:, 0, 4])) == {0.0, 1.0} and 0.75 < p[:, 0, 5].mean() < 0.85        # the flip and jitter of a global view
    cut = data_util.sample_crop_boxes(np.random.default_rng(1), np.full(n, 375), np.full(n, 500), 96, 96, area_range=(0.05, 0.14))
    assert (cut[:, 2] * cut[:, 3] / (375 * 500)).min() >= 0.1


@pytest.mark.parametrize('H,W', [(16, 16), (32, 32), (24, 40), (64, 256), (500, 60), (375, 500)])
def test_local_draws_never_fall_back_to_the_whole_image(H, W):
    n = 20000
    box = data_util.sample_crop_boxes(np.random.default_rng(3), np.full(n, H), np.full(n, W), 96, 96, area_range=(0.05, 0.14),
                                      min_object_covered=0.05)
    assert int(((box[:, 2] == H) & (box[:, 3] == W)).sum()) == 0
    assert (box[:, 0] + box[:, 2] <= H).all() and (box[:, 1] + box[:, 3] <= W).all() and (box[:, 2:] > 0).all()


def test_iterator_plan_keeps_the_global_views_and_draws_the_local_ones_apart(tmp_path):
    from tests.data_fixtures import make_dataset
    make_dataset(str(tmp_path), splits=(('train', 40),))
    split = data_lib.ArrayDatasetBuilder('waves', str(tmp_path)).split('train')
    mk = lambda L, **kw: data_lib.DatasetIterator(split, 10, 8, True, device=None, image_size=32, train_mode='pretrain',
                                                 local_crops=L, **kw)
    FLAGS.swav_local_crop_size = 16
    it0, it6 = mk(0), mk(6)
    try:
        for step in (0, 1, 5):
            i0, w0, p0 = it0.plan(step)
            i6, w6, p6 = it6.plan(step)
            assert np.array_equal(i0, i6) and p0.tobytes() == p6.tobytes()
            lp = it6.local_plan(step)
            assert lp.shape == (8, 6, 16) and lp.dtype == np.float32 and lp.tobytes() == it6.local_plan(step, i6).tobytes()
            hw = split.index[i6, 1:3]
            frac = lp[:, :, 2] * lp[:, :, 3] / (hw[:, 0] * hw[:, 1])[:, None]
            assert frac.max() <= 0.14 + 1e-6 and lp.tobytes() != it6.local_plan(step + 1).tobytes()
        h0, h6 = next(it0), next(it6)
        assert h0.local_params is None and h6.local_params.tobytes() == it6.local_plan(0).tobytes()
        assert h0.params.tobytes() == h6.params.tobytes() and np.array_equal(h0.table, h6.table)
        assert it6._o_img - it6._o_lpar >= 4 * 16 * 6 * 8 and it0._o_img == it0._o_lpar
    finally:
        it0.close()
        it6.close()


# ---------------------------------------------------------------------------------------------------------------- flags, refusals, names
def test_flags_defaults_and_refusals():
    from simclr_amd import run
    assert (FLAGS.swav_local_crops, FLAGS.swav_local_crop_size) == (0, 96)
    assert (FLAGS.swav_local_crop_min_scale, FLAGS.swav_local_crop_max_scale) == (0.05, 0.14)
    base = dict(contrastive_loss='swav', proj_out_dim=64, image_size=224, train_mode='pretrain', mode='train')
    FLAGS.update(**base)
    assert run.check_swav_local_flags() == 0 and run.check_contrastive_loss_flags() is False
    FLAGS.update(swav_local_crops=6)
    assert run.check_swav_local_flags() == 6 and run.check_contrastive_loss_flags() is False
    bad = [dict(swav_local_crops=9), dict(swav_local_crops=-1), dict(contrastive_loss='dino'), dict(contrastive_loss='ntxent'),
           dict(swav_local_crop_size=225), dict(swav_local_crop_size=0), dict(swav_local_crop_size=95),
           dict(swav_local_crop_min_scale=0.0), dict(swav_local_crop_min_scale=0.2), dict(swav_local_crop_max_scale=1.5),
           dict(swav_local_crop_min_scale=float('nan')), dict(dropblock_keep_probs='none,none,0.9,0.9', dropblock_size=3)]
    for change in bad:
        FLAGS.reset()
        FLAGS.update(**dict(dict(base, swav_local_crops=6), **change))
        with pytest.raises(ValueError, match='swav_local_crop'):
            run.check_contrastive_loss_flags()
    # an odd local size is fine on the stride-1 stem of 32-pixel images; fine-tuning and evaluation ignore the flags
    FLAGS.reset()
    FLAGS.update(**dict(base, swav_local_crops=2, image_size=32, swav_local_crop_size=15))
    assert run.check_swav_local_flags() == 2
    for change in (dict(train_mode='finetune'), dict(mode='eval')):
        FLAGS.reset()
        FLAGS.update(**dict(base, swav_local_crops=6, swav_local_crop_size=1000, contrastive_loss='ntxent', **change))
        assert run.swav_local_crops() == 0 and run.check_swav_local_flags() == 0
    FLAGS.reset()
    FLAGS.update(**dict(base, swav_local_crops=6))
    assert sorted(run.build_metrics()) == ['train/contrast_loss', 'train/supervised_acc', 'train/supervised_loss',
                                          'train/swav_code_entropy', 'train/total_loss', 'train/weight_decay']


def test_synthetic_batches_keep_the_global_tensors():
    from simclr_amd import run
    a = run.synthetic_batches(4, 32, 10, 'cpu', seed=3)
    b = run.synthetic_batches(4, 32, 10, 'cpu', seed=3, local_crops=2, local_size=16)
    for _ in range(3):
        fa, la = next(a)
        (fg, fl), lb = next(b)
        assert np.array_equal(fa.numpy(), fg.numpy()) and np.array_equal(la['labels'].numpy(), lb['labels'].numpy())
        assert tuple(fl.shape) == (4, 16, 16, 6)


# ---------------------------------------------------------------------------------------------------------------- error budget
def test_error_budget_of_the_gpu_cases():
    """The float32 emulation of the restatement over the GPU tests' cases: its worst errors are the figures recorded in
    SWAV_MULTICROP_HAND_DERIVED.md, from which the GPU tolerances (4x) derive; a local row paired with the next image misses every one of
    them by orders of magnitude."""
    worst = {}
    for case in mr.MC_CASES:
        for name, err in mr.emulation_errors(*case).items():
            worst[name] = max(worst.get(name, 0.0), err)
    print(worst)
    for name, recorded in mr.EMULATION_ERROR.items():
        assert 0.6 * recorded <= worst[name] <= 1.15 * recorded, (name, worst[name], recorded)
        assert mr.TOL[name] == 4.0 * recorded and mr.TOL[name] < 2e-5
    assert {(b, L) for b, L, _, _ in mr.MC_CASES} == {(1, 1), (3, 2), (33, 2), (11, 6), (70, 1)}
    assert {K for _, _, K, _ in mr.MC_CASES} == {2, 65, 4097} and {D for *_, D in mr.MC_CASES} == {64, 128, 256}
    assert len(mr.MC_CASES) == 45
    for b, L, K, D in mr.MC_CASES:
        if b == 1:
            continue
        r = mr.case_reference(b, L, K, D)
        s = mr.multicrop_loss_normalized(r['qh'], r['xh'], r['w'], r['alpha'], mr.MC_T, mr.MC_EPS, shift=1)
        assert mr.relerr(s['local_loss'], r['local_loss']) > 1000 * mr.TOL['loss'], (b, L, K, D)
        assert mr.relerr(s['grad_x'], r['grad_x']) > 1000 * mr.TOL['grad_x'], (b, L, K, D)
        assert mr.relerr(s['grad_w_local'], r['grad_w_local']) > 1000 * mr.TOL['grad_w'], (b, L, K, D)
