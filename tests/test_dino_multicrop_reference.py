"""The float64 restatement tests/dino_multicrop_reference.py pinned from outside: the u / m form against the official crop loop, the
analytic gradients against float64 autograd with the teacher detached (and AWAY from autograd without the detach), the hand case of
tests/golden/DINO_MULTICROP_HAND_DERIVED.md, total = global / (V - 1) + local, identical views, the error budget of the GPU tests'
cases and the paired-lse_t miss on them, flags and refusals, the input pipeline's plan under dino.  No GPU."""
import math

import numpy as np
import pytest

from simclr_amd import data as data_lib
from simclr_amd.flags import FLAGS, local_crop_flags
from tests import dino_multicrop_reference as mr
from tests import dino_reference as dr


@pytest.fixture(autouse=True)
def _flags():
    FLAGS.reset()
    yield
    FLAGS.reset()


def _raw(b, L, K, D, seed=0):
    """Raw projections and raw prototype variables (rows of many norms), a non-zero centre."""
    g = np.random.default_rng(seed)
    a = g.standard_normal((b, D))
    q = np.concatenate([a + 0.4 * g.standard_normal((b, D)), a + 0.4 * g.standard_normal((b, D))]) * 2.0
    k = q + 0.5 * g.standard_normal((2 * b, D))
    x = (np.tile(a, (L, 1)) + 0.7 * g.standard_normal((L * b, D))) * 3.0
    vs = g.standard_normal((K, D)) * (0.5 + g.random((K, 1)))
    vt = vs + 0.1 * g.standard_normal((K, D))
    return q, k, x, vs, vt, 0.1 * g.standard_normal(K)


def _normalised(q, k, x, vs, vt, c):
    n = lambda a: dr.l2_normalize(a)
    (qh, ssq), (kh, _), (xh, ssx), (ws, ssw), (wt, _) = n(q), n(k), n(x), n(vs), n(vt)
    return qh, kh, xh, ws, wt, c, ssq, ssx, ssw


@pytest.mark.parametrize('b,L,K,D,Tt', [(1, 1, 2, 4, 0.04), (3, 2, 7, 8, 0.04), (5, 6, 16, 8, 0.07), (4, 8, 5, 16, 0.04)])
def test_u_m_form_equals_the_official_crop_loop(b, L, K, D, Tt):
    qh, kh, xh, ws, wt, c, *_ = _normalised(*_raw(b, L, K, D))
    r = mr.multicrop_loss_normalized(qh, kh, xh, ws, wt, c, 0.1, Tt)
    official = mr.official_loop(qh, kh, xh, ws, wt, c, 0.1, Tt)
    assert abs(r['loss'] - official) <= 1e-12 * max(1.0, abs(official))
    # the row form: sum_j Pt[g, j] s_rj = x_r . u_g / Ts, with u stored BY ROW
    s = (xh @ ws.T) / 0.1
    i = np.arange(L * b) % b
    ms, rs, _ = dr.softmax_stats(s)
    direct = 2 * (ms + np.log1p(rs)) - ((r['Pt'][i] + r['Pt'][b + i]) * s).sum(1)
    assert np.abs(direct - r['rows']).max() <= 1e-12 * np.abs(direct).max()
    assert np.allclose(r['u'], r['Pt'] @ ws, rtol=0, atol=1e-15)


@pytest.mark.parametrize('L', [1, 2, 6])
def test_total_is_global_over_v_minus_1_plus_local(L):
    qh, kh, xh, ws, wt, c, *_ = _normalised(*_raw(4, L, 9, 8, seed=L))
    r = mr.multicrop_loss_normalized(qh, kh, xh, ws, wt, c)
    g = dr.dino_loss_normalized(qh, kh, ws, wt, c)
    V = 2 + L
    assert r['loss'] == pytest.approx(float(g['loss']) / (V - 1) + float(r['local_loss']), rel=1e-15)
    assert r['loss'] == pytest.approx(mr.official_loop(qh, kh, xh, ws, wt, c), rel=1e-13)
    assert np.allclose(r['grad_q'], g['grad_q'] / (V - 1), rtol=1e-15, atol=0)
    assert np.allclose(r['grad_w'], g['grad_ws'] / (V - 1) + r['grad_w_local'], rtol=1e-15, atol=0)
    # no local views: the plain DINO loss
    z = mr.multicrop_loss_normalized(qh, kh, xh[:0], ws, wt, c)
    assert z['loss'] == g['loss'] and np.array_equal(z['grad_q'], g['grad_q']) and np.array_equal(z['grad_w'], g['grad_ws'])
    assert mr.official_loop(qh, kh, xh[:0], ws, wt, c) == pytest.approx(float(g['loss']), rel=1e-13)


@pytest.mark.parametrize('b,L,K,D,Tt', [(3, 2, 7, 8, 0.04), (5, 6, 16, 8, 0.07), (2, 1, 3, 4, 0.04)])
def test_gradients_are_autograd_with_the_teacher_detached_and_not_without(b, L, K, D, Tt):
    raw = _raw(b, L, K, D, seed=3)
    qh, kh, xh, ws, wt, c, ssq, ssx, ssw = _normalised(*raw)
    r = mr.multicrop_loss_normalized(qh, kh, xh, ws, wt, c, 0.1, Tt)
    loss, gq, gx, gv = mr.autograd_gradients(*raw, 0.1, Tt, detach=True)
    assert abs(loss - r['loss']) <= 1e-12 * abs(loss)
    # x, the global rows and the RAW prototype variable, each through its row normalisation
    for name, got, ref in (('q', dr.l2_normalize_bwd(qh, ssq, r['grad_q']), gq), ('x', dr.l2_normalize_bwd(xh, ssx, r['grad_x']), gx),
                           ('vs', dr.l2_normalize_bwd(ws, ssw, r['grad_w']), gv)):
        assert np.abs(got - ref).max() <= 1e-10 * np.abs(ref).max(), name
    # ws itself: autograd on leaves that ARE the normalised rows
    import torch
    tw, tx = torch.tensor(ws, requires_grad=True), torch.tensor(xh, requires_grad=True)
    i = np.arange(L * b) % b
    Pt = torch.tensor(r['Pt'][i] + r['Pt'][b + i])
    (-(Pt * torch.log_softmax(tx @ tw.T / 0.1, -1)).sum() / (2 * (L + 1) * b)).backward()
    assert np.abs(tw.grad.numpy() - r['grad_w_local']).max() <= 1e-12 * np.abs(r['grad_w_local']).max()
    assert np.abs(tx.grad.numpy() - r['grad_x']).max() <= 1e-12 * np.abs(r['grad_x']).max()
    # a momentum teacher shares no leaf with the student: dropping the detach changes nothing ...
    _, gq1, gx1, gv1 = mr.autograd_gradients(*raw, 0.1, Tt, detach=False)
    assert np.array_equal(gv1, gv) and np.array_equal(gx1, gx)
    # ... but a teacher scored with the student's own prototypes (the target at step 0 is a copy) does: with the stop-gradient the
    # analytic form still holds, without it the prototype gradient is another one; the local rows never enter the teacher
    tied = (raw[0], raw[1], raw[2], raw[3], raw[3], raw[5])
    rt = mr.multicrop_loss_normalized(qh, kh, xh, ws, ws, c, 0.1, Tt)
    _, _, gx2, gv2 = mr.autograd_gradients(*tied, 0.1, Tt, detach=True, tied=True)
    assert np.abs(dr.l2_normalize_bwd(ws, ssw, rt['grad_w']) - gv2).max() <= 1e-10 * np.abs(gv2).max()
    _, _, gx3, gv3 = mr.autograd_gradients(*tied, 0.1, Tt, detach=False, tied=True)
    assert np.abs(gx3 - gx2).max() <= 1e-12 * np.abs(gx2).max()
    assert np.abs(gv3 - gv2).max() > 1e-3 * np.abs(gv2).max()


def test_hand_case():
    """b = 1, L = 1, K = 2, D = 2, prototypes e1 / e2 on both sides, c = (0.1, 0), Ts = Tt = 0.5
    (tests/golden/DINO_MULTICROP_HAND_DERIVED.md, "Hand case")."""
    sig = lambda z: 1.0 / (1.0 + math.exp(-z))
    W = np.eye(2)
    c = np.array([0.1, 0.0])
    kh = np.array([[1.0, 0.0], [0.0, 1.0]])
    qh = kh.copy()
    xh = np.array([[1.0, 0.0]])
    r = mr.multicrop_loss_normalized(qh, kh, xh, W, W, c, 0.5, 0.5)
    # teacher logits: row 0 = (1.8, 0), row 1 = (-0.2, 2)
    p0, p1 = sig(1.8), sig(-2.2)
    assert np.allclose(r['Pt'], [[p0, 1 - p0], [p1, 1 - p1]], rtol=0, atol=1e-15)
    assert np.allclose(r['u'], r['Pt'], rtol=0, atol=1e-15)                   # ws = I: u_g = Pt[g], stored by row
    lse = math.log(math.exp(2.0) + 1.0)                                     # s = (2, 0)
    value = (2 * lse - (p0 + p1) / 0.5) / 4.0                               # cst = 1 / (2 * 2 * 1)
    assert r['local_loss'] == pytest.approx(value, rel=1e-15)
    p = sig(2.0)
    k_ = 1.0 / (4.0 * 0.5)
    assert np.allclose(r['grad_x'], k_ * np.array([[2 * p - (p0 + p1), 2 * (1 - p) - (2 - p0 - p1)]]), rtol=0, atol=1e-15)
    # m_0 = x_0 for both global rows
    want_w = k_ * np.array([[2 * p - (p0 + p1), 0.0], [2 * (1 - p) - (2 - p0 - p1), 0.0]])
    assert np.allclose(r['grad_w_local'], want_w, rtol=0, atol=1e-15)
    # the paired lse_t: row 0's logits under row 1's normaliser and the reverse -- the "probabilities" no longer sum to one
    l0, l1 = math.log(math.exp(1.8) + 1.0), math.log(math.exp(-0.2) + math.exp(2.0))
    assert r['lse_t'] == pytest.approx([l0, l1], rel=1e-15)
    wrong = mr.multicrop_loss_normalized(qh, kh, xh, W, W, c, 0.5, 0.5, lse_of='paired')['grad_w_local']
    e0 = math.exp(1.8 - l1) + math.exp(-0.2 - l0)
    assert wrong[0, 0] == pytest.approx(k_ * (2 * p - e0), rel=1e-14) and abs(wrong[0, 0] - want_w[0, 0]) > 0.05        # 13 % of the entry


def test_identical_views_give_l_times_one_view():
    b, K, D = 4, 9, 8
    qh, kh, xh, ws, wt, c, *_ = _normalised(*_raw(b, 1, K, D, seed=7))
    one = mr.multicrop_loss_normalized(qh, kh, xh, ws, wt, c)
    for L in (2, 5):
        many = mr.multicrop_loss_normalized(qh, kh, np.tile(xh, (L, 1)), ws, wt, c)
        # per view the row gradient is one view's times the ratio of the two cst; the prototype gradient sums L equal views
        ratio = 2.0 / (L + 1)
        assert np.allclose(many['grad_x'], np.tile(one['grad_x'], (L, 1)) * ratio, rtol=1e-13, atol=0)
        assert np.allclose(many['grad_w_local'], L * one['grad_w_local'] * ratio, rtol=1e-12, atol=1e-18)
        assert many['local_loss'] == pytest.approx(L * float(one['local_loss']) * ratio, rel=1e-13)


# ---------------------------------------------------------------------------------------------------------------- error budget
def test_error_budget_of_the_gpu_cases():
    """The float32 emulation over the GPU tests' cases: its worst errors are the recorded ones, from which the GPU tolerances (4x)
    derive; the reference with the PAIRED row's lse_t misses the grad_w tolerance on every case by orders of magnitude."""
    worst = {}
    for case in mr.ALL_CASES:
        for name, err in mr.emulation_errors(*case).items():
            worst[name] = max(worst.get(name, 0.0), err)
    print(worst)
    for name, recorded in mr.EMULATION_ERROR.items():
        assert 0.6 * recorded <= worst[name] <= 1.15 * recorded, (name, worst[name], recorded)
        assert mr.TOL[name] == 4.0 * recorded and mr.TOL[name] < 5e-5
    assert sorted(mr.TOL) == ['grad_w', 'grad_x', 'loss']
    assert {(b, L) for b, L, _, _ in mr.MC_CASES} == {(1, 1), (3, 2), (33, 2), (11, 6), (70, 1)}
    assert {K for _, _, K, _ in mr.MC_CASES} == {2, 65, 4097} and {D for *_, D in mr.MC_CASES} == {64, 128, 256}
    assert len(mr.MC_CASES) == 45 and len(mr.ALL_CASES) == 61
    assert {c[4] for c in mr.ALL_CASES} == {0.04, 0.07} and sum(c[5] == 'onehot' for c in mr.ALL_CASES) == 1
    for case in mr.ALL_CASES:
        r = mr.case_reference(*case)
        assert bool((r['c'] != 0).all())                                    # a non-zero centre
        lse = r['global_row_stats'][:, 1]
        assert np.abs(lse - dr.pair(lse)).max() > 0.05, case                 # the two views' teacher rows differ visibly
        miss = mr.relerr(mr.paired_reference(*case), r['grad_w_local'])
        assert miss > 1000 * mr.TOL['grad_w'], (case, miss)
    hot = mr.case_reference(5, 2, 65, 64, mr.MC_TT, 'onehot')
    assert hot['Pt'].max(1).min() > 0.999 and hot['entropy'] < 0.01


def test_split_plan_reaches_several_splits():
    assert mr.row_splits(33, 2, 2) == (2, 2) and mr.row_splits(70, 1, 2) == (2, 3) and mr.row_splits(70, 1, 65) == (2, 3)
    assert mr.row_splits(11, 6, 4097) == (2, 1) and mr.row_splits(1, 1, 2) == (1, 1)


# ---------------------------------------------------------------------------------------------------------------- flags, refusals, names
def test_flags_defaults_and_refusals():
    from simclr_amd import ops, run
    assert ops.DINO_MAX_LOCAL_CROPS == 8
    assert (FLAGS.dino_local_crops, FLAGS.dino_local_crop_size) == (0, 96)
    assert (FLAGS.dino_local_crop_min_scale, FLAGS.dino_local_crop_max_scale) == (0.05, 0.14)
    base = dict(contrastive_loss='dino', proj_out_dim=64, image_size=224, train_mode='pretrain', mode='train')
    FLAGS.update(**base)
    assert run.check_dino_local_flags() == 0 and run.check_contrastive_loss_flags() is False and run.local_crop_plan()[0] == 0
    FLAGS.update(dino_local_crops=6)
    assert run.check_dino_local_flags() == 6 and run.check_contrastive_loss_flags() is False
    assert run.local_crop_plan() == (6, 96, 0.05, 0.14)
    bad = [dict(dino_local_crops=9), dict(dino_local_crops=-1), dict(contrastive_loss='swav'), dict(contrastive_loss='ntxent'),
           dict(contrastive_loss='byol'), dict(dino_local_crop_size=225), dict(dino_local_crop_size=0), dict(dino_local_crop_size=95),
           dict(dino_local_crop_min_scale=0.0), dict(dino_local_crop_min_scale=0.2), dict(dino_local_crop_max_scale=1.5),
           dict(dino_local_crop_min_scale=float('nan')), dict(dropblock_keep_probs='none,none,0.9,0.9', dropblock_size=3)]
    for change in bad:
        FLAGS.reset()
        FLAGS.update(**dict(dict(base, dino_local_crops=6), **change))
        with pytest.raises(ValueError, match='dino_local_crop'):
            run.check_contrastive_loss_flags()
    # the two cross-loss refusals: each loss's flags under the other loss
    FLAGS.reset()
    FLAGS.update(**dict(base, contrastive_loss='swav', dino_local_crops=2))
    with pytest.raises(ValueError, match='dino_local_crops belongs to --contrastive_loss=dino'):
        run.check_contrastive_loss_flags()
    FLAGS.reset()
    FLAGS.update(**dict(base, swav_local_crops=2))
    with pytest.raises(ValueError, match='swav_local_crops belongs to --contrastive_loss=swav'):
        run.check_contrastive_loss_flags()
    # an odd local size is fine on the stride-1 stem of 32-pixel images; fine-tuning and evaluation ignore the flags
    FLAGS.reset()
    FLAGS.update(**dict(base, dino_local_crops=2, image_size=32, dino_local_crop_size=15))
    assert run.check_dino_local_flags() == 2 and run.local_crop_plan()[:2] == (2, 15)
    for change in (dict(train_mode='finetune'), dict(mode='eval')):
        FLAGS.reset()
        FLAGS.update(**dict(base, dino_local_crops=6, dino_local_crop_size=1000, **change))
        assert run.dino_local_crops() == 0 and run.check_dino_local_flags() == 0 and run.local_crop_plan()[0] == 0
        run.check_contrastive_loss_flags()
    # the helper reads the flags of the ACTIVE loss and nothing under any other
    FLAGS.reset()
    FLAGS.update(**dict(base, contrastive_loss='swav', swav_local_crops=3, swav_local_crop_size=64, dino_local_crop_size=32))
    assert run.local_crop_plan() == (3, 64, 0.05, 0.14)
    FLAGS.update(contrastive_loss='ntxent')
    assert run.local_crop_plan()[0] == 0 and local_crop_flags()[0] == 0
    FLAGS.reset()
    FLAGS.update(**dict(base, dino_local_crops=6))
    assert sorted(run.build_metrics()) == ['train/contrast_loss', 'train/dino_teacher_entropy', 'train/supervised_acc',
                                          'train/supervised_loss', 'train/total_loss', 'train/weight_decay']


def test_iterator_plan_under_dino_keeps_the_global_views_and_reads_the_dino_scales(tmp_path):
    from tests.data_fixtures import make_dataset
    make_dataset(str(tmp_path), splits=(('train', 40),))
    split = data_lib.ArrayDatasetBuilder('waves', str(tmp_path)).split('train')
    mk = lambda **kw: data_lib.DatasetIterator(split, 10, 8, True, device=None, image_size=32, train_mode='pretrain', **kw)
    FLAGS.update(contrastive_loss='dino', swav_local_crops=0, swav_local_crop_size=8, swav_local_crop_max_scale=0.9)
    it0 = mk()
    FLAGS.update(dino_local_crops=6, dino_local_crop_size=16, dino_local_crop_min_scale=0.2, dino_local_crop_max_scale=0.3)
    it6 = mk()
    try:
        assert (it0.local_crops, it6.local_crops, it6.local_size, it6.local_scale) == (0, 6, 16, (0.2, 0.3))
        for step in (0, 1, 5):
            i0, w0, p0 = it0.plan(step)
            i6, w6, p6 = it6.plan(step)
            assert np.array_equal(i0, i6) and p0.tobytes() == p6.tobytes()        # the global parameters, bitwise
            lp = it6.local_plan(step)
            assert lp.shape == (8, 6, 16) and lp.dtype == np.float32 and lp.tobytes() == it6.local_plan(step, i6).tobytes()
            hw = split.index[i6, 1:3]
            frac = lp[:, :, 2] * lp[:, :, 3] / (hw[:, 0] * hw[:, 1])[:, None]
            assert 0.2 - 0.02 <= frac.min() and frac.max() <= 0.3 + 1e-6        # the DINO scales, not SwAV's [0.05, 0.9]
        h0, h6 = next(it0), next(it6)
        assert h0.local_params is None and h6.local_params.tobytes() == it6.local_plan(0).tobytes()
        assert h0.params.tobytes() == h6.params.tobytes() and np.array_equal(h0.table, h6.table)
    finally:
        it0.close()
        it6.close()
    # another loss: the dino flags are not read
    FLAGS.update(contrastive_loss='ntxent')
    it = mk()
    try:
        assert it.local_crops == 0
    finally:
        it.close()


def test_synthetic_batches_keep_the_global_tensors():
    from simclr_amd import run
    a = run.synthetic_batches(4, 32, 10, 'cpu', seed=3)
    b = run.synthetic_batches(4, 32, 10, 'cpu', seed=3, local_crops=2, local_size=16)
    fa, la = next(a)
    (fg, fl), lb = next(b)
    assert np.array_equal(fa.numpy(), fg.numpy()) and np.array_equal(la['labels'].numpy(), lb['labels'].numpy())
    assert tuple(fl.shape) == (4, 16, 16, 6)
