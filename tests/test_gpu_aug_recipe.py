"""GPU tests (pytest -m gpu) of solarization in the blur's last pass (simclr_batch_blur_solarize, blur1d<true, true> in csrc/pool.hip), of
data_util.apply_view_plan and of the pretraining step under --aug_recipe.  The kernel runs through the C ABI into guarded, NaN-filled
buffers and every element is compared with the float64 oracle at the tolerance recorded in tests/golden/AUG_RECIPE.md (4 x the
float32 emulation's error, measured on the CPU; tests/aug_recipe_reference.py); the dyadic cases, the all-zero coin table and the
K = 1 path are bitwise.  tests/test_aug_recipe_reference.py pins cases, comparator, guard and mutants without a GPU."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import aug_recipe_reference as R
from tests import augment_reference as ar

pytestmark = pytest.mark.gpu
F32 = np.float32


def _assert(results):
    bad = [r for r in results if not r['ok']]
    worst = max((r for r in results if 'oracle' in r['name']), key=lambda r: r['err'], default=None)
    if worst is not None:
        print('%d checks; largest error vs float64 %.3e (tol %.3e) at %s' % (len(results), worst['err'], worst['tol'], worst['name']))
    assert not bad, '\n'.join('%s err=%.3e tol=%.3e' % (r['name'], r['err'], r['tol']) for r in bad)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, F32)).to('cuda')


def _filt(base):
    from simclr_amd import data_util as du
    return du.gaussian_filter(base['height'] // 10, torch.tensor(base['sigmas'], dtype=torch.float32).to('cuda')).contiguous()


def _run(c, entry='solarize', coin=None, filt=None):
    """One case through the C ABI: tmp and out are guarded buffers filled with NaN.  Returns (out as numpy, guard-band result)."""
    from simclr_amd import _lib, ops
    from tests import gpu_checks as gc
    base = c['blur']
    x, sel = _dev(base['x']), _dev(base['sel'])
    filt = _filt(base) if filt is None else filt
    b, H, W, C = x.shape
    k, K = filt.shape
    tmp, tmp_chk = gc._guarded(x.shape, torch.float32)
    out, out_chk = gc._guarded(x.shape, torch.float32)
    tmp.fill_(float('nan')); out.fill_(float('nan'))
    L = _lib.lib()
    if entry == 'solarize':
        coin = _dev(c['coin'] if coin is None else coin)
        L.batch_blur_solarize(ops._p(x), ops._p(tmp), ops._p(out), ops._p(filt), ops._p(sel), ops._p(coin), float(c['t']), b, H, W, k, K, ops._s())
    else:
        L.batch_blur(ops._p(x), ops._p(tmp), ops._p(out), ops._p(filt), ops._p(sel), b, H, W, k, K, ops._s())
    torch.cuda.synchronize()
    return out.cpu().numpy(), gc._guards(c['name'] + ' ' + entry, tmp_chk, out_chk)


# ---------------------------------------------------------------------------------------------------------------- kernel against float64
@pytest.mark.parametrize('H,W,height', ar.BLUR_SIZES)
def test_kernel_against_float64(H, W, height):
    """40x3 and 3x40 under the 5-tap filter of height 40 (wider than the short side), 3x40 and 7x9 under their 1-tap filter, 45x20;
    views 1, 2, 3; selectors none / all / mixed; coins none / all / mixed per (view, image) / different between the views;
    thresholds 0.5, 0.25, 0.75.  Every element at 4 x E32; the threshold guard admits either branch within that of t != 0.5 on a
    solarized image, at most 1 % of a case (none of the committed cases has such an element on the reference)."""
    res = []
    for c in R.cases(H, W, height):
        got, guard = _run(c)
        res += R.compare(got, c, R.tolerance()) + [guard]
    assert len(res) == 144 * 4
    _assert(res)


# ---------------------------------------------------------------------------------------------------------------- bitwise cases
@pytest.mark.parametrize('c', R.exact_cases(), ids=lambda c: 't%g' % c['t'])
def test_dyadic_images_are_bitwise_and_the_threshold_inverts(c):
    """Pixels j/64, nothing blurred, mixed coins: bitwise the expected table.  t = 0.25: the stripe of 16/64 inverts to 48/64 where
    the coin is set.  t = 0 with pixels in [-4/64, 68/64]: the clip comes first (a negative pixel becomes 0, then 1)."""
    got, guard = _run(c)
    _assert(R.compare(got, c, 0.0) + [guard])
    want = R.expected_exact(c)
    at = (np.clip(c['blur']['x'], F32(0), F32(1)) == F32(c['t'])) & R._coin_mask(c)
    assert at.sum() >= 10 and (got[at] == F32(1 - c['t'])).all() and np.array_equal(got, want)


@pytest.mark.parametrize('H,W,height', [(45, 20, 45), (7, 9, 7)])
def test_all_zero_coins_and_none_are_bitwise_the_old_entry(H, W, height):
    from simclr_amd import ops
    for c in (R.case(H, W, height, 3, ar.BLUR_SIGMAS[3][0], 'mixed', 'none', 0.25), R.case(H, W, height, 2, ar.BLUR_SIGMAS[2][0], 'all', 'none', 0.75)):
        old, g0 = _run(c, 'old')
        new, g1 = _run(c, 'solarize')
        again, g2 = _run(c, 'solarize')
        _assert([g0, g1, g2])
        assert np.array_equal(old, new) and np.array_equal(new, again) and not np.isnan(old).any()
        base = c['blur']
        x, filt, sel = _dev(base['x']), _filt(base), _dev(base['sel'])
        assert np.array_equal(ops.batch_blur(x, filt, sel).cpu().numpy(), old)                       # solarize=None: the old entry
        assert np.array_equal(ops.batch_blur(x, filt, sel, None, 0.25).cpu().numpy(), old)
        assert np.array_equal(ops.batch_blur(x, filt, sel, torch.zeros_like(sel), 0.25).cpu().numpy(), old)
        coined = ops.batch_blur(x, filt, sel, torch.ones_like(sel), 0.25).cpu().numpy()
        assert not np.array_equal(coined, old)


def test_repeat_calls_are_bitwise_equal():
    c = R.case(45, 20, 45, 3, ar.BLUR_SIGMAS[3][0], 'mixed', 'views', 0.25)
    a, _ = _run(c)
    for _ in range(3):
        assert np.array_equal(_run(c)[0], a)


def test_one_tap_filter_with_zero_selectors_is_copy_clip_solarize():
    """The --use_blur=False path: K = 1, all-zero selectors, inputs in [-0.1, 1.1]."""
    for k in (1, 2, 3):
        for t in R.THRESHOLDS:
            c = R.case(45, 20, 45, k, ar.BLUR_SIGMAS[k][0], 'none', 'views', t)
            got, guard = _run(c, filt=torch.ones(k, 1, device='cuda'))
            x = np.clip(c['blur']['x'], F32(0), F32(1))
            want = np.where(R._coin_mask(c) & (x >= F32(t)), F32(1) - x, x)
            _assert([guard])
            assert np.array_equal(got, want), (k, t)


def test_refusals_of_the_new_entry():
    from simclr_amd import _lib, ops
    L = _lib.lib()
    b, H, W, k, K = 2, 5, 6, 2, 3
    x = torch.rand(b, H, W, 3 * k, device='cuda')
    tmp, out = torch.zeros_like(x), torch.full_like(x, 7.0)
    filt, sel, coin = torch.full((k, K), 1.0 / 3, device='cuda'), torch.ones(k, b, device='cuda'), torch.ones(k, b, device='cuda')
    ptrs = [ops._p(t) for t in (x, tmp, out, filt, sel, coin)]

    def call(p=ptrs, t=0.5, shape=(b, H, W, k, K)):
        L.batch_blur_solarize(*p, ctypes.c_float(t), *shape, ops._s())
    for i in range(6):
        with pytest.raises(_lib.SimclrHipError, match='null argument'):
            call(p=ptrs[:i] + [None] + ptrs[i + 1:])
    for bad in ((b, H, W, k, 2), (b, H, W, k, 0), (b, H, W, k, -3), (0, H, W, k, K), (b, 0, W, k, K), (b, H, 0, k, K), (b, H, W, 0, K)):
        with pytest.raises(_lib.SimclrHipError, match='bad shape'):
            call(shape=bad)
    for t in (-0.01, 1.01, float('nan'), float('inf')):
        with pytest.raises(_lib.SimclrHipError, match='threshold must lie in'):
            call(t=t)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((tmp == 0.0).all())                                       # nothing was launched
    for t in (0.0, 1.0):                                                                              # the ends are thresholds
        call(t=t)
    torch.cuda.synchronize()
    assert bool((out != 7.0).all())


# ---------------------------------------------------------------------------------------------------------------- helper
def _manual(x, height, sigmas, sel, coin, t):
    """View by view through the OLD entry, then the rule in torch."""
    from simclr_amd import data_util as du
    outs = []
    for v in range(x.shape[3] // 3):
        y = du.batch_random_blur_tensor(x[..., 3 * v:3 * v + 3].contiguous(), height, height, sigmas=[sigmas[v]], selectors=sel[v:v + 1])
        m = (coin[v] != 0).reshape(-1, 1, 1, 1) & (y >= t)
        outs.append(torch.where(m, 1.0 - y, y))
    return torch.cat(outs, 3)


def test_helper_is_the_manual_composition_for_the_global_views():
    """View a is channels 0:3: its selector and coin act there and nowhere else."""
    from simclr_amd import data_util as du
    from simclr_amd import flags as flags_lib
    from simclr_amd.flags import FLAGS
    g = torch.Generator().manual_seed(3)
    b, H = 5, 32
    x = (torch.rand(b, H, H, 6, generator=g) * 1.2 - 0.1).cuda()
    sigmas = [1.7, 0.4]
    sel = torch.tensor([[1, 1, 0, 1, 0], [0, 1, 0, 0, 1]], dtype=torch.float32).cuda()
    coin = torch.tensor([[0, 0, 1, 1, 0], [1, 0, 1, 0, 1]], dtype=torch.float32).cuda()
    try:
        for t in (0.5, 0.25):
            FLAGS.reset(); FLAGS.update(aug_recipe='byol', solarize_threshold=t)
            got = du.apply_view_plan(x, flags_lib.aug_plan(), height=H, sigmas=sigmas, selectors=sel, solarize=coin)
            assert torch.equal(got, _manual(x, H, sigmas, sel, coin, t))
            swapped = du.apply_view_plan(x, flags_lib.aug_plan(), height=H, sigmas=sigmas, selectors=sel, solarize=coin.flip(0))
            assert not torch.equal(swapped[..., 0:3], got[..., 0:3]) and not torch.equal(swapped[..., 3:6], got[..., 3:6])
        # --use_blur=False: copy, clip, solarize
        FLAGS.reset(); FLAGS.update(aug_recipe='byol', use_blur=False)
        got = du.apply_view_plan(x, flags_lib.aug_plan(), height=H, solarize=coin)
        y = x.clamp(0, 1)
        m = (coin.t().reshape(b, 1, 1, 2, 1) != 0) & (y.reshape(b, H, H, 2, 3) >= 0.5)
        assert torch.equal(got, torch.where(m, 1.0 - y.reshape(b, H, H, 2, 3), y.reshape(b, H, H, 2, 3)).reshape(b, H, H, 6))
        # drawn coins: view a of the byol recipe is never solarized and always blurred
        FLAGS.reset(); FLAGS.update(aug_recipe='byol', blur_probs='0,0')
        drawn = du.apply_view_plan(x, flags_lib.aug_plan(), height=H)
        assert torch.equal(drawn[..., 0:3], y[..., 0:3])
    finally:
        FLAGS.reset()


def test_helper_leaves_the_local_views_as_they_are_without_coins():
    from simclr_amd import data_util as du
    from simclr_amd import flags as flags_lib
    from simclr_amd.flags import FLAGS
    g = torch.Generator().manual_seed(4)
    b, h = 4, 20
    x = (torch.rand(b, h, h, 9, generator=g) * 1.2 - 0.1).cuda()
    sigmas = [1.7, 0.4, 1.0]
    sel = (torch.rand(3, b, generator=g) < 0.5).float().cuda()
    want = du.batch_random_blur_tensor(x, h, h, sigmas=sigmas, selectors=sel)
    try:
        for recipe in ('simclr', 'byol', 'mocov2'):
            FLAGS.reset(); FLAGS.update(aug_recipe=recipe, solarize_probs='1,1')
            assert torch.equal(du.apply_view_plan(x, flags_lib.aug_plan(), local=True, sigmas=sigmas, selectors=sel), want)
        FLAGS.update(use_blur=False)
        assert du.apply_view_plan(x, flags_lib.aug_plan(), local=True) is x
    finally:
        FLAGS.reset()


# ---------------------------------------------------------------------------------------------------------------- the step
BASE = ['--dataset=synthetic', '--resnet_depth=18', '--image_size=32', '--train_batch_size=8', '--compute_dtype=f32', '--checkpoint_steps=2',
        '--train_steps=2', '--mode=train', '--proj_out_dim=64']
LOSS_ARGS = {'byol': ['--contrastive_loss=byol', '--byol_pred_hidden_dim=64'], 'barlow': ['--contrastive_loss=barlow'],
             'dino': ['--contrastive_loss=dino', '--dino_out_dim=200', '--dino_freeze_last_layer_epochs=0', '--dino_local_crops=2',
                      '--dino_local_crop_size=16']}


def _same(a, b):
    assert sorted(a['model']) == sorted(b['model'])
    assert all(torch.equal(a['model'][n], b['model'][n]) for n in a['model'])
    assert all(torch.equal(a['optimizer']['slots'][n], b['optimizer']['slots'][n]) for n in a['optimizer']['slots'])
    assert a['optimizer']['iterations'] == b['optimizer']['iterations']


@pytest.mark.parametrize('loss', ['byol', 'barlow', 'dino'])
def test_run_main_under_the_byol_recipe_ends_with_a_finite_loss(loss, capsys, monkeypatch):
    """ResNet-18 at 32 px, 8 images, synthetic data, two steps; dino with two local crops.  The new entry is what launches."""
    from simclr_amd import ops, run
    from simclr_amd.flags import FLAGS
    calls = []
    orig = ops.batch_blur

    def spy(images, filt, selector, solarize=None, threshold=0.5):
        calls.append((images.shape[3] // 3, solarize is not None))
        return orig(images, filt, selector, solarize, threshold)
    monkeypatch.setattr(ops, 'batch_blur', spy)
    FLAGS.reset()
    try:
        run.main(BASE + LOSS_ARGS[loss] + ['--aug_recipe=byol'])
    finally:
        FLAGS.reset()
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith('{') and 'train/total_loss' in l]
    assert lines and lines[-1]['step'] == 2
    for k in ('train/contrast_loss', 'train/total_loss'):
        assert math.isfinite(lines[-1][k]), (k, lines[-1])
    assert calls.count((2, True)) == 2                                 # the global views: one blur + solarize per step, for both networks
    assert calls.count((2, False)) == (2 if loss == 'dino' else 0)     # dino's two local views: the old entry, no coins
    assert len(calls) == (4 if loss == 'dino' else 2)


def test_explicit_simclr_recipe_is_bitwise_the_run_without_the_flag(tmp_path):
    """--use_blur=False and no solarization (the configuration whose resume is bitwise): two steps, the checkpoints are equal."""
    from simclr_amd import run
    from simclr_amd.flags import FLAGS
    a_dir, b_dir = str(tmp_path / 'a'), str(tmp_path / 'b')
    args = BASE + LOSS_ARGS['byol'] + ['--use_blur=False']
    try:
        FLAGS.reset()
        run.main(args + ['--model_dir=' + a_dir])
        FLAGS.reset()
        run.main(args + ['--aug_recipe=simclr', '--model_dir=' + b_dir])
    finally:
        FLAGS.reset()
    _same(torch.load(os.path.join(a_dir, 'ckpt-2.pt'), map_location='cpu'), torch.load(os.path.join(b_dir, 'ckpt-2.pt'), map_location='cpu'))


def test_fine_tuning_and_evaluation_ignore_the_recipe(tmp_path, capsys):
    from simclr_amd import run
    from simclr_amd.flags import FLAGS
    pre = str(tmp_path / 'pre')
    recipe = ['--aug_recipe=byol', '--solarize_probs=1,1', '--color_jitter_components=0.1,0.1,0.1,0.1']
    try:
        FLAGS.reset()
        run.main(BASE + LOSS_ARGS['barlow'] + ['--use_blur=False', '--model_dir=' + pre])
        ckpt = os.path.join(pre, 'ckpt-2.pt')
        written = []
        for tag, extra in (('plain', []), ('recipe', recipe)):
            FLAGS.reset()
            d = str(tmp_path / ('ft_' + tag))
            run.main(['--dataset=synthetic', '--resnet_depth=18', '--image_size=32', '--train_batch_size=8', '--compute_dtype=f32', '--mode=train',
                      '--train_mode=finetune', '--contrastive_loss=barlow', '--proj_out_dim=64', '--train_steps=1', '--checkpoint_steps=1',
                      '--checkpoint=' + ckpt, '--model_dir=' + d] + extra)
            written.append(torch.load(os.path.join(d, 'ckpt-1.pt'), map_location='cpu'))
        _same(*written)
        results = []
        for extra in ([], recipe):
            FLAGS.reset()
            results.append(run.main(['--dataset=synthetic', '--resnet_depth=18', '--image_size=32', '--eval_batch_size=8', '--eval_steps=1',
                                     '--compute_dtype=f32', '--mode=eval', '--contrastive_loss=barlow', '--proj_out_dim=64', '--model_dir=' + pre] + extra))
        # eval/regularization_loss is a float32 sum over the restored weights whose order is not fixed: two runs of the SAME command
        # differ in its last bit (2.5561820e-07 / 2.5561823e-07 seen).  It reads no image, so the recipe cannot reach it: compared at
        # 4 float32 ulps; everything an image can reach is compared exactly.
        reg = [r.pop('eval/regularization_loss') for r in results]
        assert results[0] == results[1] and results[0]['global_step'] == 2 and set(results[0]) >= {'eval/label_top_1_accuracy', 'eval/label_top_5_accuracy'}
        assert abs(reg[0] - reg[1]) <= 4 * 2.0 ** -24 * abs(reg[0])
    finally:
        FLAGS.reset()
