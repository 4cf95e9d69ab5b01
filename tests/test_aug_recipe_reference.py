"""CPU tests of the augmentation recipes (flags.aug_plan), of the parameter and selector draws behind them (data_util, data.py) and
of the references of tests/test_gpu_aug_recipe.py (tests/aug_recipe_reference.py): exactness of the solarization rule, the recorded
tolerance, the threshold guard and the five mutants the comparator rejects.  No GPU."""
import math

import numpy as np
import pytest
import torch

from simclr_amd import data as data_lib
from simclr_amd import data_util as du
from simclr_amd import flags as flags_lib
from simclr_amd.flags import FLAGS
from tests import aug_recipe_reference as R
from tests import augment_reference as ar
from tests.data_fixtures import make_dataset

F32, F64 = np.float32, np.float64
SIMCLR = ('simclr', True, (0.5, 0.5), (0.0, 0.0), 0.5, (0.8, 0.8, 0.8, 0.2))


@pytest.fixture(autouse=True)
def _reset_flags():
    FLAGS.reset()
    yield
    FLAGS.reset()


# ---------------------------------------------------------------------------------------------------------------- recipes and refusals
def test_recipes_resolve():
    assert tuple(flags_lib.aug_plan()) == SIMCLR                                      # FLAGS.reset(): the simclr plan
    FLAGS.update(aug_recipe='simclr')
    assert tuple(flags_lib.aug_plan()) == SIMCLR
    FLAGS.update(aug_recipe='byol')
    assert tuple(flags_lib.aug_plan()) == ('byol', True, (1.0, 0.1), (0.0, 0.2), 0.5, (0.4, 0.4, 0.2, 0.1))
    FLAGS.update(aug_recipe='mocov2')
    assert tuple(flags_lib.aug_plan()) == ('mocov2', True, (0.5, 0.5), (0.0, 0.0), 0.5, (0.4, 0.4, 0.4, 0.1))
    FLAGS.reset()
    assert tuple(flags_lib.aug_plan()) == SIMCLR


@pytest.mark.parametrize('recipe', ['simclr', 'byol', 'mocov2'])
def test_an_explicit_flag_overrides_its_column_only(recipe):
    FLAGS.update(aug_recipe=recipe)
    base = flags_lib.aug_plan()
    FLAGS.update(blur_probs='0.25,0.75')
    assert flags_lib.aug_plan() == base._replace(blur_probs=(0.25, 0.75))
    FLAGS.update(blur_probs=None, solarize_probs='1,0.5')
    assert flags_lib.aug_plan() == base._replace(solarize_probs=(1.0, 0.5))
    FLAGS.update(solarize_probs=None, solarize_threshold=0.25)
    assert flags_lib.aug_plan() == base._replace(solarize_threshold=0.25)
    FLAGS.update(solarize_threshold=0.5, color_jitter_components='0.1, 0.2,0.3,0.5')
    assert flags_lib.aug_plan() == base._replace(jitter_components=(0.1, 0.2, 0.3, 0.5))
    FLAGS.update(color_jitter_components=None, use_blur=False)                       # zeroes the blur, leaves the rest
    assert flags_lib.aug_plan() == base._replace(use_blur=False, blur_probs=(0.0, 0.0))


def test_flags_parse_from_the_command_line():
    FLAGS.parse(['--aug_recipe=byol', '--blur_probs=1,0', '--solarize_probs', '0,1', '--solarize_threshold=0.75',
                 '--color_jitter_components=0.4,0.4,0.4,0.1'])
    assert tuple(flags_lib.aug_plan()) == ('byol', True, (1.0, 0.0), (0.0, 1.0), 0.75, (0.4, 0.4, 0.4, 0.1))


@pytest.mark.parametrize('kw,flag', [
    (dict(aug_recipe='dino'), 'aug_recipe'), (dict(aug_recipe=''), 'aug_recipe'),
    (dict(blur_probs='0.5'), 'blur_probs'), (dict(blur_probs='0.5,0.5,0.5'), 'blur_probs'), (dict(blur_probs='0.5,x'), 'blur_probs'),
    (dict(blur_probs='0.5,1.5'), 'blur_probs'), (dict(blur_probs='-0.1,0.5'), 'blur_probs'), (dict(blur_probs='nan,0.5'), 'blur_probs'),
    (dict(solarize_probs='0.2'), 'solarize_probs'), (dict(solarize_probs='a,b'), 'solarize_probs'),
    (dict(solarize_probs='0,1.01'), 'solarize_probs'), (dict(solarize_probs='0,nan'), 'solarize_probs'),
    (dict(solarize_threshold=1.5), 'solarize_threshold'), (dict(solarize_threshold=-0.1), 'solarize_threshold'),
    (dict(solarize_threshold=float('nan')), 'solarize_threshold'),
    (dict(color_jitter_components='0.4,0.4,0.4'), 'color_jitter_components'), (dict(color_jitter_components='0.4,0.4,0.4,z'), 'color_jitter_components'),
    (dict(color_jitter_components='-0.4,0.4,0.4,0.1'), 'color_jitter_components'), (dict(color_jitter_components='0.4,nan,0.4,0.1'), 'color_jitter_components'),
    (dict(color_jitter_components='0.4,0.4,0.4,nan'), 'color_jitter_components'), (dict(color_jitter_components='0.4,0.4,0.4,0.6'), 'color_jitter_components'),
])
def test_refusals_name_the_flag(kw, flag):
    FLAGS.update(**kw)
    with pytest.raises(ValueError, match='--' + flag):
        flags_lib.aug_plan()


def test_run_main_refuses_before_any_device_work(monkeypatch):
    from simclr_amd import run

    def no_device(*a, **k):
        raise AssertionError('device work before the flag check')
    monkeypatch.setattr(run, 'init_distributed', no_device)
    for bad, flag in (('--aug_recipe=swav', 'aug_recipe'), ('--blur_probs=2,0', 'blur_probs'), ('--solarize_probs=0.2', 'solarize_probs'),
                      ('--solarize_threshold=1.5', 'solarize_threshold'), ('--color_jitter_components=0.4,0.4,0.4,0.9', 'color_jitter_components')):
        FLAGS.reset()
        with pytest.raises(ValueError, match='--' + flag):
            run.main(['--dataset=synthetic', '--train_steps=1', bad])


def test_fine_tuning_and_evaluation_do_not_read_the_flags():
    FLAGS.update(aug_recipe='byol', blur_probs='7', solarize_threshold=9.0, train_mode='finetune')
    assert tuple(flags_lib.aug_plan()) == SIMCLR
    FLAGS.update(train_mode='pretrain', mode='eval')
    assert tuple(flags_lib.aug_plan()) == SIMCLR
    FLAGS.update(mode='train_then_eval', blur_probs=None, solarize_threshold=0.5)
    assert flags_lib.aug_plan().recipe == 'byol'
    FLAGS.update(contrastive_loss='byol', aug_recipe='simclr')                       # the loss switches nothing on
    assert tuple(flags_lib.aug_plan()) == SIMCLR


def test_new_entry_refuses_without_a_device():
    """The argument checks of simclr_batch_blur_solarize come before any launch (the GPU test repeats them with real buffers)."""
    import ctypes
    from simclr_amd import _lib
    L = _lib.lib()
    assert 'simclr_batch_blur_solarize' in L.signatures and L.abi_version() == 8
    fake = [ctypes.c_void_p(1 << 20)] * 6                            # never dereferenced: every call below is refused
    for i in range(6):
        with pytest.raises(_lib.SimclrHipError, match='null argument'):
            L.batch_blur_solarize(*(fake[:i] + [None] + fake[i + 1:]), 0.5, 2, 4, 4, 2, 3, None)
    for K in (2, 0, -1):
        with pytest.raises(_lib.SimclrHipError, match='K must be odd'):
            L.batch_blur_solarize(*fake, 0.5, 2, 4, 4, 2, K, None)
    for t in (-0.5, 1.5, float('nan')):
        with pytest.raises(_lib.SimclrHipError, match='threshold must lie in'):
            L.batch_blur_solarize(*fake, t, 2, 4, 4, 2, 3, None)


# ---------------------------------------------------------------------------------------------------------------- parameter draws
def _draw(strength, comp, seed=5, **kw):
    rng = np.random.default_rng(seed)
    hs, ws = np.arange(20, 36), np.arange(40, 24, -1)
    return du.draw_train_params(16, hs, ws, 24, 24, strength, rng=rng, jitter_components=comp, **kw).reshape(-1, 16)


@pytest.mark.parametrize('strength', [0.5, 1.0, 1.5])
def test_default_components_are_bitwise_the_explicit_table(strength):
    none, explicit = _draw(strength, None), _draw(strength, (0.8, 0.8, 0.8, 0.2))
    assert none.tobytes() == explicit.tobytes()
    s = strength                                                    # today's expressions, spelt out
    rng = np.random.default_rng(5)
    du.sample_crop_boxes(rng, np.repeat(np.arange(20, 36), 2), np.repeat(np.arange(40, 24, -1), 2), 24, 24)
    rng.random(32); rng.random(32); rng.random((32, 4))
    want = np.stack([rng.uniform(max(1.0 - 0.8 * s, 0.0), 1.0 + 0.8 * s, 32), rng.uniform(1 - 0.8 * s, 1 + 0.8 * s, 32),
                     rng.uniform(1 - 0.8 * s, 1 + 0.8 * s, 32), rng.uniform(-0.2 * s, 0.2 * s, 32)], 1).astype(F32)
    assert none[:, 10:14].tobytes() == want.tobytes()


@pytest.mark.parametrize('strength', [0.5, 1.0, 1.5])
def test_byol_components_move_the_four_factor_columns_only(strength):
    comp = (0.4, 0.4, 0.2, 0.1)
    a, b = _draw(strength, None), _draw(strength, comp)
    rest = [c for c in range(16) if c not in (10, 11, 12, 13)]
    assert a[:, rest].tobytes() == b[:, rest].tobytes()
    eps = 1e-6
    for col, c in zip((10, 11, 12), comp):
        lo, hi = 1 - c * strength, 1 + c * strength
        assert (b[:, col] >= max(lo, 0.0) - eps).all() and (b[:, col] <= hi + eps).all(), col
        assert b[:, col].min() < lo + 0.3 * (hi - lo) and b[:, col].max() > hi - 0.3 * (hi - lo)          # and fill them
    assert (np.abs(b[:, 13]) <= 0.1 * strength + eps).all() and np.abs(b[:, 13]).max() > 0.05 * strength
    assert not np.array_equal(a[:, 10:14], b[:, 10:14])


def test_local_params_forward_the_components():
    kw = dict(b=8, heights=40, widths=50, size=16, views=3, min_scale=0.05, max_scale=0.14)
    a = du.draw_local_params(rng=np.random.default_rng(3), **kw)
    b = du.draw_local_params(rng=np.random.default_rng(3), jitter_components=(0.8, 0.8, 0.8, 0.2), **kw)
    c = du.draw_local_params(rng=np.random.default_rng(3), jitter_components=(0.4, 0.4, 0.2, 0.1), **kw)
    assert a.tobytes() == b.tobytes() and a.shape == (8, 3, 16)
    assert np.array_equal(a[..., :10], c[..., :10]) and np.array_equal(a[..., 14:], c[..., 14:]) and not np.array_equal(a[..., 10:14], c[..., 10:14])
    assert (np.abs(c[..., 12] - 1) <= 0.2 + 1e-6).all()


@pytest.fixture(scope='module')
def split(tmp_path_factory):
    d = str(tmp_path_factory.mktemp('aug_recipe_data'))
    make_dataset(d, splits=(('train', 37),))
    return data_lib.ArrayDatasetBuilder('waves', d).split('train')


def _plans(split, steps=(0, 3), **flags):
    FLAGS.reset()
    FLAGS.update(contrastive_loss='dino', dino_local_crops=2, dino_local_crop_size=16, **flags)
    it = data_lib.DatasetIterator(split, 10, 8, True, device=None, image_size=32, train_mode='pretrain')
    out = [(it.plan(s), it.local_plan(s)) for s in steps]
    it.close() if hasattr(it, 'close') else None
    return out


def test_dataset_plan_under_explicit_simclr_is_the_plan_without_flags(split):
    for ((ia, wa, pa), la), ((ib, wb, pb), lb) in zip(_plans(split), _plans(split, aug_recipe='simclr')):
        assert np.array_equal(ia, ib) and wa.tobytes() == wb.tobytes() and pa.tobytes() == pb.tobytes() and la.tobytes() == lb.tobytes()


def test_dataset_plan_under_byol_differs_in_the_factor_columns_only(split):
    rest = [c for c in range(16) if c not in (10, 11, 12, 13)]
    for ((ia, wa, pa), la), ((ib, wb, pb), lb) in zip(_plans(split), _plans(split, aug_recipe='byol')):
        assert np.array_equal(ia, ib) and wa.tobytes() == wb.tobytes()
        for a, b in ((pa, pb), (la, lb)):                            # the local views take the recipe's components too
            assert a[..., rest].tobytes() == b[..., rest].tobytes()
            assert not np.array_equal(a[..., 10:14], b[..., 10:14])
            on = b[..., 5] > 0
            assert (np.abs(b[..., 12] - 1)[on] <= 0.2 + 1e-6).all() and (np.abs(b[..., 13])[on] <= 0.1 + 1e-6).all()


# ---------------------------------------------------------------------------------------------------------------- selector draws
class _Recorder:
    def __init__(self):
        self.calls = []

    def __call__(self, images, filt, selector, solarize=None, threshold=0.5):
        self.calls.append(dict(filt=filt, selector=selector, solarize=solarize, threshold=threshold))
        return images


@pytest.fixture
def blur_calls(monkeypatch):
    """data_util on the CPU: its generator is a seeded CPU one and ops.batch_blur records what it is handed (no kernel runs)."""
    rec = _Recorder()
    gen = torch.Generator().manual_seed(1234)
    monkeypatch.setattr(du.ops, 'batch_blur', rec)
    monkeypatch.setattr(du, '_generator', lambda dev: gen)
    rec.gen = gen
    return rec


def test_probability_one_selects_all_and_zero_none(blur_calls):
    x = torch.zeros(64, 20, 20, 6)
    du.batch_random_blur_tensor(x, 20, 20, blur_probability=(1.0, 0.0), solarize_probability=(0.0, 1.0))
    c = blur_calls.calls[0]
    assert c['selector'].shape == (2, 64) and bool(c['selector'][0].all()) and not bool(c['selector'][1].any())
    assert not bool(c['solarize'][0].any()) and bool(c['solarize'][1].all())
    du.batch_random_blur_tensor(x, 20, 20, blur_probability=1.0)
    assert bool(blur_calls.calls[1]['selector'].all()) and blur_calls.calls[1]['solarize'] is None
    du.batch_random_blur_tensor(x, 20, 20, blur_probability=0.0)
    assert not bool(blur_calls.calls[2]['selector'].any())


def test_byol_shares_at_4096(blur_calls):
    b = 4096
    x = torch.zeros(b, 1, 1, 6)
    du.batch_random_blur_tensor(x, 20, 20, blur_probability=(1.0, 0.1), solarize_probability=(0.0, 0.2), threshold=0.25)
    c = blur_calls.calls[0]
    assert float(c['selector'][0].mean()) == 1.0 and float(c['solarize'][0].sum()) == 0.0 and c['threshold'] == 0.25
    for share, p in ((float(c['selector'][1].mean()), 0.1), (float(c['solarize'][1].mean()), 0.2)):
        assert abs(share - p) <= 6.0 * math.sqrt(p * (1 - p) / b), (share, p)
    assert set(c['selector'].unique().tolist()) <= {0.0, 1.0} and c['solarize'].dtype == torch.float32


def test_draw_order_is_sigmas_selectors_coins(blur_calls):
    x = torch.zeros(5, 20, 20, 6)
    du.batch_random_blur_tensor(x, 20, 20, blur_probability=(0.7, 0.3), solarize_probability=(0.0, 0.5))
    g = torch.Generator().manual_seed(1234)
    sig = 0.1 + 1.9 * torch.rand(2, generator=g)
    sel = (torch.rand(2, 5, generator=g) < torch.tensor([[0.7], [0.3]])).float()
    coin = (torch.rand(2, 5, generator=g) < torch.tensor([[0.0], [0.5]])).float()
    c = blur_calls.calls[0]
    assert torch.equal(c['filt'], du.gaussian_filter(2, sig)) and torch.equal(c['selector'], sel) and torch.equal(c['solarize'], coin)


def test_default_call_consumes_the_generator_as_before(blur_calls):
    x = torch.zeros(7, 20, 20, 6)
    nxt = []
    for kw in (dict(), dict(solarize_probability=0.0, solarize=None, threshold=0.5), dict(solarize_probability=(0.0, 0.0))):
        blur_calls.gen.manual_seed(99)
        du.batch_random_blur_tensor(x, 20, 20, **kw)
        nxt.append(torch.rand(4, generator=blur_calls.gen))
        assert blur_calls.calls[-1]['solarize'] is None                         # and the old entry is the one that launches
    g = torch.Generator().manual_seed(99)                                      # today's two draws, spelt out
    torch.rand(2, generator=g); torch.rand(2, 7, generator=g)
    want = torch.rand(4, generator=g)
    assert all(torch.equal(n, want) for n in nxt)
    assert torch.equal(blur_calls.calls[0]['selector'], blur_calls.calls[1]['selector'])
    blur_calls.gen.manual_seed(99)
    du.batch_random_blur_tensor(x, 20, 20, solarize_probability=(0.0, 0.2))     # coins on: one more draw
    assert not torch.equal(torch.rand(4, generator=blur_calls.gen), want)


def test_helper_applies_the_plan(blur_calls):
    x = torch.zeros(6, 20, 20, 6)
    plan = flags_lib.aug_plan()
    # simclr: the call of a run without the flags, draw for draw
    blur_calls.gen.manual_seed(7)
    assert du.apply_view_plan(x, plan, height=20) is x
    a = blur_calls.calls[-1]
    blur_calls.gen.manual_seed(7)
    du.batch_random_blur_tensor(x, 20, 20)
    b = blur_calls.calls[-1]
    assert a['solarize'] is None and torch.equal(a['selector'], b['selector']) and torch.equal(a['filt'], b['filt'])
    # --use_blur=False without solarization: nothing is drawn or launched
    n = len(blur_calls.calls)
    FLAGS.update(use_blur=False)
    blur_calls.gen.manual_seed(7)
    assert du.apply_view_plan(x, flags_lib.aug_plan()) is x and du.apply_view_plan(x, flags_lib.aug_plan(), local=True) is x
    assert len(blur_calls.calls) == n and torch.equal(torch.rand(1, generator=blur_calls.gen), torch.rand(1, generator=torch.Generator().manual_seed(7)))
    # --use_blur=False under byol: a 1-tap filter, zero selectors, coins for view b only, no sigma and no selector drawn
    FLAGS.update(aug_recipe='byol', solarize_probs='0,1', solarize_threshold=0.75)
    blur_calls.gen.manual_seed(7)
    du.apply_view_plan(x, flags_lib.aug_plan())
    c = blur_calls.calls[-1]
    assert c['filt'].tolist() == [[1.0], [1.0]] and not bool(c['selector'].any()) and c['threshold'] == 0.75
    assert c['solarize'].tolist() == [[0.0] * 6, [1.0] * 6]
    g = torch.Generator().manual_seed(7)
    torch.rand(2, 6, generator=g)
    assert torch.equal(torch.rand(1, generator=blur_calls.gen), torch.rand(1, generator=g))
    # byol: per-view probabilities for the global views; the local views keep 0.5 and take no coins
    FLAGS.reset(); FLAGS.update(aug_recipe='byol')
    du.apply_view_plan(torch.zeros(512, 1, 1, 6), flags_lib.aug_plan(), height=20)
    c = blur_calls.calls[-1]
    assert float(c['selector'][0].mean()) == 1.0 and 0.02 < float(c['selector'][1].mean()) < 0.2
    assert float(c['solarize'][0].sum()) == 0.0 and 0.1 < float(c['solarize'][1].mean()) < 0.3
    du.apply_view_plan(torch.zeros(512, 1, 1, 9), flags_lib.aug_plan(), height=20, local=True)
    c = blur_calls.calls[-1]
    assert c['solarize'] is None and c['selector'].shape == (3, 512) and all(0.4 < float(r.mean()) < 0.6 for r in c['selector'])
    with pytest.raises(ValueError, match='--blur_probs'):                      # two probabilities, three global views
        du.apply_view_plan(torch.zeros(4, 1, 1, 9), flags_lib.aug_plan(), height=20)


# ---------------------------------------------------------------------------------------------------------------- exactness
def test_one_minus_v_is_exact_at_and_above_one_half():
    """v in [0.5, 1] has ulp >= 2^-24 and 1 - v in [0, 0.5] is a multiple of it: Sterbenz.  Sampled densely, and at the ends."""
    rng = np.random.default_rng(0)
    v = np.concatenate([rng.uniform(0.5, 1.0, 200000).astype(F32), np.asarray([0.5, 1.0, np.nextafter(F32(0.5), F32(1)), np.nextafter(F32(1), F32(0))], F32)])
    v = v[v >= F32(0.5)]
    assert np.array_equal((F32(1) - v).astype(F64), 1.0 - v.astype(F64))


def test_one_minus_v_rounds_once_below_one_half():
    rng = np.random.default_rng(1)
    v = rng.uniform(0.25, 0.5, 200000).astype(F32)
    got, want = (F32(1) - v).astype(F64), 1.0 - v.astype(F64)
    assert not np.array_equal(got, want)                                             # it does round ...
    assert np.abs(got - want).max() <= 2.0 ** -25                                    # ... once: half an ulp of (0.5, 1]
    assert np.array_equal(got, want.astype(F32).astype(F64))


@pytest.mark.parametrize('c', R.exact_cases(), ids=lambda c: 't%g' % c['t'])
def test_exact_case_is_exact_and_holds_the_threshold(c):
    want = R.expected_exact(c)
    assert np.array_equal(want.astype(F64), R.oracle(c)) and np.array_equal(R.emulate(c, F32), want)
    x = np.clip(c['blur']['x'], F32(0), F32(1))
    at = (x == F32(c['t'])) & R._coin_mask(c)
    assert at.sum() >= 10 and (want[at] == F32(1 - c['t'])).all()                    # elements AT the threshold invert
    assert ((x == F32(c['t'])) & ~R._coin_mask(c)).sum() >= 10                       # and stay where the coin is not set
    assert set(np.unique(x * 64).astype(int).tolist()) == set(range(65))
    if c['t'] == 0.0:
        raw = c['blur']['x']
        assert ((raw < 0) & R._coin_mask(c)).sum() >= 10 and ((raw > 1) & R._coin_mask(c)).sum() >= 10     # pixels the clip moves


def test_float64_emulation_is_the_oracle():
    for c in R.cases(7, 9, 7) + R.cases(40, 3, 40):
        assert np.abs(R.emulate(c, F64) - R.oracle(c)).max() < 1e-14, c['name']


def test_tolerance_comes_from_the_float32_emulation():
    """Re-measured: 4 x the float32 emulation's worst error against float64 over the GPU cases (tests/golden/AUG_RECIPE.md)."""
    m = R.measured_e32()
    worst = max(m, key=lambda n: m[n][0])
    left_out = sum(v[1] for v in m.values())
    numel = sum(c['blur']['x'].size for c in R.all_cases())
    print('E32 solarize measured %.4e (%s) recorded %.4e tolerance %.4e; %d of %d elements on different branches left out'
          % (m[worst][0], worst, R.E32_RECORDED, R.tolerance(), left_out, numel))
    assert len(m) == 720
    assert abs(m[worst][0] / R.E32_RECORDED - 1) < 0.1                               # the blur's filter goes through exp: 10 % for another libm
    assert R.tolerance() == 4 * R.E32_RECORDED
    assert left_out <= 1e-4 * numel
    for t in R.THRESHOLDS:                                                           # the solarize step adds at most half an ulp of (0.5, 1]
        e = max(m[c['name']][0] for c in R.all_cases() if c['t'] == t)
        assert e <= ar.E32_RECORDED['blur'] * 1.1 + 2.0 ** -25, (t, e)


# ---------------------------------------------------------------------------------------------------------------- the comparator
def _ok(results):
    return all(r['ok'] for r in results)


def test_every_case_stays_under_the_guard_cap():
    shares = [R.guard_share(c, R.tolerance()) for c in R.all_cases()]
    print('threshold guard: largest share %.3e, cases with a guarded element %d of %d' % (max(shares), sum(s > 0 for s in shares), len(shares)))
    assert max(shares) <= R.GUARD_CAP
    assert all(R.guard_share(c, R.tolerance()) == 0.0 for c in R.all_cases() if c['t'] == 0.5)
    assert all(R.guard_share(c, R.tolerance()) == 0.0 for c in R.exact_cases())       # an exact case has no guard


def test_comparator_accepts_the_float32_emulation_on_every_case():
    for c in R.all_cases() + R.exact_cases():
        assert _ok(R.compare(R.emulate(c, F32), c, R.tolerance())), c['name']


def test_guard_leaves_out_elements_at_the_threshold_only():
    """A hand-made case: nothing blurred, one element of a solarized image 2e-7 above t = 0.25, one 1e-5 above.  The other branch
    passes at the first and fails at the second; it fails at the first when the coin is not set, and at t = 0.5 there is no guard."""
    tol = R.tolerance()
    x = np.full((2, 8, 8, 3), 0.6, F32)
    x[0, 0, 0, 0] = F32(0.25 + 2e-7)
    x[0, 1, 1, 1] = F32(0.25 + 1e-5)
    x[1, 0, 0, 0] = F32(0.25 + 2e-7)
    base = dict(name='guard', stage='blur', x=x, height=10, sigmas=(1.0,), sel=np.zeros((1, 2), F32))
    c = dict(name='guard', blur=base, coin=np.asarray([[1, 0]], F32), t=0.25, exact=False)
    ref = R.oracle(c)
    assert ref[0, 0, 0, 0] == pytest.approx(0.75, abs=1e-6) and ref[1, 0, 0, 0] == pytest.approx(0.25, abs=1e-6)
    assert R.guard(c, tol).sum() == 1 and _ok(R.compare(ref.astype(F32), c, tol))
    got = ref.astype(F32).copy(); got[0, 0, 0, 0] = x[0, 0, 0, 0]                     # the other branch inside the band
    assert _ok(R.compare(got, c, tol))
    got = ref.astype(F32).copy(); got[0, 1, 1, 1] = x[0, 1, 1, 1]                     # the other branch outside it
    assert not _ok(R.compare(got, c, tol))
    got = ref.astype(F32).copy(); got[1, 0, 0, 0] = F32(0.75)                         # an image whose coin is not set
    assert not _ok(R.compare(got, c, tol))
    got = ref.astype(F32).copy(); got[0, 0, 0, 0] = F32(0.5)                          # inside the band, but neither branch
    assert not _ok(R.compare(got, c, tol))
    many = dict(name='guard all', blur=dict({k: v for k, v in base.items() if k != '_ref'}, x=np.full((2, 8, 8, 3), F32(0.25 + 2e-7), F32)), coin=c['coin'], t=0.25, exact=False)
    assert R.guard_share(many, tol) == 0.5                                           # every element of image 0 guarded: over the cap
    assert not _ok(R.compare(R.oracle(many).astype(F32), many, tol))


@pytest.mark.parametrize('name', R.MUTANTS)
def test_comparator_rejects_mutant(name):
    pool = R.all_cases() + R.exact_cases()
    caught = [c['name'] for c in pool if not _ok(R.compare(R.mutant(c, name).astype(F32), c, R.tolerance()))]
    print('%s: caught by %d cases, e.g. %s' % (name, len(caught), caught[:3]))
    assert caught
    exact = [c['name'] for c in R.exact_cases()]
    if name == 'gt':
        assert caught == exact                                                       # only exact equality tells > from >=
    if name == 'before_clip':
        assert caught == exact[1:]                                                   # observable at t = 0 only (dyadic_case's docstring)
