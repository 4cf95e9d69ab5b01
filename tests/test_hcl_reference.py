"""The float64 restatement of the hard-negative / debiased NT-Xent (tests/hcl_reference.py) against independent statements, all on the
CPU: torch float64 autograd of the direct form, the NT-Xent oracle at beta = 0 and tau_plus = 0, the cases worked on paper in
tests/golden/HCL_HAND_DERIVED.md, permutation invariance, a floor case, the error budget of the GPU cases; then the two flags, the
metric names and the refusals that precede any device work."""
import math
import re

import numpy as np
import pytest
import torch

from oracle import ntxent as ont
from tests import hcl_reference as hr
from tests.hcl_reference import hcl_reference


def _case(n, R, D, seed, corr=None):
    g = np.random.default_rng(seed)
    hs = []
    for _ in range(R):
        ha = g.standard_normal((n, D))
        hs.append(np.concatenate([ha, g.standard_normal((n, D)) if corr is None else ha + corr * g.standard_normal((n, D))]))
    return hs


def _autograd(hs, T, beta, tau_plus, hidden_norm):
    R, n = len(hs), hs[0].shape[0] // 2
    leaves = [torch.tensor(h, dtype=torch.float64, requires_grad=True) for h in hs]
    zs = [torch.nn.functional.normalize(h, dim=1) if hidden_norm else h for h in leaves]
    z_all = torch.cat([z[:n] for z in zs] + [z[n:] for z in zs], 0)
    losses = hr.hcl_direct_torch(z_all, n, T, beta, tau_plus)
    (sum(losses) / R).backward()
    return [float(l.detach()) for l in losses], [l.grad.numpy() for l in leaves]


@pytest.mark.parametrize('hidden_norm', [True, False])
@pytest.mark.parametrize('beta,tau_plus', [(0.0, 0.0), (0.5, 0.0), (0.0, 0.1), (1.0, 0.1), (2.0, 0.3)])
@pytest.mark.parametrize('n,R,D,T,corr', [(3, 1, 4, 1.0, None), (4, 2, 8, 0.1, None), (5, 3, 6, 0.5, None), (4, 2, 8, 0.2, 0.05),
                                          (3, 3, 8, 0.5, 0.3)])
def test_analytic_gradient_equals_autograd_of_the_direct_form(n, R, D, T, corr, beta, tau_plus, hidden_norm):
    hs = _case(n, R, D, n + R + D, corr)
    if not hidden_norm:
        hs = [h / np.sqrt(D) for h in hs]                    # keep exp(a s) of the direct form inside float64
    ref = hcl_reference(hs, T, beta, tau_plus, hidden_norm)
    assert hr.kink_distance(ref) >= 1e-6                   # autograd's choice on the kink itself would be arbitrary
    losses, grads = _autograd(hs, T, beta, tau_plus, hidden_norm)
    for r in range(R):
        assert abs(ref['loss'][r] - losses[r]) <= 1e-11 * max(1.0, abs(losses[r]))
        assert np.abs(ref['grads'][r] - grads[r]).max() <= 1e-10 * max(1.0, np.abs(grads[r]).max())


def test_the_autograd_cases_cover_rows_on_and_above_the_floor():
    shares = set()
    for n, R, D, T, corr in [(4, 2, 8, 0.2, 0.05), (3, 3, 8, 0.5, 0.3), (4, 2, 8, 0.1, None)]:
        for tau_plus in (0.1, 0.3):
            ref = hcl_reference(_case(n, R, D, n + R + D, corr), T, 1.0, tau_plus, True)
            shares.update(ref['on_floor'].tolist())
            mixed = 0 < ref['on_floor'].sum() < ref['on_floor'].size
            shares.add('mixed') if mixed else None
    assert shares == {True, False, 'mixed'}


@pytest.mark.parametrize('hidden_norm', [True, False])
@pytest.mark.parametrize('n,R,D,T', [(6, 1, 8, 0.1), (4, 2, 8, 1.0), (3, 3, 4, 0.5)])
def test_zero_flags_give_the_ntxent_oracle(n, R, D, T, hidden_norm):
    hs = _case(n, R, D, 11 * n + R)
    ref = hcl_reference(hs, T, 0.0, 0.0, hidden_norm)
    losses, grads = ont.contrastive_loss_and_grad(hs, hidden_norm, T)
    assert not ref['on_floor'].any()
    for r in range(R):
        assert abs(ref['loss'][r] - losses[r]) <= 1e-12 * max(1.0, abs(losses[r]))
        assert np.abs(ref['grads'][r] - grads[r]).max() <= 1e-12 * max(1.0, np.abs(grads[r]).max())


def test_restatement_equals_the_hand_derived_cases():
    """tests/golden/HCL_HAND_DERIVED.md: N = 2 (M = 2), T = 1/2 (a = 2), beta = 1, tau_plus = 1/4, hidden_norm=False."""
    e = math.e
    # case 1: every row has the negatives' dot products {0, 1/2}; the positive's is 1/2 (rows a0, b0) or -1/2 (rows a1, b1)
    h = np.array([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.5, 0.5, 0.5, 0.5], [0.5, -0.5, 0.5, -0.5]])
    assert np.array_equal(h @ h.T, np.array([[1, 0, .5, .5], [0, 1, .5, -.5], [.5, .5, 1, 0], [.5, -.5, 0, 1]]))
    ref = hcl_reference([h], 0.5, 1.0, 0.25, hidden_norm=False)
    Rr = 2.0 * (1.0 + e * e) / (1.0 + e)                                  # M A / B
    rows = {}
    for name, p in (('near', e), ('far', 1.0 / e)):
        G = (Rr - 0.5 * p) / 0.75
        assert G > 2.0 * e ** -2                                           # above the floor
        w = Rr / (0.75 * (p + G))
        rows[name] = dict(l=math.log(p + G) - math.log(p), w0=2.0 * w * (2.0 / (1.0 + e * e) - 1.0 / (1.0 + e)),
                          wh=2.0 * w * (2.0 * e * e / (1.0 + e * e) - e / (1.0 + e)), wp=2.0 * (p / 3.0 / (p + G) - 1.0))
    nr, fr = rows['near'], rows['far']
    assert abs(ref['loss'][0] - (nr['l'] + fr['l'])) < 1e-14 and ref['floor_share'] == [0.0]
    W = np.array([[0.0, nr['w0'], nr['wp'], nr['wh']], [fr['w0'], 0.0, fr['wh'], fr['wp']],
                  [nr['wp'], nr['wh'], 0.0, nr['w0']], [fr['wh'], fr['wp'], fr['w0'], 0.0]])
    assert np.abs(ref['W'] - W).max() < 1e-14
    assert np.abs(ref['grads'][0] - (W + W.T) @ h / 2.0).max() < 1e-14
    assert abs(nr['l'] - 0.9347817527) < 1e-9 and abs(fr['l'] - 2.8146725488) < 1e-9      # the decimals of the document
    assert abs(nr['wh'] - 1.7912964824) < 1e-9 and abs(fr['wp'] + 1.9600504414) < 1e-9
    # case 2: rows e1, e2, e1, e2 -- the positive's dot product is 1, both negatives' 0: G_raw < 0, every row on the floor
    h = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 0.0], [0.0, 1.0]])
    ref = hcl_reference([h], 0.5, 1.0, 0.25, hidden_norm=False)
    assert (2.0 - 0.5 * e * e) / 0.75 < 0 and ref['floor_share'] == [1.0] and ref['on_floor'].all()
    assert abs(ref['loss'][0] - 2.0 * (math.log(e * e + 2.0 * e ** -2) - 2.0)) < 1e-14
    wp = -4.0 / (e ** 4 + 2.0)
    assert np.abs(ref['grads'][0] - wp * h).max() < 1e-14
    assert abs(2.0 * (math.log(e * e + 2.0 * e ** -2) - 2.0) - 0.0719525995) < 1e-9 and abs(wp + 0.0706736881) < 1e-9


def test_a_permutation_of_the_images_permutes_the_gradient():
    n, D = 6, 8
    h = _case(n, 1, D, 5, 0.2)[0]
    a = hcl_reference([h], 0.2, 1.0, 0.1)
    perm = np.random.default_rng(1).permutation(n)
    rows = np.concatenate([perm, n + perm])
    b = hcl_reference([h[rows]], 0.2, 1.0, 0.1)
    assert abs(a['loss'][0] - b['loss'][0]) < 1e-13
    assert np.abs(a['grads'][0][rows] - b['grads'][0]).max() < 1e-13 and np.array_equal(a['on_floor'][rows], b['on_floor'])
    # two replicas holding the same global batch in another split: the same rows, the same gradients
    c = hcl_reference([np.concatenate([h[:3], h[n:n + 3]]), np.concatenate([h[3:n], h[n + 3:]])], 0.2, 1.0, 0.1)
    assert abs(0.5 * (c['loss'][0] + c['loss'][1]) - a['loss'][0]) < 1e-13
    got = np.concatenate([c['grads'][0][:3], c['grads'][1][:3], c['grads'][0][3:], c['grads'][1][3:]])
    assert np.abs(got - a['grads'][0]).max() < 1e-13


def test_on_the_floor_no_negative_carries_a_gradient():
    """Nearly identical views at T = 0.1, tau_plus = 0.1: the debiasing term exceeds the negative mass, every row sits on the floor,
    the loss no longer depends on any negative, and what is left pulls each row towards its positive only."""
    n, D = 8, 16
    h = hr.l2_normalize(_case(n, 1, D, 9, 0.01)[0])[0]
    ref = hcl_reference([h], 0.1, 0.5, 0.1, hidden_norm=False)
    assert ref['on_floor'].all() and ref['floor_share'] == [1.0]
    own, pos, neg = hr._masks(n)
    assert (ref['W'][neg] == 0).all() and (ref['W'][pos] < 0).all()
    z = h
    assert np.abs(ref['grads'][0] - (ref['W'] + ref['W'].T) @ z / n).max() < 1e-15
    moved = h.copy()
    moved[3] = -moved[3]                                     # rotate a negative of every other row
    keep = np.ones(2 * n, bool)
    keep[[3, 3 + n]] = False
    assert np.array_equal(hcl_reference([moved], 0.1, 0.5, 0.1, hidden_norm=False)['row'][keep], ref['row'][keep])


def test_every_gpu_case_keeps_its_rows_away_from_the_kink_and_its_error_budget():
    """Re-measures, per (shape, family) of tests/test_gpu_hcl.py, the smallest distance of any row to the floor over all parameter sets
    and the emulation's error against float64, against the table from which the GPU tolerances (4x) derive and its copy in
    tests/golden/HCL_HAND_DERIVED.md ("Error budget")."""
    measured, near = hr.measured_budget()
    print(measured, near)
    assert list(measured) == [(s, f) for s in hr.SHAPES for f in hr.FAMILIES] == list(hr.EMULATION_ERROR)
    table = open(__file__.replace('test_hcl_reference.py', 'golden/HCL_HAND_DERIVED.md')).read()
    for case, worst in measured.items():
        assert near[case] >= hr.KINK_MARGIN, (case, near[case])
        for k, recorded in hr.EMULATION_ERROR[case].items():
            assert 0.5 * recorded <= worst[k] <= recorded, (case, k, worst[k], recorded)
            assert hr.TOL[case][k] == 4.0 * recorded and hr.TOL[case][k] < 2e-5
        (n, R, D, rank), family = case
        row = re.search(r'^\| %d \| %d \| %d \| %d \| %s \| ([^|]*) \| ([^|]*) \|' % (n, R, D, rank, family), table, re.M)
        assert row and [float(x) for x in row.groups()] == [hr.EMULATION_ERROR[case][k] for k in ('loss', 'grad')], case
    # the cases hold what they are there for: a last tile of two rows, ragged tiles, two ranks, every width, rows on both sides
    assert any(2 * s[0] % 64 == 2 for s in hr.SHAPES) and {s[2] for s in hr.SHAPES} == {64, 128, 256} and any(s[1] > 1 for s in hr.SHAPES)
    _, ref = hr.case_reference((65, 1, 64, 0), 'independent', (0.1, 0.0, 0.1))
    assert 0 < ref['on_floor'].sum() < 130


# ---------------------------------------------------------------------------------------------------------------- flags and refusals
@pytest.fixture
def flags():
    from simclr_amd.flags import FLAGS
    FLAGS.reset()
    yield FLAGS
    FLAGS.reset()


def test_flags_parse_default_to_zero_and_switch_the_entry(flags):
    from simclr_amd import pretrain_losses, run
    assert flags.hard_negative_beta == 0.0 and flags.debiased_tau_plus == 0.0
    assert not pretrain_losses.ntxent_corrections_on() and pretrain_losses.active() is pretrain_losses.LOSSES['ntxent']
    flags.parse(['--hard_negative_beta=0.5', '--debiased_tau_plus=0.1'])
    assert (flags.hard_negative_beta, flags.debiased_tau_plus) == (0.5, 0.1)
    assert run.check_contrastive_loss_flags() is False and pretrain_losses.ntxent_corrections_on()
    spec = pretrain_losses.active()
    assert spec.call is pretrain_losses.LOSSES['ntxent'].call and spec.logits_metrics == pretrain_losses.LOSSES['ntxent'].logits_metrics
    for one in (dict(hard_negative_beta=1.0, debiased_tau_plus=0.0), dict(hard_negative_beta=0.0, debiased_tau_plus=0.05)):
        flags.update(**one)
        assert pretrain_losses.ntxent_corrections_on() and run.check_contrastive_loss_flags() is False
    # fine-tuning and evaluation ignore the two flags, whatever they hold
    flags.update(hard_negative_beta=-3.0, debiased_tau_plus=7.0, train_mode='finetune')
    assert run.check_contrastive_loss_flags() is False and not pretrain_losses.ntxent_corrections_on() and pretrain_losses.active() is None
    flags.update(train_mode='pretrain', mode='eval')
    assert run.check_contrastive_loss_flags() is False and not pretrain_losses.ntxent_corrections_on()
    assert pretrain_losses.active() is pretrain_losses.LOSSES['ntxent']


def test_the_ntxent_row_dispatches_on_the_flags(flags, monkeypatch):
    from simclr_amd import objective, pretrain_losses
    calls = []
    monkeypatch.setattr(objective, 'add_contrastive_loss', lambda *a, **kw: (calls.append(('ntxent', kw)), ('loss', 'logits', None))[1])
    monkeypatch.setattr(objective, 'add_hard_negative_contrastive_loss',
                        lambda *a, **kw: (calls.append(('hcl', kw)), ('loss2', 'logits2', None))[1])

    class C:
        outputs, strategy, overlap, logits_con = 'h', None, None, None
    c = C()
    assert pretrain_losses.LOSSES['ntxent'].call(c) == 'loss' and c.logits_con == 'logits' and calls[-1][0] == 'ntxent'
    flags.update(hard_negative_beta=0.0, debiased_tau_plus=0.0)
    assert pretrain_losses.LOSSES['ntxent'].call(c) == 'loss' and calls[-1][0] == 'ntxent'
    flags.update(hard_negative_beta=0.5, debiased_tau_plus=0.1, temperature=0.2)
    assert pretrain_losses.active().call(c) == 'loss2' and c.logits_con == 'logits2'
    assert calls[-1] == ('hcl', dict(temperature=0.2, beta=0.5, tau_plus=0.1, strategy=None, overlap=None))


def test_default_flags_build_the_metric_set_of_today(flags):
    from simclr_amd import pretrain_losses, run
    today = ['train/contrast_acc', 'train/contrast_entropy', 'train/contrast_loss', 'train/supervised_acc', 'train/supervised_loss',
             'train/total_loss', 'train/weight_decay']
    assert sorted(run.build_metrics()) == today
    flags.update(hard_negative_beta=0.0, debiased_tau_plus=0.0)
    assert sorted(run.build_metrics()) == today
    assert sorted(pretrain_losses.LOSSES) == ['barlow', 'byol', 'dino', 'generalized', 'mocov2', 'ntxent', 'supcon', 'swav', 'vicreg']
    assert pretrain_losses.LOSSES['ntxent'].metrics == (('train/contrast_loss', 'value'),)
    for one in (dict(hard_negative_beta=0.5), dict(debiased_tau_plus=0.1)):
        flags.reset()
        flags.update(**one)
        assert sorted(run.build_metrics()) == sorted(today + ['train/contrast_floor_share']) and len(run.build_metrics()) <= 16
        flags.update(train_mode='finetune')
        assert sorted(run.build_metrics()) == ['train/supervised_acc', 'train/supervised_loss', 'train/total_loss', 'train/weight_decay']


@pytest.mark.parametrize('extra,match', [
    (['--hard_negative_beta=-0.5'], 'hard_negative_beta must be >= 0 and finite'),
    (['--hard_negative_beta=inf'], 'hard_negative_beta must be >= 0 and finite'),
    (['--hard_negative_beta=nan'], 'hard_negative_beta must be >= 0 and finite'),
    (['--debiased_tau_plus=1.0'], r'debiased_tau_plus must lie in \[0, 1\)'),
    (['--debiased_tau_plus=-0.1'], r'debiased_tau_plus must lie in \[0, 1\)'),
    (['--debiased_tau_plus=nan'], r'debiased_tau_plus must lie in \[0, 1\)'),
    (['--hard_negative_beta=0.5', '--contrastive_loss=supcon'], 'needs --contrastive_loss=ntxent'),
    (['--debiased_tau_plus=0.1', '--contrastive_loss=mocov2'], 'needs --contrastive_loss=ntxent'),
    (['--debiased_tau_plus=0.1', '--contrastive_loss=barlow'], 'needs --contrastive_loss=ntxent'),
    (['--hard_negative_beta=0.5', '--hidden_norm=false'], 'need --hidden_norm=true'),
    (['--debiased_tau_plus=0.1', '--proj_out_dim=100'], 'need a loss width of 64/128/256'),
    (['--debiased_tau_plus=0.1', '--proj_out_dim=512'], 'need a loss width of 64/128/256'),
    (['--hard_negative_beta=1', '--proj_head_mode=none'], 'need a loss width of 64/128/256'),
    (['--hard_negative_beta=1', '--train_batch_size=1'], 'need --train_batch_size >= 2'),
])
def test_run_main_refuses_before_any_device_work(flags, extra, match):
    from simclr_amd import run
    with pytest.raises(ValueError, match=match):
        run.main(['--dataset=synthetic', '--train_steps=1'] + extra)


def test_value_errors_of_the_entry_points_before_any_device_work():
    from simclr_amd import objective, ops
    with pytest.raises(ValueError, match='64/128/256'):
        objective.add_hard_negative_contrastive_loss(torch.zeros(8, 100), 0.1, 0.5, 0.1)
    for T, beta, tau_plus in ((0.0, 0.5, 0.1), (0.1, -1.0, 0.1), (0.1, float('inf'), 0.1), (0.1, 0.5, 1.0), (0.1, 0.5, float('nan')),
                              (float('nan'), 0.5, 0.1)):
        with pytest.raises(ValueError, match='need temperature > 0, beta >= 0 and finite, tau_plus in'):
            objective.add_hard_negative_contrastive_loss(torch.zeros(8, 128), T, beta, tau_plus)
    with pytest.raises(ValueError, match='N = R\\*n >= 2'):
        ops.hcl_fwd(torch.zeros(2, 64), torch.zeros(2, 64), 0, 0.1, 0.5, 0.1)
    with pytest.raises(ValueError, match='N = R\\*n >= 2'):
        ops.hcl_fwd(torch.zeros(8, 64), torch.zeros(12, 64), 0, 0.1, 0.5, 0.1)
    with pytest.raises(ValueError, match='64/128/256'):
        ops.hcl_bwd(torch.zeros(8, 512), torch.zeros(8, 512), 0, 0.1, 0.5, 0.1, None, 1.0, None)


def test_the_library_refuses_bad_arguments_without_a_device():
    """Every refusal of simclr_hcl_fwd / _bwd returns 1 before anything is launched: null pointers stand in for the tensors."""
    import ctypes
    from simclr_amd._lib import SimclrHipError, lib
    L = lib()
    f = ctypes.c_float
    fake = ctypes.c_void_p(1 << 20)                          # aligned, never dereferenced: every call below is refused first
    for kw, match in ((dict(D=100), 'D must be 64/128/256'), (dict(n=0), 'n >= 1'), (dict(n=1, N=1), 'N >= 2'), (dict(n=4, N=6), 'N = R\\*n'),
                      (dict(n=4, N=8, rank=2), 'rank 2 out of range'), (dict(T=0.0), 'temperature'), (dict(T=float('nan')), 'temperature'),
                      (dict(beta=-1.0), 'beta'), (dict(beta=float('inf')), 'beta'), (dict(beta=float('nan')), 'beta'),
                      (dict(tau=1.0), 'tau_plus'), (dict(tau=-0.5), 'tau_plus'), (dict(tau=float('nan')), 'tau_plus'),
                      (dict(ptr=None), 'null or misaligned'), (dict(ptr=ctypes.c_void_p((1 << 20) + 4)), 'null or misaligned')):
        a = dict(dict(n=4, N=4, D=128, rank=0, T=0.1, beta=0.5, tau=0.1, ptr=fake), **kw)
        if 'ptr' not in kw:
            a['ptr'] = None                                  # the scalar checks come first: nothing is touched
        with pytest.raises(SimclrHipError, match=match):
            L.hcl_fwd(a['ptr'], fake, a['n'], a['N'], a['D'], a['rank'], f(a['T']), f(a['beta']), f(a['tau']), fake, fake, fake, None)
        with pytest.raises(SimclrHipError, match=match):
            L.hcl_bwd(fake, fake, a['n'], a['N'], a['D'], a['rank'], f(a['T']), f(a['beta']), f(a['tau']), fake, f(1.0), a['ptr'], fake, fake,
                      None)
    assert L.hcl_workspace_bytes(4, 4, 100) == 0 and L.hcl_workspace_bytes(1, 1, 64) == 0 and L.hcl_workspace_bytes(4, 6, 64) == 0
    assert L.hcl_workspace_bytes(512, 512, 128) > 0 and L.hcl_workspace_bytes(1, 2, 64) > 0
