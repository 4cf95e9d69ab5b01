"""NNCLR without a GPU: tests/nnclr_reference.py against torch float64 autograd (the neighbour rows detached), against a cross-view
NT-Xent restatement, against the cases worked on paper in tests/golden/NNCLR_HAND_DERIVED.md; the search's tie rule, the ring position,
every start-up refusal, the metric names, and the error budget the gates of tests/test_gpu_nnclr.py are 4 x of."""
import numpy as np
import pytest
import torch

from tests import nnclr_reference as nr


def _views(n, R, D, seed):
    g = np.random.default_rng(seed)
    return [nr.l2_normalize(g.standard_normal((2 * n, D)))[0] for _ in range(R)]


def _queue(K, D, seed):
    return nr.l2_normalize(np.random.default_rng(1000 + seed).standard_normal((K, D)))[0]


# ---------------------------------------------------------------------------------------------------------------- gradient
@pytest.mark.parametrize('n,R,D,K,T', [(3, 1, 8, 7, 0.5), (4, 2, 8, 16, 0.2), (2, 3, 16, 5, 1.0), (5, 3, 8, 40, 0.1)])
def test_analytic_gradient_equals_autograd_with_detached_neighbours(n, R, D, K, T):
    zs, S = _views(n, R, D, 10 * n + R), _queue(K, D, n)
    ref = nr.nnclr_reference(zs, S, T)
    leaves = [torch.tensor(z, dtype=torch.float64, requires_grad=True) for z in zs]
    z_all = torch.cat([z[:n] for z in leaves] + [z[n:] for z in leaves], 0)
    St = torch.from_numpy(S)
    nn_rows = [St[torch.from_numpy(i)] for i in ref['nn_index']]                     # constants: no path back to z
    losses = nr.nnclr_direct_torch(z_all, nn_rows, n, T)
    for q in range(R):
        assert abs(float(losses[q].detach()) - ref['loss'][q]) <= 1e-12 * abs(ref['loss'][q])
    (sum(losses) / R).backward()
    for q in range(R):
        assert np.abs(leaves[q].grad.numpy() - ref['grads'][q]).max() <= 1e-12
    # the per-replica partial: d loss_q / d z_all
    for q in range(R):
        za = z_all.detach().clone().requires_grad_(True)
        nr.nnclr_direct_torch(za, nn_rows, n, T)[q].backward()
        assert np.abs(za.grad.numpy() - ref['partial'][q]).max() <= 1e-12
    # there is no row-side term: the sum of the partials over the replicas is the whole gradient of the objective
    assert all(np.isfinite(g).all() for g in ref['grads'])


def test_the_gradient_differs_from_autograd_through_a_soft_neighbour():
    """A neighbour that is NOT detached -- the softmax-weighted mean of the queue rows, renormalised -- gives the same loss value as
    the same rows detached, and another gradient: the rows then carry a term of their own.  So the test above can tell a detached
    neighbour from an attached one; the definition has the detached one."""
    n, D, K, T = 4, 8, 12, 0.5
    zs, S = _views(n, 1, D, 3), _queue(K, D, 3)
    St = torch.from_numpy(S)
    grads, values = [], []
    for detach in (True, False):
        z = torch.tensor(zs[0], dtype=torch.float64, requires_grad=True)
        soft = torch.softmax((z @ St.T) / 0.1, dim=1) @ St
        soft = soft / soft.norm(dim=1, keepdim=True)
        loss = nr.nnclr_direct_torch(z, [soft.detach() if detach else soft], n, T)[0]
        loss.backward()
        grads.append(z.grad.numpy())
        values.append(float(loss.detach()))
    assert values[0] == values[1]
    assert np.abs(grads[0] - grads[1]).max() > 1e-2 * np.abs(grads[0]).max()
    # and with the hard neighbour the detached form is the reference's
    ref = nr.nnclr_reference(zs, S, T)
    z = torch.tensor(zs[0], dtype=torch.float64, requires_grad=True)
    nr.nnclr_direct_torch(z, [St[torch.from_numpy(ref['nn_index'][0])]], n, T)[0].backward()
    assert np.abs(z.grad.numpy() - ref['grads'][0]).max() <= 1e-12


# ---------------------------------------------------------------------------------------------------------------- hand-derived cases
def test_restatement_equals_the_hand_derived_cases():
    """tests/golden/NNCLR_HAND_DERIVED.md, cases 1 and 2."""
    # case 1: D = 2, n = N = 2, T = 1, both views on the axes, the queue the two axes
    e1, e2 = [1.0, 0.0], [0.0, 1.0]
    ref = nr.nnclr_reference([np.array([e1, e2, e1, e2])], np.array([e1, e2]), 1.0)
    assert list(ref['nn_index'][0]) == [0, 1, 0, 1]
    assert abs(ref['loss'][0] - 2.0 * np.log1p(np.exp(-1.0))) < 1e-14 and abs(ref['loss'][0] - 0.6265233) < 1e-7
    assert ref['acc'][0] == 1.0 and ref['nn_sim'][0] == 1.0
    h = 0.5 / (1.0 + np.e)                                                           # 0.1344707
    assert abs(h - 0.1344707) < 1e-7
    assert np.abs(ref['partial'][0] - np.array([[-h, h], [h, -h], [-h, h], [h, -h]])).max() < 1e-14
    # case 2: D = 2, R = 2, n = 1, T = 0.5, a duplicated queue row (the tie goes to index 1)
    S = np.array([e2, e1, e1])
    zs = [np.array([e1, e2]), np.array([[0.6, 0.8], e1])]
    ref = nr.nnclr_reference(zs, S, 0.5)
    assert [list(i) for i in ref['nn_index']] == [[1, 0], [0, 1]]
    assert ref['gap'][0][0] == 0.0                                                   # the tie of row a0
    assert abs(ref['rows'][0][0] - 2.1269280) < 1e-7 and abs(ref['rows'][0][1] - 1.7839007) < 1e-7
    assert abs(ref['rows'][1][0] - 2.1269280) < 1e-7 and abs(ref['rows'][1][1] - 1.1711007) < 1e-7
    assert abs(ref['loss'][0] - 3.9108287) < 2e-7 and abs(ref['loss'][1] - 3.2980287) < 2e-7
    assert ref['acc'] == [0.0, 0.0] and ref['nn_sim'][0] == 1.0 and abs(ref['nn_sim'][1] - 0.9) < 1e-15
    want = np.array([[0.0, -1.6640368], [0.0, 1.6640368], [-1.7615942, 0.0], [1.7615942, 0.0]])
    assert np.abs(ref['partial'][0] - want).max() < 1e-7
    want = np.array([[1.3799490, 0.0], [-1.3799490, 0.0], [0.0, 1.7615942], [0.0, -1.7615942]])
    assert np.abs(ref['partial'][1] - want).max() < 1e-7
    # d objective / d z_q = (1 / R) (partial_0 + partial_1)[rows of q]
    assert np.abs(ref['grads'][0] - np.array([[0.6899745, -0.8320184], [-0.8807971, 0.8807971]])).max() < 1e-7
    assert np.abs(ref['grads'][1] + ref['grads'][0]).max() < 1e-15


# ---------------------------------------------------------------------------------------------------------------- properties
@pytest.mark.parametrize('n,D,T', [(3, 8, 0.5), (6, 16, 0.1)])
def test_the_other_view_as_queue_is_cross_view_ntxent(n, D, T):
    """S = the other view's rows, K = N: wherever row r's neighbour in S is the row with the largest z_r . z_c (always: S holds exactly
    the candidates of the opposite direction), the loss is NT-Xent restricted to cross-view columns with the anchor replaced.  With the
    queue = the view-b rows and both views EQUAL, the neighbour of every view-a row is its own view-b row = itself, and the view-a half
    of the loss is plain cross-view NT-Xent of z against z."""
    z = _views(n, 1, D, 5)[0]
    z[n:] = z[:n]                                                                    # both views equal
    ref = nr.nnclr_reference([z], z[n:], T)
    assert list(ref['nn_index'][0]) == list(range(n)) * 2 and abs(ref['nn_sim'][0] - 1.0) < 1e-15
    logits = (z[:n] @ z[n:].T) / T
    direct = (np.log(np.exp(logits).sum(1)) - np.diag(logits)).sum() / n
    assert abs(ref['rows'][0][:n].sum() / n - direct) <= 1e-13 * abs(direct)
    assert abs(ref['loss'][0] - 2.0 * direct) <= 1e-13 * abs(direct) and ref['acc'][0] == 1.0


def test_a_permutation_of_the_images_permutes_rows_and_gradient():
    n, D, K, T = 5, 8, 9, 0.3
    z, S = _views(n, 1, D, 8)[0], _queue(K, D, 8)
    perm = np.random.default_rng(0).permutation(n)
    both = np.concatenate([perm, n + perm])
    a, b = nr.nnclr_reference([z], S, T), nr.nnclr_reference([z[both]], S, T)
    assert abs(a['loss'][0] - b['loss'][0]) <= 1e-13 * abs(a['loss'][0])
    assert np.array_equal(a['nn_index'][0][both], b['nn_index'][0])
    assert np.abs(a['grads'][0][both] - b['grads'][0]).max() <= 1e-13


def test_duplicated_queue_rows_go_to_the_lowest_index():
    g = np.random.default_rng(2)
    base = nr.l2_normalize(g.standard_normal((6, 8)))[0]
    S = np.concatenate([base[[3, 1, 3]], base, base[[1]]])                           # 3 sits at 0, 2, 6; 1 at 1, 4, 10
    z = nr.l2_normalize(g.standard_normal((12, 8)))[0]
    idx, gap = nr.search(z, S)
    first = {3: 0, 1: 1, 0: 3, 2: 5, 4: 7, 5: 8}
    assert list(idx) == [first[j] for j in nr.search(z, base)[0]]
    assert all(gap[r] == 0.0 for r in range(12) if nr.search(z, base)[0][r] in (1, 3))
    assert list(nr.search(z[:2], S[:1])[1]) == [np.inf, np.inf]


def test_ring_position_over_three_steps():
    from simclr_amd import model as model_lib
    N, K = 8, 16
    assert [nr.queue_ptr(s, N, K) for s in range(4)] == [0, 8, 0, 8] == [model_lib.moco_queue_ptr(s, N, K) for s in range(4)]
    assert [nr.queue_ptr(s, 8, 32) for s in range(5)] == [0, 8, 16, 24, 0]
    queue = model_lib.SupportQueue(K, 4, seed=1, device='cpu')
    assert queue.NAME == 'nnclr/queue' and [v.name for v in queue.variables] == ['nnclr/queue'] and not queue.variables[0].trainable
    assert np.array_equal(queue.value.numpy(), model_lib.moco_queue_init(K, 4, 1))
    want = queue.value.numpy().copy()
    for s in range(3):
        rows = torch.full((N, 4), float(s + 1))
        assert queue.enqueue(rows, s) == nr.queue_ptr(s, N, K)
        want[nr.queue_ptr(s, N, K):nr.queue_ptr(s, N, K) + N] = s + 1
        assert np.array_equal(queue.value.numpy(), want)
    assert (want[:8] == 3).all() and (want[8:] == 2).all()
    with pytest.raises(ValueError, match='not a multiple'):
        queue.enqueue(torch.zeros(5, 4), 0)
    with pytest.raises(ValueError, match='need float32 keys'):
        queue.enqueue(torch.zeros(8, 3), 0)

    class M:
        variables, supervised_head = ['a', 'b'], None
    assert queue.checkpointable(M()).variables == ['a', 'b'] + queue.variables
    queue.reset()
    assert np.array_equal(queue.value.numpy(), model_lib.moco_queue_init(K, 4, 1))


# ---------------------------------------------------------------------------------------------------------------- error budget
def test_every_gpu_case_keeps_its_search_gap_and_its_error_budget():
    """The seeds are the first that give every searched row a float64 top-1 / top-2 gap above 4 D 2^-24; the emulation's error on each
    case is what nnclr_reference.EMULATION_ERROR records (the gates of tests/test_gpu_nnclr.py are 4 x that); the swapped view mask
    lies outside every gate."""
    assert nr.SHAPES == [(1, 2, 2, 64, 1), (2, 2, 4, 64, 0), (33, 33, 66, 64, 0), (64, 64, 64, 128, 0), (65, 130, 260, 128, 1),
                         (33, 99, 4097, 256, 2)] and nr.TEMPERATURES == (0.1, 0.5)
    for shape in nr.SHAPES:
        for family in nr.FAMILIES:
            assert nr.first_good_seed(shape, family) == nr.CASE_SEED[(shape, family)], (shape, family)
            assert nr.case_gap(shape, family) > nr.search_gap_needed(shape[3])
    budget = nr.measured_budget()
    assert sorted(budget) == sorted(nr.EMULATION_ERROR)
    for case, worst in budget.items():
        for k in ('loss', 'grad'):
            rec = nr.EMULATION_ERROR[case][k]
            assert abs(worst[k] - rec) <= 0.006 * rec, (case, k, worst[k], rec)      # recorded to three digits
            assert nr.TOL[case][k] == 4.0 * rec
    for shape in nr.SHAPES:
        for family in nr.FAMILIES:
            for T in nr.TEMPERATURES:
                _, _, ref = nr.case_reference(shape, family, T)
                _, _, wrong = nr.case_reference(shape, family, T, swapped=True)
                err = nr.relative_errors(wrong['loss'][shape[4]], wrong['partial'][shape[4]], ref, shape[4])
                assert err['loss'] > 1e3 * nr.TOL[(shape, family)]['loss'] and err['grad'] > 1e3 * nr.TOL[(shape, family)]['grad']


def test_the_emulation_keeps_a_near_one_hot_row():
    """A row whose positive carries all but 1e-5 of the softmax: the (max, rest) statistics and the stored 1 - P_pos keep the loss and
    the gradient to float32's relative precision (a (max, sum) pair and exp2(..) - 1 would lose three digits of both)."""
    D = 64
    g = np.random.default_rng(4)
    S = nr.l2_normalize(g.standard_normal((2, D)))[0].astype(np.float32)
    zs = [np.stack([S[0], S[0]]), np.stack([S[1], S[1]])]
    ref = nr.nnclr_reference(zs, S, nr.f32(0.1))
    assert 0.0 < ref['loss'][0] < 1e-3
    emu = nr.nnclr_emulated(zs, S, ref['nn_index'][0], 0, 0.1)
    err = nr.relative_errors(emu['loss'], emu['partial'], ref, 0)
    assert err['loss'] < 1e-5 and err['grad'] < 1e-5, err


# ---------------------------------------------------------------------------------------------------------------- flags and refusals
@pytest.fixture
def flags():
    from simclr_amd.flags import FLAGS
    FLAGS.reset()
    yield FLAGS
    FLAGS.reset()


def test_flags_default_to_off_and_switch_the_entry(flags):
    from simclr_amd import pretrain_losses, run
    assert flags.nn_queue_size == 0 and flags.nn_queue_seed == 0
    assert not pretrain_losses.nn_positives_on() and pretrain_losses.active() is pretrain_losses.LOSSES['ntxent']
    flags.parse(['--nn_queue_size=1024', '--nn_queue_seed=3'])
    assert (flags.nn_queue_size, flags.nn_queue_seed) == (1024, 3)
    assert run.check_contrastive_loss_flags() is False and pretrain_losses.nn_positives_on()
    spec = pretrain_losses.active()
    assert spec.call is pretrain_losses.LOSSES['ntxent'].call and spec.logits_metrics == ()
    # fine-tuning and evaluation ignore both flags, whatever they hold
    flags.update(nn_queue_size=-7, train_mode='finetune')
    assert run.check_contrastive_loss_flags() is False and not pretrain_losses.nn_positives_on() and pretrain_losses.active() is None
    flags.update(train_mode='pretrain', mode='eval')
    assert run.check_contrastive_loss_flags() is False and not pretrain_losses.nn_positives_on()
    assert pretrain_losses.active() is pretrain_losses.LOSSES['ntxent']


def test_the_ntxent_row_dispatches_on_the_flag(flags, monkeypatch):
    from simclr_amd import objective, pretrain_losses
    calls = []
    monkeypatch.setattr(objective, 'add_contrastive_loss', lambda *a, **kw: (calls.append(('ntxent', a, kw)), ('loss', 'logits', None))[1])
    monkeypatch.setattr(objective, 'add_nn_contrastive_loss', lambda *a, **kw: (calls.append(('nnclr', a, kw)), 'loss2')[1])

    class Q:
        value = 'queue'

    class C:
        outputs, strategy, overlap, logits_con, support = 'h', None, None, None, Q()
    c = C()
    assert pretrain_losses.LOSSES['ntxent'].call(c) == 'loss' and c.logits_con == 'logits' and calls[-1][0] == 'ntxent'
    flags.update(nn_queue_size=0)
    assert pretrain_losses.LOSSES['ntxent'].call(c) == 'loss' and calls[-1][0] == 'ntxent'
    c.logits_con = None
    flags.update(nn_queue_size=512, temperature=0.2)
    assert pretrain_losses.active().call(c) == 'loss2' and c.logits_con is None
    assert calls[-1] == ('nnclr', ('h', 'queue'), dict(temperature=0.2, strategy=None, overlap=None))


def test_metric_names_with_the_flag_on_and_unchanged_with_it_off(flags):
    from simclr_amd import pretrain_losses, run
    today = ['train/contrast_acc', 'train/contrast_entropy', 'train/contrast_loss', 'train/supervised_acc', 'train/supervised_loss',
             'train/total_loss', 'train/weight_decay']
    assert sorted(run.build_metrics()) == today
    flags.update(nn_queue_size=0, nn_queue_seed=4)
    assert sorted(run.build_metrics()) == today
    assert sorted(pretrain_losses.LOSSES) == ['barlow', 'byol', 'dino', 'generalized', 'mocov2', 'ntxent', 'supcon', 'swav', 'vicreg']
    assert pretrain_losses.LOSSES['ntxent'].metrics == (('train/contrast_loss', 'value'),)
    flags.update(nn_queue_size=512)
    assert sorted(run.build_metrics()) == ['train/contrast_acc', 'train/contrast_loss', 'train/nn_similarity', 'train/supervised_acc',
                                           'train/supervised_loss', 'train/total_loss', 'train/weight_decay']
    assert pretrain_losses.active().metrics == (('train/contrast_loss', 'value'), ('train/contrast_acc', 'acc'),
                                                ('train/nn_similarity', 'nn_sim'))
    flags.update(train_mode='finetune')
    assert sorted(run.build_metrics()) == ['train/supervised_acc', 'train/supervised_loss', 'train/total_loss', 'train/weight_decay']


@pytest.mark.parametrize('extra,match', [
    (['--nn_queue_size=700'], 'must be a multiple of train_batch_size = 512'),
    (['--nn_queue_size=256'], 'must be a multiple of train_batch_size = 512'),
    (['--nn_queue_size=-512'], 'must be a multiple of train_batch_size = 512'),
    (['--nn_queue_size=2097152'], 'at most 1048576'),
    (['--nn_queue_size=1024', '--contrastive_loss=supcon'], 'needs --contrastive_loss=ntxent'),
    (['--nn_queue_size=1024', '--contrastive_loss=mocov2'], 'needs --contrastive_loss=ntxent'),
    (['--nn_queue_size=1024', '--contrastive_loss=vicreg'], 'needs --contrastive_loss=ntxent'),
    (['--nn_queue_size=1024', '--hard_negative_beta=0.5'], 'does not combine with --hard_negative_beta'),
    (['--nn_queue_size=1024', '--debiased_tau_plus=0.1'], 'does not combine with --hard_negative_beta'),
    (['--nn_queue_size=1024', '--hidden_norm=false'], 'needs --hidden_norm=true'),
    (['--nn_queue_size=1024', '--proj_out_dim=100'], 'needs a loss width of 64/128/256'),
    (['--nn_queue_size=1024', '--proj_out_dim=512'], 'needs a loss width of 64/128/256'),
    (['--nn_queue_size=1024', '--proj_head_mode=none'], 'needs a loss width of 64/128/256'),
    (['--nn_queue_size=4', '--train_batch_size=1'], 'needs --train_batch_size >= 2'),
    (['--nn_queue_size=1024', '--temperature=0'], 'needs --temperature > 0'),
    (['--nn_queue_size=1024', '--temperature=-0.1'], 'needs --temperature > 0'),
    (['--nn_queue_size=1024', '--temperature=nan'], 'needs --temperature > 0'),
])
def test_run_main_refuses_before_any_device_work(flags, extra, match):
    from simclr_amd import run
    with pytest.raises(ValueError, match=match):
        run.main(['--dataset=synthetic', '--train_steps=1'] + extra)


def test_value_errors_of_the_entry_points_before_any_device_work():
    from simclr_amd import objective, ops
    with pytest.raises(ValueError, match='64/128/256'):
        objective.add_nn_contrastive_loss(torch.zeros(8, 100), torch.zeros(16, 100), 0.1)
    with pytest.raises(ValueError, match='need a float32 support queue'):
        objective.add_nn_contrastive_loss(torch.zeros(8, 128), torch.zeros(16, 64), 0.1)
    with pytest.raises(ValueError, match='need a float32 support queue'):
        objective.add_nn_contrastive_loss(torch.zeros(8, 128), torch.zeros(16, 128, dtype=torch.float64), 0.1)
    for T in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='need temperature > 0 and finite'):
            objective.add_nn_contrastive_loss(torch.zeros(8, 128), torch.zeros(16, 128), T)
    with pytest.raises(ValueError, match='N = R\\*n >= 2'):
        ops.nnclr_fwd(torch.zeros(2, 64), torch.zeros(2, 64), torch.zeros(2, 64), 0, 0.1)
    with pytest.raises(ValueError, match='N = R\\*n >= 2'):
        ops.nnclr_fwd(torch.zeros(8, 64), torch.zeros(8, 64), torch.zeros(12, 64), 0, 0.1)
    with pytest.raises(ValueError, match='64/128/256'):
        ops.nnclr_bwd(torch.zeros(8, 512), torch.zeros(8, 512), 0, 0.1, None, 1.0, None)
    with pytest.raises(ValueError, match='temperature must be > 0'):
        ops.nnclr_bwd(torch.zeros(8, 64), torch.zeros(8, 64), 0, 0.0, None, 1.0, None)
    assert ops.NNCLR_DIMS == (64, 128, 256)


def test_the_library_refuses_bad_arguments_without_a_device():
    """Every refusal of simclr_nnclr_fwd / _bwd returns 1 before anything is launched: fake pointers stand in for the tensors."""
    import ctypes
    from simclr_amd._lib import ABI_VERSION, SimclrHipError, lib
    L = lib()
    assert ABI_VERSION == 8 and L.abi_version() == 8
    f = ctypes.c_float
    fake = ctypes.c_void_p(1 << 20)                          # aligned, never dereferenced: every call below is refused first
    for kw, match in ((dict(D=100), 'D must be 64/128/256'), (dict(n=0), 'n >= 1'), (dict(n=1, N=1), 'N >= 2'), (dict(n=4, N=6), 'N = R\\*n'),
                      (dict(n=4, N=8, rank=2), 'rank 2 out of range'), (dict(T=0.0), 'temperature'), (dict(T=float('nan')), 'temperature'),
                      (dict(T=float('inf')), 'temperature'), (dict(ptr=None), 'null or misaligned'),
                      (dict(ptr=ctypes.c_void_p((1 << 20) + 4)), 'null or misaligned')):
        a = dict(dict(n=4, N=4, D=128, rank=0, T=0.1, ptr=fake), **kw)
        if 'ptr' not in kw:
            a['ptr'] = None                                  # the scalar checks come first: nothing is touched
        with pytest.raises(SimclrHipError, match=match):
            L.nnclr_fwd(a['ptr'], fake, fake, a['n'], a['N'], a['D'], a['rank'], f(a['T']), fake, fake, fake, None)
        with pytest.raises(SimclrHipError, match=match):
            L.nnclr_bwd(fake, fake, a['n'], a['N'], a['D'], a['rank'], f(a['T']), fake, f(1.0), a['ptr'], fake, None)
    assert L.nnclr_workspace_bytes(4, 4, 100) == 0 and L.nnclr_workspace_bytes(1, 1, 64) == 0 and L.nnclr_workspace_bytes(4, 6, 64) == 0
    assert L.nnclr_workspace_bytes(512, 512, 128) > 0 and L.nnclr_workspace_bytes(1, 2, 64) > 0
