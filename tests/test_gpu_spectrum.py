"""The eigen-spectrum evaluation on the device (pytest -m gpu): simclr_spectrum_colsum / _cov against the float64 reference and the
float32 emulation of tests/spectrum_reference.py, the planted 1 / i spectrum through simclr_amd.spectrum, run.main end to end and two
replicas over gloo.  Every test here fails without the feature.

Gates (spectrum_reference.gates): cov at 4 x the emulation's error on the same inputs, never below one float32 ulp of the largest entry;
column sums at 4 eps64 of the largest; counts exact; eigenvalues within the Frobenius gate (Weyl) plus the LAPACK allowance.  Measured
on the MI355X: see README "Eigen-spectrum evaluation"."""
import json
import multiprocessing as mp
import os
import socket

import numpy as np
import pytest
import torch

from tests import spectrum_reference as sr
from tests.data_fixtures import make_dataset

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _t(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _device(x, w, mu32, slabs=None):
    """The two entry points through ops on one case: dict(sums, count, raw, raw_t)."""
    from simclr_amd import ops
    x, w, mu32 = _t(x), _t(w), _t(mu32)
    sums = cov = None
    for i, (o, e) in enumerate(slabs or [(0, x.shape[0])]):
        sums = ops.spectrum_colsum(x[o:e], w[o:e], sums, accumulate=i > 0)
        cov = ops.spectrum_cov(x[o:e], w[o:e], mu32, cov, accumulate=i > 0)
    s = sums.cpu().numpy()
    return dict(sums=s[:-1], count=s[-1], raw=cov.cpu().numpy(), raw_t=cov)


@pytest.mark.parametrize('case', sr.CASES, ids=str)
def test_kernels_meet_the_emulation_gates(case):
    from simclr_amd import ops
    n, D, fam = case
    (x, w), ref, emu, gate = sr.case(*case)
    assert ops.spectrum_tile_edge(n, D) == sr.tile_edge(n, D) == (128 if (n, D) in ((8200, 128), (300, 2048)) else 64)
    assert ops.spectrum_row_parts(n, D) == sr.row_plan(n, D)[1] == {(2, 64): 1, (65, 64): 3, (64, 128): 2, (130, 192): 5,
                                                                   (8200, 128): 257, (300, 2048): 3}[(n, D)]
    if fam == 'mean5':          # on the float64 reference first: the uncentred float32 form misses this case's gate
        assert np.abs(sr.emulate(x, w, 'uncentred')['raw'] - ref['raw']).max() > gate['raw']
    got = _device(x, w, ref['mu32'])
    if ref['count'] >= 2:
        got['C'] = sr.finish(got['raw'], ref['count'], ref['mu'], ref['mu32'])
    res = sr.compare(got, ref, gate)
    for k, (err, ok) in res.items():
        print('RATIO %s %s err=%.3e gate=%.3e ratio=%.3f' % (case, k, err, gate.get(k, 0.0), err / gate[k] if gate.get(k) else err))
    assert all(ok for _, ok in res.values()), res
    assert torch.equal(got['raw_t'], got['raw_t'].t())                    # cov[a, b] and cov[b, a] are the same bits
    if ref['count'] >= 2:
        lam_ref, lam = sr.eig64(ref['C']), sr.eig64(got['C'])
        allow = gate['C_fro'] + sr.LAPACK_REL * lam_ref[0]
        print('RATIO %s eig err=%.3e gate=%.3e' % (case, np.abs(lam - lam_ref).max(), allow))
        assert np.abs(lam - lam_ref).max() <= allow


def _guarded(shape, dtype, fill):
    """A tensor of `shape` in the middle of a larger one filled with `fill`: (view, check) -- check() asserts the bands hold."""
    numel = int(np.prod(shape))
    band = 1024
    whole = torch.full((numel + 2 * band,), fill, device=DEV, dtype=dtype)
    view = whole[band:band + numel].view(*shape)

    def check():
        assert bool((whole[:band] == fill).all()) and bool((whole[band + numel:] == fill).all())
    return view, check


@pytest.mark.parametrize('shape', [(65, 64), (130, 192), (8200, 128), (300, 2048)], ids=str)
def test_bitwise_repeats_and_guard_bands(shape):
    from simclr_amd import _lib, ops
    n, D = shape
    (x, w), ref, _, _ = sr.case(n, D, 'nanpad')
    x, w, mu32 = _t(x), _t(w), _t(ref['mu32'])
    nbytes = _lib.lib().spectrum_workspace_bytes(n, D)
    assert nbytes % 8 == 0
    runs = []
    for _ in range(2):
        ws, chk_ws = _guarded((nbytes // 8,), torch.float64, -7.0)
        sums, chk_s = _guarded((D + 1,), torch.float64, -7.0)
        cov, chk_c = _guarded((D, D), torch.float64, -7.0)
        ops.spectrum_colsum(x, w, sums, ws=ws)
        ops.spectrum_cov(x, w, mu32, cov, ws=ws)
        # the column sums alone, on the small workspace of their own: the same bits
        small, chk_small = _guarded((_lib.lib().spectrum_colsum_workspace_bytes(n, D) // 8,), torch.float64, -7.0)
        alone = ops.spectrum_colsum(x, w, ws=small)
        torch.cuda.synchronize()
        for chk in (chk_ws, chk_s, chk_c, chk_small):
            chk()
        assert torch.equal(alone, sums) and small.numel() * 8 < nbytes
        assert bool((cov != -7.0).all()) and bool((sums != -7.0).all()) and bool(torch.isfinite(cov).all())
        runs.append([sums.clone(), cov.clone()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_two_slabs_accumulate_to_the_one_call_sums():
    """The slabs end on a part boundary (32 rows at this shape, for the slabs and the whole), so both ways add the same float32 parts
    and differ in the order of the double additions alone: gated at 4 eps64 x the largest entry."""
    (x, w), ref, _, _ = sr.case(130, 192, 'nanpad')
    assert sr.row_plan(130, 192)[0] == sr.row_plan(96, 192)[0] == sr.row_plan(34, 192)[0] == 32
    one, two = _device(x, w, ref['mu32']), _device(x, w, ref['mu32'], [(0, 96), (96, 130)])
    assert one['count'] == two['count'] == ref['count']
    assert np.abs(one['sums'] - two['sums']).max() <= 4 * sr.EPS64 * np.abs(one['sums']).max()
    assert np.abs(one['raw'] - two['raw']).max() <= 4 * sr.EPS64 * np.abs(one['raw']).max()
    assert torch.equal(two['raw_t'], two['raw_t'].t())


def test_planted_harmonic_spectrum_through_the_module(monkeypatch):
    """lambda_i = 1 / i at (300, 128): alpha, rankme and the numerical rank at the values of the float64 reference, within the
    eigenvalue gate propagated to first order (spectrum_reference.score_gates)."""
    from simclr_amd import spectrum
    x, w = sr.planted_harmonic()
    ref, emu = sr.reference(x, w), sr.emulate(x, w)
    gate = sr.gates(emu, ref)
    lam_ref = sr.eig64(ref['C'])
    g = gate['C_fro'] + sr.LAPACK_REL * lam_ref[0]
    assert g <= 1e-3 * lam_ref[-1]                       # the first-order propagation holds; no eigenvalue is near the rank threshold
    C, S, mu = spectrum.covariance(_t(x), _t(w))
    assert S == 300 and np.abs(mu.cpu().numpy() - ref['mu']).max() <= 4 * sr.EPS64 * np.abs(ref['mu']).max()
    assert torch.equal(C, C.t())
    err = C.cpu().numpy() - ref['C']
    print('PLANTED C err=%.3e gate=%.3e fro=%.3e gate=%.3e' % (np.abs(err).max(), gate['C'], np.linalg.norm(err), gate['C_fro']))
    assert np.abs(err).max() <= gate['C'] and np.linalg.norm(err) <= gate['C_fro']
    lam = spectrum.eigenvalues(C)
    assert np.abs(lam - lam_ref).max() <= g and np.abs(lam - 1.0 / np.arange(1, 129)).max() <= g + 1e-7
    got, want, sg = spectrum.scores(lam), sr.scores64(lam_ref), sr.score_gates(lam_ref, g)
    print('PLANTED alpha %.12g (%.12g) rankme %.12g (%.12g) gates %.3e %.3e' % (
        got['eval/spectrum_alpha'], want['eval/spectrum_alpha'], got['eval/spectrum_rankme'], want['eval/spectrum_rankme'],
        sg['alpha'], sg['rankme']))
    assert abs(got['eval/spectrum_alpha'] - want['eval/spectrum_alpha']) <= sg['alpha'] and abs(got['eval/spectrum_alpha'] - 1.0) <= 1e-3
    assert abs(got['eval/spectrum_rankme'] - want['eval/spectrum_rankme']) <= sg['rankme']
    assert got['eval/spectrum_numerical_rank'] == want['eval/spectrum_numerical_rank'] == 128
    assert abs(sr.scores64(lam_ref, rankme_on_lambda=True)['eval/spectrum_rankme'] - got['eval/spectrum_rankme']) > sg['rankme']
    # slabs of 128 rows end on part boundaries: the same float32 parts, another order of the double additions
    monkeypatch.setattr(spectrum, 'SLAB_ROWS', 128)
    C3, S3, _ = spectrum.covariance(_t(x), _t(w))
    assert S3 == 300 and float((C3 - C).abs().max()) <= 4 * sr.EPS64 * float(C.abs().max()) and torch.equal(C3, C3.t())
    # identical rows: every score 0
    Cz, _, _ = spectrum.covariance(_t(np.repeat(x[:1], 40, 0)), torch.ones(40, device=DEV))
    z = spectrum.scores(spectrum.eigenvalues(Cz))
    assert float(Cz.abs().max()) == 0.0 and z['eval/spectrum_rankme'] == 0.0 and z['eval/spectrum_numerical_rank'] == 0


def test_refusals_on_device_tensors():
    from simclr_amd import _lib, ops, spectrum
    (x, w), ref, _, _ = sr.case(65, 64, 'gauss')
    x, w, mu32 = _t(x), _t(w), _t(ref['mu32'])
    with pytest.raises(ValueError, match='multiples of 64'):
        ops.spectrum_colsum(x[:, :32].contiguous(), w)
    with pytest.raises(ValueError, match='x must be a float32'):
        ops.spectrum_cov(x.double(), w, mu32)
    with pytest.raises(ValueError, match='16-byte aligned'):
        ops.spectrum_colsum(x, torch.zeros(66, device=DEV)[1:])
    with pytest.raises(ValueError, match='contiguous'):
        ops.spectrum_cov(x, w, mu32, cov=torch.zeros(64, 128, device=DEV, dtype=torch.float64)[:, :64])
    with pytest.raises(ValueError, match='workspace must hold'):
        ops.spectrum_cov(x, w, mu32, ws=torch.zeros(8, device=DEV, dtype=torch.float64))
    with pytest.raises(ValueError, match='mu32 must be'):
        ops.spectrum_cov(x, w, mu32.double())
    with pytest.raises(ValueError, match='at least 2'):
        spectrum.covariance(x, torch.zeros(65, device=DEV))
    L = _lib.lib()
    p = lambda t: t.data_ptr()
    with pytest.raises(_lib.SimclrHipError, match='16-byte aligned'):
        L.spectrum_colsum(p(x) + 4, p(w), 65, 64, p(x), 0, p(x), None)
    with pytest.raises(_lib.SimclrHipError, match='multiple of 64'):
        L.spectrum_cov(p(x), p(w), p(mu32), 65, 32, p(x), 0, p(x), None)
    sums = ops.spectrum_colsum(x, w)                              # and still works afterwards
    assert float(sums[-1]) == 65 and bool(torch.isfinite(sums).all())


# ------------------------------------------------------------------ end to end
_MAIN = ['--resnet_depth=18', '--image_size=32', '--train_batch_size=16', '--eval_batch_size=16', '--use_blur=False',
         '--compute_dtype=f32', '--f32_matmul=exact', '--mode=train_then_eval', '--train_steps=2', '--checkpoint_steps=2',
         '--lineareval_while_pretraining=False']
_KEYS = {'eval/spectrum_rankme', 'eval/spectrum_participation_ratio', 'eval/spectrum_numerical_rank', 'eval/spectrum_top1_share',
         'eval/spectrum_dims_90', 'eval/spectrum_dims_99', 'spectrum/trace', 'spectrum/rows', 'spectrum/dim',
         'spectrum/negative_eigenvalues', 'global_step'}
_ALPHA = 'eval/spectrum_alpha'


def _check_files(model_dir, result, rows):
    keys = {k for k in result if 'spectrum' in k} | {'global_step'}
    assert _KEYS <= keys <= _KEYS | {_ALPHA}
    for name in ('spectrum_result.json', 'spectrum_result_2.json'):
        saved = json.load(open(os.path.join(model_dir, name)))
        lam = saved.pop('eigenvalues')
        assert set(saved) == keys and saved == {k: result[k] for k in keys}
        assert len(lam) == 512 and all(a >= b >= 0.0 for a, b in zip(lam, lam[1:]))
        assert abs(sum(lam) - result['spectrum/trace']) <= 1e-12 * result['spectrum/trace']
    assert result['global_step'] == 2 and result['spectrum/rows'] == rows and result['spectrum/dim'] == 512
    assert 1.0 <= result['eval/spectrum_participation_ratio'] <= result['eval/spectrum_numerical_rank'] <= min(rows - 1, 512)
    assert 1.0 <= result['eval/spectrum_rankme'] <= 512.01 and 0.0 < result['eval/spectrum_top1_share'] <= 1.0
    assert 1 <= result['eval/spectrum_dims_90'] <= result['eval/spectrum_dims_99'] <= result['eval/spectrum_numerical_rank']
    return keys


def test_run_main_on_synthetic_data(tmp_path):
    from simclr_amd import run
    from simclr_amd.flags import FLAGS
    model_dir = str(tmp_path / 'm')
    try:
        FLAGS.reset()
        result = run.main(_MAIN + ['--dataset=synthetic', '--eval_steps=2', '--model_dir=' + model_dir, '--spectrum_eval=True',
                                   '--knn_eval=True', '--knn_k=5', '--kmeans_eval=True'])
        keys = _check_files(model_dir, result, 128)
        assert {'eval/knn_top_1_accuracy', 'eval/kmeans_nmi'} <= set(result)                       # the union
        eval_args = [a for a in _MAIN if not a.startswith(('--mode', '--train_steps', '--checkpoint_steps'))] + [
            '--mode=eval', '--dataset=synthetic', '--eval_steps=2', '--model_dir=' + model_dir]
        FLAGS.reset()
        again = run.main(eval_args + ['--spectrum_eval=True'])
        assert again == {k: result[k] for k in keys}                               # bitwise, on the second wiring path
        _check_files(model_dir, again, 128)
        FLAGS.reset()
        short = run.main(eval_args + ['--spectrum_eval=True', '--spectrum_bank_examples=48', '--spectrum_rank_threshold=1e-3'])
        assert short['spectrum/rows'] == 48 and short['eval/spectrum_numerical_rank'] <= 47
        for name in ('spectrum_result.json', 'spectrum_result_2.json'):
            os.remove(os.path.join(model_dir, name))
        FLAGS.reset()
        plain = run.main(eval_args)
        assert not plain or not any('spectrum' in k for k in plain)
        assert not os.path.exists(os.path.join(model_dir, 'spectrum_result.json'))
        assert not os.path.exists(os.path.join(model_dir, 'spectrum_result_2.json'))
    finally:
        FLAGS.reset()


def test_run_main_on_a_dataset_with_padded_last_batches(tmp_path):
    from simclr_amd import data as data_lib
    from simclr_amd import knn, run, spectrum
    from simclr_amd.checkpoint import Checkpoint
    from simclr_amd.flags import FLAGS
    from simclr_amd.resnet import RT
    from simclr_amd import model as model_lib
    data_dir, model_dir, plain_dir = str(tmp_path / 'data'), str(tmp_path / 'm'), str(tmp_path / 'plain')
    make_dataset(data_dir)                                        # 103 train / 37 validation images, 10 classes
    try:
        FLAGS.reset()
        result = run.main(_MAIN + ['--dataset=waves', '--data_dir=' + data_dir, '--model_dir=' + model_dir, '--spectrum_eval=True'])
        keys = _check_files(model_dir, result, 103)
        assert set(result) == keys and not os.path.exists(os.path.join(model_dir, 'kmeans_result.json'))
        # the same spectrum by hand from the restored model: the 9 padded rows of the last batch carry weight 0
        RT.reset()
        RT.device = torch.device(DEV, torch.cuda.current_device())
        model = model_lib.Model(10)
        model(torch.zeros(2, 32, 32, 3, device=DEV), training=False)
        model.release()
        Checkpoint(model=model).restore(os.path.join(model_dir, 'ckpt-2.pt'), model_only=False).expect_partial()
        builder = data_lib.ArrayDatasetBuilder('waves', data_dir)
        dev = torch.device(DEV, torch.cuda.current_device())
        x, _, w = knn.extract_features(model, data_lib.DatasetIterator(builder.split('train'), 10, 16, False, device=dev), normalize=False)
        assert x.shape == (112, 512) and float(w.sum()) == 103
        C, S, _ = spectrum.covariance(x, w)
        lam = spectrum.eigenvalues(C)
        s = spectrum.scores(lam)
        assert S == 103 and all(result[k] == v for k, v in s.items())
        # against the float64 definition on the same features
        xn, wn = x.cpu().numpy(), w.cpu().numpy()
        ref, emu = sr.reference(xn, wn), sr.emulate(xn, wn)
        gate = sr.gates(emu, ref)
        lam_ref = sr.eig64(sr.cov64(xn, wn)[0])
        err = C.cpu().numpy() - ref['C']
        print('WAVES C err=%.3e gate=%.3e' % (np.abs(err).max(), gate['C']))
        assert np.abs(err).max() <= gate['C'] and np.abs(lam - np.maximum(lam_ref, 0.0)).max() <= gate['C_fro'] + sr.LAPACK_REL * lam_ref[0]
        FLAGS.reset()
        plain = run.main(_MAIN + ['--dataset=waves', '--data_dir=' + data_dir, '--model_dir=' + plain_dir])
        assert plain is None and not os.path.exists(os.path.join(plain_dir, 'spectrum_result.json'))
        assert os.path.exists(os.path.join(plain_dir, 'ckpt-2.pt'))
    finally:
        FLAGS.reset()


# ------------------------------------------------------------------ two replicas over gloo on one GPU
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _shard(n, rank, world=2, B=64):
    """Eval-style shards: global batch B, B / world rows per replica and step, positions past the end are row 0 with weight 0.  With
    B = 64 a replica's 32-row batches are the row parts of one process at this shape: both add the same float32 parts."""
    b = B // world
    steps = -(-n // B)
    pos = (np.arange(steps)[:, None] * B + rank * b + np.arange(b)[None, :]).reshape(-1)
    return np.where(pos < n, pos, 0), (pos < n).astype(np.float32)


def _spectrum_worker(rank, world, port, q):
    try:
        import torch.distributed as dist
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          SIMCLR_DIST_BACKEND='gloo', SIMCLR_SHARE_GPU='1')
        torch.cuda.set_device(0)
        dist.init_process_group('gloo', rank=rank, world_size=world)
        from simclr_amd import comm, spectrum
        from simclr_amd.resnet import RT
        RT.reset()
        RT.device = torch.device('cuda', 0)
        strategy = comm.Strategy()
        t = lambda a: torch.from_numpy(np.array(a)).to(RT.device)
        x, w = sr.case_inputs(130, 192, 'nanpad')
        rows, keep = _shard(len(x), rank)
        C2, S2, _ = spectrum.covariance(t(x[rows]), t(w[rows] * keep), strategy)
        lam2 = spectrum.eigenvalues(C2, strategy)
        C1, S1, _ = spectrum.covariance(t(x), t(w))
        lam1 = spectrum.eigenvalues(C1)
        torch.cuda.synchronize()
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, 'ok', dict(C2=C2.cpu().numpy(), S2=S2, lam2=lam2, C1=C1.cpu().numpy(), S1=S1, lam1=lam1)))
    except Exception:  # noqa
        import traceback
        q.put((rank, 'FAIL', traceback.format_exc()))


def test_two_ranks_over_gloo_hold_the_one_process_spectrum():
    """Disjoint shards of the bank on two ranks, two all-reduces: both ranks hold the same bits, the count is one process's, and the
    covariance lies within the two-slab gate (4 eps64 of the largest entry) of one process's."""
    assert sr.row_plan(130, 192)[0] == sr.row_plan(96, 192)[0] == 32
    os.environ['SIMCLR_PEER_STATS'] = '0'
    try:
        ctx = mp.get_context('spawn')
        q = ctx.Queue()
        port = _free_port()
        procs = [ctx.Process(target=_spectrum_worker, args=(r, 2, port, q)) for r in range(2)]
        for p in procs:
            p.start()
        res = [q.get(timeout=300) for _ in procs]
        for p in procs:
            p.join(timeout=60)
    finally:
        os.environ.pop('SIMCLR_PEER_STATS', None)
    assert all(r[1] == 'ok' for r in res), res
    a, c = res[0][2], res[1][2]
    assert np.array_equal(a['C2'], c['C2']) and np.array_equal(a['lam2'], c['lam2']) and a['S2'] == c['S2']
    for m in (a, c):
        assert m['S2'] == m['S1'] == sr.colsum64(*sr.case_inputs(130, 192, 'nanpad'))[1]
        err = np.abs(m['C2'] - m['C1']).max()
        print('GLOO C two ranks vs one %.3e gate %.3e' % (err, 4 * sr.EPS64 * np.abs(m['C1']).max()))
        assert err <= 4 * sr.EPS64 * np.abs(m['C1']).max()
        assert np.abs(m['lam2'] - m['lam1']).max() <= 192 * 4 * sr.EPS64 * np.abs(m['C1']).max() + sr.LAPACK_REL * m['lam1'][0]
