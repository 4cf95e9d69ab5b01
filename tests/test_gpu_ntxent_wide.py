"""NT-Xent for embeddings wider than 256 (pytest -m gpu): proj_out_dim > 256 and proj_head_mode='none', where the contrastive loss
reads the encoder's 512 ... 8192-wide output.  The wide kernels (csrc/ntxent.hip, simclr_ntxent_wide_*) against the float64 oracle
(oracle/ntxent.py), against the register-resident sweeps at D <= 256, bitwise run to run, and in the full step, two replicas and
run.main."""
import functools
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import gpu_checks as gc

pytestmark = pytest.mark.gpu
DEV = gc.DEV


def _assert(res):
    bad = [r for r in res if not r['ok']]
    for r in res:
        print('%-4s %-64s err=%.3e tol=%.3e' % ('ok' if r['ok'] else 'FAIL', r['name'], r['err'], r['tol']))
    assert not bad, [(r['name'], r['err'], r['tol']) for r in bad]


# ---------------------------------------------------------------- kernels against the float64 oracle
@pytest.mark.parametrize('D', [257, 384, 512, 2048])
@pytest.mark.parametrize('R', [1, 2, 4])
def test_wide_ntxent_matches_float64_oracle(D, R):
    n = 16
    for rank in sorted({0, R - 1}):
        _assert(gc.check_ntxent(n, R, D=D, rank=rank))


def test_wide_ntxent_without_hidden_norm():
    _assert(gc.check_ntxent(16, 2, D=512, temperature=1.0, rank=1, hidden_norm=False))


def test_wide_ntxent_width_8192():
    """ResNet-50 4x with proj_head_mode=none; l2norm_fwd / _bwd at that width are part of check_ntxent."""
    _assert(gc.check_ntxent(8, 2, D=8192, rank=1))


def test_wide_ntxent_closed_forms():
    """Identical rows -> 2 log(2N-1); orthogonal one-hot rows -> 2 (log(e^{1/T} + 2n - 2) - 1/T), at D = 2048."""
    from simclr_amd import ops
    n, D, T = 64, 2048, 0.1
    z, _ = ops.l2norm_fwd(torch.ones(2 * n, D, device=DEV))
    out, _, _ = ops.ntxent_fwd(z, z, 0, T)
    res = [gc._res('wide_closed_identical', out.cpu()[0], 2 * np.log(2 * n - 1), 1e-5)]
    e = torch.zeros(n, D, device=DEV)
    e[torch.arange(n), torch.arange(n) * 31] = 1.0
    z, _ = ops.l2norm_fwd(torch.cat([e, e], 0).contiguous())
    out, _, _ = ops.ntxent_fwd(z, z, 0, T)
    res.append(gc._res('wide_closed_orthogonal', out.cpu()[0], 2 * (np.log(np.exp(1 / T) + (2 * n - 2)) - 1 / T), 1e-4, 1e-7))
    _assert(res)


def test_dispatch_routes_wide_widths_to_the_wide_kernels():
    from simclr_amd import ops
    assert not ops.ntxent_is_wide(256) and ops.ntxent_is_wide(257)
    n, N, D = 8, 16, 300
    zl = torch.nn.functional.normalize(torch.randn(2 * n, D, device=DEV), dim=1)
    za = torch.nn.functional.normalize(torch.randn(2 * N, D, device=DEV), dim=1)
    ws = ops.ntxent_workspace(n, N, D, DEV)
    assert ws.numel() * 4 >= ops.lib().ntxent_wide_workspace_bytes(n, N, D)
    a = ops.ntxent_fwd(zl, za, 1, 0.1, ws)[0].clone()
    b = ops.ntxent_wide_fwd(zl, za, 1, 0.1)[0]
    assert torch.equal(a, b)


# ---------------------------------------------------------------- the two paths agree where both exist
def _both_paths(n, R, D, rank, seed=5):
    from simclr_amd import ops
    g = torch.Generator().manual_seed(seed)
    zs = [torch.nn.functional.normalize(torch.randn(2 * n, D, generator=g), dim=1).to(DEV) for _ in range(R)]
    z_all = torch.cat([z[:n] for z in zs] + [z[n:] for z in zs], 0).contiguous()
    zl = zs[rank]
    outs = []
    for fwd, bwd, lab in ((ops.ntxent_fwd, ops.ntxent_bwd, ops.ntxent_logits_ab),
                          (ops.ntxent_wide_fwd, ops.ntxent_wide_bwd, ops.ntxent_wide_logits_ab)):
        out, rs, ws = fwd(zl, z_all, rank, 0.1)
        dl, da = bwd(zl, z_all, rank, 0.1, rs, 0.5, out, ws)
        torch.cuda.synchronize()
        outs.append(dict(out=out[:3].clone(), rs=rs.clone(), dl=dl.clone(), da=da.clone(), lab=lab(zl, z_all, 0.1)))
    return outs


@pytest.mark.parametrize('D', [128, 256])
def test_wide_path_equals_register_resident_sweeps(D):
    a, b = _both_paths(32, 2, D, 1)
    assert float((a['out'][0] - b['out'][0]).abs()) <= 2e-6 * float(a['out'][0].abs())
    assert float(a['out'][1]) == float(b['out'][1])
    assert float((a['out'][2] - b['out'][2]).abs()) <= 1e-5 * float(a['out'][2].abs()) + 1e-7
    assert float((a['rs'] - b['rs']).abs().max()) <= 2e-6 * float(a['rs'].abs().max())
    for k in ('dl', 'da', 'lab'):
        assert float((a[k] - b[k]).abs().max()) <= 2e-5 * float(a[k].abs().max()), k


def test_wide_path_is_bitwise_deterministic():
    from simclr_amd import ops
    n, N, D = 64, 256, 1024
    g = torch.Generator().manual_seed(11)
    zl = torch.nn.functional.normalize(torch.randn(2 * n, D, generator=g), dim=1).to(DEV)
    za = torch.nn.functional.normalize(torch.randn(2 * N, D, generator=g), dim=1).to(DEV)
    za[n:2 * n] = zl[:n]      # rank 1 of 4
    za[N + n:N + 2 * n] = zl[n:]
    runs = []
    for _ in range(2):
        out, rs, ws = ops.ntxent_fwd(zl, za, 1, 0.1)
        dl, da = ops.ntxent_bwd(zl, za, 1, 0.1, rs, 0.25, out, ws)
        torch.cuda.synchronize()
        runs.append([out[:3].clone(), rs.clone(), dl.clone(), da.clone()])
    for x, y in zip(*runs):
        assert torch.equal(x, y)


def test_f16x3_falls_back_to_exact_at_wide_widths():
    """FLAGS.ntxent_matmul='f16x3' at D > 256 runs the exact wide kernels (the flag's help says so): bitwise the exact result, and
    the wide entry points refuse any other arithmetic rather than computing something else."""
    from simclr_amd import ops
    from simclr_amd._lib import SimclrHipError
    from simclr_amd.flags import FLAGS
    from simclr_amd import flags
    from simclr_amd.objective import add_contrastive_loss
    assert "'f16x3' falls back to it" in [d[3] for d in flags._DEFS if d[0] == 'ntxent_matmul'][0]
    n, D = 16, 640
    h = torch.randn(2 * n, D, generator=torch.Generator().manual_seed(2)).to(DEV)
    res = []
    try:
        for mode in ('exact', 'f16x3'):
            FLAGS.ntxent_matmul = mode
            loss, logits, _ = add_contrastive_loss(h, True, 0.1)
            dh = loss.backward(1.0)
            torch.cuda.synchronize()
            res.append((loss.value.clone(), logits.contrast_acc.clone(), logits.contrast_entropy.clone(), dh.clone()))
    finally:
        FLAGS.reset()
    for x, y in zip(*res):
        assert torch.equal(x, y)
    a, b = ops.ntxent_fwd(h, h, 0, 0.1, split=True)[0][:2], ops.ntxent_fwd(h, h, 0, 0.1)[0][:2]
    assert torch.equal(a, b)
    z = torch.zeros(2 * n, D, device=DEV)
    ws = ops.ntxent_wide_workspace(n, n, D, DEV)
    out = torch.zeros(4, device=DEV)
    rs = torch.zeros(2 * n, 2, device=DEV)
    with pytest.raises(SimclrHipError, match='must be exact'):
        ops.lib().ntxent_wide_fwd(ops._p(z), ops._p(z), n, n, D, 13, 0, 0.1, ops._p(out), ops._p(rs), ops._p(ws), ops._s())


# ---------------------------------------------------------------- the full step against the float64 oracle
def test_train_step_proj_out_dim_512():
    _assert(gc.check_train_step(depth=18, image_size=32, batch=16, proj_out_dim=512))


def _step_without_head(monkeypatch, depth, image_size, batch, compute_dtype, f32_matmul):
    """gc.check_train_step (calibrated gates) with proj_head_mode='none' on both sides: the product's FLAGS default and the
    oracle's Config.  The oracle cache there does not key on the head mode, so it is emptied around the check."""
    from oracle import model_torch
    from simclr_amd import flags
    from simclr_amd.flags import FLAGS
    monkeypatch.setattr(model_torch, 'Config', functools.partial(model_torch.Config, proj_head_mode='none'))
    defaults = {d[0]: d[1] for d in flags._DEFS}
    old = (defaults['proj_head_mode'], defaults['f32_matmul'])
    FLAGS.set_default('proj_head_mode', 'none')
    FLAGS.set_default('f32_matmul', f32_matmul)
    gc._TRAIN_STEP_ORACLE_CACHE.clear()
    try:
        return gc.check_train_step(depth=depth, image_size=image_size, batch=batch, compute_dtype=compute_dtype)
    finally:
        gc._TRAIN_STEP_ORACLE_CACHE.clear()
        FLAGS.set_default('proj_head_mode', old[0])
        FLAGS.set_default('f32_matmul', old[1])
        FLAGS.reset()


@pytest.mark.parametrize('depth,size,batch,dtype,matmul', [
    (18, 32, 16, 'f32', 'exact'), (18, 32, 16, 'f32', 'f16x3_3'), (18, 32, 16, 'bf16', 'exact'),
    (50, 32, 8, 'f32', 'exact'), (50, 32, 8, 'f32', 'f16x3_3')])
def test_train_step_without_projection_head(monkeypatch, depth, size, batch, dtype, matmul):
    """proj_head_mode=none: the loss reads the encoder output (512 wide for ResNet-18, 2048 for ResNet-50)."""
    res = _step_without_head(monkeypatch, depth, size, batch, dtype, matmul)
    assert any(r['name'].startswith('step_con_loss') for r in res)
    _assert(res)


# ---------------------------------------------------------------- two replicas over gloo on one GPU
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    try:
        import torch.distributed as dist
        import torch.nn.functional as F
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        torch.cuda.set_device(0)
        dist.init_process_group('gloo', rank=rank, world_size=world)
        from oracle.model_torch import Config, init_model
        from simclr_amd import comm
        from simclr_amd import model as model_lib
        from simclr_amd.flags import FLAGS
        from simclr_amd.resnet import RT
        from simclr_amd.run import make_single_step

        b, ncls, size = 8, 10, 32
        cfg = Config(resnet_depth=18, image_size=size, num_classes=ncls, proj_head_mode='none')
        params, state = init_model(cfg, seed=3, randomize_bn=True)
        g = torch.Generator().manual_seed(9)
        images = gc.structured_images(world * b, size, 2, g)                   # global batch, two views on the channels
        labels = F.one_hot(torch.randint(0, ncls, (world * b,), generator=g), ncls).float()
        allv = dict(params)
        allv.update(state)

        def fresh(strategy, batch):
            FLAGS.reset()
            FLAGS.update(resnet_depth=18, image_size=size, compute_dtype='f32', f32_matmul='exact', use_blur=False,
                         train_batch_size=batch, proj_head_mode='none')
            RT.reset()
            RT.device = torch.device('cuda', 0)
            RT.strategy = strategy
            m = model_lib.Model(ncls)
            with torch.no_grad():
                m(torch.zeros(2, size, size, 6, device='cuda'), training=True)
            for v in m.variables:
                v.value.copy_(allv[v.name].cuda())
            RT.weights_version += 1
            return m

        strategy = comm.Strategy()
        model = fresh(strategy, world * b)
        sl = slice(rank * b, (rank + 1) * b)
        out = make_single_step(model, model_lib.build_optimizer(0.1), strategy)(images[sl].cuda(), {'labels': labels[sl].cuda()})
        torch.cuda.synchronize()
        lt = torch.tensor([float(out['con_loss'].value.reshape(-1)[0])], dtype=torch.float64)
        dist.all_reduce(lt)
        grads2 = {v.name: v.grad.double().cpu().clone() for v in model.trainable_variables}
        # the loss alone on fixed 512-wide hiddens: all-gather + reduce-scatter of the key-side gradient at wide D
        from simclr_amd.objective import add_contrastive_loss
        H = torch.randn(2 * world * b, 512, generator=torch.Generator().manual_seed(4)).cuda()
        mine = torch.cat([H[rank * b:(rank + 1) * b], H[world * b + rank * b:world * b + (rank + 1) * b]]).contiguous()
        loss_r, _, _ = add_contrastive_loss(mine, True, 0.1, strategy)
        dh_r = loss_r.backward(1.0 / world)
        torch.cuda.synchronize()
        lr_ = torch.tensor([float(loss_r.value.reshape(-1)[0])], dtype=torch.float64)
        dist.all_reduce(lr_)
        dist.destroy_process_group()
        loss_1, _, _ = add_contrastive_loss(H, True, 0.1, None)
        dh_1 = loss_1.backward(1.0)
        torch.cuda.synchronize()
        want = torch.cat([dh_1[rank * b:(rank + 1) * b], dh_1[world * b + rank * b:world * b + (rank + 1) * b]])
        loss_alone = dict(loss_rel=abs(float(lr_) / world - float(loss_1.value.reshape(-1)[0])) / float(loss_1.value.reshape(-1)[0]),
                          dh_rel=float((dh_r - want).abs().max()) / float(want.abs().max()))
        one = fresh(None, world * b)
        out1 = make_single_step(one, model_lib.build_optimizer(0.1), None)(images.cuda(), {'labels': labels.cuda()})
        torch.cuda.synchronize()
        res = dict(loss_rel=abs(float(lt) / world - float(out1['con_loss'].value.reshape(-1)[0]))
                   / abs(float(out1['con_loss'].value.reshape(-1)[0])))
        worst, worst_name = 0.0, None
        for v in one.trainable_variables:
            r = v.grad.double().cpu()
            if float(r.abs().max()) < 1e-12:
                continue
            e = float((grads2[v.name] - r).abs().max()) / float(r.abs().max())
            if e > worst:
                worst, worst_name = e, v.name
        res['vs_one_replica_worst_rel'], res['vs_one_replica_worst_name'] = worst, worst_name
        g1 = torch.cat([v.grad.double().cpu().reshape(-1) for v in one.trainable_variables])
        g2 = torch.cat([grads2[v.name].reshape(-1) for v in one.trainable_variables])
        res['vs_one_replica_relnorm'] = float((g2 - g1).norm() / g1.norm())
        res['D'] = int(out['con_loss'].normalized.shape[1])
        res['loss_alone'] = loss_alone
        q.put((rank, 'ok', res))
    except Exception:  # noqa
        import traceback
        q.put((rank, 'FAIL', traceback.format_exc()))


def test_two_replica_step_without_projection_head_equals_global_batch():
    """Two ranks over gloo (all-gather of the 512-wide embeddings, reduce-scatter of the key-side gradient): the contrastive loss
    and the summed gradients of loss / R equal the one-replica step on the concatenated batch."""
    os.environ['SIMCLR_PEER_STATS'] = '0'
    try:
        ctx = mp.get_context('spawn')
        q = ctx.Queue()
        port = _free_port()
        procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
        for p in procs:
            p.start()
        res = [q.get(timeout=600) for _ in procs]
        for p in procs:
            p.join(timeout=60)
    finally:
        os.environ.pop('SIMCLR_PEER_STATS', None)
    assert all(r[1] == 'ok' for r in res), res
    for _, _, m in res:
        assert m['D'] == 512, m
        # the loss on its own: the hidden gradient of each rank is the one-replica gradient's slice to fp32 rounding
        assert m['loss_alone']['loss_rel'] < 1e-6 and m['loss_alone']['dh_rel'] < 1e-5, m
        # the whole step: the gates of tests/test_gpu_distributed.py's fast mode (all gradients 2e-3 relative L2; the worst single
        # tensor, max-abs relative, looser: a ResNet-18 of randomised BatchNorm statistics on 8 rows per replica amplifies the fp32
        # reordering of the replicated statistics)
        assert m['loss_rel'] < 1e-5, m
        assert m['vs_one_replica_relnorm'] < 2e-3 and m['vs_one_replica_worst_rel'] < 3e-2, m


# ---------------------------------------------------------------- the driver
def test_run_main_without_projection_head(tmp_path):
    from simclr_amd import run
    from simclr_amd.flags import FLAGS
    FLAGS.reset()
    try:
        result = run.main(['--dataset=synthetic', '--proj_head_mode=none', '--resnet_depth=18', '--image_size=32',
                           '--train_batch_size=16', '--eval_batch_size=16', '--eval_steps=1', '--train_steps=2', '--use_blur=False',
                           '--compute_dtype=f32', '--checkpoint_steps=2', '--mode=train_then_eval', '--model_dir=' + str(tmp_path)])
    finally:
        FLAGS.reset()
    assert result is not None and 'eval/label_top_1_accuracy' in result and result['global_step'] == 2
    import json
    rows = [json.loads(line) for line in open(os.path.join(str(tmp_path), 'summaries.jsonl'))]
    for k in ('train/contrast_loss', 'train/contrast_acc', 'train/contrast_entropy'):
        vals = [r['value'] for r in rows if r['tag'] == k]
        assert vals and all(np.isfinite(v) for v in vals), (k, sorted({r['tag'] for r in rows}))
