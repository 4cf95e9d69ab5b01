"""GPU test of the multi-replica training step (pytest -m gpu).

Only one MI355X is reachable from the build session, so two ranks share cuda:0 and talk over gloo
(RCCL refuses two ranks on one device).  Everything except the transport is the production path:
per-replica HIP kernels, the all-gather / reduce-scatter of the hidden block, SyncBN statistic
all-reduces in forward and backward, loss/R, the bucketed gradient all-reduce, LARS.  The result
must equal the float64 oracle's single-replica step on the GLOBAL batch (R replicas == 1 replica on
the global batch)."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q, backend='gloo'):
    try:
        import torch.distributed as dist
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        devno = rank if backend == 'nccl' else 0          # RCCL needs one device per rank; gloo ranks share cuda:0
        torch.cuda.set_device(devno)
        if backend == 'nccl':
            dist.init_process_group('nccl', rank=rank, world_size=world, device_id=torch.device('cuda', devno))
        else:
            dist.init_process_group('gloo', rank=rank, world_size=world)
        from collections import OrderedDict
        from oracle.model_torch import Config, init_model, train_step
        from simclr_amd import comm
        from simclr_amd import model as model_lib
        from simclr_amd.flags import FLAGS
        from simclr_amd.resnet import RT
        from simclr_amd.run import make_single_step

        depth, image_size, b, num_classes, lr, wd = int(os.environ.get('SIMCLR_TEST_DEPTH', '18')), 32, 8, 10, 0.1, 1e-4
        matmul = os.environ.get('SIMCLR_TEST_F32_MATMUL', 'exact')
        cfg = Config(resnet_depth=depth, image_size=image_size, num_classes=num_classes, weight_decay=wd)
        params, state = init_model(cfg, seed=0, randomize_bn=False)
        g = torch.Generator().manual_seed(5)
        images = torch.rand(world * b, image_size, image_size, 6, generator=g)          # global batch
        labels = torch.nn.functional.one_hot(torch.randint(0, num_classes, (world * b,), generator=g), num_classes).float()
        def run_step():
            FLAGS.reset()
            FLAGS.update(resnet_depth=depth, image_size=image_size, compute_dtype='f32', use_blur=False,
                         weight_decay=wd, train_batch_size=world * b, f32_matmul=matmul)
            RT.reset()
            RT.device = torch.device('cuda', devno)
            strategy = comm.Strategy()
            RT.strategy = strategy
            model = model_lib.Model(num_classes)
            with torch.no_grad():
                model(torch.zeros(2, image_size, image_size, 6, device='cuda'), training=False)
            allv = dict(params); allv.update(state)
            for v in model.variables:
                v.value.copy_(allv[v.name].cuda())
            RT.weights_version += 1
            opt = model_lib.build_optimizer(lr)
            step = make_single_step(model, opt, strategy)
            sl = slice(rank * b, (rank + 1) * b)
            out = step(images[sl].cuda(), {'labels': labels[sl].cuda()})
            return strategy, model, out
        strategy, model, out = run_step()
        torch.cuda.synchronize()
        # oracle: ONE replica on the global batch, float64
        p64 = OrderedDict((k, v.double()) for k, v in params.items())
        s64 = OrderedDict((k, v.double()) for k, v in state.items())
        m64 = OrderedDict((k, torch.zeros_like(v)) for k, v in p64.items())
        np64, ns64, nm64, t64 = train_step(cfg, p64, s64, m64, images.double(), labels.double(), lr)
        # per-replica contrastive loss differs per rank; its mean over ranks is the global loss
        lt = torch.tensor([float(out['con_loss'].value.item())], dtype=torch.float64, device='cuda' if backend == 'nccl' else 'cpu')
        dist.all_reduce(lt)
        lt = lt.cpu()
        res = {}
        res['loss_rel'] = abs(float(lt) / world - float(t64['con_loss'])) / float(t64['con_loss'])
        byname = {v.name: v for v in model._flat_order}
        worst, worst_name, num, den = 0.0, None, 0.0, 0.0
        for k, ref in t64['grads'].items():
            if ref is None or float(ref.abs().max()) < 1e-12:
                continue
            d = byname[k].grad.double().cpu() - ref
            e = float(d.abs().max()) / float(ref.abs().max())
            num += float((d * d).sum())
            den += float((ref * ref).sum())
            if e > worst:
                worst, worst_name = e, k
        res['grad_worst_rel'] = worst
        res['grad_worst_name'] = worst_name
        res['grad_rel_l2'] = (num / den) ** 0.5                 # over ALL gradient tensors at once
        res['param_worst_rel'] = max(
            float((byname[k].value.double().cpu() - np64[k]).abs().max()) / (float(np64[k].abs().max()) + 1e-30)
            for k in np64)
        res['param_rel_l2'] = (sum(float(((byname[k].value.double().cpu() - np64[k]) ** 2).sum()) for k in np64)
                               / sum(float((np64[k] ** 2).sum()) for k in np64)) ** 0.5
        res['stat_collectives'] = strategy.stat_collectives
        res['hidden_collectives'] = strategy.hidden_collectives
        res['peer_exchanges'] = strategy.peer_stats.exchanges if strategy.peer_stats is not None else 0
        res['peer_missing'] = int(strategy.peer_stats.status.item()) if strategy.peer_stats is not None else 0
        # bit-level fingerprint of the updated weights (the peer-mapped exchange must not change a single bit for R = 2)
        res['checksum'] = [float(sum(float(byname[k].value.double().sum()) for k in np64)),
                           float(max(float(byname[k].value.double().abs().max()) for k in np64))]
        res['bn_moving_worst_rel'] = max(
            float((v.value.double().cpu() - ns64[v.name]).abs().max()) / (float(ns64[v.name].abs().max()) + 1e-30)
            for v in model.variables if v.name in ns64)
        # the same two replicas against the REFERENCE's own two-replica step (tf2/run.py:557-622 compiled from its source and run on two
        # emulated replicas, tests/golden/reference_pin.npz): replica r's scaled loss = (con_r + sup_r + weight_decay) / R
        if world == 2 and os.environ.get('SIMCLR_PEER_STATS') != '1' and depth == 18 and matmul == 'exact':
            from tests import gpu_checks as gc
            mg, ref = gc.reference_pin()
            pin = {}
            for tag in ('r18_cifar', 'r18_img'):
                mm = next(c for c in mg.MODELS if c['tag'] == tag)
                imgs, labs = mg._model_inputs(mm)
                per = mm['batch'] // world
                pm = gc.pinned_product_model(mm, 'f32', 'exact', weight_decay=1e-4, strategy=strategy)
                pstep = make_single_step(pm, model_lib.build_optimizer(0.1), strategy)
                psl = slice(rank * per, (rank + 1) * per)
                po = pstep(torch.from_numpy(imgs[psl]).float().cuda(), {'labels': torch.from_numpy(labs[psl]).float().cuda()})
                torch.cuda.synchronize()
                want = float(ref['step_%s_R2_scaled_loss' % tag][rank])
                pin[tag] = abs(float(po['total_loss'].reshape(-1)[0]) / world - want) / abs(want)
            res['pin_scaled_loss_rel'] = pin
        if os.environ.get('SIMCLR_TEST_ALSO_PEER') == '1':
            # the same step once more with collective C on the peer-mapped exchange (csrc/comm.hip), in the same processes (one spawn +
            # one oracle step instead of two of each): counters and the bit-level fingerprint of the updated weights
            os.environ['SIMCLR_PEER_STATS'] = '1'
            try:
                st2, model2, _ = run_step()
                torch.cuda.synchronize()
                st2.check_health(wait=True)
                by2 = {v.name: v for v in model2._flat_order}
                res['peer'] = dict(stat_collectives=st2.stat_collectives,
                                   peer_exchanges=st2.peer_stats.exchanges if st2.peer_stats is not None else 0,
                                   peer_missing=int(st2.peer_stats.status.item()) if st2.peer_stats is not None else -1,
                                   fallback=st2.peer_stats_fallback,
                                   checksum=[float(sum(float(by2[k].value.double().sum()) for k in np64)),
                                             float(max(float(by2[k].value.double().abs().max()) for k in np64))])
            finally:
                os.environ['SIMCLR_PEER_STATS'] = '0'
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, 'ok', res))
    except Exception:  # noqa
        import traceback
        q.put((rank, 'FAIL', traceback.format_exc()))


def _run(world, backend, env=None):
    for k, v in (env or {}).items():
        os.environ[k] = v
    try:
        return _run_inner(world, backend, fast_mode=bool(env and env.get('SIMCLR_TEST_F32_MATMUL', 'exact') != 'exact'))
    finally:
        for k in (env or {}):
            os.environ.pop(k, None)


def _run_inner(world, backend, fast_mode=False):
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, backend)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=600) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert all(r[1] == 'ok' for r in res), res
    if fast_mode:
        # the product default (three fp16-piece terms forward, three bf16-piece terms backward, pre-split gradients, fused fp32 tails with
        # Gram statistics all-reduced over the replicas): forward quantities as tight as the exact mode, gradients at the three-term level
        for _, _, m in res:
            assert m['loss_rel'] < 1e-5 and m['bn_moving_worst_rel'] < 1e-4, m
            # all gradients at once: the gate of tools/step_modes.py (2e-3 relative L2); the worst single tensor, max-abs relative, is looser
            # (ResNet-50 at 32 px normalises over 16 rows in its last group -- measured 1.1e-2 here, round 6).  A zero-initialised variable
            # (BatchNorm beta, the zero-initialised gamma of each block's last BatchNorm) becomes -lr * gradient after one step, so the
            # worst updated variable carries exactly its gradient's relative error; all variables at once stay at the 1e-4 * that level.
            assert m['grad_rel_l2'] < 2e-3 and m['grad_worst_rel'] < 3e-2, m
            assert m['param_worst_rel'] < 3e-2 and m['param_rel_l2'] < 1e-4, m
            assert m['hidden_collectives'] == 2, m
        return [m for _, _, m in sorted(res)]
    for _, _, m in res:
        # fp32 parity mode, reference initialisation: tight
        assert m['loss_rel'] < 1e-5, m
        assert m['grad_worst_rel'] < 2e-3, m
        assert m['param_worst_rel'] < 1e-4, m
        assert m['bn_moving_worst_rel'] < 1e-4, m
        # ResNet-18: 21 encoder BNs (stem, 8 x 2, 4 projection shortcuts) + 3 head BNs, forward and backward; the 4
        # projection blocks batch (shortcut BN, bn1) forward and (tail BN, shortcut BN) backward into one exchange each
        assert m['hidden_collectives'] == 2, m
        assert m['stat_collectives'] <= 2 * 24 - 8, m
        # replica r's scaled loss of the reference's own two-replica step (north_star: 1e-3 relative)
        for tag, e in m.get('pin_scaled_loss_rel', {}).items():
            assert e < 1e-3, (tag, m)
    return [m for _, _, m in sorted(res)]


_GLOO2 = {}       # the plain two-replica run is shared by the two tests that need it (each run spawns two processes + two oracle steps)


def _gloo2():
    if 'res' not in _GLOO2:
        _GLOO2['res'] = _run(2, 'gloo', env={'SIMCLR_PEER_STATS': '0', 'SIMCLR_TEST_ALSO_PEER': '1'})
    return _GLOO2['res']


def test_two_replica_step_equals_global_batch_oracle():
    res = _gloo2()
    assert all('pin_scaled_loss_rel' in m and len(m['pin_scaled_loss_rel']) == 2 for m in res), res


def test_two_replica_step_in_the_default_fast_parity_mode():
    """ResNet-50 (bottleneck blocks: fused fp32 tails whose Gram-matrix statistics travel through the SyncBN exchange, folded tail BatchNorm
    backward, pre-split gradients) on two replicas in the product's default arithmetic ('f16x3_3') = ONE replica on the global batch (float64
    oracle).  Covers what the 8-GPU run of the headline mode executes per rank."""
    res = _run(2, 'gloo', env={'SIMCLR_PEER_STATS': '0', 'SIMCLR_TEST_DEPTH': '50', 'SIMCLR_TEST_F32_MATMUL': 'f16x3_3'})
    assert len(res) == 2 and all(m['stat_collectives'] > 50 for m in res), res


def _peer_worker(rank, world, port, q, soak):
    try:
        import time
        import numpy as np
        import torch.distributed as dist
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        torch.cuda.set_device(0)
        dist.init_process_group('gloo', rank=rank, world_size=world)
        from simclr_amd import comm
        ps = comm.PeerStats(None, rank, world, torch.device('cuda', 0), max_doubles=4096)      # set-up includes the self-test
        g = torch.Generator().manual_seed(100 + rank)
        worst = 0.0
        for it in range(40):
            n = [1, 2, 128, 130, 1024, 4096, 777, 2 * 2048][it % 8]
            x = (torch.randn(n, generator=g, dtype=torch.float64) * 10.0 ** (it % 5 - 2)).cuda()
            mine = x.clone()
            ps.all_reduce_sum(mine)
            # reference: every rank's block gathered over gloo, added in rank order
            blocks = [torch.zeros(n, dtype=torch.float64) for _ in range(world)]
            dist.all_gather(blocks, x.cpu())
            ref = torch.zeros(n, dtype=torch.float64)
            for b in blocks:
                ref = ref + b
            torch.cuda.synchronize()
            worst = max(worst, float((mine.cpu() - ref).abs().max()))
        # soak: `soak` back-to-back exchanges of random sizes with NO host synchronisation in between, one rank
        # falling behind at random (sleeps of 1 ... 50 ms and one of 1 s): payload rank r, exchange k, index i = (r + 1)(k + 1) + i / 2
        # (exact in fp64), so every rank knows the sum in closed form; the error is accumulated on the device
        sizes = np.random.default_rng(7).integers(1, 4097, soak)            # the same sequence on every rank
        naps = np.random.default_rng(8 + rank)
        tri = world * (world + 1) // 2
        idx = torch.arange(4096, dtype=torch.float64, device='cuda') * 0.5
        err = torch.zeros((), dtype=torch.float64, device='cuda')
        t0 = time.time()
        for k in range(soak):
            n = int(sizes[k])
            x = idx[:n] + float((rank + 1) * (k + 1))
            ps.all_reduce_sum(x)
            err = torch.maximum(err, (x - (world * idx[:n] + float(tri * (k + 1)))).abs().max())
            if rank == world - 1 and (k % 499 == 17 or k == 1234):
                torch.cuda.synchronize()
                time.sleep(1.0 if k == 1234 else float(naps.integers(1, 51)) * 1e-3)
            if k % 200 == 0:
                ps.check_health()
        ps.check_health(wait=True)
        soak_err = float(err.item())
        missing = int(ps.status.item())
        dist.barrier()
        ps.close()
        dist.destroy_process_group()
        q.put((rank, 'ok', dict(worst=worst, missing=missing, exchanges=ps.exchanges, soak_err=soak_err, soak_s=time.time() - t0)))
    except Exception:  # noqa
        import traceback
        q.put((rank, 'FAIL', traceback.format_exc()))


@pytest.mark.parametrize('world', [2, 4])
def test_peer_mapped_stats_exchange(world):
    """csrc/comm.hip: `world` processes on ONE GPU map each other's mailboxes through hipIpc; 40 exchanges of 1 ... 4096 fp64 values
    checked against the rank-ordered sum bit for bit, then a 10 000-exchange soak (random sizes, one rank delayed at random): every
    sum exact, no peer may time out, the sticky health word stays 0."""
    soak = 10000
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_peer_worker, args=(r, world, port, q, soak)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=600) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert all(r[1] == 'ok' for r in res), res
    for _, _, m in res:
        assert m['worst'] == 0.0 and m['soak_err'] == 0.0 and m['missing'] == 0 and m['exchanges'] == 40 + soak, m


def test_two_replica_step_with_peer_mapped_statistics():
    """The two-replica training step with collective C on the peer-mapped exchange (SIMCLR_PEER_STATS=1): every statistic all-reduce
    taken by the new path, no peer ever missing, and the updated weights bit-identical to the gloo run (both runs happen in the worker
    processes of test_two_replica_step_equals_global_batch_oracle: one spawn, one oracle step)."""
    for m in _gloo2():
        p = m['peer']
        assert p['fallback'] is None, p
        assert m['peer_exchanges'] == 0 and p['peer_exchanges'] >= p['stat_collectives'] - 2 and p['peer_missing'] == 0, (m, p)
        assert m['checksum'] == p['checksum'], (m['checksum'], p['checksum'])


def test_two_replica_step_over_rccl():
    """The same identity with one rank per GPU over RCCL ('nccl' backend): all-gather / reduce-scatter of the hidden
    block, SyncBN all-reduces on their own communicator, bucketed gradient all-reduce.  Needs two visible GPUs."""
    if torch.cuda.device_count() < 2:
        pytest.skip('needs >= 2 GPUs (the build session reaches one); the driver runs the multi-GPU bench')
    _run(2, 'nccl')


def _worker_bf16_fused_tail(rank, world, port, q):
    """Two replicas (gloo, both on cuda:0) of a ResNet-50 bf16 step -- the configuration the multi-GPU bench runs: fused
    bottleneck tail with Gram-matrix statistics, folded BatchNorm backward, SyncBN sums all-reduced -- against THIS
    library's single-replica step on the global batch (R replicas == 1 replica on the global batch)."""
    try:
        import torch.distributed as dist
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        torch.cuda.set_device(0)
        dist.init_process_group('gloo', rank=rank, world_size=world)
        from simclr_amd import comm
        from simclr_amd import model as model_lib
        from simclr_amd.flags import FLAGS
        from simclr_amd.resnet import RT
        from simclr_amd.run import make_single_step

        depth, image_size, b, num_classes, lr = 50, 64, 8, 10, 0.1
        g = torch.Generator().manual_seed(11)
        images = torch.rand(world * b, image_size, image_size, 6, generator=g)
        labels = torch.nn.functional.one_hot(torch.randint(0, num_classes, (world * b,), generator=g), num_classes).float()

        def run(strategy, feats, labs):
            FLAGS.reset()
            FLAGS.update(resnet_depth=depth, image_size=image_size, compute_dtype='bf16', use_blur=False,
                         train_batch_size=world * b)
            RT.reset()
            RT.device = torch.device('cuda', 0)
            RT.seed = 77                                     # identical initial weights in every run / rank
            RT.strategy = strategy
            model = model_lib.Model(num_classes)
            opt = model_lib.build_optimizer(lr)
            step = make_single_step(model, opt, strategy)
            out = step(feats.cuda(), {'labels': labs.cuda()})
            torch.cuda.synchronize()
            fused = sum(1 for grp in model.resnet_model.block_groups for blk in grp.layers if getattr(blk, 'fused_tail', False))
            grads = torch.cat([v.grad.reshape(-1).double().cpu() for v in model._flat_order])
            return float(out['con_loss'].value.item()), grads, fused

        strategy = comm.Strategy()
        sl = slice(rank * b, (rank + 1) * b)
        loss_r, grads_r, fused = run(strategy, images[sl], labels[sl])
        lt = torch.tensor([loss_r], dtype=torch.float64)
        dist.all_reduce(lt)
        res = dict(fused_blocks=fused, stat_collectives=strategy.stat_collectives)
        dist.barrier()
        if rank == 0:
            loss_1, grads_1, _ = run(None, images, labels)
            res['loss_rel'] = abs(float(lt) / world - loss_1) / abs(loss_1)
            res['grad_one_minus_cos'] = 1.0 - float(torch.dot(grads_r, grads_1) / (grads_r.norm() * grads_1.norm()))
            res['grad_rel_l2'] = float((grads_r - grads_1).norm() / grads_1.norm())
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, 'ok', res))
    except Exception:  # noqa
        import traceback
        q.put((rank, 'FAIL', traceback.format_exc()))


def test_two_replica_bf16_resnet50_fused_tail_equals_single_replica():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker_bf16_fused_tail, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=900) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert all(r[1] == 'ok' for r in res), res
    for rank, _, m in res:
        assert m['fused_blocks'] == 15, m                # every bottleneck block of ResNet-50 but the network's last one
        if rank == 0:
            # same arithmetic up to the summation order of the statistics (fp64 all-reduce of per-replica sums); bf16 storage
            # rounding turns that into small, not bitwise-zero, differences
            assert m['loss_rel'] < 2e-3, m
            assert m['grad_one_minus_cos'] < 2e-3, m
            assert m['grad_rel_l2'] < 6e-2, m


def _worker_one_rank_rccl(q, port):
    """ONE rank on the 'nccl' backend (= RCCL) with every collective forced on: all_gather_into_tensor and
    reduce_scatter_tensor of the hidden block, the SyncBN all-reduces on their own communicator, the bucketed
    asynchronous gradient all-reduce -- each is the identity with one rank, so the step must equal the strategy-free
    step; what this buys is that none of those calls meets RCCL for the first time inside the multi-GPU bench."""
    try:
        import torch.distributed as dist
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK='0', WORLD_SIZE='1', LOCAL_RANK='0',
                          SIMCLR_FORCE_COLLECTIVES='1')
        from simclr_amd import model as model_lib
        from simclr_amd.flags import FLAGS
        from simclr_amd.resnet import RT
        from simclr_amd.run import init_distributed, make_single_step
        strategy = init_distributed()
        assert strategy is not None and strategy.force and dist.get_backend() == 'nccl'
        assert strategy.stat_group is not strategy.grad_group and strategy.stat_group is not strategy.group
        depth, image_size, b, num_classes, lr = 18, 32, 16, 10, 0.1
        g = torch.Generator().manual_seed(3)
        images = torch.rand(b, image_size, image_size, 6, generator=g).cuda()
        labels = torch.nn.functional.one_hot(torch.randint(0, num_classes, (b,), generator=g), num_classes).float().cuda()

        def run(st):
            FLAGS.reset()
            FLAGS.update(resnet_depth=depth, image_size=image_size, compute_dtype='f32', use_blur=False, train_batch_size=b)
            RT.reset()
            RT.device = torch.device('cuda', 0)
            RT.seed = 9
            RT.strategy = st
            model = model_lib.Model(num_classes)
            step = make_single_step(model, model_lib.build_optimizer(lr), st)
            out = step(images, {'labels': labels})
            torch.cuda.synchronize()
            return float(out['con_loss'].value.item()), torch.cat([v.grad.reshape(-1).double().cpu() for v in model._flat_order])
        l_c, g_c = run(strategy)
        res = dict(stat_collectives=strategy.stat_collectives, hidden_collectives=strategy.hidden_collectives)
        # the raw collectives, shapes as the step issues them ([2n, 128] fp32 hidden block)
        z = torch.randn(2 * b, 128, device='cuda')
        ga = strategy.all_gather_concat(z)
        rs, work = strategy.reduce_scatter_sum(z.clone(), async_op=True)
        work.wait()
        torch.cuda.synchronize()
        res['gather_exact'] = bool(torch.equal(ga, z)) and bool(torch.equal(rs, z))
        l_1, g_1 = run(None)
        res['loss_rel'] = abs(l_c - l_1) / abs(l_1)
        res['grad_rel_l2'] = float((g_c - g_1).norm() / g_1.norm())
        dist.destroy_process_group()
        q.put((0, 'ok', res))
    except Exception:  # noqa
        import traceback
        q.put((0, 'FAIL', traceback.format_exc()))


def test_rccl_collectives_with_one_rank():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    p = ctx.Process(target=_worker_one_rank_rccl, args=(q, _free_port()))
    p.start()
    res = q.get(timeout=600)
    p.join(timeout=60)
    assert res[1] == 'ok', res
    m = res[2]
    assert m['gather_exact'], m
    assert m['hidden_collectives'] == 2 and m['stat_collectives'] > 20, m
    # SyncBN sums go through fp64 [2, C] tensors instead of the fused slot reduction: same values up to fp32 rounding
    assert m['loss_rel'] < 1e-5 and m['grad_rel_l2'] < 1e-3, m


def test_bench_two_ranks_over_gloo_on_one_gpu():
    """`python bench.py --gpus 2 --backend gloo --full`: the self-launch path (torch.distributed.run, one rank per process), the
    N > 1 JSON line and the collective micro-benchmark, with both ranks on cuda:0 over gloo."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, 'bench.py'), '--gpus', '2', '--backend', 'gloo', '--steps', '2', '--warmup', '1',
           '--per_gpu_batch', '16', '--image_size', '64', '--full', '--no_cpu_baseline', '--no_f32', '--prof_steps', '1']
    env = dict(os.environ)
    env.pop('WORLD_SIZE', None)
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=root)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d['n_gpus'] == 2 and d['steps'] == 2 and d['scaling'] == 'weak' and d['config']['global_batch'] == 32
    assert d['value'] > 0 and d['value'] == d['value'] and d['ms_per_step'] > 0
    ag = d['allgather']
    assert ag['ranks'] == 2 and ag['backend'] == 'gloo' and ag['bytes_gathered'] == 2 * ag['bytes_contributed'] and ag['us'] > 0
    assert ag['grad_allreduce']['us'] > 0
    assert ag['hidden_collectives_per_step'] == 2 and ag['stat_collectives_per_step'] > 50
    assert d['roofline'] is not None and d['cpu_baseline'] is None


def _worker_local_bn(rank, world, port, q):
    """--global_bn=False with two replicas: every replica normalises with ITS OWN batch statistics, so a
    replica's forward and gradients equal the single-replica step on its own shard except for the contrastive negatives;
    here the check is on what the bug broke -- the fused tails' Gram-matrix statistics must be divided by the local row
    count: the bf16 ResNet-50 step with fused tails must match the same step with SIMCLR_CONV3_FUSED=0."""
    try:
        import torch.distributed as dist
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        torch.cuda.set_device(0)
        dist.init_process_group('gloo', rank=rank, world_size=world)
        from simclr_amd import comm
        from simclr_amd import model as model_lib
        from simclr_amd.flags import FLAGS
        from simclr_amd.resnet import RT
        from simclr_amd.run import make_single_step
        depth, image_size, b, num_classes, lr = 50, 64, 8, 10, 0.1
        g = torch.Generator().manual_seed(21 + rank)
        images = torch.rand(b, image_size, image_size, 6, generator=g)
        labels = torch.nn.functional.one_hot(torch.randint(0, num_classes, (b,), generator=g), num_classes).float()

        def run(fused):
            os.environ['SIMCLR_CONV3_FUSED'] = fused
            FLAGS.reset()
            FLAGS.update(resnet_depth=depth, image_size=image_size, compute_dtype='bf16', use_blur=False,
                         train_batch_size=world * b, global_bn=False)
            RT.reset()
            RT.device = torch.device('cuda', 0)
            RT.seed = 5
            strategy = comm.Strategy()
            RT.strategy = strategy
            model = model_lib.Model(num_classes)
            step = make_single_step(model, model_lib.build_optimizer(lr), strategy)
            out = step(images.cuda(), {'labels': labels.cuda()})
            torch.cuda.synchronize()
            return (float(out['con_loss'].value.item()), torch.cat([v.grad.reshape(-1).double().cpu() for v in model._flat_order]),
                    strategy.stat_collectives)
        l2, g2, sc = run('2')
        l0, g0, _ = run('0')
        os.environ.pop('SIMCLR_CONV3_FUSED')
        res = dict(loss_rel=abs(l2 - l0) / abs(l0), grad_one_minus_cos=1.0 - float(torch.dot(g2, g0) / (g2.norm() * g0.norm())),
                   stat_collectives=sc)
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, 'ok', res))
    except Exception:  # noqa
        import traceback
        q.put((rank, 'FAIL', traceback.format_exc()))


def test_two_replicas_without_global_bn_fused_tail_matches_unfused():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker_local_bn, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=900) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert all(r[1] == 'ok' for r in res), res
    for _, _, m in res:
        assert m['stat_collectives'] == 0, m           # no statistic exchange without global BatchNorm
        assert m['loss_rel'] < 2e-3 and m['grad_one_minus_cos'] < 5e-3, m


def _peer_fallback_worker(rank, world, port, q):
    try:
        import torch.distributed as dist
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          SIMCLR_PEER_STATS='1', SIMCLR_PEER_TEST_FAIL='1')
        torch.cuda.set_device(0)
        dist.init_process_group('gloo', rank=rank, world_size=world)
        from simclr_amd import comm
        st = comm.Strategy()                      # rank 1 fails to create its mailbox: EVERY rank must fall back, nobody may hang
        x = torch.full((2, 64), float(rank + 1), dtype=torch.float64, device='cuda')
        st.all_reduce_sum(x)                      # collective C over the collective library
        torch.cuda.synchronize()
        st.check_health(wait=True)
        ok = bool((x == float(world * (world + 1) // 2)).all())
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, 'ok', dict(peer=st.peer_stats is None, why=st.peer_stats_fallback, sum_ok=ok)))
    except Exception:  # noqa
        import traceback
        q.put((rank, 'FAIL', traceback.format_exc()))


def test_peer_mapped_exchange_falls_back_collectively():
    """a rank that cannot set up the peer-mapped exchange must not leave the others waiting -- the set-up result is agreed
    collectively and ALL ranks keep the collective library for the SyncBatchNormalization statistics."""
    world = 3
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_peer_fallback_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert all(r[1] == 'ok' for r in res), res
    for _, _, m in res:
        assert m['peer'] and m['sum_ok'] and 'create failed on rank 1' in m['why'], m
