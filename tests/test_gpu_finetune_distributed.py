"""train_mode=finetune on two replicas (pytest -m gpu): two ranks share cuda:0 over gloo (SIMCLR_SHARE_GPU=1's transport; RCCL
refuses two ranks on one device), fine_tune_after_block=2.  The frozen BatchNorms still exchange their batch statistics, the gradient
buckets cover the trainable groups only, and the summed gradients of loss / R must equal the product's one-replica step on the
concatenated batch (per tensor within tests/test_gpu_distributed.py's 2e-3) and stay near the float64 oracle."""
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
        from simclr_amd.run import GradSync, make_single_step
        from tests.gpu_checks import structured_images
        from tests.test_gpu_finetune import LR, MOM, WD, _oracle

        k, sel, b, ncls = 2, 1, 8, 10
        cfg = Config(resnet_depth=18, image_size=32, num_classes=ncls, weight_decay=WD, ft_proj_selector=sel)
        params, state = init_model(cfg, seed=3)
        g = torch.Generator().manual_seed(9)
        images = structured_images(world * b, 32, 1, g)                        # global batch, one view
        labels = F.one_hot(torch.randint(0, ncls, (world * b,), generator=g), ncls).float()
        FLAGS.reset()
        FLAGS.update(resnet_depth=18, image_size=32, compute_dtype='f32', f32_matmul='exact', use_blur=False, weight_decay=WD,
                     train_batch_size=world * b, train_mode='finetune', fine_tune_after_block=k, ft_proj_selector=sel, momentum=MOM)
        RT.reset()
        RT.device = torch.device('cuda', 0)
        strategy = comm.Strategy()
        RT.strategy = strategy
        model = model_lib.Model(ncls)
        with torch.no_grad():
            model(torch.zeros(2, 32, 32, 3, device='cuda'), training=False)
        allv = dict(params)
        allv.update(state)
        for v in model.variables:
            v.value.copy_(allv[v.name].cuda())
        RT.weights_version += 1
        before = {v.name: v.value.clone() for v in model.variables}
        step = make_single_step(model, model_lib.build_optimizer(LR), strategy)
        sl = slice(rank * b, (rank + 1) * b)
        out = step(images[sl].cuda(), {'labels': labels[sl].cuda()})
        torch.cuda.synchronize()
        trainable = {v.name for v in model.trainable_variables}
        nograd = {v.name for v in model.variables_without_gradient()}
        ref = _oracle(cfg, params, state, images, labels, trainable - nograd)
        lt = torch.tensor([float(out['sup_loss'].value)], dtype=torch.float64)
        dist.all_reduce(lt)
        res = dict(loss_rel=abs(float(lt) / world - ref['loss']) / ref['loss'])
        worst, worst_name = 0.0, None
        for v in model.trainable_variables:
            if v.name in nograd:
                continue
            r = ref['grads'][v.name]
            if float(r.abs().max()) < 1e-12:
                continue
            e = float((v.grad.double().cpu() - r).abs().max()) / float(r.abs().max())
            if e > worst:
                worst, worst_name = e, v.name
        res['grad_worst_rel'], res['grad_worst_name'] = worst, worst_name
        res['bn_moving_worst_rel'] = max(
            float((v.value.double().cpu() - ref['new_state'][v.name]).abs().max()) / (float(ref['new_state'][v.name].abs().max()) + 1e-30)
            for v in model.variables if 'moving_' in v.name)
        res['frozen_unchanged'] = all(torch.equal(v.value, before[v.name]) and v.grad is None
                                      for v in model.variables if v.name not in trainable and 'moving_' not in v.name)
        res['nograd_unchanged'] = all(torch.equal(v.value, before[v.name]) for v in model.variables if v.name in nograd)
        res['buckets'] = len(GradSync(model, strategy).ranges)
        # against the oracle: all gradients at once, each tensor measured against the global gradient norm (small-batch BatchNorm makes
        # single tensors ill-conditioned against float64 -- the one-replica comparison below is the tight one)
        gn = sum(float((ref['grads'][n] ** 2).sum()) for n in ref['grads']) ** 0.5
        res['oracle_worst_vs_norm'] = max(float((v.grad.double().cpu() - ref['grads'][v.name]).abs().max())
                                          for v in model.trainable_variables if v.name not in nograd) / gn
        grads2 = {v.name: v.grad.double().cpu().clone() for v in model.trainable_variables}
        dist.destroy_process_group()
        # the product's ONE-replica step on the concatenated batch, same process, same variables
        FLAGS.update(train_batch_size=world * b)
        RT.reset()
        RT.device = torch.device('cuda', 0)
        one = model_lib.Model(ncls)
        with torch.no_grad():
            one(torch.zeros(2, 32, 32, 3, device='cuda'), training=False)
        for v in one.variables:
            v.value.copy_(allv[v.name].cuda())
        RT.weights_version += 1
        make_single_step(one, model_lib.build_optimizer(LR), None)(images.cuda(), {'labels': labels.cuda()})
        torch.cuda.synchronize()
        worst, worst_name = 0.0, None
        for v in one.trainable_variables:
            r = v.grad.double().cpu()
            if v.name in nograd or float(r.abs().max()) < 1e-12:
                continue
            e = float((grads2[v.name] - r).abs().max()) / float(r.abs().max())
            if e > worst:
                worst, worst_name = e, v.name
        res['vs_one_replica_worst_rel'], res['vs_one_replica_worst_name'] = worst, worst_name
        q.put((rank, 'ok', res))
    except Exception:  # noqa
        import traceback
        q.put((rank, 'FAIL', traceback.format_exc()))


def test_two_replica_finetune_step_equals_global_batch_oracle():
    os.environ['SIMCLR_PEER_STATS'] = '0'          # the statistics travel over gloo (the peer-mapped exchange has its own tests)
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
        assert m['loss_rel'] < 1e-5, m
        assert m['vs_one_replica_worst_rel'] < 2e-3, m          # two replicas == one replica on the concatenated batch
        assert m['oracle_worst_vs_norm'] < 1e-3, m               # and both near the float64 oracle
        assert m['bn_moving_worst_rel'] < 1e-4, m
        assert m['frozen_unchanged'] and m['nograd_unchanged'], m
        assert m['buckets'] == 2, m              # block groups 4 and 3 (the heads ride in group 4's bucket); no stem bucket
