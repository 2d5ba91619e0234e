"""CPU, 2 processes over gloo: DataParallel(sync_bn=True, device_noise_seed=s) makes two ranks compute what one process computes
on the whole batch, forward after forward -- the equivalence global_noise_seed gives, with every rank drawing the noise of its
own clips only (clip_offset = rank * bs). Uses the test double of the kernel interface with the device-noise entry points."""
import os
import sys

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_distributed_cpu import ROOT, _batch, _loss_train, _tiny_model

SEED, STEPS = 77, 2


def _worker(rank, world, port, ret):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    import twog_gcn_amd  # noqa: F401
    from twog_gcn_amd import kernels
    from twog_gcn_amd.distributed import DataParallel
    from tests.gumbel_noise_fake import GumbelNoiseFakeKernels
    fake = GumbelNoiseFakeKernels()
    kernels._set_backend_for_tests(fake)
    torch.set_num_threads(2)
    model = _tiny_model(seed=0)
    dp = DataParallel(model, bucket_mb=1, sync_bn=True, device_noise_seed=SEED)
    xh, xo, mask, tgt, _ = _batch(4)
    sl = slice(rank * 2, rank * 2 + 2)
    torch.manual_seed(rank)            # the host generators of the ranks differ: the noise must not care
    grads = []
    for _ in range(STEPS):
        dp.zero_grad()
        _loss_train(model, xh[sl], xo[sl], mask[sl], tgt[sl]).backward()
        dp.all_reduce_gradients()
        grads.append(dp.flat.grad.clone() * dp.grad_scale)
    ret[rank] = (grads, [c[3] for c in fake.noise_calls], model.device_noise_state())
    dist.destroy_process_group()


def test_two_ranks_with_device_noise_reproduce_the_full_batch_steps():
    import twog_gcn_amd  # noqa: F401
    from twog_gcn_amd import kernels
    from twog_gcn_amd.distributed import DataParallel
    from tests.gumbel_noise_fake import GumbelNoiseFakeKernels
    port = 33500 + os.getpid() % 2000
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(2, port, ret), nprocs=2, join=True)
    for r in (0, 1):
        assert ret[r][1] == [2 * r] * STEPS and ret[r][2] == (SEED, STEPS), ret[r][1:]
    kernels._set_backend_for_tests(GumbelNoiseFakeKernels())
    try:
        model = _tiny_model(seed=0)
        dp = DataParallel(model, sync_bn=True, device_noise_seed=SEED)   # world 1: the whole batch, clip offset 0
        xh, xo, mask, tgt, _ = _batch(4)
        for k in range(STEPS):
            dp.zero_grad()
            _loss_train(model, xh, xo, mask, tgt).backward()
            ref = dp.flat.grad
            for r in (0, 1):
                err = (ret[r][0][k] - ref).abs().max().item()
                assert err < 2e-5 * max(1.0, ref.abs().max().item()), (k, r, err)
        assert not torch.equal(ret[0][0][0], ret[0][0][1])     # the second forward drew other noise
    finally:
        kernels._set_backend_for_tests(None)
