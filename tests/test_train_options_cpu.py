"""CPU: the reference trainer's two training-step options on the fused step -- gradient-norm clipping
(`clip_gradient_at`, FusedAdam(max_grad_norm=...)) and the multi-task loss learner (MultiTaskLossLearner under
DataParallel(extra_modules=...)) -- on the kernel test double (tests/train_options_helpers.TrainOptionKernels).

  * G14 (a) and (b) (tools/make_golden_train_options.py, the live reference) are reproduced at G12's tolerances;
  * two gloo ranks in the equivalence mode give the single-process result, with the norm of the AVERAGED gradient;
  * with the defaults the step issues the same kernel calls as without the options.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import twog_gcn_amd  # noqa: F401
from twog_gcn_amd import kernels as twog_kernels
from tests.train_options_helpers import G14_CASES, TrainOptionKernels, product_g14_trajectory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def double():
    K = TrainOptionKernels()
    twog_kernels._set_backend_for_tests(K)
    yield K
    twog_kernels._set_backend_for_tests(None)


@pytest.mark.parametrize('case', G14_CASES)
def test_g14_trajectory_with_clipping_and_the_learner_on_the_kernel_test_double(double, case):
    r = product_g14_trajectory(case, 'cpu')
    names = [c[0] for c in double.calls]
    assert names.count('grad_norm') == names.count('adam_step_coef') == len(r['norms'])
    assert names.count('mtl_weight_fwd') == names.count('mtl_weight_bwd') == len(r['norms'])


def _tiny_model(seed=0):
    from twog_gcn_amd.models import TGGCN
    torch.manual_seed(seed)
    return TGGCN(input_size=(2048 + 4 * 26, 2048), num_classes=(13, None), hidden_size=8, gcn_node=26,
                 attention_style='v3', discrete_optimization_strategy='gs', message_segment=True, message_type='v2',
                 message_granularity='v1', message_aggregation='att', object_segment_update_strategy='ind')


def _batch(bs=4, T=4, H=2, O=3, N=26, seed=1):
    g = torch.Generator().manual_seed(seed)
    xh = torch.rand(bs, T, H, 2048 + 4 * N, generator=g)
    xo = torch.rand(bs, T, O, 2048, generator=g)
    cls = torch.randint(0, 13, (bs, T, H), generator=g)
    seg = (torch.rand(bs, T, H, generator=g) < 0.5).float()
    for b, n in enumerate([T, 1, 2, T][:bs]):   # ragged clips: the ranks hold different numbers of valid targets
        cls[b, n:] = -1
        seg[b, n:] = -1.0
    return xh, xo, torch.ones(bs, O), cls, seg


def _steps(dp, opt, mtll, xh, xo, mask, cls, seg, n_steps=2):
    from twog_gcn_amd.losses import select_loss
    crit, _ = select_loss('2G-GCN', 'multiple', 'mphoi', dict(misc=dict(budget_loss=dict(add=True, human_weight=0.7),
                                                                         segmentation_loss=dict(add=True, weight=1.3),
                                                                         first_level_loss_weight=0.5)))
    norms = []
    for _ in range(n_steps):
        dp.zero_grad()
        out = dp.model(xh, xo, mask)
        with dp.loss_scope():
            losses = crit(out, [seg, seg, cls, cls, cls, cls])
        sum(mtll(losses)).backward()
        dp.all_reduce_gradients()
        norms.append(float(opt.step(dp.grad_scale)))
    return norms


MAX_NORM, SEED = 0.05, 11


def _make(dp_kwargs, device='cpu'):
    from twog_gcn_amd.distributed import DataParallel, FusedAdam
    from twog_gcn_amd.losses import select_loss_types, select_loss_learning_mask
    from twog_gcn_amd.multi_task import MultiTaskLossLearner
    model = _tiny_model().to(device).train()
    mtll = MultiTaskLossLearner(select_loss_types('2G-GCN', 'mphoi', {}),
                                select_loss_learning_mask('2G-GCN', 'mphoi', {})).to(device)
    dp = DataParallel(model, extra_modules=[mtll], bucket_mb=1, sync_bn=True, count_weighted_loss=True,
                      global_noise_seed=SEED, **dp_kwargs)
    return dp, FusedAdam(dp.flat, lr=1e-3, max_grad_norm=MAX_NORM), mtll


def _worker(rank, world, port, ret):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    import twog_gcn_amd  # noqa: F401
    from twog_gcn_amd import kernels
    from tests.train_options_helpers import TrainOptionKernels
    kernels._set_backend_for_tests(TrainOptionKernels())
    torch.set_num_threads(2)
    dp, opt, mtll = _make({})
    xh, xo, mask, cls, seg = _batch()
    sl = slice(rank * 2, rank * 2 + 2)
    norms = _steps(dp, opt, mtll, xh[sl], xo[sl], mask[sl], cls[sl], seg[sl])
    ret[rank] = (dp.flat.flat.clone(), mtll.log_sds.detach().clone(), norms, dp.collective_calls)
    dp.close()
    dist.destroy_process_group()


def test_two_ranks_clip_and_learn_like_one_process():
    """Sync-BN, count-weighted loss and global noise: W = 2 ranks compute what one process computes on the whole batch.
    Both options included, every rank ends with the same parameters and log_sds, and the norm is that of the AVERAGED
    gradient (the single-process norm), not W times it."""
    port = 36100 + os.getpid() % 2000
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(2, port, ret), nprocs=2, join=True)
    twog_kernels._set_backend_for_tests(TrainOptionKernels())
    try:
        dp, opt, mtll = _make({})
        norms = _steps(dp, opt, mtll, *_batch())
        flat, log_sds = dp.flat.flat, mtll.log_sds.detach()
        dp.close()
    finally:
        twog_kernels._set_backend_for_tests(None)
    assert torch.equal(ret[0][0], ret[1][0]) and torch.equal(ret[0][1], ret[1][1])
    assert ret[0][2] == ret[1][2]
    assert all(n > MAX_NORM for n in norms)   # every step clips
    for a, b in zip(ret[0][2], norms):
        assert abs(a - b) <= 1e-5 * b, (ret[0][2], norms)
    assert ret[0][3] > 1
    # parameters: one Adam step of lr 1e-3 per step; the ranks' summation order differs from the single process's
    assert float((ret[0][0] - flat).abs().max()) < 2e-2 * 1e-3 * 2
    assert float((ret[0][1] - log_sds).abs().max()) < 1e-5
    assert float((log_sds).abs().max()) > 1e-4   # the learner did move


def test_defaults_issue_the_same_kernel_calls(double):
    """No option: the optimizer step is the one fused Adam launch over the whole flat buffer it always was, and nothing
    of the new entry points runs anywhere in the step."""
    from twog_gcn_amd.distributed import DataParallel, FusedAdam
    xh, xo, mask, cls, seg = _batch()
    model = _tiny_model().train()
    dp = DataParallel(model)
    opt = FusedAdam(dp.flat, lr=1e-3)
    dp.zero_grad()
    out = model(xh, xo, mask)
    torch.nn.functional.nll_loss(out[4], cls, ignore_index=-1).backward()
    dp.all_reduce_gradients()
    before = len(double.calls)
    assert opt.step(dp.grad_scale) is None
    assert double.calls[before:] == [('adam_step', dp.flat.numel)]
    assert not [c for c in double.calls if c[0] in ('grad_norm', 'adam_step_coef', 'mtl_weight_fwd', 'mtl_weight_bwd')]
    assert dp.flat.module_ranges == [(0, dp.flat.numel)]
    dp.close()


def test_extra_modules_follow_the_model_in_the_flat_buffers(double):
    from twog_gcn_amd import ops
    from twog_gcn_amd.distributed import DataParallel, FusedAdam
    from twog_gcn_amd.multi_task import MultiTaskLossLearner
    model = _tiny_model()
    n_model = sum((p.numel() + 3) // 4 * 4 for p in model.parameters())
    mtll = MultiTaskLossLearner(['budget', 'bce'] + ['softmax'] * 4, [False] * 2 + [True] * 4)
    dp = DataParallel(model, extra_modules=[mtll])
    assert dp.flat.module_ranges == [(0, n_model), (n_model, n_model + 8)]
    assert mtll.log_sds.data_ptr() == dp.flat.flat[n_model:].data_ptr()
    assert mtll.log_sds.grad.data_ptr() == dp.flat.grad[n_model:].data_ptr()
    last = max(dp.flat.stage_ranges)
    assert dp.flat.stage_ranges[last] == (n_model, n_model + 8)
    assert max(ops.grad_ready_stage(n) for n, _ in model.named_parameters()) < last
    # max_grad_norm 0 with a learner: still one launch over everything (the learner is stepped with the model)
    opt = FusedAdam(dp.flat)
    before = len(double.calls)
    opt.step()
    assert double.calls[before:] == [('adam_step', dp.flat.numel)]
    # clipping: the norm over the model's slice only, the learner's slice stepped without the coefficient
    opt = FusedAdam(dp.flat, max_grad_norm=1.0)
    before = len(double.calls)
    opt.step()
    assert double.calls[before:] == [('grad_norm', ((0, n_model),)), ('adam_step_coef', n_model), ('adam_step', 8)]
    other = _tiny_model()
    with pytest.raises(ValueError):   # a parameter may live in one place of the flat buffers only
        DataParallel(other, extra_modules=[other])
    dp.close()


def test_learner_mirrors_the_reference_interface(double):
    from twog_gcn_amd.multi_task import MultiTaskLossLearner
    types = ['softmax', 'mse', 'mean_squared_error', 'mae', 'mean_absolute_error', 'budget']
    mtll = MultiTaskLossLearner(types, [True] * 5 + [False])
    assert list(mtll.state_dict()) == ['log_sds'] and mtll.log_sds.shape == (6,)
    with torch.no_grad():
        mtll.log_sds.copy_(torch.tensor([0.3, -0.2, 0.1, 0.4, -0.5, 0.7]))
    L = torch.tensor([1.5, 0.7, 2.0, 0.3, 1.1, 0.9], requires_grad=True)
    out = mtll(list(L.unbind(0)))
    s = mtll.log_sds.detach().double()
    w = torch.stack([torch.exp(-2 * s[0]), 0.5 * torch.exp(-2 * s[1]), 0.5 * torch.exp(-2 * s[2]),
                     2 ** 0.5 * torch.exp(-s[3]), 2 ** 0.5 * torch.exp(-s[4])])
    want = torch.cat([w * L.detach().double()[:5] + s[:5], L.detach().double()[5:]])
    assert torch.allclose(torch.stack(out).double(), want, rtol=1e-6)
    sum(out).backward()
    assert torch.allclose(L.grad.double(), torch.cat([w, torch.ones(1, dtype=torch.float64)]), rtol=1e-6)
    dw = torch.cat([-2 * w[:3], -w[3:]])
    assert torch.allclose(mtll.log_sds.grad.double()[:5], dw * L.detach().double()[:5] + 1, rtol=1e-5)
    assert float(mtll.log_sds.grad[5]) == 0.0
    got = mtll.get_weights()
    assert got[5] is None and np.allclose(got[:5], w.numpy(), rtol=1e-6)
    with torch.no_grad():   # the reference's test() loop
        assert len(mtll.eval()([torch.tensor(1.0)] * 6)) == 6
    with pytest.raises(ValueError, match='loss_type must be one of'):
        MultiTaskLossLearner(['budget'], [True])([torch.tensor(1.0)])
    with pytest.raises(AssertionError, match='must match'):
        mtll([torch.tensor(1.0)] * 5)
