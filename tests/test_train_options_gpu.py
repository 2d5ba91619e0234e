"""GPU: the kernels of the training-step options (csrc/train_opts.hip) and the product path built on them.

  * twog_grad_norm against numpy fp64 (sizes 1, 3, 4097, several ranges, the 45.5 M-element buffer of the headline
    model), with fp32 squares that underflow or overflow, bit-identical over repeated calls; NaN / inf inputs;
  * twog_adam_step_coef bit-identical to twog_adam_step on the host-prepared gradient, and to twog_adam_step itself when
    nothing clips; a sub-range leaves everything outside it untouched;
  * twog_mtl_weight_fwd / _bwd against the reference's formulas restated here in fp64, and against finite differences;
  * G14 (a) and (b) on the HIP kernels; the learner's gradient through a one-rank RCCL group; no host synchronisation.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import twog_gcn_amd  # noqa: F401
from twog_gcn_amd import _lib as L
from twog_gcn_amd import kernels as twog_kernels
from tests.train_options_helpers import G14_CASES, product_g14_trajectory

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE_NUMEL = 45_500_000   # the flat gradient buffer of the headline model (bench.py c3) is ~45.5 M floats


@pytest.fixture(autouse=True)
def hip():
    twog_kernels._set_backend_for_tests(None)
    K = twog_kernels.get_kernels()
    assert K.name == 'hip'
    return K


def _want(buf, ranges, scale, max_norm):
    """The contract (include/twog_gcn.h): fp32(sqrt(fp64 sum of squares) * |scale|); coef = torch's fp32 arithmetic."""
    x = buf.detach().cpu().numpy().astype(np.float64)
    s = sum(float(np.sum(x[b:e] ** 2)) for b, e in ranges)
    norm = np.float32(math.sqrt(s) * abs(scale))
    coef = (torch.tensor(norm, device=DEV) + 1e-6).reciprocal() * max_norm
    return norm, coef.cpu()


def _wide(n, seed):
    """Values over 2^-100 .. 2^100 (fp32 squares underflow at the low end and overflow at the high end), both signs."""
    g = torch.Generator().manual_seed(seed)
    mant = torch.rand(n, generator=g) + 0.5
    expo = torch.randint(-100, 101, (n,), generator=g).float()
    sign = torch.randint(0, 2, (n,), generator=g).float() * 2 - 1
    return (sign * mant * torch.pow(2.0, expo)).float()


@pytest.mark.parametrize('n,ranges', [(1, [(0, 1)]), (3, [(0, 3)]), (4097, [(0, 4097)]), (4097, [(1, 4096)]),
                                      (10_001, [(0, 5), (7, 7), (9, 4099), (4101, 10_001)]),
                                      (70_000, [(3, 17), (64, 65_536), (65_541, 69_999)])])
def test_grad_norm_matches_numpy_fp64(hip, n, ranges):
    buf = _wide(n, seed=n).to(DEV)
    for scale, max_norm in ((1.0, 1.0), (0.5, 3.0), (1.0 / 3.0, 1e30)):
        out = hip.grad_norm(buf, ranges, scale, max_norm)
        norm, coef = _want(buf, ranges, scale, max_norm)
        got = out.cpu()
        assert np.isfinite(norm)
        assert abs(float(got[0]) - float(norm)) <= 1e-6 * float(norm), (float(got[0]), float(norm))
        # the coefficient from the kernel's own norm, as torch computes it: exact
        c_from_got = ((got[0:1].to(DEV) + 1e-6).reciprocal() * max_norm).cpu()
        assert torch.equal(got[1:2], c_from_got), (got, c_from_got, coef)
        for _ in range(3):
            assert torch.equal(hip.grad_norm(buf, ranges, scale, max_norm).cpu(), got)   # fixed summation order


def test_grad_norm_of_the_headline_buffer_is_exact_and_repeatable(hip):
    g = torch.Generator(device=DEV).manual_seed(5)
    buf = torch.randn(HEADLINE_NUMEL, device=DEV, generator=g) * 1e-3
    buf[::1000] *= 1e6   # a few large gradients
    out = hip.grad_norm(buf, [(0, HEADLINE_NUMEL)], 0.25, 1.0)
    norm, _ = _want(buf, [(0, HEADLINE_NUMEL)], 0.25, 1.0)
    got = out.cpu()
    assert abs(float(got[0]) - float(norm)) <= 1e-6 * float(norm)
    for _ in range(3):
        assert torch.equal(hip.grad_norm(buf, [(0, HEADLINE_NUMEL)], 0.25, 1.0).cpu(), got)
    # fp32 squares of every normal value stay finite in the fp64 sum: the largest fp32 magnitudes
    buf[:4] = 3.0e38
    out = hip.grad_norm(buf, [(0, 8)], 1e-30, 1.0).cpu()
    assert math.isfinite(float(out[0])) and abs(float(out[0]) - 6.0e8) < 1e-6 * 6.0e8


def _adam_state(n, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    p = torch.randn(n, device=DEV, generator=g)
    grad = torch.randn(n, device=DEV, generator=g) * 3.0
    m = torch.randn(n, device=DEV, generator=g) * 0.1
    v = torch.rand(n, device=DEV, generator=g) * 0.01
    return p, grad, m, v


def _clone(*ts):
    return [t.clone() for t in ts]


@pytest.mark.parametrize('c', [0.37, 1e-3])
def test_coefficient_adam_equals_adam_on_the_host_prepared_gradient(hip, c):
    p, g, m, v = _adam_state(100_003, seed=1)
    coef = torch.tensor([c], device=DEV)
    a = _clone(p, g, m, v)
    hip.adam_step_coef(a[0], a[1], a[2], a[3], 1e-3, 0.9, 0.999, 1e-8, 0.0, 3, 0.5, coef)
    b = _clone(p, g, m, v)
    prepared = (b[1] * 0.5) * coef   # fl(fl(g * grad_scale) * k) on the device
    hip.adam_step(b[0], prepared, b[2], b[3], 1e-3, 0.9, 0.999, 1e-8, 0.0, 3, 1.0)
    for x, y in zip(a, b):
        if x is not a[1]:
            assert torch.equal(x, y)


@pytest.mark.parametrize('c', [1.0, 7.5, float('nan')])
@pytest.mark.parametrize('wd', [0.0, 0.01])
def test_coefficient_adam_without_clipping_is_adam(hip, c, wd):
    p, g, m, v = _adam_state(65_537, seed=2)
    a, b = _clone(p, g, m, v), _clone(p, g, m, v)
    hip.adam_step_coef(a[0], a[1], a[2], a[3], 1e-3, 0.9, 0.999, 1e-8, wd, 5, 0.25, torch.tensor([c], device=DEV))
    hip.adam_step(b[0], b[1], b[2], b[3], 1e-3, 0.9, 0.999, 1e-8, wd, 5, 0.25)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_coefficient_adam_over_a_sub_range_touches_nothing_else(hip):
    p, g, m, v = _adam_state(10_000, seed=3)
    a = _clone(p, g, m, v)
    lo, hi = 1_001, 8_190
    hip.adam_step_coef(*(t[lo:hi] for t in a), 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.0, torch.tensor([0.5], device=DEV))
    for x, y in zip(a, (p, g, m, v)):
        assert torch.equal(x[:lo], y[:lo]) and torch.equal(x[hi:], y[hi:])
    assert not torch.equal(a[0][lo:hi], p[lo:hi])


def test_non_finite_gradients(hip):
    p, g, m, v = _adam_state(4_099, seed=4)
    # NaN: the norm is NaN and nothing is clipped (torch 1.5.1: `if clip_coef < 1` is false)
    g[17] = float('nan')
    out = hip.grad_norm(g, [(0, g.numel())], 1.0, 1.0)
    assert math.isnan(float(out[0].cpu()))
    a, b = _clone(p, g, m, v), _clone(p, g, m, v)
    hip.adam_step_coef(*a, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.0, out[1:2])
    hip.adam_step(*b, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.0)
    for x, y in zip(a, b):
        assert torch.equal(x.isnan(), y.isnan()) and torch.equal(x.nan_to_num(), y.nan_to_num())
    # inf: norm inf, coefficient 0 -> the reference multiplies every gradient by 0 (inf * 0 = NaN)
    g[17] = float('inf')
    out = hip.grad_norm(g, [(0, g.numel())], 1.0, 1.0).cpu()
    assert math.isinf(float(out[0])) and float(out[1]) == 0.0
    a, b = _clone(p, g, m, v), _clone(p, g, m, v)
    hip.adam_step_coef(*a, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.0, out[1:2].to(DEV))
    hip.adam_step(b[0], b[1] * 0.0, b[2], b[3], 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.0)
    for x, y in zip((a[0], a[2], a[3]), (b[0], b[2], b[3])):
        assert torch.equal(x.isnan(), y.isnan()) and torch.equal(x.nan_to_num(), y.nan_to_num())


# ---- the multi-task loss learner's formulas (pyrutils/torch/multi_task.py:62-71), restated in fp64
def _ref_weight(kind, s):
    if kind == L.MTL_MAE:
        return math.sqrt(2.0) * math.exp(-s)
    return (0.5 if kind == L.MTL_MSE else 1.0) * math.exp(-2 * s)


def _ref_out(kind, L_, s):
    return L_ if kind == L.MTL_PASS else _ref_weight(kind, s) * L_ + s


KINDS = [L.MTL_PASS, L.MTL_SOFTMAX, L.MTL_MSE, L.MTL_MAE, L.MTL_SOFTMAX, L.MTL_MAE, L.MTL_PASS, L.MTL_MSE,
         L.MTL_SOFTMAX, L.MTL_SOFTMAX, L.MTL_MAE, L.MTL_MSE]


def test_weighting_kernels_against_the_restated_formulas_and_finite_differences(hip):
    g = torch.Generator().manual_seed(9)
    n = len(KINDS)
    losses = (torch.rand(n, generator=g) * 3 + 0.05).to(DEV)
    s = (torch.rand(n, generator=g) * 2 - 1).to(DEV)
    dout = (torch.rand(n, generator=g) + 0.5).to(DEV)
    out = hip.mtl_weight_fwd(KINDS, losses, s).cpu().double()
    Lh, sh, dh = losses.cpu().double().tolist(), s.cpu().double().tolist(), dout.cpu().double().tolist()
    for i, k in enumerate(KINDS):
        assert abs(float(out[i]) - _ref_out(k, Lh[i], sh[i])) <= 1e-6 * max(1.0, abs(_ref_out(k, Lh[i], sh[i]))), i
    acc = torch.full((n,), 0.25, device=DEV)
    ds = torch.empty(n, device=DEV)
    dl = hip.mtl_weight_bwd(KINDS, losses, s, dout, ds, accumulate=False).cpu().double()
    dl2 = hip.mtl_weight_bwd(KINDS, losses, s, dout, acc, accumulate=True).cpu().double()
    assert torch.equal(dl, dl2)
    assert torch.allclose((ds + 0.25).cpu(), acc.cpu(), rtol=0, atol=1e-6)
    h = 1e-6
    for i, k in enumerate(KINDS):
        fd_L = (_ref_out(k, Lh[i] + h, sh[i]) - _ref_out(k, Lh[i] - h, sh[i])) / (2 * h) * dh[i]
        fd_s = (_ref_out(k, Lh[i], sh[i] + h) - _ref_out(k, Lh[i], sh[i] - h)) / (2 * h) * dh[i] if k else 0.0
        assert abs(float(dl[i]) - fd_L) <= 1e-5 * max(1.0, abs(fd_L)), (i, float(dl[i]), fd_L)
        assert abs(float(ds[i]) - fd_s) <= 1e-5 * max(1.0, abs(fd_s)), (i, float(ds[i]), fd_s)


@pytest.mark.parametrize('case', G14_CASES)
def test_g14_trajectory_with_clipping_and_the_learner_on_the_hip_kernels(case):
    product_g14_trajectory(case, DEV)


def test_step_and_learner_run_without_a_host_synchronisation(hip):
    from tests.test_train_options_cpu import _tiny_model
    from twog_gcn_amd.distributed import DataParallel, FusedAdam
    from twog_gcn_amd.multi_task import MultiTaskLossLearner
    model = _tiny_model().to(DEV)
    mtll = MultiTaskLossLearner(['budget', 'bce'] + ['softmax'] * 4, [False] * 2 + [True] * 4).to(DEV)
    dp = DataParallel(model, extra_modules=[mtll])
    opt = FusedAdam(dp.flat, lr=1e-3, max_grad_norm=0.1)
    with torch.no_grad():
        dp.flat.grad.copy_(torch.randn(dp.flat.numel, device=DEV))
    raw = torch.rand(6, device=DEV, requires_grad=True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        losses = mtll(list(raw.unbind(0)))
        sum(losses).backward()
        norm = opt.step(dp.grad_scale)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert norm.is_cuda and norm.dim() == 0 and float(norm) > 0.1
    assert raw.grad is not None
    dp.close()


def _nccl_worker(rank, world, port, ret):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY='0')
    torch.cuda.set_device(0)
    dist.init_process_group('nccl', rank=rank, world_size=world, device_id=torch.device('cuda', 0))
    import twog_gcn_amd  # noqa: F401
    from tests.test_train_options_cpu import _batch, _steps, _make
    res = {}
    for forced in (True, False):
        dp, opt, mtll = _make(dict(force_collectives=forced), device=DEV)
        log = []
        real = dp._reduce_range
        dp._reduce_range = lambda b, e, real=real: (log.append((b, e)), real(b, e))[1]
        xh, xo, mask, cls, seg = (t.to(DEV) for t in _batch())
        norms = _steps(dp, opt, mtll, xh, xo, mask, cls, seg)
        torch.cuda.synchronize()
        res[forced] = (dp.flat.flat.cpu(), mtll.log_sds.detach().cpu(), norms, dp.collective_calls, log,
                       dp.flat.module_ranges)
        dp.close()
    ret['forced'], ret['plain'] = res[True], res[False]
    dist.destroy_process_group()


def test_learner_gradient_goes_through_the_collective():
    port = 37100 + os.getpid() % 2000
    ret = mp.Manager().dict()
    mp.spawn(_nccl_worker, args=(1, port, ret), nprocs=1, join=True)
    f, p = ret['forced'], ret['plain']
    (mb, me) = f[5][1]
    assert any(b <= mb and me <= e for b, e in f[4]), (f[4], f[5])   # the learner's slice was all-reduced
    assert p[3] == 0 and f[3] > 0
    assert torch.equal(f[0], p[0]) and torch.equal(f[1], p[1]) and f[2] == p[2]
