"""CPU: the temporal smoothing loss (truncated MSE between adjacent steps' log-probabilities) off the device --
  * its numpy specification (tests/smooth_loss_ref.py) on hand-computed cases and against torch fp64 autograd of
    clamp((x[t] - x[t-1].detach())^2, max=tau^2), masked and averaged;
  * the host layer (2g-gcn_amd/losses.py: multi_task_loss(..., smoothing=), select_loss with misc.smoothing_loss, the loss-type
    and mask lists, the count reducer) on the test double tests/smooth_loss_fake.py;
  * that nothing changes with the option absent; the ctypes layout of twog_smooth_loss_t against gcc's."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import twog_gcn_amd  # noqa: F401
from twog_gcn_amd import _lib, kernels as twog_kernels, losses, multi_task
from tests import smooth_loss_ref as S
from tests.fake_kernels import FakeKernels
from tests.helpers import ROOT
from tests.smooth_loss_fake import SmoothLossFakeKernels

SHAPES = [(1, 1, 1, 1), (1, 2, 2, 1), (3, 13, 17, 2), (2, 10, 33, 3), (5, 17, 40, 5), (8, 17, 120, 5)]   # (bs, C, T, E)
F32 = np.float32


@pytest.fixture()
def double():
    k = SmoothLossFakeKernels()
    twog_kernels._set_backend_for_tests(k)
    yield k
    twog_kernels._set_backend_for_tests(None)


def _x(steps):
    """(1, 2, T, 1) log-probability-like input: class 0 takes `steps`, class 1 stays at -1."""
    x = np.full((1, 2, len(steps), 1), -1.0, F32)
    x[0, 0, :, 0] = steps
    return x


def _y(labels):
    return np.asarray(labels, np.int64).reshape(1, -1, 1)


# ------------------------------------------------------------------------------------------------ the specification
def test_specification_hand_computed_cases():
    # two steps, D = 1 in class 0 and 0 in class 1: sum 1 over 1 pair x 2 classes
    loss, (s, c), g = S.smooth_loss(_x([-2.0, -1.0]), _y([0, 1]))
    assert (s, c, loss) == (1.0, 2.0, F32(0.5))
    assert g[0, :, :, 0].tolist() == [[0.0, 1.0], [0.0, 0.0]]          # g = 1/2, d = g * 2 D at step t only
    # D = 4 exactly: inside the clamp (boundary included), gradient 8 g
    loss, (s, c), g = S.smooth_loss(_x([-5.0, -1.0]), _y([0, 0]), weight=0.5, dloss=2.0)
    assert (s, c, loss) == (16.0, 2.0, F32(4.0))
    assert g[0, 0, :, 0].tolist() == [0.0, 8.0 * (0.5 * 2.0 / 2.0)]
    # D = 4.125: clamped to tau^2, gradient 0
    loss, (s, c), g = S.smooth_loss(_x([-5.125, -1.0]), _y([0, 0]))
    assert (s, c, loss) == (16.0, 2.0, F32(8.0)) and not g.any()
    # ... and inside a wider clamp
    loss, (s, c), g = S.smooth_loss(_x([-5.125, -1.0]), _y([0, 0]), tau=4.125)
    assert s == 4.125 ** 2 and g[0, 0, 1, 0] == F32(4.125)
    # an ignored middle step removes the two pairs it belongs to: of 4 pairs, (3, 4) and (0, 1) stay
    x = _x([-1.0, -2.0, -4.0, -1.0, -1.5])
    loss, (s, c), g = S.smooth_loss(x, _y([0, 1, -1, 1, 0]))
    assert (s, c) == (1.0 + 0.25, 4.0)
    assert g[0, 0, :, 0].tolist() == [0.0, -0.5, 0.0, 0.0, -0.25]
    # an out-of-range label is an ignored one (the NLL term's rule)
    assert S.forward(x, _y([0, 1, 2, 1, 0]))[1] == (1.25, 4.0)
    assert S.forward(x, _y([0, 1, 1, 1, 0]))[1][1] == 8.0
    # T = 1, and every target ignored: nothing to smooth -- 0, not NaN
    for xs, ys in ((_x([-1.0]), _y([0])), (x, _y([-1] * 5))):
        loss, (s, c), g = S.smooth_loss(xs, ys)
        assert (loss, s, c) == (F32(0.0), 0.0, 0.0) and not g.any() and g.shape == xs.shape


def grid_case(shape, seed, ignored=0.2):
    """Inputs on a 1/8 grid in [-12, 0] (differences exact, many exactly on |D| = 4), about 20 % ignored targets."""
    bs, C, T, E = shape
    g = torch.Generator().manual_seed(seed)
    x = -torch.randint(0, 97, shape, generator=g).float() / 8
    y = torch.randint(0, C, (bs, T, E), generator=g)
    y[torch.rand(bs, T, E, generator=g) < ignored] = -1
    return x, y


@pytest.mark.parametrize('shape', SHAPES)
def test_specification_against_torch_fp64_autograd(shape):
    tau, w = 4.0, 0.7
    x, y = grid_case(shape, seed=sum(shape))
    loss, (s, count), grad = S.smooth_loss(x.numpy(), y.numpy(), weight=w, tau=tau)
    x64 = x.double().requires_grad_(True)
    kept = y != -1
    pair = (kept[:, 1:] & kept[:, :-1]).unsqueeze(1)
    v = torch.clamp((x64[:, :, 1:] - x64.detach()[:, :, :-1]) ** 2, max=tau * tau)
    n = int(pair.sum()) * shape[1]
    assert count == n
    if n == 0:
        assert loss == 0 and not grad.any()
        return
    want = w * (v * pair).sum() / n
    want.backward()
    # at most five fp32 roundings (difference: exact on the grid; quotient, weight, g, the product) ~ 3e-7
    assert abs(float(loss) - float(want.detach())) <= 1e-6 * abs(float(want.detach()))
    gw = x64.grad.numpy()
    assert np.array_equal(grad == 0, gw == 0)
    assert np.all(np.abs(grad.astype(np.float64) - gw) <= 1e-6 * np.abs(gw))
    if shape[2] >= 17:
        d = (x[:, :, 1:] - x[:, :, :-1]).abs()
        assert int((d == tau).sum()) > 0 and int((d > tau).sum()) > 0   # the case sits on the boundary and beyond it


# ------------------------------------------------------------------------------------------------ the host layer
def nll_case(shape, seed, n_terms=3):
    bs, C, T, E = shape
    g = torch.Generator().manual_seed(seed)
    xs = [torch.log_softmax(torch.randn(shape, generator=g) * 3, 1) for _ in range(n_terms)]
    ys = []
    for _ in range(n_terms):
        y = torch.randint(0, C, (bs, T, E), generator=g)
        y[torch.rand(bs, T, E, generator=g) < 0.2] = -1
        ys.append(y)
    return xs, ys


def test_multi_task_loss_with_smoothing_on_the_double(double):
    shape = (3, 5, 9, 2)
    xs, ys = nll_case(shape, 1)
    fns, w = (losses.nll_loss,) * 3, [1.0, 0.5, 2.0]
    smoothing = [(2, 0.3, 4.0), (0, 0.15, 1.5)]
    leaves = [x.clone().requires_grad_(True) for x in xs]
    got = losses.multi_task_loss(leaves, ys, fns, w, smoothing=smoothing)
    # three zipped terms, then the smoothing terms in list order
    assert len(got) == 5
    plain = losses.multi_task_loss([x.clone() for x in xs], ys, fns, w)
    assert all(torch.equal(a.detach(), b) for a, b in zip(got[:3], plain))
    for v, (i, sw, tau) in zip(got[3:], smoothing):
        assert float(v.detach()) == float(S.forward(xs[i].numpy(), ys[i].numpy(), sw, tau)[0])
    # the list is the unbind of ONE contiguous base: the loss learner reads it in place
    base = got[0]._base
    assert base is not None and base.shape == (5,) and base.is_contiguous() and base.dtype == torch.float32
    assert multi_task._loss_tensor(got) is base
    names = [c[0] for c in double.calls]
    assert names == ['multitask_loss_fwd', 'smooth_loss_fwd', 'multitask_loss_fwd']
    assert double.calls[0][2:] == ((), {'room': 2}) and double.calls[2][2:] == ((), {})
    # one gradient per input: NLL gradient + smoothing gradient, the smoothing launch adding into the NLL launch's buffer
    double.calls.clear()
    up = torch.tensor([1.0, 2.0, 0.5, 3.0, 0.25])
    (torch.stack(got) * up).sum().backward()
    assert [c[0] for c in double.calls] == ['multitask_loss_bwd', 'smooth_loss_bwd']
    assert double.calls[1][1:] == ((True, True), (True, True))
    for i, (x, y) in enumerate(zip(xs, ys)):
        xr = x.clone().requires_grad_(True)
        (w[i] * up[i] * torch.nn.functional.nll_loss(xr, y, ignore_index=-1)).backward()
        want = xr.grad
        for j, (k, sw, tau) in enumerate(smoothing):
            if k == i:
                want = want + torch.from_numpy(S.gradient(x.numpy(), y.numpy(), sw, tau, dloss=float(up[3 + j])))
        assert torch.allclose(leaves[i].grad, want, rtol=1e-6, atol=1e-9), i


def test_smoothing_terms_without_backward_work(double):
    xs, ys = nll_case((2, 4, 6, 2), 2)
    fns = (losses.nll_loss,) * 3
    # weight 0 on the smoothing term of input 0; input 1 needs no gradient; input 2: NLL weight 0, smoothing stores
    leaves = [xs[0].clone().requires_grad_(True), xs[1].clone(), xs[2].clone().requires_grad_(True)]
    got = losses.multi_task_loss(leaves, ys, fns, [1.0, 1.0, 0.0], smoothing=[(0, 0.0, 4.0), (1, 0.2, 4.0), (2, 0.2, 4.0)])
    assert float(got[3].detach()) == 0.0 and float(got[2].detach()) == 0.0
    double.calls.clear()
    sum(got).backward()
    assert double.calls == [('multitask_loss_bwd', (True, False, False)),
                            ('smooth_loss_bwd', (False, False, True), (False, False, False))]
    assert torch.equal(leaves[2].grad, torch.from_numpy(S.gradient(xs[2].numpy(), ys[2].numpy(), 0.2, 4.0)))
    # nothing to do at all: no backward launch of either kind
    leaves = [x.clone().requires_grad_(True) for x in xs]
    got = losses.multi_task_loss(leaves, ys, fns, [0.0] * 3, smoothing=[(0, 0.0, 4.0)])
    double.calls.clear()
    sum(got).backward()
    assert double.calls == [] and all(x.grad is None for x in leaves)
    # only smoothing needs a gradient: the NLL backward launch is skipped
    leaves = [x.clone().requires_grad_(True) for x in xs]
    got = losses.multi_task_loss(leaves, ys, fns, [0.0] * 3, smoothing=[(1, 1.0, 4.0)])
    double.calls.clear()
    sum(got).backward()
    assert [c[0] for c in double.calls] == ['smooth_loss_bwd']
    assert leaves[0].grad is None and leaves[1].grad is not None


def test_stand_alone_function_and_argument_checks(double):
    xs, ys = nll_case((2, 4, 6, 2), 3, n_terms=1)
    x = xs[0].clone().requires_grad_(True)
    v = losses.temporal_smoothing_loss(x, ys[0], tau=2.0)
    loss, _, grad = S.smooth_loss(xs[0].numpy(), ys[0].numpy(), 1.0, 2.0)
    assert float(v.detach()) == float(loss)
    v.backward()
    assert torch.equal(x.grad, torch.from_numpy(grad))
    assert float(losses.temporal_smoothing_loss(xs[0][:, :, :1], ys[0][:, :1])) == 0.0       # one step: 0, not NaN
    fns = (losses.nll_loss, losses.budget_loss)
    two = [xs[0], torch.rand(2, 6, 2)], [ys[0], torch.ones(2, 6, 2)]
    with pytest.raises(ValueError):
        losses.multi_task_loss(*two, fns, smoothing=[(1, 1.0, 4.0)])       # not an NLL term
    with pytest.raises(ValueError):
        losses.multi_task_loss(*two, fns, smoothing=[(2, 1.0, 4.0)])       # past the zipped terms
    with pytest.raises(ValueError):
        losses.multi_task_loss(*two, fns, smoothing=[(0, 1.0, 0.0)])       # tau <= 0
    with pytest.raises(ValueError):
        losses.multi_task_loss(*two, fns, smoothing=[(0, 1.0, 4.0), (0, 1.0, 2.0)])   # two launch columns, one buffer


# ------------------------------------------------------------------------------------------------ nothing changes without it
MISC = dict(anticipation_loss_weight=0.6, budget_loss=dict(add=True, human_weight=0.5, object_weight=0.25),
            first_level_loss_weight=0.3, segmentation_loss=dict(add=True, pretrain=False, weight=0.7))
TODAY = {   # what the three functions return on the parent commit, per dataset: (names, weights under MISC, types, mask)
    'mphoi': (['B_HS', 'BCE_HS', 'NLL_SAR_F', 'NLL_SAP_F', 'NLL_SAR', 'NLL_SAP'], [0.5, 0.7, 0.3, 0.3, 1.0, 0.6],
              ['budget', 'bce'] + ['softmax'] * 4, [False] * 2 + [True] * 4),
    'bimanual': (['B_HS', 'BCE_HS', 'NLL_SAR_F', 'NLL_SAP_F', 'NLL_SAR', 'NLL_SAP'], [0.5, 0.7, 0.3, 0.3, 1.0, 0.6],
                 ['budget', 'bce'] + ['softmax'] * 4, [False] * 2 + [True] * 4),
    'cad120': (['B_HS', 'B_OS', 'BCE_HS', 'BCE_OS', 'NLL_SAR_F', 'NLL_SAP_F', 'NLL_OAR_F', 'NLL_OAP_F', 'NLL_SAR', 'NLL_SAP',
                'NLL_OAR', 'NLL_OAP'], [0.5, 0.25, 0.7, 0.7] + [0.3] * 4 + [1.0, 0.6, 1.0, 0.6],
               ['budget'] * 2 + ['bce'] * 2 + ['softmax'] * 8, [False] * 4 + [True] * 8),
}


@pytest.mark.parametrize('ds', sorted(TODAY))
@pytest.mark.parametrize('extra', [{}, {'smoothing_loss': {'add': False, 'weight': 0.5, 'tau': 2.0}}])
def test_without_the_key_the_lists_are_todays(ds, extra):
    names, weights, types, mask = TODAY[ds]
    cfg = dict(misc=dict(MISC, **extra))
    crit, got_names = losses.select_loss('2G-GCN', 'multiple', ds, cfg)
    assert got_names == names
    assert crit.func is losses.multi_task_loss and crit.args == () and sorted(crit.keywords) == ['loss_functions', 'weight']
    assert crit.keywords['weight'] == weights and len(crit.keywords['loss_functions']) == len(names)
    assert losses.select_loss_types('2G-GCN', ds, cfg) == types
    assert losses.select_loss_learning_mask('2G-GCN', ds, cfg) == mask


def test_without_smoothing_the_old_calls_are_made():
    """On the UNCHANGED test double (no `room` parameter, no smooth_* method): the call shape of the parent commit."""
    class Recording(FakeKernels):
        def multitask_loss_fwd(self, *args, **kwargs):
            self.calls.append(('multitask_loss_fwd', len(args), dict(kwargs)))
            return FakeKernels.multitask_loss_fwd(self, *args, **kwargs)

    k = Recording()
    twog_kernels._set_backend_for_tests(k)
    try:
        xs, ys = nll_case((2, 4, 6, 2), 4, n_terms=4)
        outs = [torch.rand(2, 6, 2) * 0.9 + 0.05 for _ in range(2)] + xs
        tgts = [torch.ones(2, 6, 2)] * 2 + ys
        for cfg in (dict(misc=MISC), dict(misc=dict(MISC, smoothing_loss=dict(add=False)))):
            crit, _ = losses.select_loss('2G-GCN', 'multiple', 'mphoi', cfg)
            leaves = [o.clone().requires_grad_(True) for o in outs]
            sum(crit(leaves, tgts)).backward()
        leaves = [o.clone().requires_grad_(True) for o in outs]
        fns = (losses.budget_loss, losses.binary_cross_entropy_loss) + (losses.nll_loss,) * 4
        sum(losses.multi_task_loss(leaves, tgts, fns, smoothing=None)).backward()
        assert k.calls == [('multitask_loss_fwd', 1, {})] * 3
        assert not [m for m in dir(k) if m.startswith('smooth_')]
    finally:
        twog_kernels._set_backend_for_tests(None)


# ------------------------------------------------------------------------------------------------ with the key
@pytest.mark.parametrize('ds,n_main,suffixes', [('mphoi', 6, ['SAR', 'SAP']), ('bimanual', 6, ['SAR', 'SAP']),
                                                ('cad120', 12, ['SAR', 'SAP', 'OAR', 'OAP'])])
@pytest.mark.parametrize('pretrain', [False, True])
def test_select_loss_with_the_key(ds, n_main, suffixes, pretrain):
    names, weights, types, mask = TODAY[ds]
    misc = dict(MISC, smoothing_loss=dict(add=True, weight=0.25, tau=3.0))
    misc['segmentation_loss'] = dict(MISC['segmentation_loss'], pretrain=pretrain)
    crit, got_names = losses.select_loss('2G-GCN', 'multiple', ds, dict(misc=misc))
    m = len(suffixes)
    assert got_names == names + ['TMSE_' + s for s in suffixes] and len(got_names) == n_main + m
    w = crit.keywords['weight']
    final = [0.0, 0.6] * (m // 2) if pretrain else weights[-m:]        # pretraining zeroes the recognition terms only
    assert w[-m:] == final and len(w) == n_main
    assert crit.keywords['smoothing'] == [(n_main - m + j, 0.25 * final[j], 3.0) for j in range(m)]
    assert losses.select_loss_types('2G-GCN', ds, dict(misc=misc)) == types + ['mse'] * m
    assert losses.select_loss_learning_mask('2G-GCN', ds, dict(misc=misc)) == mask + [False] * m
    # the defaults of the key: weight 0.15, tau 4 (MS-TCN's)
    crit, _ = losses.select_loss('2G-GCN', 'multiple', ds, dict(misc=dict(MISC, smoothing_loss=dict(add=True))))
    assert crit.keywords['smoothing'] == [(n_main - m + j, 0.15 * weights[n_main - m + j], 4.0) for j in range(m)]


def _criterion_case(ds, seed=5, shape=(3, 6, 8)):
    bs, T, C = shape
    cad = ds == 'cad120'
    g = torch.Generator().manual_seed(seed)
    outs, tgts = [], []
    for i in range(12 if cad else 6):
        E = 2 + i % 2
        if i < (4 if cad else 2):
            outs.append(torch.rand(bs, T, E, generator=g) * 0.9 + 0.05)
            t = (torch.rand(bs, T, E, generator=g) > 0.5).float()
            t[torch.rand(bs, T, E, generator=g) < 0.2] = -1.0
        else:
            outs.append(torch.log_softmax(torch.randn(bs, C, T, E, generator=g) * 3, 1))
            t = torch.randint(0, C, (bs, T, E), generator=g)
            t[torch.rand(bs, T, E, generator=g) < 0.2] = -1
        tgts.append(t)
    return outs, tgts


@pytest.mark.parametrize('ds', ['mphoi', 'cad120'])
def test_loss_learner_passes_the_smoothing_terms_through(ds, double):
    cfg = dict(misc=dict(MISC, smoothing_loss=dict(add=True)))
    crit, names = losses.select_loss('2G-GCN', 'multiple', ds, cfg)
    learner = multi_task.MultiTaskLossLearner(losses.select_loss_types('2G-GCN', ds, cfg),
                                              losses.select_loss_learning_mask('2G-GCN', ds, cfg))
    with torch.no_grad():
        learner.log_sds.copy_(torch.linspace(-0.5, 0.5, len(names)))
    outs, tgts = _criterion_case(ds)
    raw = crit([o.clone().requires_grad_(True) for o in outs], tgts)
    assert len(raw) == len(names) == (16 if ds == 'cad120' else 8)
    out = learner(raw)
    m = 4 if ds == 'cad120' else 2
    assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(out[-m:], raw[-m:]))      # not learned: unchanged
    assert not torch.equal(out[-m - 1].detach(), raw[-m - 1].detach())                         # the NLL terms are
    assert ('mtl_weight_fwd', len(names)) in double.calls
    assert learner.get_weights()[-m:] == [None] * m


# ------------------------------------------------------------------------------------------------ the count reducer
def _run_reduced(ds, reducer):
    cfg = dict(misc=dict(MISC, smoothing_loss=dict(add=True)))
    crit, _ = losses.select_loss('2G-GCN', 'multiple', ds, cfg)
    outs, tgts = _criterion_case(ds)
    leaves = [o.clone().requires_grad_(True) for o in outs]
    if reducer is None:
        got = crit(leaves, tgts)
    else:
        with losses.count_reducer_scope(reducer):
            got = crit(leaves, tgts)
    sum(got).backward()
    return [v.detach().clone() for v in got], [x.grad for x in leaves]


def test_count_reducer_covers_the_smoothing_terms(double):
    plain_l, plain_g = _run_reduced('mphoi', None)
    seen = []
    same_l, same_g = _run_reduced('mphoi', lambda c: (seen.append(c.clone()), c)[1])
    assert len(seen) == 1 and seen[0].shape == (8,)                       # ONE reduction covers all eight counts
    assert all(torch.equal(a, b) for a, b in zip(plain_l, same_l))        # identity reducer: bit-identical
    assert all(torch.equal(a, b) for a, b in zip(plain_g, same_g))
    half_l, half_g = _run_reduced('mphoi', lambda c: c * 2)               # twice the count: half the loss and the gradient
    for a, b in zip(plain_l[6:], half_l[6:]):
        assert float(a) != 0 and torch.equal(a * 0.5, b)
    # (inputs 4 and 5 carry NLL + smoothing; both halve, and powers of two commute with every rounding)
    assert all(torch.equal(a * 0.5, b) for a, b in zip(plain_g[4:], half_g[4:]))


def test_count_reducer_zero_count_gives_zero_not_nan(double):
    xs, ys = nll_case((2, 4, 6, 2), 6, n_terms=1)
    ys[0][:] = -1                                                         # every target ignored: no pair on this rank
    x = xs[0].clone().requires_grad_(True)
    with losses.count_reducer_scope(lambda c: c * 0):                     # ... nor on any other
        got = losses.multi_task_loss([x], ys, (losses.nll_loss,), [1.0], smoothing=[(0, 0.5, 4.0)])
    assert torch.isnan(got[0]) and float(got[1].detach()) == 0.0                   # NLL: torch's empty mean; smoothing: 0
    got[1].backward()
    assert float(x.grad.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ the C ABI
def test_struct_layout_matches_the_c_compiler(tmp_path):
    header = os.path.join(ROOT, 'include', 'twog_gcn.h')
    src = tmp_path / 'sz.c'
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{header}"\nint main(void){{'
                   'printf("%zu %zu %zu %zu\\n", sizeof(twog_smooth_loss_t), offsetof(twog_smooth_loss_t, input), '
                   'offsetof(twog_smooth_loss_t, weight), offsetof(twog_smooth_loss_t, accumulate));return 0;}\n')
    exe = tmp_path / 'sz'
    subprocess.run(['gcc', str(src), '-o', str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    T = _lib.SmoothLoss
    assert [int(v) for v in out] == [ctypes.sizeof(T), T.input.offset, T.weight.offset, T.accumulate.offset]
    assert ctypes.sizeof(T) % 8 == 0
    assert {'twog_smooth_loss_fwd', 'twog_smooth_loss_bwd'} <= set(_lib.exported_symbols())
