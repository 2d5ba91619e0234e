"""CPU: class weights on the NLL terms and the positive-class weight of the BCE terms, off the device --
  * the numpy specification (tests/class_weight_ref.py) against golden G19 (the reference's binary_cross_entropy_loss with
    positive_class_weight, F.nll_loss(weight=)) and against torch fp64 autograd;
  * losses.class_weights against sklearn and against the effective-number formula; losses.class_counts;
  * the host layer (2g-gcn_amd/losses.py: nll_loss(weight=), binary_cross_entropy_loss(positive_class_weight=),
    multi_task_loss(class_weights=, positive_class_weights=), select_loss with misc.class_weights and
    misc.segmentation_loss.positive_class_weight, the count reducer) on the test double tests/class_weight_fake.py;
  * the ctypes layout of twog_wloss_t against gcc's."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import twog_gcn_amd  # noqa: F401
from twog_gcn_amd import _lib, kernels as twog_kernels, losses, multi_task
from tests import class_weight_ref as W
from tests import smooth_loss_ref as S
from tests.class_weight_fake import ClassWeightFakeKernels
from tests.helpers import GOLDEN, ROOT
from tests.test_smooth_loss_cpu import MISC, TODAY, _criterion_case, nll_case

F32, F64 = np.float32, np.float64
ULP = float(np.finfo(F32).eps)
# tools/make_golden_class_weights.py prints, for the fp64 form of the specification against the reference:
GOLDEN_DEV = {'bce': (7.690e-08, 1.590e-07), 'nll': (1.966e-07, 1.916e-07)}     # (loss, gradient), relative


@pytest.fixture()
def double():
    k = ClassWeightFakeKernels()
    twog_kernels._set_backend_for_tests(k)
    yield k
    twog_kernels._set_backend_for_tests(None)


def rel(a, b):
    """Largest |a - b| / |b| over the elements where b != 0; the zeros must coincide."""
    a, b = np.asarray(a, F64).ravel(), np.asarray(b, F64).ravel()
    assert np.array_equal(a == 0, b == 0)
    nz = b != 0
    return float(np.max(np.abs(a[nz] - b[nz]) / np.abs(b[nz]))) if nz.any() else 0.0


# ------------------------------------------------------------------------------------------------ the specification
def test_specification_against_golden_g19():
    """The fp64 form of the specification deviates from the reference by at most (printed by the tool that wrote G19)
        BCE with positive_class_weight: loss 7.690e-08, gradient 1.590e-07
        NLL with class weights:         loss 1.966e-07, gradient 1.916e-07
    relative, the reference's own fp32 rounding. Gate: four times those (far inside the project's loss gate of 1e-5). The
    fp32 specification adds its own roundings, at most five of half an ulp each per value (the quotient sum / den, the
    product with w, g, and the two or three operations of the gradient): its gate is wider by 4 ulp."""
    G = np.load(os.path.join(GOLDEN, 'g19_class_weights.npz'))
    x, t = G['bce_x'], G['bce_t']
    assert x.min() >= 1e-3 and x.max() <= 1 - 1e-3 and {0.0, 0.5, 1.0, -1.0} <= set(t.ravel().tolist())
    gate_l, gate_g = (4 * v for v in GOLDEN_DEV['bce'])
    assert gate_l <= 1e-5 and gate_g <= 1e-5
    for p in G['bce_p'].tolist():
        for real, slack in ((F64, 0.0), (F32, 4 * ULP)):
            loss, (_, den) = W.forward(W.BCE, x, t, positive_class_weight=p, real=real)
            grad = W.gradient(W.BCE, x, t, positive_class_weight=p, den=den, real=real)
            dl, dg = rel(loss, G[f'bce_loss_{p}']), rel(grad, G[f'bce_grad_{p}'])
            print(f'BCE p={p} {real.__name__}: loss {dl:.3e}, gradient {dg:.3e}')
            assert dl <= gate_l + slack and dg <= gate_g + slack
    assert np.array_equal(G['bce_grad_0.5'], G['bce_grad_1.0']) and not np.array_equal(G['bce_grad_1.0'], G['bce_grad_2.0'])
    xn, y, cws = G['nll_x'], G['nll_y'], G['nll_cw']
    assert (y == -1).any() and cws[1, 4] == 0 and (y == 4).any()
    gate_l, gate_g = (4 * v for v in GOLDEN_DEV['nll'])
    assert gate_l <= 1e-5 and gate_g <= 1e-5
    for k, cw in enumerate(cws):
        for real, slack in ((F64, 0.0), (F32, 4 * ULP)):
            loss, (_, den) = W.forward(W.NLL, xn, y, class_weight=cw, real=real)
            grad = W.gradient(W.NLL, xn, y, class_weight=cw, den=den, real=real)
            dl, dg = rel(loss, G[f'nll_loss_{k}']), rel(grad, G[f'nll_grad_{k}'])
            print(f'NLL weights {k} {real.__name__}: loss {dl:.3e}, gradient {dg:.3e}')
            assert dl <= gate_l + slack and dg <= gate_g + slack


def bce_case(shape, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(shape, generator=g) * (1 - 2e-3) + 1e-3
    t = (torch.rand(shape, generator=g) < 0.35).float()
    t[torch.rand(shape, generator=g) < 0.2] = -1.0
    t.view(-1)[::7] = 0.5
    return x, t


CW13 = [0.7, 1.3, 0.0, 1e-3, 1e3, 2.0, 0.5, 1.0, 1.0, 3.0, 0.25, 1.5, 0.9]


@pytest.mark.parametrize('shape', [(1, 13, 1, 1), (3, 13, 17, 2), (5, 13, 40, 5)])
def test_nll_specification_against_torch_fp64_autograd(shape):
    xs, ys = nll_case(shape, seed=sum(shape), n_terms=1)
    x, y, cw = xs[0], ys[0], torch.tensor(CW13)
    loss, (s, den) = W.forward(W.NLL, x.numpy(), y.numpy(), 0.7, class_weight=cw.numpy())
    grad = W.gradient(W.NLL, x.numpy(), y.numpy(), 0.7, class_weight=cw.numpy(), dloss=1.5, den=den)
    x64 = x.double().requires_grad_(True)
    want = 0.7 * F.nll_loss(x64, y, weight=cw.double(), ignore_index=-1)
    if den == 0:
        assert np.isnan(loss) and torch.isnan(want) and not grad.any()
        return
    (1.5 * want).backward()
    # at most four fp32 roundings per value (quotient, weight, g, the product with cw) ~ 2.4e-7
    assert rel(loss, float(want.detach())) <= 1e-6
    assert rel(grad, x64.grad.numpy()) <= 1e-6
    assert den == float(cw.double()[y[y >= 0]].sum())


@pytest.mark.parametrize('p', [0.5, 1.0, 1.5, 2.0, 3.0])
def test_bce_specification_against_torch_fp64_autograd(p):
    x, t = bce_case((3, 17, 2), seed=7)
    loss, (s, den) = W.forward(W.BCE, x.numpy(), t.numpy(), 0.7, positive_class_weight=p)
    grad = W.gradient(W.BCE, x.numpy(), t.numpy(), 0.7, positive_class_weight=p, dloss=1.5, den=den)
    x64, t64 = x.double().requires_grad_(True), t.double()
    plain = -(t64 * torch.log(x64) + (1 - t64) * torch.log(1 - x64))
    term = torch.where((t64 == 1) & (p > 1), -p * torch.log(x64), plain)
    kept = t64 != -1
    want = 0.7 * (term * kept).sum() / kept.sum()
    (1.5 * want).backward()
    assert den == float(kept.sum())
    # fp32 log (1 ulp) and at most six roundings per value; x - t and 1 - x cancel at most three bits on [1e-3, 1 - 1e-3]
    assert rel(loss, float(want.detach())) <= 2e-6
    assert rel(grad, x64.grad.numpy()) <= 2e-6
    if p <= 1:
        assert W.forward(W.BCE, x.numpy(), t.numpy(), 0.7)[0] == loss
        assert np.array_equal(W.gradient(W.BCE, x.numpy(), t.numpy(), 0.7, dloss=1.5), grad)


def test_specification_clamps_and_zero_weight():
    x, t = np.asarray([0.0, 1.0, 0.5, 0.25], F32), np.asarray([1.0, 1.0, -1.0, 0.5], F32)
    loss, (s, den) = W.forward(W.BCE, x, t, 0.5, positive_class_weight=2.0)
    half = -(0.5 * np.log(F32(0.25)) + 0.5 * np.log(F32(0.75)))
    assert den == 3 and abs(s - (100.0 + 0.0 + float(half))) < 1e-5                # x = 0: clamped to 100; x = 1: 0
    g = W.gradient(W.BCE, x, t, 0.5, positive_class_weight=2.0, den=den)
    assert g[0] == F32(F32(F32(0.5) / F32(3)) * F32(-1) / F32(1e-12) * F32(2)) and g[1] == 0 and g[2] == 0
    assert g[3] == W.gradient(W.BCE, x, t, 0.5, den=den)[3]                         # the smoothed 0.5 is not touched by p
    xn = np.log(np.full((2, 3, 2), 1 / 3, F32))
    y = np.asarray([[1, -1], [1, 1]], np.int64)
    loss, (s, den) = W.forward(W.NLL, xn, y, class_weight=np.asarray([1, 0, 2], F32))
    assert np.isnan(loss) and (s, den) == (0.0, 0.0)                                # all kept weight is zero: 0 / 0
    assert not W.gradient(W.NLL, xn, y, class_weight=np.asarray([1, 0, 2], F32), den=den).any()


# ------------------------------------------------------------------------------------------------ the weights
def test_class_weights_balanced_against_sklearn_and_effective_against_its_formula():
    from sklearn.utils.class_weight import compute_class_weight
    counts = np.asarray([900, 40, 0, 7, 53, 1], np.int64)                            # class 2 is absent
    y = np.repeat(np.arange(6), counts)
    w = losses.class_weights(torch.from_numpy(counts), 'balanced')
    assert w.dtype == torch.float32 and w.shape == (6,) and w.device.type == 'cpu'
    present = np.flatnonzero(counts)
    want = np.zeros(6)
    want[present] = compute_class_weight('balanced', classes=present, y=y)
    assert np.array_equal(w.numpy(), want.astype(F32)) and w[2] == 0
    assert np.array_equal(losses.class_weights(counts.tolist()).numpy(), w.numpy())   # a host sequence is taken too
    beta = 0.99
    e = losses.class_weights(torch.from_numpy(counts), 'effective', beta=beta).numpy()
    raw = np.where(counts > 0, (1 - beta) / (1 - np.power(beta, np.maximum(counts, 1).astype(F64))), 0.0)
    assert np.allclose(e, raw * 5 / raw.sum(), rtol=1e-6) and e[2] == 0 and abs(e.sum() - 5) < 1e-5
    assert e[5] > e[3] > e[1] > e[4] > e[0] > 0                                       # rarer classes weigh more
    d = losses.class_weights(torch.from_numpy(counts), 'effective').numpy()          # the default beta, 0.999
    raw = np.where(counts > 0, 1e-3 / (1 - np.power(0.999, np.maximum(counts, 1).astype(F64))), 0.0)
    assert np.allclose(d, raw * 5 / raw.sum(), rtol=1e-6)
    with pytest.raises(ValueError):
        losses.class_weights(torch.from_numpy(counts), 'inverse')
    with pytest.raises(ValueError):
        losses.class_weights(torch.from_numpy(counts), 'effective', beta=1.0)


def test_class_counts_accumulates_on_the_double(double):
    y = torch.tensor([[0, 3, 3, -1], [5, 9, -5, 3]])
    c = losses.class_counts(y, 6)
    assert c.dtype == torch.int64 and c.tolist() == [1, 0, 0, 3, 0, 1]
    assert losses.class_counts(y.to(torch.int32), 6, out=c) is c and c.tolist() == [2, 0, 0, 6, 0, 2]
    assert losses.class_counts(y, 6, ignore_index=3).tolist() == [1, 0, 0, 0, 0, 1]


# ------------------------------------------------------------------------------------------------ the host layer
def test_stand_alone_functions_on_the_double(double):
    xs, ys = nll_case((3, 13, 9, 2), 1, n_terms=1)
    x = xs[0].clone().requires_grad_(True)
    v = losses.nll_loss(x, ys[0], weight=CW13)
    assert [c[0] for c in double.calls] == ['weighted_loss_fwd']
    xr = xs[0].clone().requires_grad_(True)
    want = F.nll_loss(xr, ys[0], weight=torch.tensor(CW13), ignore_index=-1)
    assert abs(float(v.detach()) - float(want.detach())) <= 1e-5 * abs(float(want.detach()))
    v.backward()
    want.backward()
    assert torch.allclose(x.grad, xr.grad, rtol=1e-5, atol=1e-9)
    assert torch.equal(losses.nll_loss(xs[0], ys[0], weight=torch.tensor(CW13)), v.detach())     # a tensor is taken too
    double.calls.clear()
    plain = losses.nll_loss(xs[0], ys[0], -1, 'mean')                                             # positional callers
    assert [c[0] for c in double.calls] == ['multitask_loss_fwd'] and float(plain) != float(v.detach())
    bx, bt = bce_case((3, 9, 2), 2)
    double.calls.clear()
    b1 = losses.binary_cross_entropy_loss(bx, bt)
    assert [c[0] for c in double.calls] == ['multitask_loss_fwd']
    b2 = losses.binary_cross_entropy_loss(bx, bt, positive_class_weight=2.0)
    b05 = losses.binary_cross_entropy_loss(bx, bt, 0.5)
    assert [c[0] for c in double.calls[1:]] == ['weighted_loss_fwd'] * 2
    assert float(b2) == float(W.forward(W.BCE, bx.numpy(), bt.numpy(), positive_class_weight=2.0)[0]) > float(b1)
    assert abs(float(b05) - float(b1)) <= 1e-6 * float(b1)                                         # p <= 1 changes nothing
    with pytest.raises(NotImplementedError):
        losses.nll_loss(xs[0], ys[0], reduction='sum', weight=CW13)


def test_a_call_without_options_records_only_the_plain_entry_points(double):
    outs, tgts = _criterion_case('mphoi')
    fns = (losses.budget_loss, losses.binary_cross_entropy_loss) + (losses.nll_loss,) * 4
    for kw in ({}, dict(class_weights=None, positive_class_weights=None),
               dict(class_weights=[None] * 6, positive_class_weights=[None, 1, None, None, None, None])):
        double.calls.clear()
        leaves = [o.clone().requires_grad_(True) for o in outs]
        sum(losses.multi_task_loss(leaves, tgts, fns, **kw)).backward()
        assert [c[0] for c in double.calls] == ['multitask_loss_fwd', 'multitask_loss_bwd'], kw
        assert all('class_weight' not in c for c in double.calls)


def test_any_option_sends_all_terms_through_the_weighted_pair_once_per_direction(double):
    outs, tgts = _criterion_case('mphoi')
    fns = (losses.budget_loss, losses.binary_cross_entropy_loss) + (losses.nll_loss,) * 4
    w = [0.5, 0.7, 0.3, 0.3, 1.0, 0.6]
    cw = [0.5, 1.0, 2.0, 0.0, 1.5, 1.0, 0.25, 3.0]
    for kw in (dict(class_weights=[None] * 4 + [cw, None]), dict(positive_class_weights=[None, 2.0] + [None] * 4),
               dict(class_weights=[None, None, cw, cw, cw, torch.tensor(cw)], positive_class_weights=[None, 3.0] + [None] * 4)):
        double.calls.clear()
        leaves = [o.clone().requires_grad_(True) for o in outs]
        got = losses.multi_task_loss(leaves, tgts, fns, w, **kw)
        assert double.calls == [('weighted_loss_fwd', 6, (), {})]
        assert got[0]._base is not None and got[0]._base.shape == (6,)
        sum(got).backward()
        assert double.calls[1:] == [('weighted_loss_bwd', (True,) * 6)]
        cws = kw.get('class_weights', [None] * 6)
        pws = kw.get('positive_class_weights', [None] * 6)
        for i in range(6):
            xr = outs[i].clone().requires_grad_(True)
            if i >= 2:
                c = None if cws[i] is None else torch.as_tensor(cws[i], dtype=torch.float32)
                ref = w[i] * F.nll_loss(xr, tgts[i], weight=c, ignore_index=-1)
                ref.backward()
                want_l, want_g = float(ref.detach()), xr.grad
            else:
                kind = W.BUDGET if i == 0 else W.BCE
                l, (_, den) = W.forward(kind, outs[i].numpy(), tgts[i].numpy(), w[i], positive_class_weight=pws[i] or 1.0)
                want_l = float(l)
                want_g = torch.from_numpy(W.gradient(kind, outs[i].numpy(), tgts[i].numpy(), w[i],
                                                     positive_class_weight=pws[i] or 1.0, den=den))
            assert abs(float(got[i].detach()) - want_l) <= 1e-5 * max(1.0, abs(want_l)), i
            assert torch.allclose(leaves[i].grad, want_g, rtol=1e-5, atol=1e-9), i
    # a host sequence is uploaded once and reused
    a = losses._class_weight(cw, 4, 0, outs[4])
    assert a.data_ptr() == losses._class_weight(list(cw), 4, 0, outs[4]).data_ptr()


def test_weight_zero_terms_get_no_backward_work(double):
    outs, tgts = _criterion_case('mphoi')
    fns = (losses.budget_loss, losses.binary_cross_entropy_loss) + (losses.nll_loss,) * 4
    cw = [1.0] * 7 + [2.0]
    kw = dict(class_weights=[None, None, cw, cw, cw, cw], positive_class_weights=[None, 2.0, None, None, None, None])
    leaves = [o.clone().requires_grad_(True) for o in outs[:5]] + [outs[5].clone()]
    got = losses.multi_task_loss(leaves, tgts, fns, [0.0, 0.0, 0.0, 0.3, 1.0, 0.6], **kw)
    double.calls.clear()
    sum(got).backward()
    assert double.calls == [('weighted_loss_bwd', (False, False, False, True, True, False))]
    assert all(x.grad is None for x in leaves[:3]) and leaves[3].grad is not None
    leaves = [o.clone().requires_grad_(True) for o in outs]
    got = losses.multi_task_loss(leaves, tgts, fns, [0.0] * 6, **kw)
    double.calls.clear()
    sum(got).backward()
    assert double.calls == []


SUB, AFF = [0.5, 1.0, 2.0, 0.0, 1.5, 1.0, 0.25, 3.0], [1.0, 2.0, 0.5, 1.0, 4.0, 1.0, 1.0, 0.1]


@pytest.mark.parametrize('ds', ['mphoi', 'cad120'])
@pytest.mark.parametrize('smoothing', [False, True])
def test_select_loss_with_the_new_keys(ds, smoothing, double):
    cad = ds == 'cad120'
    names, weights, types, mask = TODAY[ds]
    misc = dict(MISC, class_weights=dict(add=True, subactivity=SUB, affordance=AFF))
    misc['segmentation_loss'] = dict(MISC['segmentation_loss'], positive_class_weight=2.5)
    if smoothing:
        misc['smoothing_loss'] = dict(add=True)
    cfg = dict(misc=misc)
    crit, got_names = losses.select_loss('2G-GCN', 'multiple', ds, cfg)
    n, m = len(names), (4 if cad else 2) * smoothing
    # the names, types and mask are those of the same configuration without the new keys
    plain_cfg = dict(misc=dict(MISC, **({'smoothing_loss': dict(add=True)} if smoothing else {})))
    assert got_names == losses.select_loss('2G-GCN', 'multiple', ds, plain_cfg)[1] and got_names[:n] == names
    assert losses.select_loss_types('2G-GCN', ds, cfg) == types + ['mse'] * m
    assert losses.select_loss_learning_mask('2G-GCN', ds, cfg) == mask + [False] * m
    assert crit.keywords['weight'] == weights
    want_cw = [SUB if nm.startswith('NLL_SA') else AFF if nm.startswith('NLL_OA') else None for nm in names]
    assert crit.keywords['class_weights'] == want_cw
    assert crit.keywords['positive_class_weights'] == [2.5 if nm.startswith('BCE') else None for nm in names]
    assert ('smoothing' in crit.keywords) == smoothing
    outs, tgts = _criterion_case(ds)
    leaves = [o.clone().requires_grad_(True) for o in outs]
    raw = crit(leaves, tgts)
    assert len(raw) == n + m
    assert [c[0] for c in double.calls] == ['weighted_loss_fwd'] + ['smooth_loss_fwd'] * smoothing
    assert double.calls[0][1:] == (n, (), {'room': m} if smoothing else {})
    learner = multi_task.MultiTaskLossLearner(losses.select_loss_types('2G-GCN', ds, cfg),
                                              losses.select_loss_learning_mask('2G-GCN', ds, cfg))
    out = learner(raw)
    assert ('mtl_weight_fwd', n + m) in double.calls and multi_task._loss_tensor(raw) is raw[0]._base
    double.calls.clear()
    sum(out).backward()
    assert [c[0] for c in double.calls if 'loss' in c[0]] == ['weighted_loss_bwd'] + ['smooth_loss_bwd'] * smoothing
    # values: the weighted terms differ from the unweighted run, the smoothing terms (unweighted by class) do not
    plain = losses.select_loss('2G-GCN', 'multiple', ds, plain_cfg)[0]([o.clone() for o in outs], tgts)
    for nm, a, b in zip(got_names, raw, plain):
        if nm.startswith('B_'):      # no option, but the other entry point of the double: another fp64 summation order
            assert abs(float(a.detach()) - float(b)) <= 1e-6 * abs(float(b)), nm
        else:
            assert torch.equal(a.detach(), b) == nm.startswith('TMSE'), nm
    for i, nm in enumerate(names):
        if want_cw[i] is not None:
            xr = outs[i].clone().requires_grad_(True)
            ref = weights[i] * F.nll_loss(xr, tgts[i], weight=torch.tensor(want_cw[i]), ignore_index=-1)
            assert abs(float(raw[i].detach()) - float(ref.detach())) <= 1e-5 * max(1.0, abs(float(ref.detach()))), nm
    # only one of the keys; `add: False`; a key with no list for the objects
    for over, keys in ((dict(class_weights=dict(add=True, subactivity=SUB)), ['class_weights']),
                       (dict(class_weights=dict(add=False, subactivity=SUB, affordance=AFF)), []),
                       (dict(segmentation_loss=dict(MISC['segmentation_loss'], positive_class_weight=1)), []),
                       (dict(segmentation_loss=dict(MISC['segmentation_loss'], positive_class_weight=4)),
                        ['positive_class_weights'])):
        c, nm = losses.select_loss('2G-GCN', 'multiple', ds, dict(misc=dict(MISC, **over)))
        assert nm == names and sorted(c.keywords) == sorted(['loss_functions', 'weight'] + keys)
        if keys == ['class_weights']:
            assert [w is not None for w in c.keywords['class_weights']] == [x.startswith('NLL_SA') for x in names]


def test_value_errors_before_any_launch(double):
    outs, tgts = _criterion_case('mphoi')
    fns = (losses.budget_loss, losses.binary_cross_entropy_loss) + (losses.nll_loss,) * 4
    ok = [1.0] * 8
    bad = [dict(class_weights=[ok] + [None] * 5),                                    # a class weight on a budget term
           dict(class_weights=[None, torch.ones(8)] + [None] * 4),                   # ... on a BCE term
           dict(positive_class_weights=[None] * 5 + [2.0]),                          # a positive weight on an NLL term
           dict(positive_class_weights=[2.0] + [None] * 5),                          # ... on a budget term
           dict(class_weights=[None] * 5 + [[1.0] * 7]),                             # wrong length (the input has 8 classes)
           dict(class_weights=[None] * 5 + [torch.ones(9)]),
           dict(class_weights=[None] * 5 + [torch.ones(2, 4)]),
           dict(class_weights=[None] * 5 + [[1.0] * 7 + [-0.5]]),                    # negative
           dict(class_weights=[None] * 5 + [[1.0] * 7 + [float('nan')]]),
           dict(class_weights=[None] * 5 + [[1.0] * 7 + [float('inf')]]),
           dict(positive_class_weights=[None, -1.0] + [None] * 4),
           dict(positive_class_weights=[None, float('nan')] + [None] * 4),
           dict(positive_class_weights=[None, float('inf')] + [None] * 4),
           dict(class_weights=[None] * 5)]                                           # not aligned with the six terms
    for kw in bad:
        with pytest.raises(ValueError):
            losses.multi_task_loss(outs, tgts, fns, **kw)
    with pytest.raises(ValueError):
        losses.binary_cross_entropy_loss(outs[1], tgts[1], positive_class_weight=-2)
    with pytest.raises(ValueError):
        losses.nll_loss(outs[2], tgts[2], weight=[1.0] * 3)
    assert double.calls == []


# ------------------------------------------------------------------------------------------------ the count reducer
def _weighted_run(outs, tgts, reducer, seen=None):
    fns = (losses.budget_loss, losses.binary_cross_entropy_loss) + (losses.nll_loss,) * 4
    kw = dict(class_weights=[None, None, SUB, None, SUB, AFF], positive_class_weights=[None, 2.0] + [None] * 4)
    leaves = [o.clone().requires_grad_(True) for o in outs]
    if reducer is None:
        got = losses.multi_task_loss(leaves, tgts, fns, [0.5, 0.7, 0.3, 0.3, 1.0, 0.6], **kw)
    else:
        with losses.count_reducer_scope(reducer):
            got = losses.multi_task_loss(leaves, tgts, fns, [0.5, 0.7, 0.3, 0.3, 1.0, 0.6], **kw)
    sum(got).backward()
    return [v.detach().clone() for v in got], [x.grad for x in leaves]


def test_count_reducer_receives_den_and_gives_the_global_weighted_mean(double):
    outs, tgts = _criterion_case('mphoi', seed=9, shape=(5, 6, 8))
    for t in tgts:                                                         # ragged: the second shard is mostly padding
        t[3:, 2:] = -1
    whole_l, whole_g = _weighted_run(outs, tgts, None)
    shards = [([o[:2] for o in outs], [t[:2] for t in tgts]), ([o[2:] for o in outs], [t[2:] for t in tgts])]
    dens = []
    for o, t in shards:
        _weighted_run(o, t, lambda c: (dens.append(c.clone()), c)[1])
    # what is handed over is den: for the class-weighted NLL terms the sum of the kept weights, not a count
    y = shards[0][1][4]
    assert float(dens[0][4]) == float(torch.tensor(SUB, dtype=torch.float64)[y[y >= 0]].sum()) != float((y >= 0).sum())
    eff = (dens[0] + dens[1]) / 2
    part = [_weighted_run(o, t, lambda c: eff) for o, t in shards]
    for i in range(6):
        mean = torch.cat([part[0][1][i], part[1][1][i]]) / 2
        assert torch.allclose(mean, whole_g[i], rtol=1e-6, atol=1e-10), i
        assert abs(float((part[0][0][i] + part[1][0][i]) / 2) - float(whole_l[i])) <= 1e-6 * abs(float(whole_l[i])), i
    assert not torch.allclose(torch.cat([_weighted_run(o, t, None)[1][4] for o, t in shards]) / 2, whole_g[4], rtol=1e-3)
    # a reducer that returns den unchanged: bit-equal to no reducer
    same_l, same_g = _weighted_run(outs, tgts, lambda c: c)
    assert all(torch.equal(a, b) for a, b in zip(whole_l, same_l)) and all(torch.equal(a, b) for a, b in zip(whole_g, same_g))


# ------------------------------------------------------------------------------------------------ the C ABI
def test_struct_layout_matches_the_c_compiler(tmp_path):
    header = os.path.join(ROOT, 'include', 'twog_gcn.h')
    src = tmp_path / 'sz.c'
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{header}"\nint main(void){{'
                   'printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(twog_wloss_t), sizeof(twog_loss_t), '
                   'offsetof(twog_wloss_t, ignore_value), offsetof(twog_loss_t, ignore_value), '
                   'offsetof(twog_wloss_t, class_weight), offsetof(twog_wloss_t, positive_class_weight));return 0;}\n')
    exe = tmp_path / 'sz'
    subprocess.run(['gcc', str(src), '-o', str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    T, P = _lib.WLoss, _lib.Loss
    assert [int(v) for v in out] == [ctypes.sizeof(T), ctypes.sizeof(P), T.ignore_value.offset, P.ignore_value.offset,
                                     T.class_weight.offset, T.positive_class_weight.offset]
    assert ctypes.sizeof(T) % 8 == 0 and T.ignore_value.offset == P.ignore_value.offset
    assert {'twog_weighted_loss_fwd', 'twog_weighted_loss_bwd', 'twog_class_counts'} <= set(_lib.exported_symbols())
