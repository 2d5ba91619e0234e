"""GPU: the temporal smoothing loss kernels (twog_smooth_loss_fwd / _bwd through the C ABI) against the numpy specification
tests/smooth_loss_ref.py, at kernel level, through losses.multi_task_loss with the term lists of select_loss, and through a
small model.

Convention (the specification fixes every fp32 rounding; only the fp64 summation order is free): the count is exact, the
sum within 1e-12 relative, the loss within 2 fp32 ulp (one for the rounding of sum / count to fp32 on the other side of a
tie, one for the product with the weight), the gradient bit-equal."""
import numpy as np
import pytest
import torch

import twog_gcn_amd  # noqa: F401
from twog_gcn_amd import kernels as twog_kernels
from twog_gcn_amd import losses
from twog_gcn_amd.models import TGGCN
from oracle import cpu_ref
from tests import smooth_loss_ref as S
from tests.helpers import synth_inputs
from tests.test_smooth_loss_cpu import SHAPES, grid_case

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = 7.25


@pytest.fixture(autouse=True)
def hip_backend():
    twog_kernels._set_backend_for_tests(None)
    assert twog_kernels.get_kernels().name == 'hip'
    yield


def softmax_case(shape, seed, ignored=0.2):
    """log_softmax(randn) inputs (scaled: a share of the differences lies beyond tau = 4), about 20 % ignored targets."""
    bs, C, T, E = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.log_softmax(torch.randn(shape, generator=g) * 3, 1)
    y = torch.randint(0, C, (bs, T, E), generator=g)
    y[torch.rand(bs, T, E, generator=g) < ignored] = -1
    return x, y


def term(x, y, weight=1.0, tau=4.0):
    return dict(input=x.to(DEV), target=y.to(DEV), weight=weight, tau=tau, ignore=-1)


def forward(terms):
    K = twog_kernels.get_kernels()
    loss = torch.full((len(terms),), SENTINEL, dtype=torch.float32, device=DEV)
    stats = torch.full((len(terms), 2), SENTINEL, dtype=torch.float64, device=DEV)
    K.smooth_loss_fwd(terms, loss, stats)
    return loss, stats


def backward(terms, stats, dlosses, dins=None, accumulate=None):
    """Store mode by default, into buffers prefilled with a sentinel: every element must have been written."""
    K = twog_kernels.get_kernels()
    if dins is None:
        dins = [torch.full_like(t['input'], SENTINEL) for t in terms]
        accumulate = [False] * len(terms)
    K.smooth_loss_bwd(terms, stats, torch.tensor(dlosses, dtype=torch.float32, device=DEV), dins, accumulate)
    return dins


def check_forward(x, y, weight, tau, loss, stats):
    want, (s, c) = S.forward(x.numpy(), y.numpy(), weight, tau)
    got_s, got_c = (float(v) for v in stats.cpu())
    print(f'count {got_c:.0f} (spec {c:.0f}); sum {got_s!r} (spec {float(s)!r}); loss {float(loss)!r} (spec {float(want)!r})')
    assert got_c == c
    assert abs(got_s - s) <= 1e-12 * abs(s)
    assert abs(np.float32(float(loss)) - want) <= 2 * np.spacing(np.abs(want))
    return c


def check_term(x, y, weight=1.0, tau=4.0, dloss=1.0):
    t = term(x, y, weight, tau)
    loss, stats = forward([t])
    count = check_forward(x, y, weight, tau, loss[0], stats[0])
    grad = backward([t], stats, [dloss])[0].cpu()
    want = torch.from_numpy(S.gradient(x.numpy(), y.numpy(), weight, tau, dloss=dloss, count=count))
    print(f'gradient: {int((want != 0).sum())} non-zero of {want.numel()}, {int((grad != want).sum())} differ')
    assert torch.equal(grad, want)
    return loss, stats, grad


# one more shape than the CPU list: 67 200 (o, t, e) positions, more than the 65 536 threads of the backward grid (and the
# 16 384 of the forward grid), so the grid-stride loops of both directions take a second trip
@pytest.mark.parametrize('shape', SHAPES + [(70, 2, 120, 8)])
def test_shapes_against_the_specification(shape):
    x, y = softmax_case(shape, seed=sum(shape))
    loss, stats, grad = check_term(x, y, weight=0.7, dloss=1.5)
    if shape[2] == 1:   # no pair: loss 0, count 0 and an all-zero gradient that was stored over the sentinel
        assert float(loss) == 0.0 and stats.cpu().tolist() == [[0.0, 0.0]] and not grad.any()
    elif shape[2] >= 17:
        assert float(stats[0, 1]) > 0 and grad.any()


def test_inputs_on_the_clamp_boundary():
    shape = (5, 17, 40, 5)
    x, y = grid_case(shape, seed=3)
    d = (x[:, :, 1:] - x[:, :, :-1]).abs()
    assert int((d == 4.0).sum()) > 100 and int((d > 4.0).sum()) > 100      # exactly on |D| = tau, and beyond it
    check_term(x, y, weight=0.15)
    check_term(x, y, weight=0.15, tau=2.5)


@pytest.mark.parametrize('pattern', ['padded_tail', 'single_steps', 'everything', 'out_of_range'])
def test_ignore_patterns(pattern):
    shape = (3, 13, 17, 2)
    x, _ = softmax_case(shape, seed=11)
    y = torch.randint(0, 13, (3, 17, 2), generator=torch.Generator().manual_seed(12))
    if pattern == 'padded_tail':
        y[0, 12:], y[1, 16:], y[2, 1:] = -1, -1, -1
    elif pattern == 'single_steps':
        y[0, 5, 0], y[0, 6, 1], y[1, 0, 0], y[1, 16, 1], y[2, 8] = -1, -1, -1, -1, -1
    elif pattern == 'everything':
        y[:] = -1
    else:
        y[0, 4, 0], y[1, 9, 1], y[2, 2, 0] = 13, 1 << 40, -5                # treated as ignored, like the NLL term does
    loss, stats, grad = check_term(x, y, weight=0.5)
    if pattern == 'everything':
        assert float(loss) == 0.0 and float(stats[0, 1]) == 0.0 and not grad.any()
    if pattern == 'out_of_range':
        y_ignored = torch.where((y < 0) | (y >= 13), torch.full_like(y, -1), y)
        assert torch.equal(grad, check_term(x, y_ignored, weight=0.5)[2])
        assert float(stats[0, 1]) == (3 * 16 * 2 - 6) * 13


def test_accumulate_into_the_nll_gradient():
    """The buffer the NLL backward launch filled, between guard words; the input a view at an odd offset of a larger
    allocation."""
    K = twog_kernels.get_kernels()
    shape, guard = (3, 13, 17, 2), 64
    x, y = softmax_case(shape, seed=21)
    n = x.numel()
    big_x = torch.full((n + 7,), SENTINEL, device=DEV)
    xd = big_x[3:3 + n].view(shape)
    xd.copy_(x)
    assert xd.is_contiguous() and xd.storage_offset() == 3
    yd = y.to(DEV)
    nll = dict(kind=0, input=xd, target=yd, weight=0.8, ignore=-1)
    nll_losses, nll_stats = K.multitask_loss_fwd([nll])
    nll_grad = K.multitask_loss_bwd([nll], nll_stats, torch.tensor([1.25], device=DEV), [True])[0]
    big_d = torch.full((guard + n + guard,), SENTINEL, device=DEV)
    dd = big_d[guard:guard + n].view(shape)
    dd.copy_(nll_grad)
    t = dict(input=xd, target=yd, weight=0.15, tau=4.0, ignore=-1)
    loss, stats = forward([t])
    count = check_forward(x, y, 0.15, 4.0, loss[0], stats[0])
    backward([t], stats, [0.75], dins=[dd], accumulate=[True])
    smooth = torch.from_numpy(S.gradient(x.numpy(), y.numpy(), 0.15, 4.0, dloss=0.75, count=count))
    before, after = nll_grad.cpu(), dd.cpu()
    assert smooth.any() and int((smooth == 0).sum()) > 0
    assert torch.equal(after, before + smooth)                               # nll_grad + fl32(g * 2 D): one fp32 addition
    untouched = smooth == 0
    assert torch.equal(after.view(torch.int32)[untouched], before.view(torch.int32)[untouched])   # bit-unchanged
    edges = torch.cat([big_d[:guard], big_d[guard + n:]]).cpu()
    assert torch.equal(edges, torch.full_like(edges, SENTINEL))
    assert torch.equal(big_x[:3].cpu(), torch.full((3,), SENTINEL)) and torch.equal(big_x[3 + n:].cpu(), torch.full((4,), SENTINEL))
    assert torch.equal(xd.cpu(), x)


def test_four_terms_in_one_launch_equal_four_launches():
    cases = [((3, 13, 17, 2), 0.15, 4.0), ((2, 10, 33, 3), 1.0, 2.0), ((5, 17, 40, 5), 0.6, 5.5), ((1, 2, 2, 1), 2.0, 0.5)]
    terms = [term(*softmax_case(shape, seed=31 + i), weight=w, tau=tau) for i, (shape, w, tau) in enumerate(cases)]
    dl = [1.0, 0.5, 2.0, 0.25]
    runs = []
    for _ in range(2):
        loss, stats = forward(terms)
        runs.append((loss, stats, backward(terms, stats, dl)))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert all(torch.equal(a, b) for a, b in zip(runs[0][2], runs[1][2]))
    for i, t in enumerate(terms):
        loss, stats = forward([t])
        assert torch.equal(loss[0], runs[0][0][i]) and torch.equal(stats[0], runs[0][1][i])
        assert torch.equal(backward([t], stats, dl[i:i + 1])[0], runs[0][2][i])
        assert runs[0][2][i].any() or i == 3
    K = twog_kernels.get_kernels()
    with pytest.raises(RuntimeError, match='code -1'):     # a malformed term: tau <= 0
        K.smooth_loss_fwd([dict(terms[0], tau=0.0)], runs[0][0][:1].clone(), runs[0][1][:1].clone())


MISC = dict(anticipation_loss_weight=0.6, budget_loss=dict(add=True, human_weight=0.5, object_weight=0.25),
            first_level_loss_weight=0.3, segmentation_loss=dict(add=True, pretrain=False, weight=0.7))


def criterion_case(ds, bs=3, T=17, seed=41):
    """Random outputs of the shapes of the model's output list, as test_losses_gpu.test_random_terms_vs_oracle builds them."""
    cad = ds == 'cad120'
    g = torch.Generator().manual_seed(seed)
    n_gate = 4 if cad else 2
    ents = [1, 5] if cad else [2]                      # humans (and objects) per clip
    classes = [10, 12] if cad else [13]
    outs, tgts = [], []
    for i in range(12 if cad else 6):
        if i < n_gate:
            E = ents[i % len(ents)]
            o = torch.rand(bs, T, E, generator=g) * 0.9 + 0.05
            t = (torch.rand(bs, T, E, generator=g) > 0.5).float()
            t[torch.rand(bs, T, E, generator=g) < 0.2] = -1.0
        else:
            k = ((i - n_gate) % 4) // 2 if cad else 0  # CAD-120: SAR, SAP (human), OAR, OAP (objects)
            E, C = ents[k], classes[k]
            o = torch.log_softmax(torch.randn(bs, C, T, E, generator=g) * 3, 1)
            t = torch.randint(0, C, (bs, T, E), generator=g)
            t[torch.rand(bs, T, E, generator=g) < 0.2] = -1
        outs.append(o)
        tgts.append(t)
    return outs, tgts


@pytest.mark.parametrize('ds', ['mphoi', 'cad120'])
def test_criterion_with_the_key_on_and_off(ds):
    cad = ds == 'cad120'
    outs, tgts = criterion_case(ds)
    on = dict(misc=dict(MISC, smoothing_loss=dict(add=True, weight=0.15, tau=4.0)))
    crit, names = losses.select_loss('2G-GCN', 'multiple', ds, on)
    n, m = (12, 4) if cad else (6, 2)
    assert len(names) == n + m
    xs = [o.clone().to(DEV).requires_grad_(True) for o in outs]
    got = crit(xs, [t.to(DEV) for t in tgts])
    assert len(got) == n + m and got[0]._base is not None and got[0]._base.shape == (n + m,)
    w = crit.keywords['weight']
    xo = [o.clone().requires_grad_(True) for o in outs]
    want = [float(v.detach()) for v in cpu_ref.loss_list(xo, tgts, w, cad120=cad)]
    smooth = [S.smooth_loss(outs[i].numpy(), tgts[i].numpy(), sw, tau) for i, sw, tau in crit.keywords['smoothing']]
    want += [float(r[0]) for r in smooth]
    for name, a, b in zip(names, got, want):
        a = float(a.detach())
        print(f'{name}: {a!r} (reference {b!r})')
        assert abs(a - b) <= 1e-5 * max(1.0, abs(b)), name
    assert all(b != 0 for b in want[n:])
    sum(got).backward()
    sum(cpu_ref.loss_list(xo, tgts, w, cad120=cad)).backward()
    for i, (a, b) in enumerate(zip(xs, xo)):
        gb = b.grad.clone()
        for (k, _, _), r in zip(crit.keywords['smoothing'], smooth):
            if k == i:
                gb += torch.from_numpy(r[2])
        assert torch.allclose(a.grad.cpu(), gb, rtol=1e-5, atol=1e-7), (i, float((a.grad.cpu() - gb).abs().max()))
    # key off: bit-equal to a plain multi_task_loss call, values and gradients
    crit_off, names_off = losses.select_loss('2G-GCN', 'multiple', ds, dict(misc=dict(MISC, smoothing_loss=dict(add=False))))
    assert names_off == names[:n]
    runs = []
    for fn in (crit_off, lambda i, t: losses.multi_task_loss(i, t, crit.keywords['loss_functions'], w)):
        leaves = [o.clone().to(DEV).requires_grad_(True) for o in outs]
        v = fn(leaves, [t.to(DEV) for t in tgts])
        sum(v).backward()
        runs.append((torch.stack(v).detach(), [x.grad for x in leaves]))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][0], torch.stack(got).detach()[:n])
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))


STAGE1 = dict(attention_style='v3', discrete_optimization_strategy='gs', filter_discrete_updates=False,
              message_humans_to_human=True, message_human_to_objects=True, message_objects_to_human=True,
              message_objects_to_object=True, message_geometry_to_objects=True, message_geometry_to_human=False,
              message_segment=True, message_type='v2', message_granularity='v1', message_aggregation='att',
              object_segment_update_strategy='ind', update_segment_threshold=0.5)


def test_small_model_trains_through_the_smoothing_terms():
    bs, T, H, O, N, h, C = 2, 6, 2, 4, 26, 32, 13
    torch.manual_seed(5)
    m = TGGCN(input_size=(2048 + 4 * N, 2048), num_classes=(C, None), hidden_size=h, gcn_node=N, **STAGE1).to(DEV).train()
    xh, xo, mask = (torch.from_numpy(a).to(DEV) for a in synth_inputs('smooth', H, O, N, bs, T, seed=5))
    seg = torch.ones(bs, T, H, device=DEV)
    m._gumbel_noise_override = torch.distributions.gumbel.Gumbel(0.0, 1.0).sample((T * O, bs, 2))
    g = torch.Generator().manual_seed(6)
    cls = [torch.randint(0, C, (bs, T, H), generator=g) for _ in range(2)]
    for c in cls:
        c[1, T - 2:] = -1
    gate = (torch.rand(bs, T, H, generator=g) > 0.5).float()
    tgts = [t.to(DEV) for t in [gate, gate] + cls * 2]
    misc = dict(MISC, smoothing_loss=dict(add=True, weight=0.5, tau=4.0))
    bn = m.geometry_embedding_gcn.joint_embed.cnn[0].bn

    def step(cfg):
        crit, _ = losses.select_loss('2G-GCN', 'multiple', 'mphoi', dict(misc=cfg))
        m.zero_grad(set_to_none=True)
        bn.running_mean.zero_(); bn.running_var.fill_(1.0)
        out = m(xh, xo, mask, human_segmentation=seg)
        for o in out[4:]:
            o.retain_grad()
        got = crit(out, tgts)
        sum(got).backward()
        return ([v.detach().clone() for v in got], [o.detach().clone() for o in out], [o.grad.clone() for o in out[4:]],
                {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}, crit)

    vals, outs, ograds, pgrads, crit = step(misc)
    assert len(vals) == 8 and all(torch.isfinite(v) for v in vals) and all(float(v) > 0 for v in vals[6:])
    # the gradient that reaches each final output: the NLL launch's (a plain criterion call on the same outputs) plus the
    # specification's smoothing gradient, one fp32 addition
    leaves = [o.clone().requires_grad_(True) for o in outs]
    sum(losses.multi_task_loss(leaves, tgts, crit.keywords['loss_functions'], crit.keywords['weight'])).backward()
    for j, (i, sw, tau) in enumerate(crit.keywords['smoothing']):
        x, y = outs[i].cpu(), tgts[i].cpu()
        want, (s, c) = S.forward(x.numpy(), y.numpy(), sw, tau)
        assert abs(np.float32(float(vals[6 + j])) - want) <= 2 * np.spacing(np.abs(want))
        smooth = torch.from_numpy(S.gradient(x.numpy(), y.numpy(), sw, tau, count=c))
        assert smooth.any()
        assert torch.equal(ograds[i - 4].cpu(), leaves[i].grad.cpu() + smooth)
    assert all(torch.isfinite(v).all() for v in pgrads.values())
    vals2, _, ograds2, pgrads2, _ = step(misc)                                # a second run is bit-equal
    assert all(torch.equal(a, b) for a, b in zip(vals, vals2)) and all(torch.equal(a, b) for a, b in zip(ograds, ograds2))
    assert pgrads.keys() == pgrads2.keys() and all(torch.equal(pgrads[k], pgrads2[k]) for k in pgrads)
    vals0, _, _, pgrads0, _ = step(MISC)                                      # ... and differs from the smoothing-off run
    assert len(vals0) == 6 and all(torch.equal(a, b) for a, b in zip(vals0, vals[:6]))
    assert any(not torch.equal(pgrads[k], pgrads0[k]) for k in pgrads0)
