"""GPU: the criterion with class weights and the positive-class weight (twog_weighted_loss_fwd / _bwd through the C ABI) and
twog_class_counts, against the numpy specification tests/class_weight_ref.py at kernel level, against the plain entry points
with neutral options, together with the smoothing launches, through losses.multi_task_loss and through a small model.

Convention (the specification fixes every fp32 rounding; only the fp64 summation order is free): NLL terms -- den and sum
within 1e-12 relative, the loss within 2 fp32 ulp (one for the rounding of sum / den to fp32 on the other side of a tie, one
for the product with the weight), the gradient bit-equal. BCE terms -- logf is the one operation the specification cannot
fix, so the forward value is held to the project's loss gate, 1e-5 * max(1, |spec|); the count is exact and the gradient
(no logarithm in it) bit-equal. Every buffer the kernels write is prefilled with a sentinel and sits between guard words."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import twog_gcn_amd  # noqa: F401
from twog_gcn_amd import _lib, kernels as twog_kernels
from twog_gcn_amd import losses
from twog_gcn_amd.models import TGGCN
from oracle import cpu_ref
from tests import class_weight_ref as W
from tests import smooth_loss_ref as S
from tests.helpers import synth_inputs
from tests.test_smooth_loss_gpu import MISC, STAGE1, criterion_case, softmax_case

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL, GUARD = 7.25, 64
WEIGHTS = [1e3, 1e-3, 0.0, 0.7, 2.0, 0.5, 1.0, 3.0, 0.25, 1.5, 0.9, 1.0, 4.0, 0.125, 1.0, 2.5, 0.75]   # cut to C classes


@pytest.fixture(autouse=True)
def hip_backend():
    twog_kernels._set_backend_for_tests(None)
    assert twog_kernels.get_kernels().name == 'hip'
    yield


def term(kind, x, y, weight=1.0, cw=None, p=1.0):
    return dict(kind=kind, input=x.to(DEV), target=y.to(DEV), weight=weight, ignore=-1,
                class_weight=None if cw is None else torch.as_tensor(cw, dtype=torch.float32).to(DEV),
                positive_class_weight=p)


def spec_args(t):
    cw = t['class_weight']
    return (t['kind'], t['input'].cpu().numpy(), t['target'].cpu().numpy(), t['weight'], t['ignore'],
            None if cw is None else cw.cpu().numpy(), t['positive_class_weight'])


def forward(terms):
    """twog_weighted_loss_fwd into tensors prefilled with a sentinel."""
    K, n = twog_kernels.get_kernels(), len(terms)
    loss = torch.full((n,), SENTINEL, dtype=torch.float32, device=DEV)
    stats = torch.full((n, 2), SENTINEL, dtype=torch.float64, device=DEV)
    partials = K.workspace(n * _lib.LOSS_BLOCKS * 2 * 8, torch.device(DEV), 'loss')
    K._check(K.lib.twog_weighted_loss_fwd(K._loss_terms(terms, struct=_lib.WLoss), n, partials.data_ptr(), stats.data_ptr(),
                                          loss.data_ptr(), K._stream()), 'twog_weighted_loss_fwd')
    return loss, stats


def backward(terms, stats, dlosses, need=None):
    """twog_weighted_loss_bwd into views of larger allocations prefilled with a sentinel: every element of a view must have
    been written, and nothing around it."""
    K = twog_kernels.get_kernels()
    need = [True] * len(terms) if need is None else need
    bigs = [torch.full((GUARD + t['input'].numel() + GUARD,), SENTINEL, device=DEV) if nd else None
            for t, nd in zip(terms, need)]
    dins = [None if b is None else b[GUARD:GUARD + t['input'].numel()].view(t['input'].shape) for b, t in zip(bigs, terms)]
    dl = torch.tensor(dlosses, dtype=torch.float32, device=DEV)
    K._check(K.lib.twog_weighted_loss_bwd(K._loss_terms(terms, dins, struct=_lib.WLoss), len(terms), stats.data_ptr(),
                                          dl.data_ptr(), K._stream()), 'twog_weighted_loss_bwd')
    for b, t in zip(bigs, terms):
        if b is not None:
            n = t['input'].numel()
            edges = torch.cat([b[:GUARD], b[GUARD + n:]]).cpu()
            assert torch.equal(edges, torch.full_like(edges, SENTINEL)), 'the kernel wrote outside the gradient view'
    return [None if d is None else d.cpu() for d in dins]


def check_term(t, dloss=1.0):
    """One term against the specification; returns (loss, stats row, gradient) from the device."""
    loss, stats = forward([t])
    want, (s, den) = W.forward(*spec_args(t))
    got_s, got_den = (float(v) for v in stats[0].cpu())
    got = np.float32(float(loss[0]))
    print(f'den {got_den!r} (spec {float(den)!r}); sum {got_s!r} (spec {float(s)!r}); loss {float(got)!r} (spec {float(want)!r})')
    if t['kind'] == W.NLL:
        assert abs(got_den - den) <= 1e-12 * abs(den) and abs(got_s - s) <= 1e-12 * abs(s)
        assert (np.isnan(got) and np.isnan(want)) or abs(got - want) <= 2 * np.spacing(np.abs(want))
    else:
        assert got_den == den
        assert abs(float(got) - float(want)) <= 1e-5 * max(1.0, abs(float(want)))
    grad = backward([t], stats, [dloss])[0]
    want_g = torch.from_numpy(W.gradient(*spec_args(t), dloss=np.float32(dloss), den=got_den)).view(grad.shape)
    print(f'gradient: {int((want_g != 0).sum())} non-zero of {want_g.numel()}, {int((grad != want_g).sum())} differ')
    assert torch.equal(grad, want_g) and not torch.isnan(grad).any()
    return loss[0], stats[0].cpu(), grad


# ------------------------------------------------------------------------------------------------ NLL with class weights
# the last shape has 67 200 positions, more than the 65 536 threads of the backward grid (and the 16 384 of the forward
# grid), so the grid-stride loops of both directions take a second trip
@pytest.mark.parametrize('shape', [(1, 1, 1, 1), (2, 2, 3, 1), (3, 13, 17, 2), (5, 17, 40, 5), (70, 2, 120, 8)])
def test_nll_shapes_against_the_specification(shape):
    x, y = softmax_case(shape, seed=sum(shape))
    if shape[1] == 1:
        x = x - 1.5                                                  # log_softmax over one class is 0 everywhere
    cw = WEIGHTS[:shape[1]]
    loss, stats, grad = check_term(term(W.NLL, x, y, 0.7, cw), dloss=1.5)
    if shape[2] >= 17:
        assert float(stats[1]) > 0 and grad.any()
    # without weights (a NULL pointer): den is the count of kept targets
    loss, stats, grad = check_term(term(W.NLL, x, y, 0.7), dloss=1.5)
    assert float(stats[1]) == float(((y >= 0) & (y < shape[1])).sum())


def test_nll_integer_weights_are_exact():
    x, y = softmax_case((5, 17, 40, 5), seed=3)
    x = torch.round(x * 64) / 64                                     # inputs on a grid: every product and partial sum exact
    cw = [float(1 + (c * 7) % 5) for c in range(17)]
    t = term(W.NLL, x, y, 1.0, cw)
    loss, stats = forward([t])
    _, (s, den) = W.forward(*spec_args(t))
    assert stats[0].cpu().tolist() == [float(s), float(den)]


@pytest.mark.parametrize('pattern', ['zero_weight_class', 'everything_ignored', 'out_of_range'])
def test_nll_ignore_patterns(pattern):
    shape, C = (3, 13, 17, 2), 13
    x, _ = softmax_case(shape, seed=11)
    y = torch.randint(0, C, (3, 17, 2), generator=torch.Generator().manual_seed(12))
    cw = WEIGHTS[:C]
    if pattern == 'zero_weight_class':
        y[:] = 2                                                     # WEIGHTS[2] == 0: every kept target has no weight
        y[0, :5] = -1
    elif pattern == 'everything_ignored':
        y[:] = -1
    else:
        y[0, 4, 0], y[1, 9, 1], y[2, 2, 0] = C, 1 << 40, -5          # treated as ignored
    loss, stats, grad = check_term(term(W.NLL, x, y, 0.5, cw))
    if pattern != 'out_of_range':
        assert torch.isnan(loss) and stats.tolist() == [0.0, 0.0] and not grad.any()      # 0 / 0; zeros stored over the sentinel
    else:
        y_ignored = torch.where((y < 0) | (y >= C), torch.full_like(y, -1), y)
        loss2, stats2, grad2 = check_term(term(W.NLL, x, y_ignored, 0.5, cw))
        assert torch.equal(loss, loss2) and torch.equal(stats, stats2) and torch.equal(grad, grad2)


# ------------------------------------------------------------------------------------------------ BCE with p
def bce_case(shape, seed):
    """Inputs in [0.05, 0.95]; targets 0, 1, ignored (-1) and a smoothed 0.5; x = 0 and x = 1 at t = 1 (the clamps)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(shape, generator=g) * 0.9 + 0.05
    t = (torch.rand(shape, generator=g) < 0.35).float()
    t[torch.rand(shape, generator=g) < 0.2] = -1.0
    t.view(-1)[3::11] = 0.5
    x.view(-1)[:2] = torch.tensor([0.0, 1.0])
    t.view(-1)[:2] = 1.0
    return x, t


@pytest.mark.parametrize('p', [0.5, 1.0, 1.5, 2.0, 3.0])
def test_bce_positive_class_weight_against_the_specification(p):
    x, t = bce_case((5, 40, 5), seed=5)
    assert {0.0, 0.5, 1.0, -1.0} <= set(t.view(-1).tolist())
    loss, stats, grad = check_term(term(W.BCE, x, t, 0.7, p=p), dloss=1.5)
    base_l, base_s, base_g = check_term(term(W.BCE, x, t, 0.7, p=1.0), dloss=1.5)
    g = np.float32(0.7) * np.float32(1.5) / np.float32(float(stats[1]))
    scale = np.float32(p) if p > 1 else np.float32(1.0)
    assert grad.view(-1)[0] == (g * np.float32(-1.0) / np.float32(1e-12)) * scale and grad.view(-1)[1] == 0    # x = 0, x = 1
    half = (t == 0.5).view(-1)
    assert torch.equal(grad.view(-1)[half], base_g.view(-1)[half])                      # a smoothed target: p must not touch it
    if p <= 1:
        assert torch.equal(loss, base_l) and torch.equal(stats, base_s) and torch.equal(grad, base_g)
    else:
        # the x = 0 element contributes 100 with or without p (both clamp), every other t == 1 element p times its -log x
        pos = (t == 1).view(-1)
        pos[:2] = False
        extra = (p - 1) * float(-(torch.log(x.view(-1)[pos].double())).sum())
        assert abs(float(stats[0]) - float(base_s[0]) - extra) <= 1e-5 * float(stats[0])
        other = (t != 1).view(-1)
        assert torch.equal(grad.view(-1)[other], base_g.view(-1)[other]) and not torch.equal(grad, base_g)


def test_bce_clamps_alone():
    """x = 0 and x = 1 at t = 1, nothing else: the loss is 100 w / count, the x = 1 element adds 0."""
    x, t = torch.tensor([0.0, 1.0, 0.5]), torch.tensor([1.0, 1.0, -1.0])
    loss, stats, grad = check_term(term(W.BCE, x, t, 0.5, p=2.0))
    assert stats.tolist() == [100.0, 2.0] and float(loss) == 100.0 * 0.5 / 2 and grad[1] == 0 and grad[2] == 0


def test_bce_second_trip_of_the_grid_stride_loops():
    x, t = bce_case((70, 120, 8), seed=6)                          # 67 200 elements
    check_term(term(W.BCE, x, t, 1.0, p=2.5), dloss=0.5)
    check_term(term(W.BUDGET, x, t, 0.3), dloss=0.5)


def test_malformed_terms_are_refused():
    x, t = bce_case((3, 5, 2), seed=7)
    for p in (-1.0, float('nan'), float('inf')):
        with pytest.raises(RuntimeError, match='code -1'):
            forward([term(W.BCE, x, t, p=p)])
        with pytest.raises(RuntimeError, match='code -1'):
            backward([term(W.BCE, x, t, p=p)], torch.ones(1, 2, dtype=torch.float64, device=DEV), [1.0])


# ------------------------------------------------------------------------------------------------ neutral options
@pytest.mark.parametrize('ds', ['mphoi', 'cad120'])
def test_neutral_options_equal_the_plain_entry_points_bit_for_bit(ds):
    """Class weights of ones and p = 1 through twog_weighted_loss_*, against twog_multitask_loss_*: the six-term MPHOI list and
    the twelve-term CAD-120 list, BCE targets in {0, 1, ignore} (with those a fused and a separate multiply-add agree)."""
    K = twog_kernels.get_kernels()
    cad = ds == 'cad120'
    outs, tgts = criterion_case(ds)
    n_gate = 4 if cad else 2
    kinds = [W.BUDGET] * (n_gate // 2) + [W.BCE] * (n_gate // 2) + [W.NLL] * (len(outs) - n_gate)
    w = [0.5, 0.25, 0.7, 0.7] + [0.3] * 4 + [1.0, 0.6, 1.0, 0.6] if cad else [0.5, 0.7, 0.3, 0.3, 1.0, 0.6]
    assert all(set(t.view(-1).tolist()) <= {0.0, 1.0, -1.0} for t in tgts[:n_gate])
    plain = [dict(kind=k, input=o.to(DEV), target=t.to(DEV), weight=wi, ignore=-1) for k, o, t, wi in zip(kinds, outs, tgts, w)]
    for null_weights in (False, True):
        neutral = [dict(p, class_weight=(torch.ones(p['input'].shape[1], device=DEV)
                                         if p['kind'] == W.NLL and not null_weights else None), positive_class_weight=1.0)
                   for p in plain]
        l0, s0 = K.multitask_loss_fwd(plain)
        l1, s1 = forward(neutral)
        assert torch.equal(l0, l1) and torch.equal(s0, s1) and not torch.isnan(l0).any()
        dl = [1.0, 0.5, 2.0, 0.25, 1.5, 0.75] * (2 if cad else 1)
        g0 = K.multitask_loss_bwd(plain, s0, torch.tensor(dl, device=DEV), [True] * len(plain))
        g1 = backward(neutral, s1, dl)
        assert all(torch.equal(a.cpu(), b) for a, b in zip(g0, g1)) and all(g.any() for g in g1)


# ------------------------------------------------------------------------------------------------ with the smoothing launches
def test_mixed_twelve_terms_with_room_and_the_smoothing_launches_behind():
    K = twog_kernels.get_kernels()
    outs, tgts = criterion_case('cad120')
    kinds = [W.BUDGET] * 2 + [W.BCE] * 2 + [W.NLL] * 8
    w = [0.5, 0.25, 0.7, 0.7] + [0.3] * 4 + [1.0, 0.6, 1.0, 0.6]
    # options on SOME terms: p on one BCE term, class weights on the human NLL terms and one object term
    cws = [None] * 4 + [WEIGHTS[:10], None, None, WEIGHTS[:12], WEIGHTS[:10], WEIGHTS[:10], None, WEIGHTS[:12]]
    pws = [1.0, 1.0, 2.0, 1.0] + [1.0] * 8
    terms = [term(k, o, t, wi, cw, p) for k, o, t, wi, cw, p in zip(kinds, outs, tgts, w, cws, pws)]
    smooth = [dict(input=terms[i]['input'], target=terms[i]['target'], weight=0.15 * w[i], tau=4.0, ignore=-1)
              for i in range(8, 12)]
    losses_, stats = K.weighted_loss_fwd(terms, room=4)
    assert losses_.shape == (16,) and stats.shape == (16, 2)
    K.smooth_loss_fwd(smooth, losses_[12:], stats[12:])
    for i, t in enumerate(terms):                                   # one launch of twelve == twelve launches of one
        l, s = forward([t])
        assert torch.equal(l[0], losses_[i]) and torch.equal(s[0], stats[i])
    for j, i in enumerate(range(8, 12)):
        want, (s, c) = S.forward(outs[i].numpy(), tgts[i].numpy(), 0.15 * w[i], 4.0)
        assert float(stats[12 + j, 1]) == c and abs(np.float32(float(losses_[12 + j])) - want) <= 2 * np.spacing(np.abs(want))
    dl = torch.tensor([1.0, 0.5, 2.0, 0.25, 1.5, 0.75, 1.0, 1.25] * 2, device=DEV)
    dins = K.weighted_loss_bwd(terms, stats, dl[:12], [True] * 12)
    nll = [d.cpu().clone() for d in dins]
    for i, t in enumerate(terms):
        want = torch.from_numpy(W.gradient(*spec_args(t), dloss=np.float32(float(dl[i])), den=float(stats[i, 1])))
        assert torch.equal(nll[i], want.view(nll[i].shape)), i
    K.smooth_loss_bwd(smooth, stats[12:], dl[12:], dins[8:], [True] * 4)
    for j, i in enumerate(range(8, 12)):
        sm = torch.from_numpy(S.gradient(outs[i].numpy(), tgts[i].numpy(), 0.15 * w[i], 4.0, dloss=float(dl[12 + j]),
                                         count=float(stats[12 + j, 1])))
        assert sm.any() and torch.equal(dins[i].cpu(), nll[i] + sm)                     # NLL part + smoothing part, one addition
    assert all(torch.equal(dins[i].cpu(), nll[i]) for i in range(8))


# ------------------------------------------------------------------------------------------------ class counts
def test_class_counts_accumulate_over_two_calls():
    g = torch.Generator().manual_seed(8)
    C = 13
    ys = [torch.randint(0, C, (70, 120, 8), generator=g) for _ in range(2)]
    for y in ys:
        y[torch.rand(y.shape, generator=g) < 0.2] = -1
        y.view(-1)[5::97] = C
        y.view(-1)[7::101] = -5
        y.view(-1)[11] = 1 << 40
    out = None
    for y in ys:
        out = losses.class_counts(y.to(DEV), C, out=out)
    both = torch.cat(ys).view(-1).numpy()
    want = np.bincount(both[(both >= 0) & (both < C)], minlength=C)
    assert out.dtype == torch.int64 and out.device.type == 'cuda' and np.array_equal(out.cpu().numpy(), want)
    # another ignore value: class 3 is skipped, -1 is out of range anyway
    got = losses.class_counts(ys[0].to(DEV), C, ignore_index=3).cpu().numpy()
    one = ys[0].view(-1).numpy()
    want = np.bincount(one[(one >= 0) & (one < C) & (one != 3)], minlength=C)
    assert np.array_equal(got, want) and got[3] == 0
    w = losses.class_weights(out)                                   # the weights land where the counts are
    assert w.device.type == 'cuda' and w.dtype == torch.float32 and torch.equal(w.cpu(), losses.class_weights(out.cpu()))


# ------------------------------------------------------------------------------------------------ through the host layer
def weighted_loss_list(outs, tgts, w, cad, cws, pws):
    """cpu_ref.loss_list (the oracle) extended with F.nll_loss(weight=) and the reference's positive-class composition
    (pyrutils/torch/losses.py:17-18: the input raised to the power p where the target is 1)."""
    base = cpu_ref.loss_list(outs, tgts, w, cad120=cad)
    for i, (o, t) in enumerate(zip(outs, tgts)):
        if cws[i] is not None:
            base[i] = w[i] * F.nll_loss(o, t, weight=torch.as_tensor(cws[i], dtype=torch.float32), ignore_index=-1)
        elif pws[i] is not None and pws[i] > 1:
            base[i] = w[i] * cpu_ref.bce_loss(torch.where(t == 1.0, o ** pws[i], o), t)
    return base


@pytest.mark.parametrize('ds', ['mphoi', 'cad120'])
def test_criterion_on_the_device_against_the_oracle(ds):
    cad = ds == 'cad120'
    outs, tgts = criterion_case(ds)
    sub, aff = WEIGHTS[:10 if cad else 13], WEIGHTS[3:15]
    misc = dict(MISC, class_weights=dict(add=True, subactivity=sub, affordance=aff))
    misc['segmentation_loss'] = dict(MISC['segmentation_loss'], positive_class_weight=2.0)
    crit, names = losses.select_loss('2G-GCN', 'multiple', ds, dict(misc=misc))
    cws, pws, w = crit.keywords['class_weights'], crit.keywords['positive_class_weights'], crit.keywords['weight']
    assert sum(c is not None for c in cws) == (8 if cad else 4) and sum(p is not None for p in pws) == (2 if cad else 1)
    xs = [o.clone().to(DEV).requires_grad_(True) for o in outs]
    got = crit(xs, [t.to(DEV) for t in tgts])
    xo = [o.clone().requires_grad_(True) for o in outs]
    want = weighted_loss_list(xo, tgts, w, cad, cws, pws)
    plain = cpu_ref.loss_list(outs, tgts, w, cad120=cad)
    for name, a, b, c in zip(names, got, want, plain):
        a, b = float(a.detach()), float(b.detach())
        print(f'{name}: {a!r} (oracle {b!r}, unweighted {float(c)!r})')
        assert abs(a - b) <= 1e-5 * max(1.0, abs(b)), name
        assert name.startswith('B_') or abs(b - float(c)) > 1e-3 * abs(b), name        # the options change every other term
    sum(got).backward()
    sum(want).backward()
    for i, (a, b) in enumerate(zip(xs, xo)):
        assert torch.allclose(a.grad.cpu(), b.grad, rtol=1e-5, atol=1e-7), (i, float((a.grad.cpu() - b.grad).abs().max()))
    # a class-weight tensor that lives on the device is taken as it is
    dev_cws = [None if c is None else torch.tensor(c, device=DEV) for c in cws]
    again = losses.multi_task_loss([o.to(DEV) for o in outs], [t.to(DEV) for t in tgts], crit.keywords['loss_functions'], w,
                                   class_weights=dev_cws, positive_class_weights=pws)
    assert torch.equal(torch.stack(again), torch.stack(got).detach())


def test_small_model_trains_through_the_class_weights():
    """MPHOI layout of golden G4 c2 (2 humans, 4 objects, 26 joints) at h = 8, T = 6. Parameter gradients against the oracle
    (cpu_ref.tggcn_forward + the extended loss list) at the gate of the small-model parity tests: 5e-4 of the tensor's largest
    gradient + 5e-6."""
    bs, T, H, O, N, h, C = 2, 6, 2, 4, 26, 8, 13
    torch.manual_seed(5)
    m = TGGCN(input_size=(2048 + 4 * N, 2048), num_classes=(C, None), hidden_size=h, gcn_node=N, **STAGE1)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m = m.to(DEV).train()
    xh, xo, mask = (torch.from_numpy(a) for a in synth_inputs('class_weights', H, O, N, bs, T, seed=5))
    seg = torch.ones(bs, T, H)
    noise = torch.distributions.gumbel.Gumbel(0.0, 1.0).sample((T * O, bs, 2))
    m._gumbel_noise_override = noise
    g = torch.Generator().manual_seed(6)
    cls = [torch.randint(0, C, (bs, T, H), generator=g) for _ in range(2)]
    for c in cls:
        c[1, T - 2:] = -1
    gate = (torch.rand(bs, T, H, generator=g) > 0.5).float()
    tgts = [gate, gate] + cls * 2
    bn = m.geometry_embedding_gcn.joint_embed.cnn[0].bn

    def step(cfg):
        crit, _ = losses.select_loss('2G-GCN', 'multiple', 'mphoi', dict(misc=cfg))
        m.zero_grad(set_to_none=True)
        bn.running_mean.zero_(); bn.running_var.fill_(1.0)
        out = m(xh.to(DEV), xo.to(DEV), mask.to(DEV), human_segmentation=seg.to(DEV))
        got = crit(out, [t.to(DEV) for t in tgts])
        sum(got).backward()
        return ([float(v.detach()) for v in got],
                {k: p.grad.detach().cpu().clone() for k, p in m.named_parameters() if p.grad is not None}, crit)

    misc = dict(MISC, class_weights=dict(add=True, subactivity=WEIGHTS[:C]))
    vals, grads, crit = step(misc)
    assert all(np.isfinite(v) for v in vals) and all(torch.isfinite(v).all() for v in grads.values())
    vals0, grads0, _ = step(MISC)
    assert vals0[:2] == vals[:2] and all(a != b for a, b in zip(vals[2:], vals0[2:]))
    assert any(not torch.equal(grads[k], grads0[k]) for k in grads0)                     # it differs from the unweighted run
    osd = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and 'running' not in k else v.clone()) for k, v in sd.items()}
    ref = cpu_ref.tggcn_forward(osd, dict(m.cfg), xh, xo, mask, training=True, gumbel_noise=noise, human_segmentation=seg)
    w = crit.keywords['weight']
    want = weighted_loss_list(ref, tgts, w, False, crit.keywords['class_weights'], [None] * 6)
    for a, b in zip(vals, want):
        assert abs(a - float(b.detach())) <= 1e-4 * max(1.0, abs(float(b.detach())))
    sum(want).backward()
    worst = 0.0
    for k, ga in grads.items():
        g_ref = osd[k].grad
        if g_ref is None:
            assert float(ga.abs().max()) == 0.0, k
            continue
        scale = max(g_ref.abs().max().item(), 1e-6)
        err = (ga - g_ref).abs().max().item()
        worst = max(worst, err / scale)
        assert err < 5e-4 * scale + 5e-6, (k, err / scale)
    print(f'worst relative parameter-gradient error {worst:.2e}')
