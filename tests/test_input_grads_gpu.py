"""GPU: gradients with respect to x_human and x_objects on the HIP path.

  7. twog_gcn_input_bwd alone against its specification (tests/input_grad_fake.py) run in fp64, per (frame, node) row;
  8. the full path against the oracle: the G16 cases in both modes, and the BASELINE shapes of tests/test_parity_gpu.py
     (T = 120, h = 512; CAD-120, MPHOI, Bimanual and synthetic layouts) under that file's ReLU-boundary conditioning and
     fp64 yardstick; outputs and parameter gradients bit-identical to a run that asks for no input gradient;
  9. determinism, also at the bench size.

The fp64 yardstick is the one of tests/test_parity_gpu.py (_oracle_vs_hip): a result may be no further from the fp64
evaluation than 3 x the distance of the fp32 evaluation of the same specification, + 2e-5 of the tensor's scale.
"""
import pytest
import torch

import twog_gcn_amd  # noqa: F401
from twog_gcn_amd import kernels as twog_kernels
from twog_gcn_amd.models import TGGCN
from oracle import cpu_ref
from tests import test_parity_gpu as P
from tests.helpers import load_g4
from tests.input_grad_cases import G16_CASES, G16_MODES, oracle_run, product_forward
from tests.input_grad_fake import InputGradFakeKernels

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CANARY = -12345.0
YARD_FACTOR, YARD_FLOOR = 3.0, 2e-5     # tests/test_parity_gpu.py: err64 <= 3.0 * own + 2e-5 * scale


@pytest.fixture(autouse=True)
def hip_backend():
    twog_kernels._set_backend_for_tests(None)
    assert twog_kernels.get_kernels().name == 'hip'
    yield


# ---------------------------------------------------------------------------------------------------------------- 7
def _kernel_case(N, H, nF, training, seed):
    """Inputs of one launch, fp32 on the CPU. The BatchNorm quantities are consistent with x and de1 (batch statistics of x;
    dgamma / dbeta the sums of the fp64 specification, rounded), so the train-mode cancellation is the real one."""
    g = torch.Generator().manual_seed(seed)
    x_human = torch.zeros(1, nF, H, 2048 + 4 * N)
    x_human[..., 2048:] = torch.randn(1, nF, H, 4 * N, generator=g) * 0.7 + 0.3
    de1 = torch.randn(nF * N, 64, generator=g) * (torch.rand(nF * N, 64, generator=g) < 0.5)
    w1 = torch.randn(64, 4, generator=g) * 0.5
    gamma = torch.rand(4 * N, generator=g) + 0.5
    xg = x_human[0, :, 0, 2048:].double().view(nF, N, 4).permute(2, 1, 0).reshape(4 * N, nF)   # channel c*N + n
    if training:
        mean, var = xg.mean(1), xg.var(1, unbiased=False)
    else:
        mean, var = torch.randn(4 * N, generator=g).double() * 0.2, (torch.rand(4 * N, generator=g) + 0.5).double()
    invstd = 1.0 / torch.sqrt(var + 1e-5)
    ab = torch.stack([gamma.double() * invstd, torch.zeros(4 * N, dtype=torch.float64)]).float()
    mi = torch.stack([mean, invstd]).float()
    dgamma = dbeta = None
    if training:
        dxh = (de1.double() @ w1.double()).view(nF, N, 4).permute(2, 1, 0).reshape(4 * N, nF)
        x_n = (xg - mi[0].double()[:, None]) * mi[1].double()[:, None]
        dgamma, dbeta = (dxh * x_n).sum(1).float(), dxh.sum(1).float()
    return x_human, ab, mi, w1, de1, dgamma, dbeta


def _spec(args, N, training, dtype):
    x_human, ab, mi, w1, de1, dgamma, dbeta = [None if a is None else a.to(dtype) for a in args]
    out = torch.full(x_human.shape, CANARY, dtype=dtype)
    InputGradFakeKernels().gcn_input_bwd(x_human, N, ab, mi, w1, de1, dgamma, dbeta, training, out)
    return out[..., 2048:]


@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('nF', [1, 7, 960, 7680])
@pytest.mark.parametrize('H', [1, 2, 4])
def test_input_bwd_kernel_against_its_fp64_specification(H, nF, training):
    """Every (frame, node) row of the kernel's result is judged against the yardstick as tests/test_parity_gpu.py defines it:
    no further from the fp64 specification than 3 x the fp32 specification's distance from it -- the tensor's, i.e. its worst
    row's -- + 2e-5 of the tensor's scale. (A row's OWN fp32 error is no bar: it is zero wherever the fp32 evaluation
    happens to round exactly; the share of rows beyond 3 x their own row is printed, not asserted. With one frame in train
    mode the exact answer is pure cancellation, dx^ - dbeta, and both evaluations return rounding residue: the scale is then
    the residue's own and the factor 3 decides alone.)"""
    K = twog_kernels.get_kernels()
    for N in (19, 26, 30, 34, K.lib.twog_gcn_max_nodes()):
        args = _kernel_case(N, H, nF, training, seed=1000 * N + 10 * H + nF % 7)
        s32, s64 = _spec(args, N, training, torch.float32), _spec(args, N, training, torch.float64)
        dargs = [None if a is None else a.to(DEV) for a in args]
        outs = []
        for _ in range(2):
            grad = torch.full(args[0].shape, CANARY, device=DEV)
            K.gcn_input_bwd(dargs[0], N, dargs[1], dargs[2], dargs[3], dargs[4], dargs[5], dargs[6], training, grad)
            outs.append(grad.cpu())
        assert torch.equal(outs[0], outs[1]), 'two launches differ'
        got = outs[0]
        assert bool((got[..., :2048] == CANARY).all()), 'the kernel wrote outside the geometry columns'
        geo = got[..., 2048:]
        assert not bool((geo == CANARY).any()), 'geometry elements left unwritten'
        assert not geo[:, :, 1:].any() and not s64[:, :, 1:].any(), 'humans >= 1 must get exact zeros'
        hip = geo[0, :, 0].reshape(nF * N, 4).double()
        r32, r64 = s32[0, :, 0].reshape(nF * N, 4).double(), s64[0, :, 0].reshape(nF * N, 4)
        scale = max(float(r64.abs().max()), 1e-30)
        er_hip, er_ref = (hip - r64).abs().amax(1), (r32 - r64).abs().amax(1)
        bar = YARD_FACTOR * float(er_ref.max()) + YARD_FLOOR * scale
        own_row = float((er_hip > YARD_FACTOR * er_ref + YARD_FLOOR * scale).double().mean())
        print(f'N {N} H {H} frames {nF} {"train" if training else "eval"}: worst row hip-fp64 {float(er_hip.max()) / scale:.2e}, '
              f'spec32-fp64 {float(er_ref.max()) / scale:.2e} (of the scale {scale:.2e}); share of the bar used '
              f'{float(er_hip.max()) / bar:.3f}; rows beyond 3 x their OWN row of the fp32 specification: {100 * own_row:.3f} %')
        bad = er_hip > bar
        assert not bool(bad.any()), (N, int(bad.sum()), float(er_hip.max()) / scale, float(er_ref.max()) / scale)


def test_input_bwd_refuses_bad_arguments_without_launching():
    K = twog_kernels.get_kernels()
    lib, N = K.lib, 34
    args = [a if a is None else a.to(DEV) for a in _kernel_case(N, 2, 4, True, seed=5)]
    xh, ab, mi, w1, de1, dgamma, dbeta = args
    grad = torch.full(xh.shape, CANARY, device=DEV)
    Fh = xh.shape[-1]
    st = K._stream()

    def call(n_nodes=N, x=xh.data_ptr() + 8192, ab_=ab.data_ptr(), mi_=mi.data_ptr(), w=w1.data_ptr(), d=de1.data_ptr(),
             dg=dgamma.data_ptr(), db=dbeta.data_ptr(), training=1, out=grad.data_ptr() + 8192, n_humans=2, blocks=1):
        return lib.twog_gcn_input_bwd(x, 2 * Fh, 4, n_nodes, n_humans, Fh, ab_, mi_, w, d, dg, db, training, out, blocks, st)

    assert call(n_nodes=0) == -1 and call(n_nodes=lib.twog_gcn_max_nodes() + 1) == -1 and call(n_nodes=-3) == -1
    for kw in (dict(x=None), dict(ab_=None), dict(w=None), dict(d=None), dict(out=None), dict(mi_=None), dict(dg=None),
               dict(db=None), dict(n_humans=0), dict(blocks=0), dict(out=grad.data_ptr() + 8196)):
        assert call(**kw) < 0, kw
    torch.cuda.synchronize()
    assert bool((grad == CANARY).all()), 'a refused call launched'
    assert call(training=0, mi_=None, dg=None, db=None) == 0      # eval mode needs none of the three
    torch.cuda.synchronize()
    assert not bool((grad[..., 2048:] == CANARY).any())


# ---------------------------------------------------------------------------------------------------------------- 8
def _gate(name, got, ref):
    scale = max(ref.abs().max().item(), 1e-6)
    err = (got.cpu() - ref).abs().max().item()
    print(f'{name}: err / scale {err / scale:.2e} (scale {scale:.2e})')
    return err, scale, err < P.GRAD_REL * scale + P.GRAD_ABS


@pytest.mark.parametrize('mode', G16_MODES)
@pytest.mark.parametrize('name', G16_CASES)
def test_full_path_g16_cases_against_the_oracle(name, mode):
    ref = oracle_run(name, mode)
    m0, kw0, out0, loss0 = product_forward(name, mode, need=(False, False), device=DEV)
    loss0.backward()
    m, kw, out, loss = product_forward(name, mode, device=DEV)
    loss.backward()
    gh, go = kw['x_human'].grad, kw['x_objects'].grad
    assert gh is not None and go is not None
    for what, got, want in (('x_human.grad', gh, ref['xh']), ('x_objects.grad', go, ref['xo']),
                            ('x_human.grad geometry', gh[:, :, 0, 2048:], ref['xh'][:, :, 0, 2048:])):
        err, scale, ok = _gate(f'{name} {mode} {what}', got, want)
        assert ok, (name, mode, what, err, scale)
    assert not gh[:, :, 1:, 2048:].any()
    z4, meta = load_g4(name)
    if meta['layout'] != 'cad120':
        assert not go.permute(0, 2, 1, 3)[torch.from_numpy(z4['objects_mask']).to(DEV) == 0].any()
    # asking for the input gradients changes no output and no parameter gradient
    for a, b in zip(out0, out):
        assert torch.equal(a, b)
    for (n, p0), (_, p1) in zip(m0.named_parameters(), m.named_parameters()):
        assert (p0.grad is None) == (p1.grad is None), n
        assert p0.grad is None or torch.equal(p0.grad, p1.grad), n


def _input_grads_vs_oracle(bs, T, H, O, N, h, seed, n_sub=13, n_aff=None, both_given=False, max_nudged_share=0.04,
                           max_rounds=8):
    """tests/test_parity_gpu.py::_oracle_vs_hip for the two input gradients: the same model, inputs and noise, the same
    conditioning of the case (tests/relu_boundary.py::condition_case with its bounds on the nudged share), every output at
    1e-4, then x_human.grad, its geometry block on its own scale and x_objects.grad at GRAD_REL of the tensor's scale +
    GRAD_ABS; a tensor beyond that must meet the fp64 yardstick, and at most MAX_YARDSTICK_TENSORS may need it."""
    from tests import relu_boundary as _rb
    cfg = dict(P.STAGE1)
    if H == 1:
        cfg['message_humans_to_human'] = False
    torch.manual_seed(seed)
    m = TGGCN(input_size=(2048 + 4 * N, 2048), num_classes=(n_sub, n_aff), hidden_size=h, gcn_node=N, **cfg)
    buffers = {k: v.detach().clone() for k, v in m.state_dict().items() if 'running_' in k or 'num_batches' in k}
    x_human, x_objects, mask = P._synthetic(bs, T, H, O, N, seed)
    g = torch.Generator().manual_seed(seed + 100)
    if both_given:
        kw = dict(human_segmentation=(torch.rand(bs, T, H, generator=g) < 0.3).float(),
                  objects_segmentation=(torch.rand(bs, T, O, generator=g) < 0.3).float())
        noise = None
    else:
        kw = dict(human_segmentation=torch.ones(bs, T, H))
        noise = torch.distributions.gumbel.Gumbel(0.0, 1.0).sample((T * O, bs, 2))
    m = m.to(DEV).train()
    m._gumbel_noise_override = noise
    dkw = {k: v.to(DEV) for k, v in kw.items()}
    xh_d, xo_d, mask_d = x_human.to(DEV), x_objects.to(DEV), mask.to(DEV)

    def fwd(xh=xh_d, xo=xo_d):
        return m(xh, xo, mask_d, **dkw)

    rounds, nudged = _rb.condition_case(m, fwd, max_rounds=max_rounds)
    totals = dict(_rb.LAST_TOTALS)
    if totals['units']:
        n_nudged = sum(nudged.values())
        assert n_nudged <= max(P.MAX_NUDGED_UNIT_SHARE, max_nudged_share) * totals['units'], ('too many ReLU units nudged', nudged, totals)
        assert n_nudged <= max_nudged_share * totals['units'], (n_nudged, totals['units'], max_nudged_share)
    m.load_state_dict(buffers, strict=False)
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}

    def oracle(dtype):
        osd = {k: (v.to(dtype).requires_grad_(True) if v.is_floating_point() and 'running' not in k
                   else (v.to(dtype) if v.is_floating_point() else v.clone())) for k, v in sd.items()}
        xh = x_human.detach().clone().to(dtype).requires_grad_(True)
        xo = x_objects.detach().clone().to(dtype).requires_grad_(True)
        ref = cpu_ref.tggcn_forward(osd, dict(m.cfg), xh, xo, mask.to(dtype), training=True,
                                    gumbel_noise=None if noise is None else noise.to(dtype),
                                    **{k: v.to(dtype) for k, v in kw.items()})
        return ref, xh, xo

    ref, xh_o, xo_o = oracle(torch.float32)
    rs = [torch.randn(o.shape, generator=torch.Generator().manual_seed(i)) for i, o in enumerate(ref)]
    sum((o * r).sum() for o, r in zip(ref, rs) if o.requires_grad).backward()

    def hip(need):
        m.zero_grad(set_to_none=True)
        m.load_state_dict(buffers, strict=False)
        xh = xh_d.detach().clone().requires_grad_(need)
        xo = xo_d.detach().clone().requires_grad_(need)
        out = fwd(xh, xo)
        sum((o * r.to(DEV)).sum() for o, r in zip(out, rs) if o.requires_grad).backward()
        return out, {n: (None if p.grad is None else p.grad.clone()) for n, p in m.named_parameters()}, xh.grad, xo.grad

    out0, pg0, gh0, go0 = hip(False)
    assert gh0 is None and go0 is None
    out, pg, gh, go = hip(True)
    for i, (o, r) in enumerate(zip(out, ref)):
        err = (o.detach().cpu() - r.detach()).abs().max().item() / max(1.0, r.detach().abs().max().item())
        assert err < P.REL, (i, err)
    for a, b in zip(out0, out):
        assert torch.equal(a, b), 'an output changed when the input gradients were requested'
    for n in pg0:
        assert (pg0[n] is None) == (pg[n] is None), n
        assert pg0[n] is None or torch.equal(pg0[n], pg[n]), ('a parameter gradient changed', n)
    assert not gh[:, :, 1:, 2048:].any(), 'geometry columns of the humans >= 1 must be exact zeros'
    cut = {'x_human.grad': lambda t: t, 'x_human.grad geometry': lambda t: t[:, :, 0, 2048:], 'x_objects.grad': lambda t: t}
    src = {'x_human.grad': (gh, xh_o), 'x_human.grad geometry': (gh, xh_o), 'x_objects.grad': (go, xo_o)}
    off = []
    for what, f in cut.items():
        got, leaf = src[what]
        err, scale, ok = _gate(f'{what} (bs {bs} T {T} H {H} O {O} N {N} h {h})', f(got), f(leaf.grad))
        if not ok:
            off.append((what, err / scale))
    if off:
        assert len(off) <= P.MAX_YARDSTICK_TENSORS, off
        f64 = torch.float64
        ref64, xh64, xo64 = oracle(f64)
        n_hard = 2 if n_aff is not None else 1
        assert all(torch.equal(ref64[i].float(), ref[i].detach()) for i in range(n_hard)), 'hard gates differ in fp64'
        sum((o * r.to(f64)).sum() for o, r in zip(ref64, rs) if o.requires_grad).backward()
        leaf64 = {'x_human.grad': xh64, 'x_human.grad geometry': xh64, 'x_objects.grad': xo64}
        for what, e in off:
            got, leaf = src[what]
            g64, g32 = cut[what](leaf64[what].grad), cut[what](leaf.grad)
            scale = max(g32.abs().max().item(), 1e-6)
            own = (g32.to(f64) - g64).abs().max().item()
            err64 = (cut[what](got).cpu().to(f64) - g64).abs().max().item()
            print(f'{what}: beyond 5e-4 ({e:.2e}); hip-fp64 {err64 / scale:.2e}, oracle32-fp64 {own / scale:.2e}')
            assert err64 <= YARD_FACTOR * own + YARD_FLOOR * scale, ('beyond the fp64 yardstick', what, e, err64 / scale, own / scale)
    print(f'ReLU-boundary units nudged in {rounds} round(s): {nudged}; on the fp64 yardstick: {off}')


def test_full_path_synthetic_layout_full_width():
    """BASELINE configs[2]: H=2, O=8, N=34, T=120, h=512 (the shape of test_oracle_parity_full_width_forward_backward)."""
    _input_grads_vs_oracle(bs=2, T=120, H=2, O=8, N=34, h=512, seed=7, max_nudged_share=0.01)


def test_full_path_cad120_layout_full_width():
    """BASELINE configs[0]: one human, five objects, N=19, object heads, both segmentations given; masked objects receive a
    gradient through the object frame heads."""
    _input_grads_vs_oracle(bs=2, T=120, H=1, O=5, N=19, h=512, seed=21, n_sub=10, n_aff=12, both_given=True)


def test_full_path_mphoi_layout_full_width():
    """BASELINE configs[1]: H=2, O=4, N=26, T=120, h=512."""
    _input_grads_vs_oracle(bs=2, T=120, H=2, O=4, N=26, h=512, seed=9)


def test_full_path_bimanual_layout_full_width():
    """The Bimanual layout (H=2, O=9, N=30) at T=120, h=512."""
    _input_grads_vs_oracle(bs=2, T=120, H=2, O=9, N=30, h=512, seed=17, n_sub=14, max_nudged_share=0.20, max_rounds=24)


# ---------------------------------------------------------------------------------------------------------------- 9
@pytest.mark.parametrize('shape', [dict(bs=3, T=7, H=2, O=4, N=26, h=16), dict(bs=64, T=120, H=2, O=8, N=34, h=512)],
                         ids=['small', 'bench'])
def test_input_gradients_are_bit_reproducible(shape):
    bs, T, H, O, N, h = (shape[k] for k in ('bs', 'T', 'H', 'O', 'N', 'h'))
    torch.manual_seed(3)
    m = TGGCN(input_size=(2048 + 4 * N, 2048), num_classes=(13, None), hidden_size=h, gcn_node=N, **P.STAGE1).to(DEV).train()
    m._gumbel_noise_override = torch.distributions.gumbel.Gumbel(0.0, 1.0).sample((T * O, bs, 2))
    x_human, x_objects, mask = P._synthetic(bs, T, H, O, N, 3)
    seg = torch.ones(bs, T, H, device=DEV)
    runs = []
    for _ in range(2):
        xh, xo = x_human.to(DEV).requires_grad_(True), x_objects.to(DEV).requires_grad_(True)
        out = m(xh, xo, mask.to(DEV), human_segmentation=seg)
        sum((o * o).sum() for o in out if o.requires_grad).backward()
        runs.append((xh.grad.clone(), xo.grad.clone()))
        m.zero_grad(set_to_none=True)
    assert torch.isfinite(runs[0][0]).all() and torch.isfinite(runs[0][1]).all()
    assert runs[0][0].any() and runs[0][1].any()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
