"""GPU: the linear-chain CRF loss kernels (twog_crf_nll_fwd / _bwd) against the fp64 specification tests/crf_ref.py, at
kernel level over the cases of tests/crf_cases.py, through losses.multi_task_loss with the term lists of select_loss, and
through a small model trained for one step.

Tolerance: the gate of a quantity is 4 x the error of the fp32 specification (the same recurrences in numpy fp32) against
fp64 over the cases of the same kind, as recorded in profiles/crf_loss_fp64.json by tools/crf_loss_fp64.py; the factor
covers the device's expf / logf and a different but valid summation order. Loss and per-sequence nll are compared relative
to max(1, |logZ|), the gradients in absolute terms before the factor g. The counts K are exact; the rerun and the
alone-versus-batch comparisons are bit-equal."""
import json
import os

import numpy as np
import pytest
import torch

import twog_gcn_amd  # noqa: F401
from twog_gcn_amd import kernels as twog_kernels
from twog_gcn_amd import losses
from tests import crf_ref as R
from tests import viterbi_ref as V
from tests.crf_cases import BY_NAME, CASES, IGNORE, make, run_kernel_layer
from tests.helpers import ROOT

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = 7.25
GATES = json.load(open(os.path.join(ROOT, 'profiles', 'crf_loss_fp64.json')))['gate']
_SPEC = {}


@pytest.fixture(autouse=True)
def hip_backend():
    twog_kernels._set_backend_for_tests(None)
    assert twog_kernels.get_kernels().name == 'hip'
    yield


def spec(name):
    """The fp64 specification of a case with g = 1, computed once and shared."""
    if name not in _SPEC:
        _SPEC[name] = R.crf_nll(*make(BY_NAME[name]), g=1.0)
    return _SPEC[name]


@pytest.mark.parametrize('name', [c['name'] for c in CASES])
def test_cases_against_the_specification(name):
    case = BY_NAME[name]
    got = run_kernel_layer(twog_kernels.get_kernels(), make(case), DEV)
    want = spec(name)
    err, gate = R.errors(got, want), GATES[case['kind']]
    print(name, {q: f'{err[q]:.3e} (gate {gate[q]:.3e})' for q in R.QUANTITIES})
    assert np.array_equal(got.K, want.K) and got.count == want.count
    assert np.isfinite(got.dinput).all() and np.isfinite(got.dA).all() and np.isfinite(got.dpi).all()
    for q in R.QUANTITIES:
        assert err[q] <= gate[q], (q, err[q], gate[q])
    removed = np.broadcast_to(((make(case)[1] < 0) | (make(case)[1] >= case['C']))[:, None], got.dinput.shape)
    assert not got.dinput[removed].any()                                      # exact zeros at every removed step
    assert (got.nll[want.K > 0] >= -gate['nll'] * np.maximum(1, np.abs(want.logZ[want.K > 0]))).all()


def test_two_runs_give_the_same_bits():
    for name in ('small-bs3-C6-T20-E9-tail-softmax', 'wide-bs2-C33-T17-E3-tail-wide'):
        a = run_kernel_layer(twog_kernels.get_kernels(), make(BY_NAME[name]), DEV, before_g=False)
        b = run_kernel_layer(twog_kernels.get_kernels(), make(BY_NAME[name]), DEV, before_g=False)
        assert a.loss == b.loss
        for q in ('nll', 'logZ', 'gold', 'dinput', 'dA', 'dpi'):
            assert np.array_equal(getattr(a, q).view(np.uint32), getattr(b, q).view(np.uint32)), (name, q)


@pytest.mark.parametrize('name', ['small-bs3-C40-T18-E5-tail-softmax', 'small-bs1-C4-T35-E9-holes-softmax'])
def test_a_rerun_is_byte_identical(name):
    """Forward + backward twice where the shared staging does the most: a second workgroup per clip with idle waves (E = 5
    beyond 32 classes, E = 9 below) and a last chunk that is not whole. Every output of the kernel layer, byte for byte."""
    K = twog_kernels.get_kernels()
    first, again = (run_kernel_layer(K, make(BY_NAME[name]), DEV) for _ in range(2))
    assert first.loss == again.loss and first.count == again.count
    for q in ('nll', 'logZ', 'gold', 'K', 'dinput', 'dA', 'dpi'):
        assert getattr(first, q).tobytes() == getattr(again, q).tobytes(), q


@pytest.mark.parametrize('name,b,e', [('small-bs3-C6-T20-E3-holes-softmax', 1, 2), ('small-bs3-C6-T20-E9-tail-softmax', 2, 8),
                                      ('small-bs3-C40-T18-E5-tail-softmax', 1, 4)])
def test_a_sequence_alone_and_inside_a_batch(name, b, e):
    """Nothing depends on the launch geometry: the per-sequence values are bit-equal, and with g = 1 on both sides (the
    upstream gradient is each call's own count) so is the sequence's slab of d input."""
    K = twog_kernels.get_kernels()
    x, y, A, pi = make(BY_NAME[name])
    batch = run_kernel_layer(K, (x, y, A, pi), DEV)
    alone = run_kernel_layer(K, (np.ascontiguousarray(x[b:b + 1, :, :, e:e + 1]), np.ascontiguousarray(y[b:b + 1, :, e:e + 1]),
                                 A, pi), DEV)
    assert alone.K[0, 0] == batch.K[b, e] > 0
    for q in ('nll', 'logZ', 'gold'):
        assert getattr(alone, q)[0, 0].view(np.uint32) == getattr(batch, q)[b, e].view(np.uint32), q
    assert np.array_equal(alone.dinput[0, :, :, 0].view(np.uint32), batch.dinput[b, :, :, e].view(np.uint32))


def _guarded(n, dtype, pad=64):
    """A buffer of n elements with `pad` sentinel elements on either side: (whole, view)."""
    whole = torch.full((n + 2 * pad,), SENTINEL, dtype=dtype, device=DEV)
    return whole, whole[pad:pad + n]


def _guards_intact(whole, pad=64):
    return bool((whole[:pad] == SENTINEL).all()) and bool((whole[-pad:] == SENTINEL).all())


@pytest.mark.parametrize('name', ['small-bs3-C6-T20-E9-empty-softmax', 'small-bs3-C40-T18-E5-tail-softmax',
                                  'small-bs3-C5-T31-E9-head-softmax'])
def test_store_and_accumulate_and_the_guard_regions(name):
    """Through the C ABI on buffers with sentinels around them: every output is written completely and nothing beside it;
    accumulate is the store result added to the prior contents in fp32, bit for bit."""
    K = twog_kernels.get_kernels()
    x, y, A, pi = (torch.from_numpy(a).to(DEV) for a in make(BY_NAME[name]))
    bs, C, T, E = x.shape
    alpha_b, seq_b, part_b = K.crf_workspace(bs, C, T, E)
    bufs = dict(alpha=_guarded(alpha_b // 4, torch.float32), seq=_guarded(seq_b // 4, torch.float32),
                partials=_guarded(part_b // 4, torch.float32), stats=_guarded(2, torch.float64),
                loss=_guarded(1, torch.float32), dinput=_guarded(x.numel(), torch.float32),
                dA=_guarded(C * C, torch.float32), dpi=_guarded(C, torch.float32))
    v = {k: b[1] for k, b in bufs.items()}
    stream = K._stream()
    rc = K.lib.twog_crf_nll_fwd(x.data_ptr(), y.data_ptr(), bs, C, T, E, A.data_ptr(), pi.data_ptr(), IGNORE, 0.75,
                                v['alpha'].data_ptr(), v['seq'].data_ptr(), v['stats'].data_ptr(), v['loss'].data_ptr(), stream)
    assert rc == 0
    dl = torch.tensor([1.5], dtype=torch.float32, device=DEV)

    def bwd(dinput, accumulate, dA, dpi, acc_params):
        rc = K.lib.twog_crf_nll_bwd(x.data_ptr(), y.data_ptr(), bs, C, T, E, A.data_ptr(), IGNORE, 0.75, v['alpha'].data_ptr(),
                                    v['seq'].data_ptr(), v['stats'].data_ptr(), dl.data_ptr(), dinput.data_ptr(), accumulate,
                                    v['partials'].data_ptr(), dA.data_ptr(), dpi.data_ptr(), acc_params, stream)
        assert rc == 0

    bwd(v['dinput'], 0, v['dA'], v['dpi'], 0)
    torch.cuda.synchronize()
    for k, (whole, _) in bufs.items():
        assert _guards_intact(whole), k
    for k in ('seq', 'stats', 'loss', 'dinput', 'dA', 'dpi', 'partials'):
        assert not bool((v[k] == SENTINEL).any()), k                          # written completely
    want = R.crf_nll(x.cpu().numpy(), y.cpu().numpy(), A.cpu().numpy(), pi.cpu().numpy())
    assert float(v['stats'][1]) == want.count
    assert abs(float(v['loss'][0]) - 0.75 * want.loss) <= 0.75 * GATES['small']['loss'] * max(1.0, np.abs(want.logZ).max()) \
        + 2 * np.spacing(np.float32(0.75 * want.loss))
    g = 0.75 * 1.5 / want.count
    assert np.abs(v['dinput'].view(x.shape).cpu().numpy() - g * want.count * want.dinput).max() <= g * (GATES['small']['dinput'] + 2.0 ** -23)
    # accumulate: prior + store, one fp32 addition per element
    prior = torch.randn(x.numel(), generator=torch.Generator().manual_seed(1)).to(DEV)
    whole, acc = _guarded(x.numel(), torch.float32)
    acc.copy_(prior)
    pA, ppi = torch.full((C * C,), 0.5, device=DEV), torch.full((C,), -2.0, device=DEV)
    accA, accpi = pA.clone(), ppi.clone()
    bwd(acc, 1, accA, accpi, 1)
    torch.cuda.synchronize()
    assert _guards_intact(whole)
    assert torch.equal(acc, prior + v['dinput']) and torch.equal(accA, pA + v['dA']) and torch.equal(accpi, ppi + v['dpi'])


# ------------------------------------------------------------------------------------------------ through the criterion
MISC = dict(anticipation_loss_weight=0.6, budget_loss=dict(add=True, human_weight=0.5, object_weight=0.25),
            first_level_loss_weight=0.3, segmentation_loss=dict(add=True, pretrain=False, weight=0.7))


def _criterion_case(ds, seed=5, bs=3, T=19, C=6):
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
            outs.append(torch.log_softmax(torch.randn(bs, C, T, E, generator=g) * 2, 1))
            t = torch.randint(0, C, (bs, T, E), generator=g)
            t[torch.rand(bs, T, E, generator=g) < 0.2] = -1
        outs[-1], t = outs[-1].to(DEV), t.to(DEV)
        tgts.append(t)
    return outs, tgts


def _module(C, seed):
    g = torch.Generator().manual_seed(seed)
    crf = losses.LinearChainCRF(C)
    with torch.no_grad():
        crf.transitions.copy_(torch.randn(C, C, generator=g))
        crf.initial.copy_(torch.randn(C, generator=g))
    return crf.to(DEV)


@pytest.mark.parametrize('ds', ['mphoi', 'cad120'])
def test_through_multi_task_loss_beside_smoothing_terms_and_class_weights(ds):
    outs, tgts = _criterion_case(ds)
    C = outs[-1].shape[1]
    keys = ['SAR', 'SAP', 'OAR', 'OAP'][:4 if ds == 'cad120' else 2]
    crfs = {k: _module(C, i) for i, k in enumerate(keys)}
    base = dict(MISC, smoothing_loss=dict(add=True), class_weights=dict(add=True, subactivity=[1.0 + 0.1 * c for c in range(C)]))
    crit, names = losses.select_loss('2G-GCN', 'multiple', ds, dict(misc=dict(base, crf_loss=dict(add=True, weight=0.5))), crf=crfs)
    plain_crit, plain_names = losses.select_loss('2G-GCN', 'multiple', ds, dict(misc=base))
    m, n = len(keys), len(plain_names)
    assert names == plain_names + ['CRF_' + k for k in keys]
    leaves = [o.clone().requires_grad_(True) for o in outs]
    plain_leaves = [o.clone().requires_grad_(True) for o in outs]
    got, plain = crit(leaves, tgts), plain_crit(plain_leaves, tgts)
    assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(got[:n], plain))       # the other terms: the same bits
    sum(got).backward()
    sum(plain).backward()
    weights = crit.keywords['weight']
    gate = GATES['small']
    for j, k in enumerate(keys):
        i = names.index('NLL_' + k)
        w = 0.5 * weights[i]
        A, pi = crfs[k].transitions.detach().cpu().numpy(), crfs[k].initial.detach().cpu().numpy()
        want = R.crf_nll(outs[i].cpu().numpy(), tgts[i].cpu().numpy(), A, pi, g=1.0)
        scale = max(1.0, np.abs(want.logZ).max())
        err = abs(float(got[n + j].detach()) - w * want.loss)
        print(ds, k, 'loss error', err, 'gate', w * gate['loss'] * scale)
        assert err <= w * gate['loss'] * scale + 2 * np.spacing(np.float32(w * want.loss))
        g = w / want.count
        # one gradient per input: the CRF launch added to what the NLL and smoothing launches wrote (one fp32 addition)
        crf_part = (leaves[i].grad - plain_leaves[i].grad).cpu().numpy()
        slack = 2 * np.spacing(np.abs(plain_leaves[i].grad.cpu().numpy()) + np.abs(g * want.dinput).astype(np.float32))
        assert (np.abs(crf_part - g * want.dinput) <= g * gate['dinput'] + slack).all()
        assert np.abs(crfs[k].transitions.grad.cpu().numpy() - g * want.dA).max() <= g * gate['dA']
        assert np.abs(crfs[k].initial.grad.cpu().numpy() - g * want.dpi).max() <= g * gate['dpi']
    for i in range(len(outs) - m):                                            # inputs without a CRF term: untouched
        assert torch.equal(leaves[i].grad, plain_leaves[i].grad)


def test_without_crf_the_criterion_is_the_launches_it_was():
    """The MPHOI term list without the key: the losses and gradients of the host path are, bit for bit, those of the two
    launches it has always made, called directly."""
    K = twog_kernels.get_kernels()
    outs, tgts = _criterion_case('mphoi')
    crit, names = losses.select_loss('2G-GCN', 'multiple', 'mphoi', dict(misc=MISC))
    leaves = [o.clone().requires_grad_(True) for o in outs]
    got = crit(leaves, tgts)
    up = torch.linspace(0.5, 1.5, len(got), device=DEV)
    (torch.stack(got) * up).sum().backward()
    kinds = [2, 1, 0, 0, 0, 0]
    terms = [dict(kind=k, input=o, target=t if k else t.to(torch.int64), weight=w, ignore=-1)
             for k, o, t, w in zip(kinds, outs, tgts, crit.keywords['weight'])]
    want_l, stats = K.multitask_loss_fwd(terms)
    want_g = K.multitask_loss_bwd(terms, stats, up, [True] * 6)
    assert torch.equal(torch.stack(got).detach(), want_l)
    assert all(torch.equal(a.grad, b) for a, b in zip(leaves, want_g))


def test_model_and_crf_train_one_step_together():
    """A small TGGCN and a LinearChainCRF under DataParallel(world 1, extra_modules=[crf]) + FusedAdam: the module's
    parameter gradients are the specification's on the captured outputs, and `transitions` moves by the Adam update of
    that gradient."""
    from tests.test_train_options_cpu import _batch, _tiny_model
    from twog_gcn_amd.distributed import DataParallel, FusedAdam
    model = _tiny_model().to(DEV).train()
    crf = _module(13, 3)
    dp = DataParallel(model, extra_modules=[crf], count_weighted_loss=True)
    lr = 1e-2
    opt = FusedAdam(dp.flat, lr=lr)
    crit, names = losses.select_loss('2G-GCN', 'multiple', 'mphoi', dict(misc=dict(crf_loss=dict(add=True, weight=0.8))),
                                     crf={'SAR': crf})
    assert names[-1] == 'CRF_SAR'
    xh, xo, mask, cls, seg = (t.to(DEV) for t in _batch())
    dp.zero_grad()
    out = dp.model(xh, xo, mask)
    captured = out[4].detach().clone()
    before_A, before_pi = crf.transitions.detach().clone(), crf.initial.detach().clone()
    with dp.loss_scope():
        terms = crit(out, [seg, seg, cls, cls, cls, cls])
    sum(terms).backward()
    dp.all_reduce_gradients()
    want = R.crf_nll(captured.cpu().numpy(), cls.cpu().numpy(), before_A.cpu().numpy(), before_pi.cpu().numpy(), g=1.0)
    g = 0.8 / want.count                                                      # world 1: the reducer returns the count itself
    gA, gpi = crf.transitions.grad.detach().clone(), crf.initial.grad.detach().clone()
    print('dA error', np.abs(gA.cpu().numpy() - g * want.dA).max(), 'gate', g * GATES['small']['dA'])
    assert np.abs(gA.cpu().numpy() - g * want.dA).max() <= g * GATES['small']['dA']
    assert np.abs(gpi.cpu().numpy() - g * want.dpi).max() <= g * GATES['small']['dpi']
    assert abs(float(terms[-1].detach()) - 0.8 * want.loss) <= 0.8 * GATES['small']['loss'] * max(1.0, np.abs(want.logZ).max()) \
        + 2 * np.spacing(np.float32(0.8 * want.loss))
    assert float(gA.abs().max()) > 1e-3
    opt.step(dp.grad_scale)
    torch.cuda.synchronize()
    # the first Adam step: m / (1 - b1) = g, v / (1 - b2) = g^2, so the update is -lr g / (|g| + eps); each of its fp32
    # operations is within 2^-23 relative, and the update is at most lr
    for p, b, gr in ((crf.transitions, before_A, gA), (crf.initial, before_pi, gpi)):
        gr = gr.double() * dp.grad_scale
        expect = b.double() - lr * gr / (gr.abs() + opt.eps)
        assert float((p.detach().double() - expect).abs().max()) <= 16 * 2.0 ** -23 * lr + float(np.spacing(np.float32(4.0)))
        assert float((p.detach() - b).abs().max()) > 0.5 * lr
    dp.close()


def test_the_modules_decoder_is_the_viterbi_specification():
    crf = _module(6, 9)
    with torch.no_grad():
        crf.transitions.mul_(3.0)
    g = torch.Generator().manual_seed(2)
    logp = torch.log_softmax(torch.randn(3, 6, 21, 2, generator=g), 1)
    labels = crf.decoder()(logp.to(DEV))
    want, _ = V.viterbi_labels(logp.numpy(), crf.transitions.detach().cpu().numpy(), crf.initial.detach().cpu().numpy(),
                               None, 1, 21)
    assert np.array_equal(labels.cpu().numpy(), want)
    assert not np.array_equal(want, logp.numpy().argmax(1))
