"""GPU: the semi-Markov CRF loss kernels (twog_semicrf_nll_fwd / _bwd) against the fp64 specification tests/semicrf_ref.py,
at kernel level over the cases of tests/semicrf_cases.py, through losses.multi_task_loss with the term lists of select_loss,
and through a small model trained for one step.

Tolerance: the gate of a quantity is 4 x the error of the fp32 specification (the same recurrences in numpy fp32) against
fp64 over the cases of the same kind, as recorded in profiles/semicrf_loss_fp64.json by tools/semicrf_loss_fp64.py; the factor
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
from tests import segdecode_ref as S
from tests import semicrf_ref as R
from tests.crf_cases import run_kernel_layer as run_crf_layer
from tests.helpers import ROOT
from tests.semicrf_cases import BY_NAME, CASES, IGNORE, make, run_kernel_layer
from tests.semicrf_fake import SemiCrfFakeKernels

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = 7.25
GATES = json.load(open(os.path.join(ROOT, 'profiles', 'semicrf_loss_fp64.json')))['gate']
CRF_GATES = json.load(open(os.path.join(ROOT, 'profiles', 'crf_loss_fp64.json')))['gate']
_SPEC = {}


@pytest.fixture(autouse=True)
def hip_backend():
    twog_kernels._set_backend_for_tests(None)
    assert twog_kernels.get_kernels().name == 'hip'
    yield
    twog_kernels._set_backend_for_tests(None)


def spec(name):
    """The fp64 specification of a case with g = 1, computed once and shared."""
    if name not in _SPEC:
        _SPEC[name] = R.semicrf_nll(*make(BY_NAME[name]), g=1.0)
    return _SPEC[name]


def test_no_gate_is_vacuous():
    per_case = json.load(open(os.path.join(ROOT, 'profiles', 'semicrf_loss_fp64.json')))['fp32_spec_per_case']
    assert sorted(per_case) == sorted(BY_NAME)
    for q in R.QUANTITIES:
        assert any(e[q] > 0 for e in per_case.values()), q


@pytest.mark.parametrize('name', [c['name'] for c in CASES])
def test_cases_against_the_specification(name):
    case = BY_NAME[name]
    tensors = make(case)
    got = run_kernel_layer(twog_kernels.get_kernels(), tensors, DEV)
    want = spec(name)
    err, gate = R.errors(got, want), GATES[case['kind']]
    print(name, '--', case['claim'], {q: f'{err[q]:.3e} (gate {gate[q]:.3e})' for q in R.QUANTITIES})
    assert np.array_equal(got.K, want.K) and got.count == want.count
    for q in ('nll', 'dinput', 'dA', 'dpi', 'ddur'):
        assert np.isfinite(getattr(got, q)).all(), q
    for q in R.QUANTITIES:
        assert err[q] <= gate[q], (q, err[q], gate[q])
    y, A, pi, dur = tensors[1:]
    removed = np.broadcast_to(((y < 0) | (y >= case['C']))[:, None], got.dinput.shape)
    assert not got.dinput[removed].any()                                      # exact zeros at every removed step
    assert (got.nll[want.K > 0] >= -gate['nll'] * np.maximum(1, np.abs(want.logZ[want.K > 0]))).all()
    # a -inf entry gets gradient exactly 0.0
    assert not got.dA[np.isneginf(A)].any() and not got.dpi[np.isneginf(pi)].any() and not got.ddur[np.isneginf(dur)].any()
    if case['D'] > case['T']:
        assert not got.ddur[:, case['T']:].any()                              # a duration that cannot occur


@pytest.mark.parametrize('name', ['small-bs1-C40-T18-E5-D6-tail-infdiag', 'small-bs1-C5-T16-E9-D4-all-softmax'])
def test_a_rerun_is_byte_identical(name):
    """Forward + backward twice where the shared staging does the most: a second workgroup per clip with idle waves (E = 5
    beyond 32 classes in the backward, E = 9 below). Every output of the kernel layer, byte for byte."""
    K = twog_kernels.get_kernels()
    first, again = (run_kernel_layer(K, make(BY_NAME[name]), DEV) for _ in range(2))
    assert first.loss == again.loss and first.count == again.count
    for q in ('nll', 'logZ', 'gold', 'K', 'dinput', 'dA', 'dpi', 'ddur'):
        assert getattr(first, q).tobytes() == getattr(again, q).tobytes(), q


@pytest.mark.parametrize('name,b,e', [('small-bs3-C6-T20-E3-D6-holes-softmax', 1, 2), ('small-bs3-C6-T20-E9-D6-tail-softmax', 2, 8),
                                      ('small-bs1-C40-T18-E5-D6-tail-infdiag', 0, 4)])
def test_a_sequence_alone_and_inside_a_batch(name, b, e):
    """Nothing depends on the launch geometry: the per-sequence values are bit-equal, and with g = 1 on both sides (the
    upstream gradient is each call's own count) so is the sequence's slab of d input."""
    K = twog_kernels.get_kernels()
    x, y, A, pi, dur = make(BY_NAME[name])
    batch = run_kernel_layer(K, (x, y, A, pi, dur), DEV)
    alone = run_kernel_layer(K, (np.ascontiguousarray(x[b:b + 1, :, :, e:e + 1]), np.ascontiguousarray(y[b:b + 1, :, e:e + 1]),
                                 A, pi, dur), DEV)
    assert alone.K[0, 0] == batch.K[b, e] > 0
    for q in ('nll', 'logZ', 'gold'):
        assert getattr(alone, q)[0, 0].view(np.uint32) == getattr(batch, q)[b, e].view(np.uint32), q
    assert np.array_equal(alone.dinput[0, :, :, 0].view(np.uint32), batch.dinput[b, :, :, e].view(np.uint32))


def _sentinel(dtype):
    return SENTINEL if dtype.is_floating_point else int(SENTINEL)             # the marks are 0 or 1


def _guarded(n, dtype, pad=64):
    """A buffer of n elements with `pad` sentinel elements on either side: (whole, view)."""
    whole = torch.full((n + 2 * pad,), _sentinel(dtype), dtype=dtype, device=DEV)
    return whole, whole[pad:pad + n]


def _guards_intact(whole, pad=64):
    s = _sentinel(whole.dtype)
    return bool((whole[:pad] == s).all()) and bool((whole[-pad:] == s).all())


@pytest.mark.parametrize('name', ['small-bs3-C6-T20-E9-D6-absent-softmax', 'small-bs1-C40-T18-E5-D6-tail-infdiag',
                                  'small-bs2-C6-T20-E2-D23-all-softmax'])
def test_store_and_accumulate_and_the_guard_regions(name):
    """Through the C ABI on buffers with sentinels around them: every output is written completely and nothing beside it;
    accumulate is the store result added to the prior contents in fp32, bit for bit."""
    K = twog_kernels.get_kernels()
    x, y, A, pi, dur = (torch.from_numpy(a).to(DEV) for a in make(BY_NAME[name]))
    bs, C, T, E = x.shape
    D = dur.shape[1]
    p = K.semicrf_plan(bs, C, T, E, D)
    bufs = dict(ed=_guarded(p['ed_bytes'] // 4, torch.float32), marks=_guarded(p['marks_bytes'] // 4, torch.int32),
                seq=_guarded(p['seq_bytes'] // 4, torch.float32), partials=_guarded(p['partial_bytes'] // 4, torch.float32),
                stats=_guarded(2, torch.float64), loss=_guarded(1, torch.float32), dinput=_guarded(x.numel(), torch.float32),
                dA=_guarded(C * C, torch.float32), dpi=_guarded(C, torch.float32), ddur=_guarded(C * D, torch.float32))
    v = {k: b[1] for k, b in bufs.items()}
    stream = K._stream()
    rc = K.lib.twog_semicrf_nll_fwd(x.data_ptr(), y.data_ptr(), bs, C, T, E, A.data_ptr(), pi.data_ptr(), dur.data_ptr(), D,
                                    IGNORE, 0.75, v['ed'].data_ptr(), v['marks'].data_ptr(), v['seq'].data_ptr(),
                                    v['stats'].data_ptr(), v['loss'].data_ptr(), stream)
    assert rc == 0
    dl = torch.tensor([1.5], dtype=torch.float32, device=DEV)

    def bwd(dinput, accumulate, dA, dpi, ddur, acc_params):
        rc = K.lib.twog_semicrf_nll_bwd(x.data_ptr(), y.data_ptr(), bs, C, T, E, A.data_ptr(), dur.data_ptr(), D, IGNORE, 0.75,
                                        v['ed'].data_ptr(), v['marks'].data_ptr(), v['seq'].data_ptr(), v['stats'].data_ptr(),
                                        dl.data_ptr(), dinput.data_ptr(), accumulate, v['partials'].data_ptr(), dA.data_ptr(),
                                        dpi.data_ptr(), ddur.data_ptr(), acc_params, stream)
        assert rc == 0

    bwd(v['dinput'], 0, v['dA'], v['dpi'], v['ddur'], 0)
    torch.cuda.synchronize()
    for k, (whole, _) in bufs.items():
        assert _guards_intact(whole), k
    for k in ('marks', 'seq', 'stats', 'loss', 'dinput', 'dA', 'dpi', 'ddur', 'partials'):
        assert not bool((v[k] == _sentinel(v[k].dtype)).any()), k             # written completely
    want = R.semicrf_nll(*(a.cpu().numpy() for a in (x, y, A, pi, dur)))
    assert float(v['stats'][1]) == want.count
    assert abs(float(v['loss'][0]) - 0.75 * want.loss) <= 0.75 * GATES['small']['loss'] * max(1.0, np.abs(want.logZ).max()) \
        + 2 * np.spacing(np.float32(0.75 * want.loss))
    g = 0.75 * 1.5 / want.count
    assert np.abs(v['dinput'].view(x.shape).cpu().numpy() - g * want.count * want.dinput).max() <= g * (GATES['small']['dinput'] + 2.0 ** -23)
    assert np.abs(v['ddur'].view(C, D).cpu().numpy() - g * want.count * want.ddur).max() <= g * (GATES['small']['ddur'] + 2.0 ** -23)
    # accumulate: prior + store, one fp32 addition per element
    prior = torch.randn(x.numel(), generator=torch.Generator().manual_seed(1)).to(DEV)
    whole, acc = _guarded(x.numel(), torch.float32)
    acc.copy_(prior)
    pA, ppi, pdur = torch.full((C * C,), 0.5, device=DEV), torch.full((C,), -2.0, device=DEV), torch.full((C * D,), 1.25, device=DEV)
    accA, accpi, accdur = pA.clone(), ppi.clone(), pdur.clone()
    bwd(acc, 1, accA, accpi, accdur, 1)
    torch.cuda.synchronize()
    assert _guards_intact(whole)
    assert torch.equal(acc, prior + v['dinput']) and torch.equal(accA, pA + v['dA']) and torch.equal(accpi, ppi + v['dpi'])
    assert torch.equal(accdur, pdur + v['ddur'])
    # d input alone (no parameter gradients, no partials): the same bits
    whole, only = _guarded(x.numel(), torch.float32)
    rc = K.lib.twog_semicrf_nll_bwd(x.data_ptr(), y.data_ptr(), bs, C, T, E, A.data_ptr(), dur.data_ptr(), D, IGNORE, 0.75,
                                    v['ed'].data_ptr(), v['marks'].data_ptr(), v['seq'].data_ptr(), v['stats'].data_ptr(),
                                    dl.data_ptr(), only.data_ptr(), 0, None, None, None, None, 0, stream)
    torch.cuda.synchronize()
    assert rc == 0 and _guards_intact(whole) and torch.equal(only, v['dinput'])


def test_at_one_step_per_segment_against_the_crf_kernels():
    """D = 1 and dur = 0 is the linear-chain CRF (tests/test_semicrf_cpu.py derives it): the two kernel families on the same
    inputs agree within the sum of both gates, and ddur[c, 0] is the sum of d input over the steps."""
    from tests.crf_cases import BY_NAME as CRF_BY_NAME, make as crf_make
    K = twog_kernels.get_kernels()
    for name in ('small-bs3-C6-T20-E9-tail-softmax', 'small-bs3-C40-T18-E5-tail-softmax'):
        x, y, A, pi = crf_make(CRF_BY_NAME[name])
        semi = run_kernel_layer(K, (x, y, A, pi, np.zeros((x.shape[1], 1), np.float32)), DEV)
        chain = run_crf_layer(K, (x, y, A, pi), DEV)
        assert np.array_equal(semi.K, chain.K)
        scale = np.maximum(1.0, np.abs(chain.logZ.astype(np.float64)))
        assert (np.abs(semi.nll.astype(np.float64) - chain.nll) / scale).max() <= GATES['small']['nll'] + CRF_GATES['small']['nll']
        for q in ('dinput', 'dA', 'dpi'):
            assert np.abs(getattr(semi, q).astype(np.float64) - getattr(chain, q)).max() <= GATES['small'][q] + CRF_GATES['small'][q], q
        assert np.abs(semi.ddur[:, 0] - semi.dinput.astype(np.float64).sum((0, 2, 3))).max() <= GATES['small']['ddur'] + \
            x.shape[0] * x.shape[2] * x.shape[3] * 2.0 ** -23


def test_every_return_code():
    K = twog_kernels.get_kernels()
    x, y, A, pi, dur = (torch.from_numpy(a).to(DEV) for a in make(BY_NAME['small-bs2-C6-T20-E2-D2-all-softmax']))
    bs, C, T, E = x.shape
    D = dur.shape[1]
    p = K.semicrf_plan(bs, C, T, E, D)
    ed, marks = torch.empty(p['ed_bytes'] // 4, device=DEV), torch.empty(p['marks_bytes'] // 4, dtype=torch.int32, device=DEV)
    seq, partials = torch.empty(p['seq_bytes'] // 4, device=DEV), torch.empty(p['partial_bytes'] // 4, device=DEV)
    stats, loss = torch.empty(2, dtype=torch.float64, device=DEV), torch.empty(1, device=DEV)
    dl, dx = torch.ones(1, device=DEV), torch.empty_like(x)
    dA, dpi, ddur = torch.empty(C, C, device=DEV), torch.empty(C, device=DEV), torch.empty(C, D, device=DEV)
    ptr = lambda t: None if t is None else t.data_ptr()

    def fwd(bs=bs, C=C, T=T, E=E, D=D, A=A, pi=pi, dur=dur, x=x, ed=ed, marks=marks, seq=seq, stats=stats, loss=loss):
        return K.lib.twog_semicrf_nll_fwd(ptr(x), y.data_ptr(), bs, C, T, E, ptr(A), ptr(pi), ptr(dur), D, IGNORE, 1.0, ptr(ed),
                                          ptr(marks), ptr(seq), ptr(stats), ptr(loss), K._stream())

    def bwd(bs=bs, C=C, T=T, E=E, D=D, A=A, dur=dur, ed=ed, marks=marks, dx=dx, partials=partials, dA=dA, dpi=dpi, ddur=ddur):
        return K.lib.twog_semicrf_nll_bwd(x.data_ptr(), y.data_ptr(), bs, C, T, E, ptr(A), ptr(dur), D, IGNORE, 1.0, ptr(ed),
                                          ptr(marks), seq.data_ptr(), stats.data_ptr(), dl.data_ptr(), ptr(dx), 0, ptr(partials),
                                          ptr(dA), ptr(dpi), ptr(ddur), 0, K._stream())

    for call in (fwd, bwd):
        assert call(D=0) == -1 and call(C=0) == -1 and call(T=0) == -1 and call(E=0) == -1 and call(bs=-1) == -1
        assert call(C=65) == -2 and call(T=4097) == -2 and call(D=129) == -2 and call(bs=65536) == -2
        assert call(A=None) == -3 and call(dur=None) == -3 and call(ed=None) == -3 and call(marks=None) == -3
    assert fwd(pi=None) == -3 and fwd(x=None) == -3 and fwd(seq=None) == -3 and fwd(stats=None) == -3 and fwd(loss=None) == -3
    assert fwd() == 0
    # the parameter gradients come together or not at all, and need the partials
    assert bwd(dA=None) == -3 and bwd(dpi=None) == -3 and bwd(ddur=None) == -3 and bwd(partials=None) == -3
    assert bwd() == 0 and bwd(dx=None) == 0 and bwd(dA=None, dpi=None, ddur=None, partials=None) == 0
    assert bwd(dx=None, dA=None, dpi=None, ddur=None) == 0                    # nothing asked for: nothing launched
    # no sequence: the sums alone, over nothing
    assert fwd(bs=0, x=None, ed=None, marks=None, seq=None) == 0
    torch.cuda.synchronize()
    assert float(loss[0]) == 0.0 and stats.tolist() == [0.0, 0.0]
    assert K.semicrf_limits() == (64, 4096, 128)
    with pytest.raises(ValueError):
        K.semicrf_plan(1, 4, 8, 1, 129)


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
            t = torch.randint(0, C, (bs, T, E), generator=g).repeat_interleave(3, 1)[:, :T]      # runs of three
            t[torch.rand(bs, T, E, generator=g) < 0.2] = -1
        outs[-1], t = outs[-1].to(DEV), t.to(DEV)
        tgts.append(t)
    return outs, tgts


def _module(C, D, seed):
    g = torch.Generator().manual_seed(seed)
    m = losses.SemiMarkovCRF(C, D)
    with torch.no_grad():
        m.transitions.copy_(torch.randn(C, C, generator=g))
        m.durations.copy_(torch.randn(C, D, generator=g))
        m.initial.copy_(torch.randn(C, generator=g))
    return m.to(DEV)


def _want(out, tgt, m):
    return R.semicrf_nll(out.cpu().numpy(), tgt.cpu().numpy(), m.transitions.detach().cpu().numpy(),
                         m.initial.detach().cpu().numpy(), m.durations.detach().cpu().numpy(), g=1.0)


@pytest.mark.parametrize('ds', ['mphoi', 'cad120'])
def test_through_multi_task_loss_beside_the_other_terms(ds):
    """select_loss with smoothing terms, class weights, a LinearChainCRF on the first key and SemiMarkovCRF modules on the
    others: the other terms keep their bits, the semi-Markov terms and all their gradients are the specification's."""
    outs, tgts = _criterion_case(ds)
    C = outs[-1].shape[1]
    keys = ['SAR', 'SAP', 'OAR', 'OAP'][:4 if ds == 'cad120' else 2]
    mods = {k: _module(C, 5, i) for i, k in enumerate(keys)}
    chain = losses.LinearChainCRF(C).to(DEV)
    with torch.no_grad():
        chain.transitions.copy_(torch.randn(C, C, generator=torch.Generator().manual_seed(40)))
    mods[keys[0]] = chain
    base = dict(MISC, smoothing_loss=dict(add=True), class_weights=dict(add=True, subactivity=[1.0 + 0.1 * c for c in range(C)]))
    with_crf = dict(base, crf_loss=dict(add=True, weight=0.5))
    crit, names = losses.select_loss('2G-GCN', 'multiple', ds, dict(misc=with_crf), crf=mods)
    chain_crit, chain_names = losses.select_loss('2G-GCN', 'multiple', ds, dict(misc=with_crf), crf={keys[0]: chain})
    n = len(chain_names)
    assert names == chain_names + ['SCRF_' + k for k in keys[1:]]
    leaves = [o.clone().requires_grad_(True) for o in outs]
    chain_leaves = [o.clone().requires_grad_(True) for o in outs]
    got = crit(leaves, tgts)
    sum(got).backward()
    chain_grad = chain.transitions.grad.clone()
    chain.transitions.grad = None
    only_chain = chain_crit(chain_leaves, tgts)
    sum(only_chain).backward()
    assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(got[:n], only_chain))     # the other terms: the same bits
    assert torch.equal(chain_grad, chain.transitions.grad)
    weights = crit.keywords['weight']
    gate = GATES['small']
    for j, k in enumerate(keys[1:]):
        i = names.index('NLL_' + k)
        w = 0.5 * weights[i]
        want = _want(outs[i], tgts[i], mods[k])
        scale = max(1.0, np.abs(want.logZ).max())
        err = abs(float(got[n + j].detach()) - w * want.loss)
        print(ds, k, 'loss error', err, 'gate', w * gate['loss'] * scale)
        assert err <= w * gate['loss'] * scale + 2 * np.spacing(np.float32(w * want.loss))
        g = w / want.count
        # one gradient per input: the launch added to what the NLL and smoothing launches wrote (one fp32 addition)
        part = (leaves[i].grad - chain_leaves[i].grad).cpu().numpy()
        slack = 2 * np.spacing(np.abs(chain_leaves[i].grad.cpu().numpy()) + np.abs(g * want.dinput).astype(np.float32))
        assert (np.abs(part - g * want.dinput) <= g * gate['dinput'] + slack).all()
        assert np.abs(mods[k].transitions.grad.cpu().numpy() - g * want.dA).max() <= g * gate['dA']
        assert np.abs(mods[k].initial.grad.cpu().numpy() - g * want.dpi).max() <= g * gate['dpi']
        assert np.abs(mods[k].durations.grad.cpu().numpy() - g * want.ddur).max() <= g * gate['ddur']
    for i in range(len(outs)):                                                # inputs without a semi-Markov term: untouched
        if names[i][len('NLL_'):] not in keys[1:]:
            assert torch.equal(leaves[i].grad, chain_leaves[i].grad)


def _train_one_step(backend):
    """A small TGGCN and a SemiMarkovCRF (from counts: a -inf diagonal) under DataParallel(world 1, extra_modules=[scrf]) +
    FusedAdam, one step; `backend` None: the HIP kernels, else the test double in place of the two semi-Markov launches."""
    from tests.test_train_options_cpu import _batch, _tiny_model
    from twog_gcn_amd.distributed import DataParallel, FusedAdam
    torch.manual_seed(0)
    model = _tiny_model().to(DEV).train()
    xh, xo, mask, cls, seg = (t.to(DEV) for t in _batch())
    cls = cls.repeat_interleave(2, 1)[:, :cls.shape[1]].contiguous()          # runs of two
    C, D = 13, cls.shape[1]
    scrf = losses.SemiMarkovCRF(C, D)
    with torch.no_grad():
        g = torch.Generator().manual_seed(3)
        scrf.transitions.copy_(torch.randn(C, C, generator=g))
        scrf.transitions.fill_diagonal_(float('-inf'))                       # D covers every run
        scrf.durations.copy_(torch.randn(C, D, generator=g))
    scrf = scrf.to(DEV)
    dp = DataParallel(model, extra_modules=[scrf], count_weighted_loss=True)
    opt = FusedAdam(dp.flat, lr=1e-2)
    crit, names = losses.select_loss('2G-GCN', 'multiple', 'mphoi', dict(misc=dict(crf_loss=dict(add=True, weight=0.8))),
                                     crf={'SAR': scrf})
    assert names[-1] == 'SCRF_SAR'
    dp.zero_grad()
    out = dp.model(xh, xo, mask)
    captured = out[4].detach().clone()
    before = [p.detach().clone() for p in scrf.parameters()]
    K = twog_kernels.get_kernels()
    if backend is not None:
        # the double's two methods stand in for the launches, on host copies; everything else stays on the device
        def fwd(terms, losses_out, stats_out):
            host = [{k: (v.cpu() if torch.is_tensor(v) else v) for k, v in t.items()} for t in terms]
            lo, so = losses_out.cpu(), stats_out.cpu()
            backend.semicrf_nll_fwd(host, lo, so)
            losses_out.copy_(lo)
            stats_out.copy_(so)
            for t, h in zip(terms, host):
                t.update(ed=h['ed'], marks=h['marks'], seq=h['seq'])

        def bwd(terms, stats, dlosses, dins, accumulate, need_params):
            host = [{k: (v.cpu() if torch.is_tensor(v) else v) for k, v in t.items()} for t in terms]
            hd = [None if d is None else d.cpu() for d in dins]
            out = backend.semicrf_nll_bwd(host, stats.cpu(), dlosses.cpu(), hd, accumulate, need_params)
            for d, h in zip(dins, hd):
                if d is not None:
                    d.copy_(h)
            return [None if o is None else tuple(t.to(DEV) for t in o) for o in out]
        K.semicrf_nll_fwd, K.semicrf_nll_bwd = fwd, bwd                       # instance attributes over the methods
    try:
        with dp.loss_scope():
            terms = crit(out, [seg, seg, cls, cls, cls, cls])
        sum(terms).backward()
    finally:
        if backend is not None:
            del K.semicrf_nll_fwd, K.semicrf_nll_bwd
    dp.all_reduce_gradients()
    grads = [p.grad.detach().clone() for p in scrf.parameters()]
    opt.step(dp.grad_scale)
    torch.cuda.synchronize()
    after = [p.detach().clone() for p in scrf.parameters()]
    loss = float(terms[-1].detach())
    dp.close()
    return dict(captured=captured, cls=cls, before=before, grads=grads, after=after, loss=loss, lr=1e-2)


def test_model_and_module_train_one_step_together():
    """The kernels' step against the same step with the test double (the fp32 specification) in place of the two launches, and
    against the fp64 specification on the captured outputs: the three parameter gradients within the gates, `durations` and
    `transitions` moved by the Adam update, the -inf diagonal still -inf with gradient exactly 0."""
    hip = _train_one_step(None)
    fake = _train_one_step(SemiCrfFakeKernels())
    assert torch.equal(hip['captured'], fake['captured'])                     # the same model, the same outputs
    A, dur, pi = (t.cpu().numpy() for t in hip['before'])                     # the order of the module's parameters
    want = R.semicrf_nll(hip['captured'].cpu().numpy(), hip['cls'].cpu().numpy(), A, pi, dur, g=1.0)
    g = 0.8 / want.count                                                      # world 1: the reducer returns the count itself
    gate = GATES['small']
    for run in (hip, fake):
        gA, gdur, gpi = (t.cpu().numpy() for t in run['grads'])
        assert np.abs(gA - g * want.dA).max() <= g * gate['dA'] and np.abs(gpi - g * want.dpi).max() <= g * gate['dpi']
        assert np.abs(gdur - g * want.ddur).max() <= g * gate['ddur']
        assert abs(run['loss'] - 0.8 * want.loss) <= 0.8 * gate['loss'] * max(1.0, np.abs(want.logZ).max()) \
            + 2 * np.spacing(np.float32(0.8 * want.loss))
    gA = hip['grads'][0]
    diag = torch.eye(13, dtype=torch.bool, device=DEV)
    assert not gA[diag].any() and torch.isneginf(hip['after'][0][diag]).all()     # -inf: gradient 0, left where it is
    assert float(gA.abs().max()) > 1e-4 and float(hip['grads'][1].abs().max()) > 1e-4
    lr = hip['lr']
    for b, gr, a in zip(hip['before'], hip['grads'], hip['after']):
        moved = (gr != 0) & torch.isfinite(b)
        assert float((a[moved] - b[moved]).abs().max()) > 0.5 * lr and float((a[moved] - b[moved]).abs().max()) <= 1.001 * lr
        assert torch.equal(a[~moved], b[~moved])


def test_the_modules_decoder_is_the_segmental_specification():
    m = _module(6, 5, 9)
    with torch.no_grad():
        m.transitions.mul_(3.0)
    g = torch.Generator().manual_seed(2)
    logp = torch.log_softmax(torch.randn(3, 6, 21, 2, generator=g), 1)
    labels = m.decoder()(logp.to(DEV))
    want, _ = S.segment_labels(logp.numpy(), m.transitions.detach().cpu().numpy(), m.durations.detach().cpu().numpy(),
                               m.initial.detach().cpu().numpy(), None, 1, 21)
    assert np.array_equal(labels.cpu().numpy(), want)
    assert not np.array_equal(want, logp.numpy().argmax(1))
