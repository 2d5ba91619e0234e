"""CPU: the linear-chain CRF loss off the device --
  * its numpy specification (tests/crf_ref.py at fp64) against brute force over all paths, against torch fp64 autograd of a
    direct logsumexp restatement, and on its identities;
  * the host layer (2g-gcn_amd/losses.py: LinearChainCRF, crf_loss, multi_task_loss(..., crf=), select_loss with misc.crf_loss,
    the loss-type and mask lists, the count reducer) on the test double tests/crf_fake.py;
  * that nothing changes with the option absent; the C ABI; the launch-free entry points of the loaded library."""
import json
import os

import numpy as np
import pytest
import torch

import twog_gcn_amd  # noqa: F401
from twog_gcn_amd import _lib, kernels as twog_kernels, losses, multi_task, postprocess as pp
from tests import crf_ref as R
from tests import viterbi_ref as V
from tests.crf_cases import BY_NAME, CASES, CHUNK, KINDS, make
from tests.crf_fake import CrfFakeKernels
from tests.fake_kernels import FakeKernels
from tests.helpers import ROOT
from tests.test_smooth_loss_cpu import MISC, TODAY, _criterion_case, nll_case


@pytest.fixture()
def double():
    k = CrfFakeKernels()
    twog_kernels._set_backend_for_tests(k)
    yield k
    twog_kernels._set_backend_for_tests(None)


def _random_chain(rng, K, C, scale=1.5):
    return rng.normal(size=(K, C)) * scale, rng.integers(0, C, size=K), rng.normal(size=(C, C)), rng.normal(size=C)


# ------------------------------------------------------------------------------------------------ the specification
@pytest.mark.parametrize('C,K', [(c, k) for c in (1, 2, 3) for k in (1, 2, 3, 5)])
def test_specification_equals_brute_force(C, K):
    rng = np.random.default_rng(100 * C + K)
    x, y, A, pi = _random_chain(rng, K, C)
    ch = R.chain(x, y, A, pi)
    logZ, gamma, xi = R.brute_force(x, A, pi)
    assert abs(ch.logZ - logZ) <= 1e-12 * max(1.0, abs(logZ))
    assert np.abs(ch.gamma - gamma).max() <= 1e-12 and np.abs(ch.xi - xi).max(initial=0.0) <= 1e-12
    gold = pi[y[0]] + x[0, y[0]] + sum(A[y[k - 1], y[k]] + x[k, y[k]] for k in range(1, K))
    assert abs(ch.gold - gold) <= 1e-12 and ch.logZ - ch.gold >= -1e-12


@pytest.mark.parametrize('removed', ['head', 'middle', 'tail', 'all three'])
def test_removed_steps_leave_the_chain(removed):
    """A removed step at the head, in the middle, at the tail: the sequence is its kept steps, linked directly."""
    rng = np.random.default_rng(7)
    C, T = 3, 7
    x = rng.normal(size=(1, C, T, 1))
    y = rng.integers(0, C, size=(1, T, 1))
    A, pi = rng.normal(size=(C, C)), rng.normal(size=C)
    gone = {'head': [0, 1], 'middle': [3], 'tail': [6], 'all three': [0, 2, 3, 6]}[removed]
    y[0, gone, 0] = [-1, C, -7, C + 5][:len(gone)]                       # the ignore value and labels outside [0, C)
    kept = [t for t in range(T) if t not in gone]
    assert R.kept_steps(y[0, :, 0], C).tolist() == kept
    res = R.crf_nll(x, y, A, pi)
    logZ, gamma, xi = R.brute_force(x[0][:, kept, 0].T, A, pi)
    assert res.K[0, 0] == len(kept) and abs(res.logZ[0, 0] - logZ) <= 1e-12
    d = res.dinput[0, :, :, 0] * res.count                               # g = 1 / count
    assert not d[:, gone].any()
    ind = np.zeros((len(kept), C))
    ind[np.arange(len(kept)), y[0, kept, 0]] = 1
    assert np.abs(d[:, kept].T - (gamma - ind)).max() <= 1e-12
    pairs = np.zeros((C, C))
    for a, b in zip(y[0, kept[:-1], 0], y[0, kept[1:], 0]):
        pairs[a, b] += 1
    assert np.abs(res.dA * res.count - (xi.sum(0) - pairs)).max() <= 1e-12
    assert np.abs(res.dpi * res.count - (gamma[0] - ind[0])).max() <= 1e-12


def _torch_restatement(x, y, A, pi, ignore=-1):
    """loss of the definition by torch.logsumexp on the compacted sequences, fp64, differentiable."""
    bs, C, T, E = x.shape
    total, count = 0.0, 0
    for b in range(bs):
        for e in range(E):
            ts = [t for t in range(T) if y[b, t, e] != ignore and 0 <= y[b, t, e] < C]
            if not ts:
                continue
            alpha = pi + x[b, :, ts[0], e]
            gold = pi[y[b, ts[0], e]] + x[b, y[b, ts[0], e], ts[0], e]
            for p, t in zip(ts[:-1], ts[1:]):
                alpha = x[b, :, t, e] + torch.logsumexp(alpha[:, None] + A, 0)
                gold = gold + A[y[b, p, e], y[b, t, e]] + x[b, y[b, t, e], t, e]
            total = total + torch.logsumexp(alpha, 0) - gold
            count += len(ts)
    return total / count, count


@pytest.mark.parametrize('name', ['small-bs3-C6-T20-E3-holes-softmax', 'small-bs3-C6-T20-E3-oob-softmax',
                                  'small-bs3-C6-T20-E9-empty-softmax', 'small-bs3-C6-T20-E3-k1-softmax',
                                  'small-bs3-C5-T2-E3-all-softmax', 'wide-bs3-C6-T33-E3-holes-wide'])
def test_specification_gradients_against_torch_fp64_autograd(name):
    x, y, A, pi = make(BY_NAME[name])
    res = R.crf_nll(x, y, A, pi)
    tx, tA, tpi = (torch.from_numpy(a.astype(np.float64)).requires_grad_(True) for a in (x, A, pi))
    loss, count = _torch_restatement(tx, y, tA, tpi)
    loss.backward()
    assert count == res.count == res.K.sum()
    assert abs(float(loss.detach()) - res.loss) <= 1e-10 * max(1.0, abs(res.loss))
    for got, want in ((res.dinput, tx.grad), (res.dA, tA.grad), (res.dpi, tpi.grad)):
        want = np.zeros_like(got) if want is None else want.numpy()         # K = 1 everywhere: A is never used
        assert np.abs(got - want).max() <= 1e-10


def test_zero_scores_and_normalised_inputs_are_the_per_step_nll():
    rng = np.random.default_rng(3)
    K, C = 9, 4
    z = rng.normal(size=(K, C)) * 2
    x = z - np.log(np.exp(z).sum(1, keepdims=True))
    y = rng.integers(0, C, size=K)
    ch = R.chain(x, y, np.zeros((C, C)), np.zeros(C))
    assert abs(ch.logZ) <= 1e-12                                          # every step sums to one
    assert abs((ch.logZ - ch.gold) + x[np.arange(K), y].sum()) <= 1e-12
    assert np.abs(ch.gamma - np.exp(x)).max() <= 1e-12


@pytest.mark.parametrize('dtype,tol', [(np.float64, 1e-12), (np.float32, 2e-5)])
def test_marginals_sum_to_one(dtype, tol):
    rng = np.random.default_rng(11)
    x, y, A, pi = _random_chain(rng, 12, 5)
    ch = R.chain(x, y, A, pi, dtype)
    assert ch.gamma.dtype == dtype and ch.xi.dtype == dtype
    assert np.abs(ch.gamma.sum(1) - 1).max() <= tol
    assert np.abs(ch.xi.sum(1) - ch.gamma[1:]).max() <= tol                # sum over c' of xi_k[c', c] = gamma_k[c]
    assert np.abs(ch.xi.sum(2) - ch.gamma[:-1]).max() <= tol               # ... and over c: gamma_{k-1}[c']


def test_nothing_kept_is_zero_not_nan():
    x, y, A, pi = make(BY_NAME['small-bs3-C6-T20-E3-all-softmax'])
    for dtype in (np.float64, np.float32):
        res = R.crf_nll(x, np.full_like(y, -1), A, pi, dtype=dtype)
        assert res.loss == 0 and res.count == 0 and not res.K.any()
        assert not res.dinput.any() and not res.dA.any() and not res.dpi.any()


def test_the_case_list_covers_what_it_must():
    Cs = {c['C'] for c in CASES}
    assert {1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64} <= Cs
    assert {1, 2, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1} <= {c['T'] for c in CASES}
    assert {1, 3, 9} <= {c['E'] for c in CASES} and {1, 3} <= {c['bs'] for c in CASES}
    assert {c['labels'] for c in CASES} == {'all', 'tail', 'head', 'holes', 'empty', 'oob', 'k1', 'k2'}
    assert {c['kind'] for c in CASES} == set(KINDS)
    assert any(c['T'] == 4096 and c['C'] == 4 for c in CASES) and any(c['T'] == 512 and c['C'] == 64 for c in CASES)
    x, y, A, pi = make(BY_NAME['wide-bs3-C6-T33-E3-holes-wide'])
    assert x.min() < -75 and A.min() < -15 and A.max() > 3 and pi.min() < -7
    x, y, _, _ = make(BY_NAME['sharp-bs3-C6-T33-E3-holes-sharp'])
    assert set(np.unique(x)) == {np.float32(-15.0), np.float32(-1e-6)}
    _, y, _, _ = make(BY_NAME['small-bs3-C6-T20-E3-oob-softmax'])
    assert (y >= 6).any() and (y < -1).any()
    _, y, _, _ = make(BY_NAME['small-bs3-C6-T20-E9-tail-softmax'])
    assert len({int((y[b, :, 0] >= 0).sum()) for b in range(3)}) == 3      # a different length per clip


def test_recorded_fp32_errors_are_those_of_the_specification():
    """profiles/crf_loss_fp64.json: the gates of the GPU tests are 4 x the fp32-specification errors it records, per case
    kind; the kernels' own errors, once measured, lie beneath them. Recomputed here for the short kinds."""
    rec = json.load(open(os.path.join(ROOT, 'profiles', 'crf_loss_fp64.json')))
    assert rec['factor'] == 4 and rec['cases'] == [c['name'] for c in CASES]
    for kind in ('small', 'sharp'):
        worst = dict.fromkeys(R.QUANTITIES, 0.0)
        for c in CASES:
            if c['kind'] == kind:
                t = make(c)
                err = R.errors(R.crf_nll(*t, dtype=np.float32, g=1.0), R.crf_nll(*t, g=1.0))
                worst = {q: max(worst[q], err[q]) for q in worst}
        for q in R.QUANTITIES:
            assert rec['fp32_spec'][kind][q] == pytest.approx(worst[q], rel=1e-6, abs=1e-300)
    for kind in KINDS:
        for q in R.QUANTITIES:
            assert rec['gate'][kind][q] == 4 * rec['fp32_spec'][kind][q]
            if rec.get('kernel'):
                assert rec['kernel'][kind][q] <= rec['gate'][kind][q]


# ------------------------------------------------------------------------------------------------ the module
def test_module_parameters_and_state_dict():
    crf = losses.LinearChainCRF(5)
    assert [n for n, _ in crf.named_parameters()] == ['transitions', 'initial']
    assert crf.transitions.shape == (5, 5) and crf.initial.shape == (5,) and crf.transitions.dtype == torch.float32
    assert not crf.transitions.any() and not crf.initial.any()
    with torch.no_grad():
        crf.transitions.copy_(torch.arange(25.0).view(5, 5))
        crf.initial.copy_(torch.arange(5.0))
    sd = crf.state_dict()
    assert sorted(sd) == ['initial', 'transitions']
    other = losses.LinearChainCRF(5)
    other.load_state_dict(sd)
    assert torch.equal(other.transitions, crf.transitions) and torch.equal(other.initial, crf.initial)
    with pytest.raises(ValueError):
        losses.LinearChainCRF(0)


def test_from_counts_is_transition_log_probs():
    counts = torch.tensor([[5, 0, 1], [2, 2, 0], [0, 0, 0]])
    crf = losses.LinearChainCRF.from_counts(counts, smoothing=0.5)
    assert torch.equal(crf.transitions.detach(), pp.transition_log_probs(counts, 0.5)) and not crf.initial.any()
    crf = losses.LinearChainCRF.from_counts(counts, initial_counts=[3, 1, 0])
    assert torch.equal(crf.transitions.detach(), pp.transition_log_probs(counts, 1.0))
    want = np.log((np.array([3.0, 1.0, 0.0]) + 1) / 7).astype(np.float32)
    assert np.array_equal(crf.initial.detach().numpy(), want)
    assert crf.transitions.requires_grad and crf.initial.requires_grad
    with pytest.raises(ValueError):
        losses.LinearChainCRF.from_counts(counts, smoothing=0.0)              # -inf scores are out of contract


def test_decoder_decodes_with_the_current_values(double):
    rng = np.random.default_rng(5)
    crf = losses.LinearChainCRF(4)
    with torch.no_grad():
        crf.transitions.copy_(torch.from_numpy(rng.normal(size=(4, 4)).astype(np.float32) * 3))
        crf.initial.copy_(torch.from_numpy(rng.normal(size=4).astype(np.float32)))
    logp = torch.log_softmax(torch.from_numpy(rng.normal(size=(2, 4, 11, 3)).astype(np.float32)), 1)
    dec = crf.decoder()
    assert isinstance(dec, pp.ViterbiDecoder) and not dec.transitions.requires_grad
    want, _ = V.viterbi_labels(logp.numpy(), crf.transitions.detach().numpy(), crf.initial.detach().numpy(), None, 1, 11)
    assert np.array_equal(dec(logp).numpy(), want) and double.calls == ['viterbi_decode']
    assert not np.array_equal(want, logp.numpy().argmax(1))                   # the scores matter in this case
    before = dec.transitions.clone()
    with torch.no_grad():
        crf.transitions.zero_()                                               # detached copies: a later step does not reach it
    assert torch.equal(dec.transitions, before)


# ------------------------------------------------------------------------------------------------ the host layer
def _crf(C, seed):
    g = torch.Generator().manual_seed(seed)
    crf = losses.LinearChainCRF(C)
    with torch.no_grad():
        crf.transitions.copy_(torch.randn(C, C, generator=g))
        crf.initial.copy_(torch.randn(C, generator=g))
    return crf


def _spec32(x, y, crf, g=None):
    return R.crf_nll(x.detach().numpy(), y.numpy(), crf.transitions.detach().numpy(), crf.initial.detach().numpy(), -1,
                     np.float32, g=g)


def test_crf_loss_on_the_double(double):
    xs, ys = nll_case((3, 5, 9, 2), 1, n_terms=1)
    crf = _crf(5, 1)
    x = xs[0].clone().requires_grad_(True)
    v = losses.crf_loss(x, ys[0], crf)
    want = _spec32(xs[0], ys[0], crf)
    assert v.shape == () and float(v.detach()) == float(want.loss)
    assert [c[0] for c in double.calls] == ['multitask_loss_fwd', 'crf_nll_fwd']
    assert double.calls[0][2:] == ((), {'room': 1})
    double.calls.clear()
    (3.0 * v).backward()
    # the carrying NLL term has weight 0: no NLL backward launch, the CRF launch stores into a buffer of its own
    assert double.calls == [('crf_nll_bwd', (True,), (False,), (True,))]
    want3 = _spec32(xs[0], ys[0], crf, g=np.float32(3.0) / np.float32(want.count))
    assert torch.equal(x.grad, torch.from_numpy(want3.dinput))
    assert torch.equal(crf.transitions.grad, torch.from_numpy(want3.dA))
    assert torch.equal(crf.initial.grad, torch.from_numpy(want3.dpi))
    assert float(losses.crf_loss(xs[0], torch.full_like(ys[0], -1), crf).detach()) == 0.0      # nothing kept: 0, not NaN


@pytest.mark.parametrize('ds', ['mphoi', 'cad120'])
@pytest.mark.parametrize('beside', ['alone', 'smoothing', 'class weights'])
def test_multi_task_loss_with_crf_terms_on_the_double(ds, beside, double):
    outs, tgts = _criterion_case(ds)
    C = outs[-1].shape[1]
    keys = ['SAR', 'SAP', 'OAR', 'OAP'][:4 if ds == 'cad120' else 2]
    crfs = {k: _crf(C, i) for i, k in enumerate(keys)}
    misc = dict(MISC, crf_loss=dict(add=True, weight=0.5))
    if beside == 'smoothing':
        misc['smoothing_loss'] = dict(add=True)
    if beside == 'class weights':
        misc['class_weights'] = dict(add=True, subactivity=[1.0 + 0.1 * c for c in range(C)])
    cfg = dict(misc=misc)
    crit, names = losses.select_loss('2G-GCN', 'multiple', ds, cfg, crf=crfs)
    n_main, m = len(TODAY[ds][0]), len(keys)
    ns = m if beside == 'smoothing' else 0
    assert names == TODAY[ds][0] + ['TMSE_' + k for k in keys][:ns] + ['CRF_' + k for k in keys]
    leaves = [o.clone().requires_grad_(True) for o in outs]
    got = crit(leaves, tgts)
    assert len(got) == n_main + ns + m
    fwd = 'weighted_loss_fwd' if beside == 'class weights' else 'multitask_loss_fwd'
    assert [c[0] for c in double.calls] == [fwd] + ['smooth_loss_fwd'] * bool(ns) + ['crf_nll_fwd']
    assert double.calls[0][2:] == ((), {'room': ns + m}) and double.calls[-1] == ('crf_nll_fwd', m)
    base = got[0]._base                                                       # ONE tensor: the loss learner reads it in place
    assert base is not None and base.shape == (n_main + ns + m,) and multi_task._loss_tensor(got) is base
    # the terms before the CRF ones are those of the same call without them
    plain_cfg = dict(misc={k: v for k, v in misc.items() if k != 'crf_loss'})
    plain = losses.select_loss('2G-GCN', 'multiple', ds, plain_cfg)[0]([o.clone() for o in outs], tgts)
    assert all(torch.equal(a.detach(), b) for a, b in zip(got[:n_main + ns], plain))
    weights = crit.keywords['weight']
    for j, k in enumerate(keys):
        i = n_main - m + j
        assert crit.keywords['crf'][j] == (i, 0.5 * weights[i], crfs[k])
        want = _spec32(outs[i], tgts[i], crfs[k])
        assert float(got[n_main + ns + j].detach()) == float(np.float32(0.5 * weights[i]) * want.loss)
    double.calls.clear()
    sum(got).backward()
    bwd = [c[0] for c in double.calls]
    assert bwd == [fwd.replace('fwd', 'bwd')] + ['smooth_loss_bwd'] * bool(ns) + ['crf_nll_bwd']
    # one gradient per input: the CRF launch adds into the buffer the NLL launch wrote
    assert double.calls[-1] == ('crf_nll_bwd', (True,) * m, (True,) * m, (True,) * m)
    plain_leaves = [o.clone().requires_grad_(True) for o in outs]
    sum(losses.select_loss('2G-GCN', 'multiple', ds, plain_cfg)[0](plain_leaves, tgts)).backward()
    for j, k in enumerate(keys):
        i = n_main - m + j
        want = _spec32(outs[i], tgts[i], crfs[k])
        g = np.float32(0.5 * weights[i]) * np.float32(1.0) / np.float32(want.count)
        wg = _spec32(outs[i], tgts[i], crfs[k], g=g)
        assert torch.equal(leaves[i].grad, plain_leaves[i].grad + torch.from_numpy(wg.dinput))
        assert torch.equal(crfs[k].transitions.grad, torch.from_numpy(wg.dA))
        assert torch.equal(crfs[k].initial.grad, torch.from_numpy(wg.dpi))
    for i in range(n_main - m):
        assert torch.equal(leaves[i].grad, plain_leaves[i].grad)


@pytest.mark.parametrize('ds,keys', [('mphoi', ['SAR', 'SAP']), ('mphoi', ['SAP']), ('cad120', ['OAP', 'SAR']),
                                     ('cad120', ['SAR', 'SAP', 'OAR', 'OAP'])])
@pytest.mark.parametrize('pretrain', [False, True])
def test_select_loss_names_types_and_masks(ds, keys, pretrain):
    names, weights, types, mask = TODAY[ds]
    misc = dict(MISC, crf_loss=dict(add=True, weight=0.25), smoothing_loss=dict(add=True))
    misc['segmentation_loss'] = dict(MISC['segmentation_loss'], pretrain=pretrain)
    cfg = dict(misc=misc)
    crfs = {k: losses.LinearChainCRF(6) for k in keys}
    crit, got = losses.select_loss('2G-GCN', 'multiple', ds, cfg, crf=crfs)
    final = [n[len('NLL_'):] for n in names[-(4 if ds == 'cad120' else 2):]]
    order = [k for k in final if k in keys]                                   # term order, not dict order
    assert got == names + ['TMSE_' + k for k in final] + ['CRF_' + k for k in order]
    w = crit.keywords['weight']
    assert [(i, cw) for i, cw, _ in crit.keywords['crf']] == [(names.index('NLL_' + k), 0.25 * w[names.index('NLL_' + k)])
                                                              for k in order]
    if pretrain:                                                              # the stage-1 zeros carry over
        assert all(cw == 0.0 for (i, cw, _), k in zip(crit.keywords['crf'], order) if k.endswith('AR'))
    assert losses.select_loss_types('2G-GCN', ds, cfg, crf=crfs) == types + ['mse'] * len(final) + ['crf'] * len(keys)
    assert losses.select_loss_learning_mask('2G-GCN', ds, cfg, crf=crfs) == mask + [False] * (len(final) + len(keys))
    assert len(losses.select_loss_types('2G-GCN', ds, cfg)) == len(types) + 2 * len(final)     # no dict: every final term
    learner = multi_task.MultiTaskLossLearner(losses.select_loss_types('2G-GCN', ds, cfg, crf=crfs),
                                              losses.select_loss_learning_mask('2G-GCN', ds, cfg, crf=crfs))
    assert learner.get_weights()[-len(keys):] == [None] * len(keys)
    # the default weight of the key is 1
    crit, _ = losses.select_loss('2G-GCN', 'multiple', ds, dict(misc=dict(MISC, crf_loss=dict(add=True))), crf=crfs)
    assert [cw for _, cw, _ in crit.keywords['crf']] == [weights[names.index('NLL_' + k)] for k in order]


def test_every_refusal_comes_before_the_backend(double):
    xs, ys = nll_case((2, 4, 6, 2), 3, n_terms=2)
    crf = _crf(4, 0)
    fns = (losses.nll_loss, losses.budget_loss)
    two = [xs[0], torch.rand(2, 6, 2)], [ys[0], torch.ones(2, 6, 2)]
    for bad in ([(1, 1.0, crf)],                                              # not an NLL term
                [(2, 1.0, crf)],                                              # past the zipped terms
                [(0, 1.0, _crf(5, 0))],                                       # class-count mismatch
                [(0, 1.0, crf), (0, 0.5, _crf(4, 1))],                        # two CRF terms, one gradient buffer
                [(0, 1.0, torch.nn.Linear(4, 4))]):                           # not a LinearChainCRF
        with pytest.raises(ValueError):
            losses.multi_task_loss(*two, fns, crf=bad)
    with pytest.raises(ValueError, match='up to 64 classes and 4096 model steps'):
        losses.crf_loss(torch.zeros(1, 65, 3, 1), torch.zeros(1, 3, 1, dtype=torch.int64), losses.LinearChainCRF(65))
    with pytest.raises(ValueError, match='up to 64 classes and 4096 model steps'):
        losses.crf_loss(torch.zeros(1, 2, 4097, 1), torch.zeros(1, 4097, 1, dtype=torch.int64), losses.LinearChainCRF(2))
    with pytest.raises(ValueError):
        losses.multi_task_loss([xs[0][:, :, :, 0]], [ys[0][:, :, 0]], (losses.nll_loss,), crf=[(0, 1.0, crf)])   # not 4-D
    cfg = dict(misc=dict(MISC, crf_loss=dict(add=True)))
    with pytest.raises(ValueError):
        losses.select_loss('2G-GCN', 'multiple', 'mphoi', cfg)                # add: true without modules
    with pytest.raises(ValueError):
        losses.select_loss('2G-GCN', 'multiple', 'mphoi', cfg, crf={})
    with pytest.raises(ValueError):
        losses.select_loss('2G-GCN', 'multiple', 'mphoi', cfg, crf={'OAR': crf})   # no object terms in this list
    assert double.calls == []
    assert float(losses.crf_loss(torch.zeros(1, 2, 4096, 1), torch.zeros(1, 4096, 1, dtype=torch.int64),
                                 losses.LinearChainCRF(2)).detach()) > 0                        # at the limit: taken


def test_crf_terms_without_backward_work(double):
    xs, ys = nll_case((2, 4, 6, 2), 2)
    fns = (losses.nll_loss,) * 3
    crfs = [_crf(4, i) for i in range(3)]
    for p in crfs[1].parameters():
        p.requires_grad_(False)
    # weight 0 on the CRF term of input 0; input 1 and its module need no gradient; input 2: NLL weight 0, the CRF launch stores
    leaves = [xs[0].clone().requires_grad_(True), xs[1].clone(), xs[2].clone().requires_grad_(True)]
    got = losses.multi_task_loss(leaves, ys, fns, [1.0, 1.0, 0.0], crf=[(0, 0.0, crfs[0]), (1, 0.2, crfs[1]), (2, 0.2, crfs[2])])
    assert float(got[3].detach()) == 0.0 and float(got[4].detach()) != 0.0
    double.calls.clear()
    sum(got).backward()
    assert double.calls == [('multitask_loss_bwd', (True, False, False)),
                            ('crf_nll_bwd', (False, False, True), (False, False, False), (False, False, True))]
    assert crfs[0].transitions.grad is None and crfs[1].transitions.grad is None and crfs[2].transitions.grad is not None
    # nothing to differentiate at all: no backward launch of any kind
    leaves = [x.clone().requires_grad_(True) for x in xs]
    got = losses.multi_task_loss(leaves, ys, fns, [0.0] * 3, crf=[(0, 0.0, crfs[0])])
    double.calls.clear()
    sum(got).backward()
    assert double.calls == [] and all(x.grad is None for x in leaves)
    # the input needs no gradient, the parameters do: no d(input) buffer, and no NLL launch
    got = losses.multi_task_loss([x.clone() for x in xs], ys, fns, [1.0] * 3, crf=[(1, 1.0, crfs[2])])
    double.calls.clear()
    sum(got).backward()
    assert double.calls == [('crf_nll_bwd', (False,), (False,), (True,))]
    # the parameters need none, the input does: the CRF launch adds into the NLL launch's buffer
    x = xs[1].clone().requires_grad_(True)
    got = losses.multi_task_loss([x], ys[1:2], fns[:1], [1.0], crf=[(0, 1.0, crfs[1])])
    double.calls.clear()
    sum(got).backward()
    assert double.calls == [('multitask_loss_bwd', (True,)), ('crf_nll_bwd', (True,), (True,), (False,))]


def _run_reduced(reducer):
    outs, tgts = _criterion_case('mphoi')
    crfs = {k: _crf(outs[-1].shape[1], i) for i, k in enumerate(('SAR', 'SAP'))}
    crit, _ = losses.select_loss('2G-GCN', 'multiple', 'mphoi', dict(misc=dict(MISC, crf_loss=dict(add=True))), crf=crfs)
    leaves = [o.clone().requires_grad_(True) for o in outs]
    if reducer is None:
        got = crit(leaves, tgts)
    else:
        with losses.count_reducer_scope(reducer):
            got = crit(leaves, tgts)
    sum(got[6:]).backward()                                                   # the CRF terms alone
    params = [p.grad for m in crfs.values() for p in m.parameters()]
    return [v.detach().clone() for v in got], [leaves[4].grad, leaves[5].grad] + params


def test_count_reducer_covers_the_crf_terms(double):
    plain_l, plain_g = _run_reduced(None)
    seen = []
    same_l, same_g = _run_reduced(lambda c: (seen.append(c.clone()), c)[1])
    assert len(seen) == 1 and seen[0].shape == (8,)                           # ONE reduction covers all eight counts
    _, tgts = _criterion_case('mphoi')
    assert seen[0][6:].tolist() == [float((t >= 0).sum()) for t in tgts[4:6]]   # the count of a CRF term: its kept steps
    assert all(torch.equal(a, b) for a, b in zip(plain_l, same_l))            # identity reducer: bit-identical
    assert all(torch.equal(a, b) for a, b in zip(plain_g, same_g))
    half_l, half_g = _run_reduced(lambda c: c * 2)                            # twice the count: half the loss and the gradients
    for a, b in zip(plain_l[6:], half_l[6:]):
        assert float(a) != 0 and torch.equal(a * 0.5, b)
    assert all(torch.equal(a * 0.5, b) for a, b in zip(plain_g, half_g))      # (powers of two commute with every rounding)


def test_count_reducer_zero_count_gives_zero_not_nan(double):
    xs, ys = nll_case((2, 4, 6, 2), 6, n_terms=1)
    ys[0][:] = -1
    x, crf = xs[0].clone().requires_grad_(True), _crf(4, 0)
    with losses.count_reducer_scope(lambda c: c * 0):
        got = losses.multi_task_loss([x], ys, (losses.nll_loss,), [1.0], crf=[(0, 0.5, crf)])
    assert torch.isnan(got[0]) and float(got[1].detach()) == 0.0              # NLL: torch's empty mean; CRF: 0
    got[1].backward()
    assert float(x.grad.abs().max()) == 0.0 and float(crf.transitions.grad.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ nothing changes without it
def test_without_crf_the_old_calls_are_made():
    """On the UNCHANGED test doubles: a call without `crf` records exactly the calls it records on the parent commit."""
    from tests.class_weight_fake import ClassWeightFakeKernels

    class Recording(FakeKernels):
        def multitask_loss_fwd(self, *args, **kwargs):
            self.calls.append(('multitask_loss_fwd', len(args), dict(kwargs)))
            return FakeKernels.multitask_loss_fwd(self, *args, **kwargs)

    xs, ys = nll_case((2, 4, 6, 2), 4, n_terms=4)
    outs = [torch.rand(2, 6, 2) * 0.9 + 0.05 for _ in range(2)] + xs
    tgts = [torch.ones(2, 6, 2)] * 2 + ys
    k = Recording()
    twog_kernels._set_backend_for_tests(k)
    try:
        for cfg in (dict(misc=MISC), dict(misc=dict(MISC, crf_loss=dict(add=False, weight=2.0)))):
            crit, names = losses.select_loss('2G-GCN', 'multiple', 'mphoi', cfg)
            assert names == TODAY['mphoi'][0] and sorted(crit.keywords) == ['loss_functions', 'weight']
            assert losses.select_loss_types('2G-GCN', 'mphoi', cfg) == TODAY['mphoi'][2]
            assert losses.select_loss_learning_mask('2G-GCN', 'mphoi', cfg) == TODAY['mphoi'][3]
            leaves = [o.clone().requires_grad_(True) for o in outs]
            sum(crit(leaves, tgts)).backward()
        fns = (losses.budget_loss, losses.binary_cross_entropy_loss) + (losses.nll_loss,) * 4
        sum(losses.multi_task_loss([o.clone().requires_grad_(True) for o in outs], tgts, fns, crf=None)).backward()
        assert k.calls == [('multitask_loss_fwd', 1, {})] * 3
        assert not [m for m in dir(k) if m.startswith('crf_')]
    finally:
        twog_kernels._set_backend_for_tests(None)
    # ... and beside smoothing terms and class weights: the record of the doubles those options came with
    k = ClassWeightFakeKernels()
    twog_kernels._set_backend_for_tests(k)
    try:
        cfg = dict(misc=dict(MISC, smoothing_loss=dict(add=True), class_weights=dict(add=True, subactivity=[1.0, 2.0, 0.5, 1.0])))
        crit, _ = losses.select_loss('2G-GCN', 'multiple', 'mphoi', cfg)
        sum(crit([o.clone().requires_grad_(True) for o in outs], tgts)).backward()
        assert [c[0] for c in k.calls] == ['weighted_loss_fwd', 'smooth_loss_fwd', 'weighted_loss_bwd', 'smooth_loss_bwd']
        assert k.calls[0][2:] == ((), {'room': 2}) and k.calls[3][1:] == ((True, True), (True, True))
        assert not [m for m in dir(k) if m.startswith('crf_')]
    finally:
        twog_kernels._set_backend_for_tests(None)


# ------------------------------------------------------------------------------------------------ the C ABI and the library
def test_abi_symbols_are_declared():
    symbols = _lib.exported_symbols()
    header = open(os.path.join(ROOT, 'include', 'twog_gcn.h')).read()
    for name, n_args in (('twog_crf_limits', 2), ('twog_crf_workspace', 7), ('twog_crf_nll_fwd', 15),
                         ('twog_crf_nll_bwd', 20)):
        assert name in symbols and f'int {name}(' in header and len(_lib.SIGNATURES[name]) == n_args
        decl = header[header.index(f'int {name}('):]
        assert decl[:decl.index(';')].count(',') + 1 == n_args              # the declaration carries as many
    assert f'#define TWOG_CRF_CHUNK {_lib.CRF_CHUNK}\n' in header and _lib.CRF_CHUNK == CHUNK
    assert f'#define TWOG_CRF_SEQ_WORDS {_lib.CRF_SEQ_WORDS}\n' in header
    lib = _lib.load()
    for name in ('twog_crf_limits', 'twog_crf_workspace', 'twog_crf_nll_fwd', 'twog_crf_nll_bwd'):
        assert getattr(lib, name) is not None


def test_the_ctypes_layer_is_launch_free_and_refuses_before_any_launch():
    """HipKernels with the library loaded and no device: limits and workspace touch none, and beyond the limits the entry
    points raise before they touch one."""
    K = twog_kernels.HipKernels()
    assert K.crf_limits() == (R.MAX_CLASSES, R.MAX_STEPS) == K.viterbi_limits()
    bs, C, T, E = 3, 13, 120, 2
    assert K.crf_workspace(bs, C, T, E) == (bs * E * T * C * 4, bs * E * 4 * 4, bs * E * (C + 1) * C * 4)
    assert K.crf_workspace(1, 64, 4096, 1)[0] == 64 * 4096 * 4
    for shape in ((1, 65, 8, 1), (1, 2, 4097, 1)):
        with pytest.raises(ValueError, match='up to 64 classes and 4096 model steps'):
            K.crf_workspace(*shape)
        x = torch.zeros(*shape)
        term = dict(input=x, target=torch.zeros(shape[0], shape[2], shape[3], dtype=torch.int64),
                    transitions=torch.zeros(shape[1], shape[1]), initial=torch.zeros(shape[1]), weight=1.0, ignore=-1)
        with pytest.raises(ValueError, match='up to 64 classes and 4096 model steps'):
            K.crf_nll_fwd([term], torch.zeros(1), torch.zeros(1, 2, dtype=torch.float64))
        assert 'alpha' not in term
