"""CPU: the semi-Markov CRF loss off the device --
  * its numpy specification (tests/semicrf_ref.py at fp64) against brute force over all labelled segmentations, against torch
    fp64 autograd of a plain restatement, against the linear-chain CRF at D = 1, and on its identities;
  * the host layer (2g-gcn_amd/losses.py: SemiMarkovCRF, semi_crf_loss, multi_task_loss(..., crf=) with both module kinds,
    select_loss with misc.crf_loss, the loss-type and mask lists) on the test double tests/semicrf_fake.py;
  * the launch-free entry points of the loaded library."""
import ctypes

import numpy as np
import pytest
import torch

import twog_gcn_amd  # noqa: F401
from twog_gcn_amd import _lib, kernels as twog_kernels, losses, postprocess as pp
from tests import crf_ref
from tests import segdecode_ref as S
from tests import semicrf_ref as R
from tests.semicrf_cases import BY_NAME, CASES, IGNORE, longest_run, make, plan
from tests.semicrf_fake import SemiCrfFakeKernels
from tests.test_smooth_loss_cpu import MISC, TODAY, _criterion_case, nll_case

_SPEC = {}


def spec(name):
    """The fp64 specification of a case with g = 1, computed once and shared."""
    if name not in _SPEC:
        _SPEC[name] = R.semicrf_nll(*make(BY_NAME[name]), g=1.0)
    return _SPEC[name]


@pytest.fixture()
def double():
    k = SemiCrfFakeKernels()
    twog_kernels._set_backend_for_tests(k)
    yield k
    twog_kernels._set_backend_for_tests(None)


def _random_sequence(rng, K, C, D, scale=1.5):
    return (rng.normal(size=(K, C)) * scale, rng.integers(0, C, size=K), rng.normal(size=(C, C)), rng.normal(size=C),
            rng.normal(size=(C, D)))


def _pieces(y, D):
    """The gold cutting rule stated a second time, independently of R.gold_pieces: a piece ends where the label changes, after
    D steps, and at the end. [(start, length, class)]."""
    out, s = [], 0
    for k in range(1, len(y) + 1):
        if k == len(y) or y[k] != y[s] or k - s == D:
            out.append((s, k - s, int(y[s])))
            s = k
    return out


def _gold_counts(y, C, D):
    """(pieces (C, D), joins (C, C), first (C,)) of the gold segmentation."""
    pieces = _pieces(y, D)
    n_dur, n_A, first = np.zeros((C, D)), np.zeros((C, C)), np.zeros(C)
    first[pieces[0][2]] = 1
    for j, (_, l, c) in enumerate(pieces):
        n_dur[c, l - 1] += 1
        if j:
            n_A[pieces[j - 1][2], c] += 1
    return n_dur, n_A, first


def _one(x, y, A, pi, dur, **kw):
    """R.semicrf_nll of one compacted sequence with g = 1."""
    return R.semicrf_nll(x.T[None, :, :, None], np.asarray(y)[None, :, None], A, pi, dur, g=1.0, **kw)


def _check_against_brute_force(K, C, D, seed, tol=1e-10, y=None):
    rng = np.random.default_rng(seed)
    x, y_random, A, pi, dur = _random_sequence(rng, K, C, D)
    y = y_random if y is None else np.asarray(y)
    bf = R.brute_force(x, A, pi, dur)
    res = _one(x, y, A, pi, dur)
    assert abs(res.logZ[0, 0] - bf['logZ']) <= tol
    assert np.abs(R.segment_marginals(x, A, pi, dur) - bf['mu']).max() <= tol
    pieces = _pieces(y, D)
    assert pieces == R.gold_pieces(y, D)
    gold = R.segmentation_score(x, [(s, l) for s, l, _ in pieces], [c for _, _, c in pieces], A, pi, dur)
    assert abs(res.gold[0, 0] - gold) <= tol and res.nll[0, 0] >= -tol
    # the gold segmentation is one of the enumerated ones: its steps are covered exactly once, by its own labels
    assert sum(l for _, l, _ in pieces) == K and all(l <= D for _, l, _ in pieces)
    ind = np.zeros((K, C))
    ind[np.arange(K), y] = 1
    n_dur, n_A, first = _gold_counts(y, C, D)
    assert np.abs(res.dinput[0, :, :, 0].T - (bf['cov'] - ind)).max() <= tol
    assert np.abs(res.ddur - (bf['E_dur'] - n_dur)).max() <= tol
    assert np.abs(res.dA - (bf['E_A'] - n_A)).max() <= tol
    assert np.abs(res.dpi - (bf['E_pi'] - first)).max() <= tol


# ------------------------------------------------------------------------------------------------ the specification
@pytest.mark.parametrize('K,C,D', [(1, 1, 1), (1, 3, 3), (2, 2, 1), (3, 3, 2), (4, 2, 3), (5, 3, 3), (6, 3, 3), (6, 2, 2),
                                   (2, 3, 3), (3, 2, 5)])
def test_specification_equals_brute_force(K, C, D):
    """logZ, the segment marginals and all four gradients, D > K included."""
    _check_against_brute_force(K, C, D, 100 * K + 10 * C + D)


@pytest.mark.parametrize('fault', ['remainder first', 'join dropped'])
def test_a_planted_fault_is_caught(fault, monkeypatch):
    """The comparison above fails when the gold rule is wrong: the remainder of a cut run put first, or the A[c, c] join
    between the pieces of one run left out of the score."""
    K, C, D, seed = 6, 2, 2, 3
    y = [1, 0, 0, 0, 1, 1]                                                    # the run of three is cut at D = 2
    _check_against_brute_force(K, C, D, seed, y=y)
    if fault == 'remainder first':
        right = R.gold_pieces

        def wrong(y, D):
            out = []
            for s, l, c in right(y, 10 ** 6):                                  # whole runs
                r = l % D
                cuts = ([r] if r else []) + [D] * (l // D)
                for n in cuts:
                    out.append((s, n, c))
                    s += n
            return out
        assert wrong(y, D) != right(y, D)
        monkeypatch.setattr(R, 'gold_pieces', wrong)
    else:
        right = R.gold_score

        def wrong(x, y, A, pi, dur, dt):
            same = sum(1 for j, (s, l, c) in enumerate(R.gold_pieces(y, dur.shape[1])) if j and y[s - 1] == c)
            assert same > 0
            return right(x, y, A, pi, dur, dt) - sum(A[c, c] for j, (s, l, c) in enumerate(R.gold_pieces(y, dur.shape[1]))
                                                     if j and y[s - 1] == c)
        monkeypatch.setattr(R, 'gold_score', wrong)
    with pytest.raises(AssertionError):
        _check_against_brute_force(K, C, D, seed, y=y)


def test_the_gold_cutting_rule_by_hand():
    assert R.gold_pieces([0, 0, 0, 0, 0, 1, 1], 2) == [(0, 2, 0), (2, 2, 0), (4, 1, 0), (5, 2, 1)]      # 2 D + 1, then D
    assert R.gold_pieces([2, 2, 2, 2], 2) == [(0, 2, 2), (2, 2, 2)]                                    # exactly 2 D
    assert R.gold_pieces([1, 1, 1], 2) == [(0, 2, 1), (2, 1, 1)]                                       # D + 1
    assert R.gold_pieces([1, 1, 1], 3) == [(0, 3, 1)] and R.gold_pieces([1, 1, 1], 7) == [(0, 3, 1)]
    assert R.gold_pieces([0, 1, 0], 1) == [(0, 1, 0), (1, 1, 1), (2, 1, 0)]
    # the score of [1, 1, 1 | 0] at D = 2, term by term
    x = np.arange(8.0).reshape(4, 2) / 10
    A, pi, dur = np.array([[0.5, -1.0], [2.0, 0.25]]), np.array([3.0, -2.0]), np.array([[0.1, 0.2], [0.3, 0.4]])
    want = pi[1] + (dur[1, 1] + x[0, 1] + x[1, 1]) + A[1, 1] + (dur[1, 0] + x[2, 1]) + A[1, 0] + (dur[0, 0] + x[3, 0])
    assert abs(R.chain(x, np.array([1, 1, 1, 0]), A, pi, dur).gold - want) <= 1e-14


def _torch_restatement(x, y, A, pi, dur, ignore=IGNORE):
    """The loss of the definition by torch.logsumexp on the compacted sequences, fp64, differentiable."""
    bs, C, T, E = x.shape
    D = dur.shape[1]
    total, count = 0.0, 0
    for b in range(bs):
        for e in range(E):
            ts = [t for t in range(T) if y[b, t, e] != ignore and 0 <= y[b, t, e] < C]
            if not ts:
                continue
            xs = x[b][:, ts, e].T
            K = len(ts)
            d = []
            for k in range(K):
                terms = []
                for l in range(1, min(D, k + 1) + 1):
                    s = k - l + 1
                    start = pi if s == 0 else torch.logsumexp(d[s - 1][:, None] + A, 0)
                    terms.append(start + dur[:, l - 1] + xs[s:k + 1].sum(0))
                d.append(torch.logsumexp(torch.stack(terms), 0))
            pieces = _pieces([int(y[b, t, e]) for t in ts], D)
            gold = pi[pieces[0][2]]
            for j, (s, l, c) in enumerate(pieces):
                gold = gold + dur[c, l - 1] + xs[s:s + l, c].sum()
                if j:
                    gold = gold + A[pieces[j - 1][2], c]
            total = total + torch.logsumexp(d[-1], 0) - gold
            count += K
    return total / count


@pytest.mark.parametrize('name', ['small-bs2-C4-T14-E2-D4-run2D1-softmax', 'small-bs3-C6-T20-E3-D6-holes-softmax'])
def test_specification_equals_torch_autograd(name):
    x, y, A, pi, dur = make(BY_NAME[name])
    tx, tA, tpi, tdur = (torch.from_numpy(a.astype(np.float64)).requires_grad_(True) for a in (x, A, pi, dur))
    loss = _torch_restatement(tx, y, tA, tpi, tdur)
    loss.backward()
    res = R.semicrf_nll(x, y, A, pi, dur)
    assert abs(float(loss.detach()) - float(res.loss)) <= 1e-12 * max(1.0, abs(float(loss.detach())))
    for got, want in ((res.dinput, tx.grad), (res.dA, tA.grad), (res.dpi, tpi.grad), (res.ddur, tdur.grad)):
        assert np.abs(got - want.numpy()).max() <= 1e-12


@pytest.mark.parametrize('labels', ['all', 'holes'])
def test_at_one_step_per_segment_it_is_the_linear_chain_crf(labels):
    """D = 1 and dur = 0: every segment is one step, so d_k = e_k + x_k is the CRF's alpha_k, the gold pieces are the steps and
    their joins the CRF's transitions: nll, dinput, dA and dpi are the CRF's. And since sum_s mu(s, 1, c) is the sum of the
    coverage over the steps and the gold pieces of class c are the steps labelled c, ddur[c, 0] = sum_{b, t, e} dinput[b, c, t, e]
    (both carry the same factor g)."""
    rng = np.random.default_rng(11)
    bs, C, T, E = 2, 4, 9, 3
    x = rng.normal(size=(bs, C, T, E))
    y = rng.integers(0, C, size=(bs, T, E))
    if labels == 'holes':
        y = np.where(rng.random(size=y.shape) < 0.3, IGNORE, y)
    A, pi = rng.normal(size=(C, C)), rng.normal(size=C)
    semi, chain = R.semicrf_nll(x, y, A, pi, np.zeros((C, 1))), crf_ref.crf_nll(x, y, A, pi)
    assert np.array_equal(semi.K, chain.K) and semi.count == chain.count
    for q in ('nll', 'logZ', 'gold', 'dinput', 'dA', 'dpi'):
        assert np.abs(getattr(semi, q) - getattr(chain, q)).max() <= 1e-12, q
    assert abs(semi.loss - chain.loss) <= 1e-12
    assert np.abs(semi.ddur[:, 0] - semi.dinput.sum((0, 2, 3))).max() <= 1e-12


@pytest.mark.parametrize('seed,K,C,D', [(0, 7, 3, 3), (1, 9, 2, 4), (2, 5, 4, 8), (3, 12, 3, 1)])
def test_the_coverage_recurrence_is_the_sum_of_the_marginals(seed, K, C, D):
    rng = np.random.default_rng(seed)
    x, y, A, pi, dur = _random_sequence(rng, K, C, D)
    if seed == 1:
        np.fill_diagonal(A, -np.inf)
        dur[0, 0] = -np.inf
    mu = R.segment_marginals(x, A, pi, dur)
    cov = np.zeros((K, C))
    for s in range(K):
        for l in range(1, D + 1):
            cov[s:s + l] += mu[s, l - 1]
    ch = R.chain(x, y, A, pi, dur)
    assert np.abs(ch.cov - cov).max() <= 1e-12
    assert np.abs(cov.sum(1) - 1.0).max() <= 1e-12                           # every step is covered by exactly one segment
    assert np.abs(ch.sum_dur - mu.sum(0).T).max() <= 1e-12


@pytest.mark.parametrize('name', [c['name'] for c in CASES])
def test_gold_is_below_the_best_segmentation_is_below_logZ(name):
    """gold <= the segmental decode's score <= logZ on every case (all are in contract: the gold score is finite). The decode
    is fp32, so it is given the slack of its own rounding: 2^-20 of the magnitude per step."""
    case = BY_NAME[name]
    x, y, A, pi, dur = make(case)
    res = spec(name)
    assert np.isfinite(res.gold).all() and np.isfinite(res.logZ).all() and (res.nll >= -1e-9).all()
    for b in range(case['bs']):
        for e in range(case['E']):
            ts = R.kept_steps(y[b, :, e], case['C'])
            if ts.size == 0:
                assert res.nll[b, e] == 0 and res.K[b, e] == 0
                continue
            _, score = S.decode_sequence_fast(x[b][:, ts, e].T, A, dur, pi)
            slack = 2.0 ** -20 * max(1.0, abs(res.logZ[b, e])) * ts.size ** 0.5
            assert res.gold[b, e] <= score + slack and score <= res.logZ[b, e] + slack, (b, e)


def _best_score(x, A, pi, dur):
    """The best segmentation's score in fp64: the recurrences of the loss with max in place of logsumexp."""
    K, C = x.shape
    D = dur.shape[1]
    d = np.empty((K, C))
    for k in range(K):
        cands = []
        for l in range(1, min(D, k + 1) + 1):
            s = k - l + 1
            start = pi if s == 0 else (d[s - 1][:, None] + A).max(0)
            cands.append(start + dur[:, l - 1] + x[s:k + 1].sum(0))
        d[k] = np.max(cands, axis=0)
    return d[K - 1].max()


def test_logZ_approaches_the_best_score_as_the_emissions_sharpen():
    """logZ - max -> 0 as the emissions are scaled up: the best frame labelling takes all the mass, and under a -inf diagonal
    with D >= K a labelling has one segmentation only (with a finite diagonal the other cuts of the same labelling keep a
    share that does not depend on the emissions). The fp32 segmental decode finds that score."""
    rng = np.random.default_rng(4)
    x, y, A, pi, dur = _random_sequence(rng, 7, 3, 7)
    np.fill_diagonal(A, -np.inf)
    gaps = []
    for scale in (1.0, 10.0, 100.0, 1000.0):
        best = _best_score(scale * x, A, dur=dur, pi=pi)
        gaps.append(R.chain(scale * x, y, A, pi, dur).logZ - best)
        _, score = S.decode_sequence(np.float32(scale * x), A, dur, pi)
        assert abs(float(score) - best) <= 2.0 ** -20 * max(1.0, abs(best))
    assert gaps[0] > gaps[1] > gaps[2] >= gaps[3] >= 0 and gaps[0] > 0.1 and gaps[3] <= 1e-9


@pytest.mark.parametrize('name', [c['name'] for c in CASES if c['values'] in ('infdiag', 'mindur')])
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_minus_infinity_gets_exactly_zero_gradient(name, dtype):
    case = BY_NAME[name]
    x, y, A, pi, dur = make(case)
    assert np.isneginf(A).any() or np.isneginf(dur).any()
    assert longest_run(y, case['C']) <= case['D']
    res = R.semicrf_nll(x, y, A, pi, dur, dtype=dtype, g=1.0)
    for q in ('nll', 'logZ', 'gold', 'dinput', 'dA', 'dpi', 'ddur'):
        assert np.isfinite(getattr(res, q)).all(), q
    assert not res.dA[np.isneginf(A)].any() and not res.ddur[np.isneginf(dur)].any() and not res.dpi[np.isneginf(pi)].any()
    assert np.abs(res.dA[~np.isneginf(A)]).max() > 0 and (res.nll[res.K > 0] > 0).all()


def test_an_all_minus_infinity_logsumexp_is_minus_infinity():
    """A class whose every way in is forbidden: its e, d and be are -inf, nothing is NaN, its marginals are 0."""
    rng = np.random.default_rng(8)
    x, y, A, pi, dur = _random_sequence(rng, 6, 3, 2)
    A[:, 2], pi[2] = -np.inf, -np.inf
    y = np.where(y == 2, 0, y)
    for dtype in (np.float64, np.float32):
        ch = R.chain(x, y, A, pi, dur, dtype)
        assert np.isneginf(ch.e[:, 2]).all() and np.isneginf(ch.d[:, 2]).all()
        assert not np.isnan(np.concatenate([a.ravel() for a in (ch.e, ch.d, ch.bd, ch.be, ch.cov, ch.sum_dur, ch.sum_A)])).any()
        assert not ch.cov[:, 2].any() and not ch.sum_dur[2].any() and np.isfinite(ch.logZ)


def test_the_case_list_claims_what_the_issue_lists():
    claims = ' | '.join(c['claim'] for c in CASES)
    for C in (8, 9, 16, 17, 32, 33, 64):
        assert f'C = {C}' in claims
    for K in (1, 15, 16, 17, 33):
        assert f'K = {K}' in claims
    for D in (1, 2, 16, 17, 20, 23, 128):
        assert f'D = {D} at K = 20' in claims
    assert {c['E'] for c in CASES} >= {1, 3, 9}
    for labels in ('all', 'head', 'tail', 'holes', 'absent', 'none'):
        assert f'removed steps: {labels}' in claims
    # the long gold runs are what they claim
    for labels, n in (('runD1', 5), ('run2D', 8), ('run2D1', 9)):
        case = next(c for c in CASES if c['labels'] == labels)
        assert longest_run(make(case)[1], case['C']) == n and case['D'] == 4
    assert any(c['T'] == 4096 and c['D'] == 128 for c in CASES)
    # the two plan outcomes, as the loaded library reports them
    full = next(c for c in CASES if c['claim'].startswith('plan: every wave'))
    lds = next(c for c in CASES if c['claim'].startswith('plan: waves given up'))
    p = plan(full['bs'], full['C'], full['T'], full['E'], full['D'])
    assert p['fwd_waves'] == p['bwd_waves'] == 8 and p['fwd_groups'] == p['bwd_groups'] == 2
    p = plan(lds['bs'], lds['C'], lds['T'], lds['E'], lds['D'])
    assert p['fwd_waves'] < 8 and p['bwd_waves'] < 4 and p['fwd_groups'] * p['fwd_waves'] >= lds['E']


# ------------------------------------------------------------------------------------------------ the loaded library
def test_plan_and_limits_of_the_loaded_library():
    lib = _lib.load()
    vals = [ctypes.c_int(0) for _ in range(3)]
    assert lib.twog_semicrf_limits(*[ctypes.byref(v) for v in vals]) == 0
    assert [v.value for v in vals] == [R.MAX_CLASSES, R.MAX_STEPS, R.MAX_DURATION]
    p = plan(3, 6, 20, 9, 6)
    assert p['class_template'] == 8 and p['ed_bytes'] == 3 * 9 * 20 * 6 * 8 and p['marks_bytes'] == 3 * 9 * 20 * 4
    assert p['seq_bytes'] == 3 * 9 * 16 and p['partial_bytes'] == 3 * 9 * 6 * (6 + 1 + 6) * 4
    assert plan(1, 6, 4, 1, 128)['partial_bytes'] == 6 * (6 + 1 + 4) * 4            # min(D, T) duration rows
    assert [plan(1, C, 8, 1, 4)['class_template'] for C in (8, 9, 16, 17, 32, 33, 64)] == [8, 16, 16, 32, 32, 64, 64]
    # the worst case the limits admit: one wave per workgroup in both directions
    p = plan(1, 64, 4096, 8, 128)
    assert (p['fwd_waves'], p['fwd_groups'], p['bwd_waves'], p['bwd_groups']) == (1, 8, 1, 8)
    out, nbytes = (ctypes.c_int32 * 5)(), (ctypes.c_size_t * 4)()
    for args, rc in (((1, 4, 8, 1, 0), -1), ((1, 0, 8, 1, 4), -1), ((1, 4, 0, 1, 4), -1), ((-1, 4, 8, 1, 4), -1),
                     ((1, 65, 8, 1, 4), -2), ((1, 4, 4097, 1, 4), -2), ((1, 4, 8, 1, 129), -2), ((65536, 4, 8, 1, 4), -2),
                     ((1, 4, 8, 1, 128), 0)):
        assert lib.twog_semicrf_plan(*args, out, nbytes) == rc, args
    with pytest.raises(ValueError, match='durations up to 128'):
        plan(1, 4, 8, 1, 129)


# ------------------------------------------------------------------------------------------------ the module
def _scrf(C, D, seed):
    g = torch.Generator().manual_seed(seed)
    m = losses.SemiMarkovCRF(C, D)
    with torch.no_grad():
        m.transitions.copy_(torch.randn(C, C, generator=g))
        m.durations.copy_(torch.randn(C, D, generator=g))
        m.initial.copy_(torch.randn(C, generator=g))
    return m


def _crf(C, seed):
    g = torch.Generator().manual_seed(seed)
    m = losses.LinearChainCRF(C)
    with torch.no_grad():
        m.transitions.copy_(torch.randn(C, C, generator=g))
        m.initial.copy_(torch.randn(C, generator=g))
    return m


def test_module_parameters_state_dict_and_repr():
    m = losses.SemiMarkovCRF(5, 7)
    assert [(n, tuple(p.shape)) for n, p in m.named_parameters()] == [('transitions', (5, 5)), ('durations', (5, 7)),
                                                                      ('initial', (5,))]
    assert sorted(m.state_dict()) == ['durations', 'initial', 'transitions']
    assert not any(p.any() for p in m.parameters()) and all(p.dtype == torch.float32 for p in m.parameters())
    assert 'num_classes=5' in repr(m) and 'max_duration=7' in repr(m)
    other = _scrf(5, 7, 0)
    m.load_state_dict(other.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(m.parameters(), other.parameters()))
    for bad in ((0, 3), (3, 0)):
        with pytest.raises(ValueError):
            losses.SemiMarkovCRF(*bad)
    assert 'weight decay' in losses.SemiMarkovCRF.__doc__ and 'NaN' in losses.SemiMarkovCRF.__doc__


def test_from_counts_and_its_decoder_are_the_segmental_decoders(double):
    rng = np.random.default_rng(6)
    C, D = 4, 6
    labels = np.repeat(rng.integers(0, C, size=(3, 12, 2)), 3, axis=1)          # runs of 3 and more
    tc = torch.zeros(C, C, dtype=torch.int64)                                   # frame-level transition counts, by hand
    for b in range(3):
        for e in range(2):
            for a, z in zip(labels[b, :-1, e], labels[b, 1:, e]):
                tc[a, z] += 1
    dc = torch.from_numpy(S.duration_counts(labels, C, D))
    for kw in (dict(), dict(smoothing=0.0), dict(smoothing=0.5, scheme='poisson', self_transition=-2.0)):
        m = losses.SemiMarkovCRF.from_counts(tc, dc, initial_counts=[3, 1, 0, 2], **kw)
        s = kw.get('smoothing', 1.0)
        A = pp.segment_transition_log_probs(tc, s, kw.get('self_transition'))
        dur = pp.duration_log_probs(dc, s, kw.get('scheme', 'empirical'))
        assert torch.equal(m.transitions.detach(), A) and torch.equal(m.durations.detach(), dur)
        assert (m.num_classes, m.max_duration) == (C, D) and all(p.requires_grad for p in m.parameters())
        if 'self_transition' not in kw:
            assert torch.isneginf(m.transitions.detach().diagonal()).all()      # the default: -inf, in contract
        with np.errstate(divide='ignore'):
            want_pi = np.log((np.array([3.0, 1.0, 0.0, 2.0]) + s) / (6 + 4 * s)).astype(np.float32)
        assert np.array_equal(m.initial.detach().numpy(), want_pi)
        logp = torch.log_softmax(torch.from_numpy(rng.normal(size=(2, C, 15, 2)).astype(np.float32)), 1)
        dec, ref = m.decoder(), pp.SegmentalDecoder(A, dur, torch.from_numpy(want_pi))
        assert isinstance(dec, pp.SegmentalDecoder) and not dec.transitions.requires_grad
        assert torch.equal(dec(logp), ref(logp)) and torch.equal(dec.last_score, ref.last_score)
    before = dec.durations.clone()
    with torch.no_grad():
        m.durations.zero_()                                                     # detached copies
    assert torch.equal(dec.durations, before)
    with pytest.raises(ValueError):
        losses.SemiMarkovCRF.from_counts(tc, torch.zeros(C + 1, D))
    with pytest.raises(ValueError):
        losses.SemiMarkovCRF.from_counts(tc, dc, initial_counts=[1, 2])


# ------------------------------------------------------------------------------------------------ the host layer
def _spec32(x, y, m, g=None):
    return R.semicrf_nll(x.detach().numpy(), y.numpy(), m.transitions.detach().numpy(), m.initial.detach().numpy(),
                         m.durations.detach().numpy(), -1, np.float32, g=g)


def _crf32(x, y, m, g=None):
    return crf_ref.crf_nll(x.detach().numpy(), y.numpy(), m.transitions.detach().numpy(), m.initial.detach().numpy(), -1,
                           np.float32, g=g)


def test_semi_crf_loss_on_the_double(double):
    xs, ys = nll_case((3, 5, 9, 2), 1, n_terms=1)
    m = _scrf(5, 3, 1)
    x = xs[0].clone().requires_grad_(True)
    v = losses.semi_crf_loss(x, ys[0], m)
    want = _spec32(xs[0], ys[0], m)
    assert v.shape == () and float(v.detach()) == float(want.loss)
    assert [c[0] for c in double.calls] == ['multitask_loss_fwd', 'semicrf_nll_fwd']
    assert double.calls[0][2:] == ((), {'room': 1})
    double.calls.clear()
    (3.0 * v).backward()
    # the carrying NLL term has weight 0: no NLL backward launch, the launch stores into a buffer of its own
    assert double.calls == [('semicrf_nll_bwd', (True,), (False,), (True,))]
    want3 = _spec32(xs[0], ys[0], m, g=np.float32(3.0) / np.float32(want.count))
    assert torch.equal(x.grad, torch.from_numpy(want3.dinput))
    assert torch.equal(m.transitions.grad, torch.from_numpy(want3.dA))
    assert torch.equal(m.initial.grad, torch.from_numpy(want3.dpi))
    assert torch.equal(m.durations.grad, torch.from_numpy(want3.ddur))
    assert float(losses.semi_crf_loss(xs[0], torch.full_like(ys[0], -1), m).detach()) == 0.0   # nothing kept: 0, not NaN


def test_both_module_kinds_in_one_call(double):
    """The linear-chain terms come first, then the semi-Markov ones, each in list order, whatever the order of the list; each
    module receives its own gradients, and each input one gradient."""
    xs, ys = nll_case((2, 4, 7, 2), 2, n_terms=3)
    fns, w = (losses.nll_loss,) * 3, [1.0, 0.5, 0.0]
    semi_a, chain, semi_b = _scrf(4, 3, 0), _crf(4, 1), _scrf(4, 9, 2)
    leaves = [x.clone().requires_grad_(True) for x in xs]
    got = losses.multi_task_loss(leaves, ys, fns, w, crf=[(2, 0.3, semi_a), (0, 0.7, chain), (1, 0.2, semi_b)])
    assert len(got) == 6
    assert [c[0] for c in double.calls] == ['multitask_loss_fwd', 'crf_nll_fwd', 'semicrf_nll_fwd']
    assert double.calls[0][2:] == ((), {'room': 3}) and double.calls[1:] == [('crf_nll_fwd', 1), ('semicrf_nll_fwd', 2)]
    plain = losses.multi_task_loss([x.clone() for x in xs], ys, fns, w)
    assert all(torch.equal(a.detach(), b) for a, b in zip(got[:3], plain))
    assert float(got[3].detach()) == float(np.float32(0.7) * _crf32(xs[0], ys[0], chain).loss)
    assert float(got[4].detach()) == float(np.float32(0.3) * _spec32(xs[2], ys[2], semi_a).loss)
    assert float(got[5].detach()) == float(np.float32(0.2) * _spec32(xs[1], ys[1], semi_b).loss)
    double.calls.clear()
    sum(got).backward()
    # input 2 has NLL weight 0: its semi-Markov launch stores, the others add to what the NLL launch wrote
    assert double.calls == [('multitask_loss_bwd', (True, True, False)), ('crf_nll_bwd', (True,), (True,), (True,)),
                            ('semicrf_nll_bwd', (True, True), (False, True), (True, True))]
    plain_leaves = [x.clone().requires_grad_(True) for x in xs]
    sum(losses.multi_task_loss(plain_leaves, ys, fns, w)).backward()
    for i, wt, m in ((2, 0.3, semi_a), (1, 0.2, semi_b)):
        g = np.float32(wt) * np.float32(1.0) / np.float32(_spec32(xs[i], ys[i], m).count)
        wg = _spec32(xs[i], ys[i], m, g=g)
        base = plain_leaves[i].grad if plain_leaves[i].grad is not None else 0.0
        assert torch.equal(leaves[i].grad, base + torch.from_numpy(wg.dinput))
        assert torch.equal(m.transitions.grad, torch.from_numpy(wg.dA)) and torch.equal(m.initial.grad, torch.from_numpy(wg.dpi))
        assert torch.equal(m.durations.grad, torch.from_numpy(wg.ddur))
    g = np.float32(0.7) * np.float32(1.0) / np.float32(_crf32(xs[0], ys[0], chain).count)
    assert torch.equal(chain.transitions.grad, torch.from_numpy(_crf32(xs[0], ys[0], chain, g=g).dA))


@pytest.mark.parametrize('ds', ['mphoi', 'cad120'])
@pytest.mark.parametrize('kinds', ['semi', 'mixed'])
def test_select_loss_with_semi_markov_modules_on_the_double(ds, kinds, double):
    outs, tgts = _criterion_case(ds)
    C = outs[-1].shape[1]
    keys = ['SAR', 'SAP', 'OAR', 'OAP'][:4 if ds == 'cad120' else 2]
    is_semi = {k: kinds == 'semi' or j % 2 == 0 for j, k in enumerate(keys)}
    mods = {k: _scrf(C, 4, j) if is_semi[k] else _crf(C, j) for j, k in enumerate(keys)}
    cfg = dict(misc=dict(MISC, crf_loss=dict(add=True, weight=0.5), smoothing_loss=dict(add=True)))
    crit, names = losses.select_loss('2G-GCN', 'multiple', ds, cfg, crf=mods)
    names0, _, types0, mask0 = TODAY[ds]
    order = [k for k in keys if not is_semi[k]] + [k for k in keys if is_semi[k]]   # the term order
    tail = ['CRF_' + k for k in keys if not is_semi[k]] + ['SCRF_' + k for k in keys if is_semi[k]]
    assert names == names0 + ['TMSE_' + k for k in keys] + tail
    assert losses.select_loss_types('2G-GCN', ds, cfg, crf=mods) == \
        types0 + ['mse'] * len(keys) + ['crf'] * sum(not s for s in is_semi.values()) + ['scrf'] * sum(is_semi.values())
    assert losses.select_loss_learning_mask('2G-GCN', ds, cfg, crf=mods) == mask0 + [False] * (2 * len(keys))
    weights = crit.keywords['weight']
    assert [(i, cw) for i, cw, _ in crit.keywords['crf']] == [(names.index('NLL_' + k), 0.5 * weights[names.index('NLL_' + k)])
                                                              for k in keys]
    leaves = [o.clone().requires_grad_(True) for o in outs]
    got = crit(leaves, tgts)
    n = len(names0) + len(keys)
    assert len(got) == len(names)
    assert [c[0] for c in double.calls] == ['multitask_loss_fwd', 'smooth_loss_fwd'] + ['crf_nll_fwd'] * (kinds == 'mixed') + \
        ['semicrf_nll_fwd']
    for j, k in enumerate(order):
        i = names.index('NLL_' + k)
        ref = _spec32(outs[i], tgts[i], mods[k]) if is_semi[k] else _crf32(outs[i], tgts[i], mods[k])
        assert float(got[n + j].detach()) == float(np.float32(0.5 * weights[i]) * ref.loss), k
    double.calls.clear()
    sum(got).backward()
    assert [c[0] for c in double.calls] == ['multitask_loss_bwd', 'smooth_loss_bwd'] + ['crf_nll_bwd'] * (kinds == 'mixed') + \
        ['semicrf_nll_bwd']
    assert all(p.grad is not None for m in mods.values() for p in m.parameters())
    # with LinearChainCRF modules only, the call is the one it was: the same launches, the same values
    chains = {k: _crf(C, j) for j, k in enumerate(keys)}
    double.calls.clear()
    crit_c, names_c = losses.select_loss('2G-GCN', 'multiple', ds, cfg, crf=chains)
    got_c = crit_c([o.clone() for o in outs], tgts)
    assert names_c == names0 + ['TMSE_' + k for k in keys] + ['CRF_' + k for k in keys]
    assert [c[0] for c in double.calls] == ['multitask_loss_fwd', 'smooth_loss_fwd', 'crf_nll_fwd']
    assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(got[:n], got_c[:n]))


def test_every_refusal_comes_before_the_backend(double):
    xs, ys = nll_case((2, 4, 6, 2), 3, n_terms=2)
    m = _scrf(4, 3, 0)
    fns = (losses.nll_loss, losses.budget_loss)
    two = [xs[0], torch.rand(2, 6, 2)], [ys[0], torch.ones(2, 6, 2)]
    for bad in ([(1, 1.0, m)],                                                # not an NLL term
                [(2, 1.0, m)],                                                # past the zipped terms
                [(0, 1.0, _scrf(5, 3, 0))],                                   # class-count mismatch
                [(0, 1.0, m), (0, 0.5, _scrf(4, 2, 1))],                      # two chain terms, one gradient buffer
                [(0, 1.0, m), (0, 0.5, _crf(4, 1))],                          # ... of either kind
                [(0, 1.0, torch.nn.Linear(4, 4))]):                           # not a CRF module
        with pytest.raises(ValueError):
            losses.multi_task_loss(*two, fns, crf=bad)
    zeros = lambda C, T: (torch.zeros(1, C, T, 1), torch.zeros(1, T, 1, dtype=torch.int64))
    with pytest.raises(ValueError, match='up to 64 classes and 4096 model steps'):
        losses.semi_crf_loss(*zeros(65, 3), losses.SemiMarkovCRF(65, 2))
    with pytest.raises(ValueError, match='up to 64 classes and 4096 model steps'):
        losses.semi_crf_loss(*zeros(2, 4097), losses.SemiMarkovCRF(2, 2))
    with pytest.raises(ValueError, match='durations up to 128'):
        losses.semi_crf_loss(*zeros(2, 5), losses.SemiMarkovCRF(2, 129))
    with pytest.raises(ValueError):
        losses.multi_task_loss([xs[0][:, :, :, 0]], [ys[0][:, :, 0]], (losses.nll_loss,), crf=[(0, 1.0, m)])   # not 4-D
    cfg = dict(misc=dict(MISC, crf_loss=dict(add=True)))
    with pytest.raises(ValueError):
        losses.select_loss('2G-GCN', 'multiple', 'mphoi', cfg, crf={'OAR': m})     # no object terms in this list
    assert double.calls == []
    assert float(losses.semi_crf_loss(*zeros(2, 40), losses.SemiMarkovCRF(2, 128)).detach()) > 0   # at the limit: taken


def test_terms_without_backward_work(double):
    xs, ys = nll_case((2, 4, 6, 2), 2)
    fns = (losses.nll_loss,) * 3
    mods = [_scrf(4, 3, i) for i in range(3)]
    for p in mods[1].parameters():
        p.requires_grad_(False)
    leaves = [xs[0].clone().requires_grad_(True), xs[1].clone(), xs[2].clone().requires_grad_(True)]
    got = losses.multi_task_loss(leaves, ys, fns, [1.0, 1.0, 0.0], crf=[(0, 0.0, mods[0]), (1, 0.2, mods[1]), (2, 0.2, mods[2])])
    assert float(got[3].detach()) == 0.0 and float(got[4].detach()) != 0.0
    double.calls.clear()
    sum(got).backward()
    assert double.calls == [('multitask_loss_bwd', (True, False, False)),
                            ('semicrf_nll_bwd', (False, False, True), (False, False, False), (False, False, True))]
    assert mods[0].durations.grad is None and mods[1].durations.grad is None and mods[2].durations.grad is not None
