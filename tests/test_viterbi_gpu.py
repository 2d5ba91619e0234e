"""GPU: twog_viterbi_decode and twog_transition_counts against the numpy specification (tests/viterbi_ref.py). Labels are
compared with array_equal and scores bit for bit: the operation order is fixed, so equality is exact. The shapes are the
smallest at which the kernel can go wrong -- every class-count template, one step either side of the staging chunk and of
the LDS / workspace boundary, more entities than one workgroup takes, the longest sequence once per route -- not
evaluation shapes."""
import numpy as np
import pytest
import torch

import twog_gcn_amd  # noqa: F401
from twog_gcn_amd import _lib
from twog_gcn_amd import kernels as twog_kernels
from twog_gcn_amd import postprocess as pp
from tests import viterbi_cases as VC
from tests import viterbi_ref as V

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
OVERLAPS = (0.1, 0.25, 0.5)
CHUNK = _lib.VITERBI_CHUNK


def K():
    k = twog_kernels.get_kernels()
    assert k.name == 'hip'
    return k


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and a.tobytes() == b.tobytes()


def lds_boundary(bs, C, E):
    """The largest T whose back-pointers stay in LDS, asked of twog_viterbi_workspace (0: none does)."""
    lo, hi = 0, V.MAX_STEPS
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if K().viterbi_route(bs, C, mid, E)[0] == 'lds':
            lo = mid
        else:
            hi = mid - 1
    return lo


def ragged(bs, T):
    """Lengths that include 0, 1 and T (and one beyond T and one below 0, which the kernel clamps)."""
    return np.asarray([T, 1, 0, max(1, T - 1), T + 5, -3, max(1, T // 2)][:bs], dtype=np.int64)


def check(logp, A, pi, lengths, ds, T_out, route, what):
    bs, C, T, E = logp.shape
    assert K().viterbi_route(bs, C, T, E)[0] == route, (what, K().viterbi_route(bs, C, T, E))
    inputs = [dev(logp), dev(A), dev(pi), dev(lengths)]
    labels, score = K().viterbi_decode(*inputs, ds, T_out)
    want, want_score = V.viterbi_labels(logp, A, pi, lengths, ds, T_out, fast=True)
    labels, score = labels.cpu().numpy(), score.cpu().numpy()
    assert labels.dtype == np.int64 and labels.shape == want.shape, what
    bad = np.argwhere(labels != want)
    assert bad.size == 0, (what, bad[:5], labels[tuple(bad[0])], want[tuple(bad[0])])
    assert same_bits(score, want_score), (what, score, want_score)
    for t, before in zip(inputs, (logp, A, pi, lengths)):       # the inputs are read only
        assert t is None or np.array_equal(t.cpu().numpy(), before, equal_nan=True), what
    return labels, score


# (bs, C, T, E, downsampling, T_out or None for T * downsampling, ragged lengths, with pi)
SHAPES = [
    (1, 1, 1, 1, 1, None, False, False),
    (3, 1, 65, 3, 3, 190, True, True),
    (2, 2, 2, 5, 1, 7, False, True),                  # T_out longer than T * ds
    (4, 2, 63, 1, 3, 100, True, False),               # T_out shorter
    (3, 10, CHUNK - 1, 3, 1, None, True, True),
    (3, 10, CHUNK, 3, 3, CHUNK * 3 + 4, True, False),
    (3, 10, CHUNK + 1, 5, 1, None, True, True),
    (2, 10, 2 * CHUNK + 1, 12, 1, None, True, True),  # 12 entities: two workgroups per clip, 8 + 4 waves
    (7, 17, 64, 3, 3, 64 * 3 - 5, True, True),        # the 32-class template
    (3, 63, 1, 5, 1, 4, True, True),
    (3, 63, 65, 1, 1, None, True, False),
    (2, 64, 2, 3, 1, None, False, True),
    (3, 64, 63, 5, 3, 200, True, True),
    (2, 64, 64, 1, 1, None, False, False),
    (1, 9, 3 * CHUNK, 9, 1, None, False, True),       # 9 entities: 8 waves + 1
]


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'bs{}-C{}-T{}-E{}-ds{}'.format(*s[:5]))
def test_decode_equals_the_specification(shape):
    bs, C, T, E, ds, T_out, with_lengths, with_pi = shape
    logp, A, pi = VC.random_batch(hash(shape[:5]) % 1000, bs, C, T, E)
    A[A < -2.2] = -np.inf                             # some transitions are forbidden
    np.fill_diagonal(A, 0.0)
    lengths = ragged(bs, T) if with_lengths else None
    check(logp, A, pi if with_pi else None, lengths, ds, T * ds if T_out is None else T_out, 'lds', shape)


@pytest.mark.parametrize('E', (1, 3))
def test_either_side_of_the_lds_boundary(E):
    """C = 64: the longest sequence whose back-pointers fit in LDS, and one step more, which goes to the workspace. The
    second also decodes one of its sequences alone, where it takes the LDS route: the route does not show in the result."""
    bs = 2
    T_lds = lds_boundary(bs, 64, E)
    assert CHUNK < T_lds < V.MAX_STEPS and K().viterbi_route(bs, 64, T_lds + 1, E)[0] == 'workspace'
    logp, A, pi = VC.random_batch(30 + E, bs, 64, T_lds + 1, E)
    lengths = np.asarray([T_lds + 1, T_lds - 2], dtype=np.int64)
    check(np.ascontiguousarray(logp[:, :, :T_lds]), A, pi, None, 1, T_lds, 'lds', ('at', T_lds, E))
    labels, score = check(logp, A, pi, lengths, 1, T_lds + 1, 'workspace', ('beyond', T_lds + 1, E))
    alone = np.ascontiguousarray(logp[1:, :, :, E - 1:])
    assert K().viterbi_route(1, 64, T_lds + 1, 1)[0] == ('lds' if E > 1 else 'workspace')
    one, one_score = K().viterbi_decode(dev(alone), dev(A), dev(pi), dev(lengths[1:]), 1, T_lds + 1)
    assert np.array_equal(one.cpu().numpy()[0, :, 0], labels[1, :, E - 1]) and same_bits(one_score.cpu().numpy()[0], score[1, E - 1:])


@pytest.mark.parametrize('C, E, route', ((64, 2, 'workspace'), (10, 2, 'lds')))
def test_the_longest_sequence(C, E, route):
    logp, A, pi = VC.random_batch(40 + C, 2, C, V.MAX_STEPS, E)
    check(logp, A, pi, np.asarray([V.MAX_STEPS, V.MAX_STEPS - 1], dtype=np.int64), 1, V.MAX_STEPS, route, (C, E))


def test_limits_and_refusals():
    assert K().viterbi_limits() == (V.MAX_CLASSES, V.MAX_STEPS) == twog_kernels.viterbi_limits()
    for shape in ((1, 65, 3, 1), (1, 2, V.MAX_STEPS + 1, 1)):
        with pytest.raises(ValueError, match='up to 64 classes and 4096 model steps'):
            K().viterbi_decode(torch.zeros(*shape, device=DEV), torch.zeros(shape[1], shape[1], device=DEV))
    route, nbytes = K().viterbi_route(64, 64, V.MAX_STEPS, 1)
    assert route == 'workspace' and nbytes == 64 * 64 * V.MAX_STEPS
    logp = torch.zeros(1, 64, V.MAX_STEPS, 1, device=DEV)
    A = torch.zeros(64, 64, device=DEV)
    labels, score = torch.zeros(1, 8, 1, dtype=torch.int64, device=DEV), torch.zeros(1, 1, device=DEV)
    small = torch.zeros(16, device=DEV)
    call = lambda ws, n: K().lib.twog_viterbi_decode(logp.data_ptr(), 1, 64, V.MAX_STEPS, 1, A.data_ptr(), 0, 0, 1, 8,
                                                     labels.data_ptr(), score.data_ptr(), ws, n, 0)
    assert call(0, 0) == -3 and call(small.data_ptr(), 64) == -3          # the workspace route without its workspace
    torch.cuda.synchronize()


@pytest.mark.parametrize('case', VC.hand_cases(), ids=lambda c: c.name)
def test_hand_cases(case):
    logp, lengths = VC.hand_batch(case, E=3)
    labels, score = K().viterbi_decode(dev(logp), dev(case.A), dev(case.pi), dev(lengths))
    T = logp.shape[2]
    want = list(case.path) + [case.path[-1] if case.path else 0] * (T - case.length)
    for e in range(3):
        assert labels[0, :, e].tolist() == want and float(score[0, e]) == case.score


@pytest.mark.parametrize('forbid', (0.0, 0.3))
def test_dyadic_ties(forbid):
    """The tie cases of the CPU file (there checked against brute force), many sequences to a launch: equal scores are the
    rule on this grid, so the strict comparison and the order of the candidates decide every label."""
    for C in (1, 2, 3):
        for L in range(1, 7):
            logp, A, pi = VC.dyadic_batch(1000 * C + 10 * L, 6, C, L, 2, forbid)
            logp, A, pi = np.round(logp), np.where(np.isinf(A), A, np.round(A / 4)), np.round(pi)
            check(logp, A, pi, None, 1, L, 'lds', ('dyadic', C, L))
    logp, A, pi = VC.dyadic_batch(77, 3, 7, 3 * CHUNK + 5, 3, forbid)           # and on the full 2^-7 grid over several chunks
    check(logp, A, pi, ragged(3, 3 * CHUNK + 5), 1, 3 * CHUNK + 5, 'lds', 'dyadic long')
    zero = np.zeros((7, 7), dtype=np.float32)
    labels, _ = check(logp, zero, None, None, 2, 6 * CHUNK + 10, 'lds', 'zero transitions')
    assert torch.equal(dev(labels), K().predict_labels(dev(logp), 2, 6 * CHUNK + 10))    # the per-step argmax


def test_a_sequence_alone_equals_the_same_sequence_in_a_batch():
    logp, A, pi = VC.random_batch(9, 5, 12, 2 * CHUNK + 3, 5)
    lengths = np.asarray([35, 20, 35, 7, 1], dtype=np.int64)
    labels, score = check(logp, A, pi, lengths, 2, 80, 'lds', 'batch')
    for b, e in ((0, 0), (1, 4), (3, 2), (4, 1)):
        alone = np.ascontiguousarray(logp[b:b + 1, :, :, e:e + 1])
        one, one_score = K().viterbi_decode(dev(alone), dev(A), dev(pi), dev(lengths[b:b + 1]), 2, 80)
        assert np.array_equal(one.cpu().numpy()[0, :, 0], labels[b, :, e]) and same_bits(one_score.cpu().numpy()[0], score[b, e:e + 1])


@pytest.mark.parametrize('C, T, E', ((10, 2 * CHUNK + 1, 3), (64, 0, 2)))
def test_guard_words_and_run_to_run_identity(C, T, E):
    """labels, score and the workspace sit inside one buffer of 0x5a bytes with 256 guard bytes around each: nothing but
    the three is written. T = 0 stands for one step beyond the LDS boundary (the workspace route)."""
    bs, ds = 3, 2
    T = T or lds_boundary(bs, C, E) + 1
    T_out = T * ds + 3
    route, ws_bytes = K().viterbi_route(bs, C, T, E)
    assert route == ('workspace' if C == 64 else 'lds') and (ws_bytes > 0) == (route == 'workspace')
    logp, A, pi = VC.random_batch(50 + C, bs, C, T, E)
    lengths = np.asarray([T, T - 3, 0], dtype=np.int64)
    sizes = [8 * bs * T_out * E, 4 * bs * E, ws_bytes]
    span = [(s + 255) // 256 * 256 for s in sizes]
    buf = torch.full((256 * 4 + sum(span),), 0x5a, dtype=torch.uint8, device=DEV)
    guards = torch.ones(buf.numel(), dtype=torch.bool)     # every byte outside labels, score and the workspace
    at, offsets = 256, []
    for s, sp in zip(sizes, span):
        offsets.append(at)
        guards[at:at + s] = False
        at += sp + 256
    guards = guards.to(DEV)
    labels = buf[offsets[0]:offsets[0] + sizes[0]].view(torch.int64).view(bs, T_out, E)
    score = buf[offsets[1]:offsets[1] + sizes[1]].view(torch.float32).view(bs, E)
    inputs = [dev(logp), dev(A), dev(pi), dev(lengths)]
    before = buf.clone()
    results = []
    for _ in range(2):
        buf.copy_(before)
        rc = K().lib.twog_viterbi_decode(inputs[0].data_ptr(), bs, C, T, E, inputs[1].data_ptr(), inputs[2].data_ptr(),
                                         inputs[3].data_ptr(), ds, T_out, labels.data_ptr(), score.data_ptr(),
                                         buf.data_ptr() + offsets[2], ws_bytes, torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
        assert torch.equal(buf[guards], before[guards])
        results.append((labels.cpu().numpy().copy(), score.cpu().numpy().copy()))
    want, want_score = V.viterbi_labels(logp, A, pi, lengths, ds, T_out, fast=True)
    for got, got_score in results:
        assert np.array_equal(got, want) and same_bits(got_score, want_score)
    for t, was in zip(inputs, (logp, A, pi, lengths)):
        assert np.array_equal(t.cpu().numpy(), was)


def test_nan_stays_inside():
    """NaN is out of contract: whatever the labels are, they are labels, and nothing outside the outputs is written."""
    logp, A, pi = VC.random_batch(3, 2, 10, 40, 3)
    logp[0, 3, 5:9, 1] = np.nan
    A[2, 4] = np.nan
    A[1, :] = np.inf
    logp[1, :, 7, 0] = -np.inf
    labels, score = K().viterbi_decode(dev(logp), dev(A), dev(pi))
    assert int(labels.min()) >= 0 and int(labels.max()) < 10


# ---------------------------------------------------------------------------------------------------- transition counts
@pytest.mark.parametrize('stride', (1, 2, 3))
def test_transition_counts(stride):
    for name, targets, C, ignore in VC.count_cases():
        want = VC.double_loop_counts(targets, C, stride, ignore)
        t = dev(targets)
        got = pp.transition_counts(t, C, stride=stride, ignore_index=ignore)
        assert got.dtype == torch.int64 and got.device == t.device and np.array_equal(got.cpu().numpy(), want), name
        assert pp.transition_counts(t, C, stride=stride, ignore_index=ignore, out=got) is got
        assert np.array_equal(got.cpu().numpy(), 2 * want), name                  # a second call accumulates
        assert np.array_equal(t.cpu().numpy(), targets)
    rng = np.random.default_rng(stride)                                           # several workgroups, 64 classes
    big = np.repeat(rng.integers(-1, 66, size=(6, 120, 3)), 3, axis=1)[:, :301].astype(np.int64)
    got = pp.transition_counts(dev(big), 64, stride=stride)
    assert np.array_equal(got.cpu().numpy(), VC.double_loop_counts(big, 64, stride, -1))
    probs = pp.transition_log_probs(got, smoothing=0.5)
    assert probs.device == got.device and np.array_equal(probs.cpu().numpy(), V.transition_log_probs(got.cpu().numpy(), 0.5))


# ---------------------------------------------------------------------------------------------------- the accumulator
def run(acc, batches, step_index=None):
    for logp, tgt, lengths in batches:
        acc.update([dev(logp)] * len(acc.names), [dev(tgt)] * len(acc.names), step_index=step_index, lengths=dev(lengths))
    return acc


def test_accumulator_with_a_decoder_is_its_kernels_on_the_specification_labels():
    batches = VC.accumulator_batches(bs=4, C=13, T=20, E=3, ds=3, T_tgt=61)
    _, A, pi = VC.random_batch(1, 1, 13, 1, 1)
    kwargs = dict(downsampling=3, overlaps=OVERLAPS, f1_route='workgroup', edit=True)
    index = dev(pp.segment_step_index([[0, 3, 4, 9, 60], [1, 2], [], [5, 6, 7, 8, 16, 17, 40]]).numpy())
    for step_index in (None, index):
        acc = run(pp.EvaluationAccumulator(['a', 'b'], 13, decoder=pp.ViterbiDecoder(A, pi), **kwargs), batches, step_index)
        spec = run(pp.EvaluationAccumulator(['a', 'b'], 13, decoder=VC.SpecDecoder(A, pi), **kwargs), batches, step_index)
        assert acc.last_f1_route == 'workgroup'
        assert torch.equal(acc._state, spec._state)                               # integers exactly, sums bit for bit
        res = acc.result()
        assert res['a']['confusion'].sum() > 0 and res['a']['edit'] == spec.result()['a']['edit']
        plain = run(pp.EvaluationAccumulator(['a', 'b'], 13, **kwargs), batches, step_index)
        assert not torch.equal(plain._state, acc._state)                          # the decoder is not the argmax here


def test_accumulator_with_zero_transitions_counts_what_the_plain_one_counts():
    batches = [(l, t, None) for l, t, _ in VC.accumulator_batches(bs=4, C=13, T=20, E=3, ds=3, T_tgt=61, dyadic=True)]
    kwargs = dict(downsampling=3, overlaps=OVERLAPS, f1_route='workgroup', edit=True)
    plain = run(pp.EvaluationAccumulator(['a'], 13, **kwargs), batches)
    zero = run(pp.EvaluationAccumulator(['a'], 13, decoder=pp.ViterbiDecoder(np.zeros((13, 13))), **kwargs), batches)
    assert torch.equal(plain._state, zero._state)
    assert plain.result()['a']['confusion'].sum() > 0
