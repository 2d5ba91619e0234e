"""CPU: the specification of the segmental decode (tests/segdecode_ref.py) against brute force, against the Viterbi
specification and against hand cases; the duration statistics; and the host layer of 2g-gcn_amd/postprocess.py on the test
double (tests/segdecode_fake.py). Every comparison is exact."""
import itertools
import math
import os

import numpy as np
import pytest
import torch

import twog_gcn_amd  # noqa: F401
from twog_gcn_amd import _lib
from twog_gcn_amd import kernels as twog_kernels
from twog_gcn_amd import postprocess as pp
from tests import segdecode_cases as SC
from tests import segdecode_ref as S
from tests import viterbi_cases as VC
from tests import viterbi_ref as V
from tests.helpers import ROOT
from tests.segdecode_fake import SegdecodeFakeKernels

OVERLAPS = (0.1, 0.25, 0.5)
NEG = -np.inf


@pytest.fixture()
def fake():
    backend = SegdecodeFakeKernels()
    twog_kernels._set_backend_for_tests(backend)
    yield backend
    twog_kernels._set_backend_for_tests(None)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------------- the specification
def compositions(L, D):
    """Every way to write L as an ordered sum of parts in 1 .. D."""
    if L == 0:
        yield ()
        return
    for first in range(1, min(D, L) + 1):
        for rest in compositions(L - first, D):
            yield (first,) + rest


def brute_force(logp, A, pi, dur):
    """The best score over every segmentation (segment lengths and one class per segment), in fp64: exact on eighths."""
    L, C = logp.shape
    best = -np.inf
    for parts in compositions(L, dur.shape[1]):
        for classes in itertools.product(range(C), repeat=len(parts)):
            s, t = float(pi[classes[0]]), 0
            for k, (l, c) in enumerate(zip(parts, classes)):
                if k:
                    s += float(A[classes[k - 1], c])
                s += float(dur[c, l - 1]) + float(logp[t:t + l, c].astype(np.float64).sum())
                t += l
            best = max(best, s)
    return best


def path_score(y, logp, A, pi, dur):
    """The best score among the segmentations whose labels are y: runs of y, each cut into parts of at most D steps."""
    L, C = logp.shape
    best = -np.inf
    runs = [(label, len(list(g))) for label, g in itertools.groupby(y.tolist())]
    options = [list(compositions(n, dur.shape[1])) for _, n in runs]
    for cut in itertools.product(*options):
        parts = [(c, l) for (c, _), ls in zip(runs, cut) for l in ls]
        s, t = float(pi[parts[0][0]]), 0
        for k, (c, l) in enumerate(parts):
            if k:
                s += float(A[parts[k - 1][0], c])
            s += float(dur[c, l - 1]) + float(logp[t:t + l, c].astype(np.float64).sum())
            t += l
        best = max(best, s)
    return best


@pytest.mark.parametrize('no_self', (False, True), ids=('diagonal', 'no-self'))
def test_specification_equals_brute_force_on_dyadic_inputs(no_self):
    seen = 0
    for C, L, D in itertools.product((1, 2, 3), range(1, 7), (1, 2, 3)):
        for seed in range(2):
            logp, A, pi, dur = SC.dyadic_batch(7000 + 100 * C + 10 * L + D + 1000 * seed, 1, C, L, 1, D,
                                               forbid=0.25 if seed else 0.0, no_self=no_self, lowest=2)
            seq = logp[0, :, :, 0].T
            y, score = S.decode_sequence(seq, A, dur, pi)
            want = brute_force(seq, A, pi, dur)
            assert float(score) == want, (C, L, D, seed, float(score), want)
            assert y.shape == (L,) and y.min() >= 0 and y.max() < C
            if np.isfinite(want):
                assert path_score(y, seq, A, pi, dur) == want, (C, L, D, seed)     # the labels are those of a best segmentation
                seen += 1
            y2, score2 = S.decode_sequence_fast(seq, A, dur, pi)
            assert np.array_equal(y, y2) and same_bits(score, score2)
    assert seen > 50


def test_the_fast_form_equals_the_literal_one():
    for seed, (C, L, D) in enumerate(((1, 1, 1), (2, 7, 3), (5, 23, 4), (7, 19, 19), (3, 9, 30), (9, 40, 8))):
        for make in (SC.random_batch, lambda *a: SC.dyadic_batch(*a, forbid=0.2)):
            logp, A, pi, dur = make(seed, 2, C, L, 2, D)
            for pi_ in (pi, None):
                a = S.segment_labels(logp, A, dur, pi_, [L, L - 1], 2, 2 * L + 3)
                b = S.segment_labels(logp, A, dur, pi_, [L, L - 1], 2, 2 * L + 3, fast=True)
                assert np.array_equal(a[0], b[0]) and same_bits(a[1], b[1]), (C, L, D)


def test_duration_one_without_scores_is_the_viterbi_decode():
    for seed, (C, T) in enumerate(((1, 4), (2, 9), (5, 33), (12, 20))):
        for logp, A, pi in (VC.random_batch(seed, 3, C, T, 2), VC.dyadic_batch(seed, 3, C, T, 2, 0.3)):
            lengths = [T, 1, max(1, T - 2)]
            want, want_score = V.viterbi_labels(logp, A, pi, lengths, 2, 2 * T + 1)
            for fast in (False, True):
                got, score = S.segment_labels(logp, A, np.zeros((C, 1), dtype=np.float32), pi, lengths, 2, 2 * T + 1, fast=fast)
                assert np.array_equal(got, want) and same_bits(score, want_score), (C, T, fast)


@pytest.mark.parametrize('case', SC.hand_cases(), ids=lambda c: c.name)
def test_specification_hand_cases(case):
    for one in (S.decode_sequence, S.decode_sequence_fast):
        y, score = one(case.logp[:case.length], case.A, case.dur, case.pi)
        assert y.tolist() == case.path and float(score) == case.score, (one.__name__, y, score)


def test_lengths_and_upsampling_of_the_specification():
    logp, A, pi, dur = SC.random_batch(4, 4, 3, 6, 2, 3)
    labels, score = S.segment_labels(logp, A, dur, pi, [6, 0, 9, 2], 3, 20)
    assert labels.shape == (4, 20, 2) and not labels[1].any() and not score[1].any()
    full, full_score = S.segment_labels(logp, A, dur, pi, None, 1, 6)
    assert np.array_equal(labels[0, :18], np.repeat(full[0], 3, axis=0)) and np.array_equal(labels[0, 18:], full[0, -1:].repeat(2, 0))
    assert np.array_equal(labels[2, :18], np.repeat(full[2], 3, axis=0)) and same_bits(score[[0, 2]], full_score[[0, 2]])   # 9 is clamped to 6
    short, short_score = S.segment_labels(np.ascontiguousarray(logp[3:, :, :2]), A, dur, pi, None, 3, 20)
    assert np.array_equal(labels[3], short[0]) and same_bits(score[3], short_score[0])


# ---------------------------------------------------------------------------------------------------- duration statistics
@pytest.mark.parametrize('stride', (1, 2, 3))
def test_duration_counts_against_the_double_loop(fake, stride):
    for name, targets, C, D, ignore in SC.count_cases():
        want = SC.double_loop_counts(targets, C, D, stride, ignore)
        assert np.array_equal(S.duration_counts(targets, C, D, stride, ignore), want), name
        t = torch.from_numpy(targets)
        got = pp.duration_counts(t, C, D, stride=stride, ignore_index=ignore)
        assert got.dtype == torch.int64 and got.shape == (C, D) and np.array_equal(got.numpy(), want), name
        assert pp.duration_counts(t, C, D, stride=stride, ignore_index=ignore, out=got) is got
        assert np.array_equal(got.numpy(), 2 * want), name                        # a second call accumulates
        n_steps = len(range(0, targets.shape[1], stride))
        kept = sum(1 for v in targets[:, ::stride].ravel() if v != ignore and 0 <= v < C)
        assert want.sum() <= kept <= targets.shape[0] * n_steps * targets.shape[2]
    flat = torch.from_numpy(SC.count_cases()[0][1][:, :, 0].copy())                # (bs, T) labels
    assert np.array_equal(pp.duration_counts(flat, 4, 5).numpy(), SC.double_loop_counts(flat.numpy()[:, :, None], 4, 5, 1, -1))


def test_duration_counts_host_checks(fake):
    t = torch.zeros(2, 5, 1, dtype=torch.int64)
    with pytest.raises(ValueError, match='stride'):
        pp.duration_counts(t, 3, 4, stride=0)
    with pytest.raises(ValueError, match='max_duration'):
        pp.duration_counts(t, 3, 0)
    with pytest.raises(ValueError, match='up to 64 classes and durations up to 128'):
        pp.duration_counts(t, 65, 4)
    with pytest.raises(ValueError, match='up to 64 classes and durations up to 128'):
        pp.duration_counts(t, 3, 129)
    with pytest.raises(ValueError, match='labels'):
        pp.duration_counts(torch.zeros(2, 2, 2, 2, dtype=torch.int64), 3, 4)
    assert fake.calls == []
    assert pp.duration_counts(t.to(torch.int32), 3, 4).tolist() == [[0, 0, 0, 2], [0] * 4, [0] * 4]   # two runs of 5, capped


def test_duration_log_probs_by_hand():
    counts = np.asarray([[1, 3, 0, 0], [0, 0, 0, 0], [0, 0, 2, 2]], dtype=np.int64)
    got = pp.duration_log_probs(torch.from_numpy(counts), smoothing=1.0)
    want = np.zeros((3, 4))
    want[0] = np.log(np.asarray([2, 4, 1, 1]) / 8.0)               # (n + 1) / (4 + 4 * 1)
    want[2] = np.log(np.asarray([1, 1, 3, 3]) / 8.0)
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), want.astype(np.float32))
    assert np.array_equal(got.numpy(), S.duration_log_probs(counts, 1.0))
    hard = pp.duration_log_probs(counts, smoothing=0.0).numpy()      # anything array-like comes in
    assert np.array_equal(hard[0], np.asarray([np.log(0.25), np.log(0.75), NEG, NEG]).astype(np.float32)) and np.isneginf(hard[0, 2:]).all()
    assert not hard[1].any() and np.array_equal(hard, S.duration_log_probs(counts, 0.0))
    poisson = pp.duration_log_probs(counts, scheme='poisson').numpy()
    lam0, lam2 = (1 * 1 + 3 * 2) / 4.0, (2 * 3 + 2 * 4) / 4.0
    want = np.zeros((3, 4))
    for l in range(1, 5):
        want[0, l - 1] = l * math.log(lam0) - lam0 - math.lgamma(l + 1)
        want[2, l - 1] = l * math.log(lam2) - lam2 - math.lgamma(l + 1)
    assert np.array_equal(poisson, want.astype(np.float32)) and np.array_equal(poisson, S.duration_log_probs(counts, 1.0, 'poisson'))
    mass = sum(math.exp(-lam0) * lam0 ** l / math.factorial(l) for l in range(1, 5))      # it is the Poisson log-probability
    assert abs(np.exp(poisson[0].astype(np.float64)).sum() - mass) < 1e-6
    with pytest.raises(ValueError, match='scheme'):
        pp.duration_log_probs(counts, scheme='gamma')
    with pytest.raises(ValueError, match=r'\(C, D\)'):
        pp.duration_log_probs(np.zeros(4))


def test_segment_transition_log_probs_by_hand():
    counts = np.asarray([[50, 1, 3], [2, 70, 0], [0, 0, 9]], dtype=np.int64)      # the diagonal: frames that stay
    got = pp.segment_transition_log_probs(torch.from_numpy(counts), smoothing=1.0).numpy()
    want = np.full((3, 3), NEG)
    want[0, 1], want[0, 2] = np.log(2 / 6.0), np.log(4 / 6.0)       # (n + 1) / (4 + 2 * 1)
    want[1, 0], want[1, 2] = np.log(3 / 4.0), np.log(1 / 4.0)
    want[2, 0], want[2, 1] = np.log(1 / 2.0), np.log(1 / 2.0)
    assert got.dtype == np.float32 and np.array_equal(got, want.astype(np.float32))
    assert np.array_equal(got, S.segment_transition_log_probs(counts, 1.0))
    hard = pp.segment_transition_log_probs(counts, smoothing=0.0, self_transition=-2.5).numpy()
    assert hard.diagonal().tolist() == [-2.5] * 3 and hard[1, 2] == NEG and hard[1, 0] == 0.0
    assert hard[2, 0] == 0.0 and hard[2, 1] == 0.0                   # a row that never leaves: nothing is known
    assert np.array_equal(hard, S.segment_transition_log_probs(counts, 0.0, -2.5))
    assert counts[0, 0] == 50                                        # the caller's counts are not touched
    with pytest.raises(ValueError, match='square'):
        pp.segment_transition_log_probs(np.zeros((2, 3)))


# ---------------------------------------------------------------------------------------------------- the host layer
def test_decoder_returns_what_predict_labels_returns(fake):
    logp, A, pi, dur = SC.random_batch(8, 3, 5, 9, 2, 4)
    out = torch.from_numpy(logp)
    target = torch.zeros(3, 20, 2, dtype=torch.int64)
    decoder = pp.SegmentalDecoder(A.astype(np.float64), dur.astype(np.float64), pi)      # any dtype comes in, fp32 is kept
    assert decoder.transitions.dtype == decoder.durations.dtype == decoder.initial.dtype == torch.float32
    assert decoder.num_classes == 5 and decoder.max_duration == 4 and decoder.last_score is None
    for tgt, ds, lengths in ((None, 1, None), (target, 2, None), (None, 2, None), (target, 1, None),
                             (target, 3, torch.tensor([9, 0, 4]))):
        plain = pp.predict_labels(out, tgt, ds)
        got = decoder(out, tgt, ds, lengths)
        assert got.shape == plain.shape and got.dtype == plain.dtype == torch.int64
        want, want_score = S.segment_labels(logp, A, dur, pi, None if lengths is None else lengths.numpy(), ds, plain.shape[1])
        assert np.array_equal(got.numpy(), want) and same_bits(decoder.last_score.numpy(), want_score)
    assert fake.segdecode_args[-1] == ([9, 0, 4], 3, 20, 4)
    labels, score = pp.segment_decode_labels(out, torch.from_numpy(A), torch.from_numpy(dur), torch.from_numpy(pi), target, 2)
    want, want_score = S.segment_labels(logp, A, dur, pi, None, 2, 20)
    assert np.array_equal(labels.numpy(), want) and same_bits(score.numpy(), want_score)
    frame = pp.SegmentalDecoder(A, np.zeros((5, 1)), pi)                 # D = 1 without scores: the Viterbi decode
    assert torch.equal(frame(out, target, 2), pp.ViterbiDecoder(A, pi)(out, target, 2))
    with pytest.raises(RuntimeError, match='Number of dimensions'):
        decoder(out[0])
    with pytest.raises(RuntimeError, match='Number of dimensions'):
        pp.segment_decode_labels(out[0], torch.from_numpy(A), torch.from_numpy(dur))
    with pytest.raises(ValueError, match='5 classes'):
        pp.SegmentalDecoder(np.zeros((4, 4)), np.zeros((4, 2)))(out)
    with pytest.raises(ValueError, match=r'\(C, C\)'):
        pp.SegmentalDecoder(np.zeros((4, 5)), np.zeros((4, 2)))
    with pytest.raises(ValueError, match='durations'):
        pp.SegmentalDecoder(np.zeros((4, 4)), np.zeros((5, 2)))
    with pytest.raises(ValueError, match='durations'):
        pp.SegmentalDecoder(np.zeros((4, 4)), np.zeros((4, 0)))
    with pytest.raises(ValueError, match='initial'):
        pp.SegmentalDecoder(np.zeros((4, 4)), np.zeros((4, 2)), np.zeros(5))


def test_process_output_with_a_decoder(fake):
    batches = [SC.random_batch(20 + n, 2, 4, 6, 3, 3)[0] for n in range(2)]
    _, A, _, dur = SC.random_batch(20, 1, 4, 1, 1, 3)
    outputs = [[torch.from_numpy(b), torch.from_numpy(b[:, :, :, :1].copy())] for b in batches]
    targets = [[torch.zeros(2, 11, 3), torch.zeros(2, 11, 1)] for _ in batches]
    lengths = [torch.tensor([6, 2]), torch.tensor([0, 5])]
    plain = pp.process_output(outputs, 2, targets)
    assert fake.calls == []                                                              # the default path asks no decoder
    got = pp.process_output(outputs, 2, targets, decoder=pp.SegmentalDecoder(A, dur), lengths=lengths)
    assert fake.calls == ['segment_decode'] * 4
    for i in (0, 1):
        want = np.concatenate([S.segment_labels(o[i].numpy(), A, dur, None, l.numpy(), 2, 11)[0] for o, l in zip(outputs, lengths)])
        assert got[i].shape == plain[i].shape and np.array_equal(got[i].numpy(), want)
    named = pp.process_output(outputs, 2, targets, index_to_name=['h', 'o'],
                              decoder={'o': pp.SegmentalDecoder(A, dur), 'h': pp.ViterbiDecoder(A)})      # the dict form
    assert fake.calls[4:] == ['viterbi_decode', 'segment_decode'] * 2
    assert np.array_equal(named['h'].numpy(), np.concatenate([V.viterbi_labels(o[0].numpy(), A, None, None, 2, 11)[0] for o in outputs]))
    assert not torch.equal(named['o'], plain[1])
    assert np.array_equal(named['o'].numpy(), np.concatenate([S.segment_labels(o[1].numpy(), A, dur, None, None, 2, 11)[0]
                                                              for o in outputs]))


def run(acc, batches, step_index=None):
    for logp, tgt, lengths in batches:
        out, target = torch.from_numpy(logp), torch.from_numpy(tgt)
        acc.update([out] * len(acc.names), [target] * len(acc.names), step_index=step_index,
                   lengths=None if lengths is None else torch.from_numpy(lengths))
    return acc


@pytest.mark.parametrize('route', ('thread', 'workgroup'))
def test_accumulator_with_a_decoder_is_its_kernels_on_the_specification_labels(fake, route):
    batches = VC.accumulator_batches()
    _, A, pi, dur = SC.random_batch(1, 1, 5, 1, 1, 4)
    kwargs = dict(downsampling=2, overlaps=OVERLAPS, f1_route=route, edit=True)
    index = pp.segment_step_index([[0, 3, 4, 9], [1, 2], [], [5, 6, 7, 8, 16]])
    for step_index in (None, index):
        fake.calls.clear()
        acc = run(pp.EvaluationAccumulator(['a', 'b'], 5, decoder=pp.SegmentalDecoder(A, dur, pi), **kwargs), batches, step_index)
        f1_calls = ['segment_f1', 'segment_f1_accumulate'] if route == 'workgroup' else ['f1_at_k'] * len(OVERLAPS)
        assert fake.calls == (['segment_decode', 'confusion_counts', 'segment_edit', 'segment_f1_accumulate'] + f1_calls) * 4
        assert fake.segdecode_args[-1] == ([9, 1, 7, 0], 2, 17, 4)                         # target steps, whatever the index
        spec = run(pp.EvaluationAccumulator(['a', 'b'], 5, decoder=SC.SpecDecoder(A, dur, pi), **kwargs), batches, step_index)
        assert torch.equal(acc._state, spec._state)
        plain = run(pp.EvaluationAccumulator(['a', 'b'], 5, **kwargs), batches, step_index)
        assert not torch.equal(plain._state, acc._state)                                   # the decoder is not the argmax here
    mixed = pp.EvaluationAccumulator(['a', 'b'], 5, decoder=[pp.ViterbiDecoder(A), pp.SegmentalDecoder(A, dur)])
    assert [type(d).__name__ for d in mixed.decoders] == ['ViterbiDecoder', 'SegmentalDecoder']
    with pytest.raises(ValueError, match='transition model 4'):
        pp.EvaluationAccumulator(['a'], 5, decoder=pp.SegmentalDecoder(np.zeros((4, 4)), np.zeros((4, 2))))


def test_refusals_above_the_limits_come_before_the_backend(fake):
    assert fake.segdecode_limits() == (64, 4096, 128) == twog_kernels.segdecode_limits()
    message = 'up to 64 classes, 4096 model steps and durations up to 128'
    with pytest.raises(ValueError, match=message):
        pp.SegmentalDecoder(np.zeros((65, 65)), np.zeros((65, 2)))(torch.zeros(1, 65, 3, 1))
    with pytest.raises(ValueError, match=message):
        pp.SegmentalDecoder(np.zeros((2, 2)), np.zeros((2, 2)))(torch.zeros(1, 2, 4097, 1))
    with pytest.raises(ValueError, match=message):
        pp.SegmentalDecoder(np.zeros((2, 2)), np.zeros((2, 129)))(torch.zeros(1, 2, 5, 1))
    acc = pp.EvaluationAccumulator(['a'], 2, decoder=pp.SegmentalDecoder(np.zeros((2, 2)), np.zeros((2, 129))))
    with pytest.raises(ValueError, match=message):
        acc.update([torch.zeros(1, 2, 7, 1)], [torch.zeros(1, 7, 1, dtype=torch.int64)])
    assert fake.calls == [] and fake.segdecode_args == []
    assert pp.SegmentalDecoder(np.zeros((2, 2)), np.zeros((2, 128)))(torch.zeros(1, 2, 130, 1)).shape == (1, 130, 1)


def test_the_ctypes_layer_refuses_before_any_launch():
    """HipKernels.segment_decode with the library loaded and no device: beyond the limits it raises before it touches one,
    and the plan is launch-free."""
    K = twog_kernels.HipKernels()
    assert K.segdecode_limits() == (S.MAX_CLASSES, S.MAX_STEPS, S.MAX_DURATION) == (64, 4096, _lib.SEGDEC_MAX_DURATION)
    for shape, D in (((1, 65, 3, 1), 2), ((1, 2, 4097, 1), 2), ((1, 2, 5, 1), 129)):
        with pytest.raises(ValueError, match='up to 64 classes, 4096 model steps and durations up to 128'):
            K.segment_decode(torch.zeros(*shape), torch.zeros(shape[1], shape[1]), torch.zeros(shape[1], D))
    for bad in ((1, 65, 8, 1, 4), (1, 4, 4097, 1, 4), (1, 4, 8, 1, 129)):
        with pytest.raises(ValueError):
            K.segdecode_plan(*bad)
    for bad in ((1, 4, 8, 1, 0), (1, 0, 8, 1, 4), (1, 4, 0, 1, 4), (1, 4, 8, 0, 4), (-1, 4, 8, 1, 4)):
        with pytest.raises(RuntimeError, match='code -1'):
            K.segdecode_plan(*bad)
    small = K.segdecode_plan(2, 10, 33, 3, 16)
    assert small == {'class_template': 16, 'waves': 3, 'groups': 1, 'route': 'lds', 'workspace_bytes': 0}
    assert [K.segdecode_plan(1, c, 8, 1, 4)['class_template'] for c in (1, 8, 9, 16, 17, 32, 33, 64)] == [8, 8, 16, 16, 32, 32, 64, 64]
    assert K.segdecode_plan(1, 10, 20, 9, 4)['waves'] == 8 and K.segdecode_plan(1, 10, 20, 9, 4)['groups'] == 2
    # the worst case: one wave holds the ring of 128 steps of 64 classes, and its 4096 steps of back-pointers go outside
    worst = K.segdecode_plan(3, 64, 4096, 2, 128)
    assert worst['waves'] == 1 and worst['groups'] == 2 and worst['route'] == 'workspace'
    assert worst['workspace_bytes'] == 3 * 2 * 2 * 4096 * 64                          # two bytes per (sequence, t, c)
    # the waves follow the LDS budget: per wave a ring of min(D, T) steps of (e, logp) and, on the LDS route, two bytes per
    # (t, c) of back-pointers; dur and the staging buffers once. The route is 'lds' whenever one wave fits with its back-pointers.
    budget, routes = 160 * 1024, set()
    for C, T, E, D in ((64, 200, 8, 128), (64, 200, 8, 32), (20, 120, 5, 120), (64, 16, 8, 128), (33, 4096, 8, 60),
                       (10, 4096, 2, 128), (64, 1100, 3, 16), (64, 1200, 3, 16)):
        plan = K.segdecode_plan(1, C, T, E, D)
        Dr, bp = min(D, T), (T + 1) // 2 * C * 4
        base = lambda w: w * Dr * C * 8 + Dr * C * 4 + 2 * C * (16 * w + 1) * 4
        lds = base(1) + bp <= budget
        need = lambda w: base(w) + (w * bp if lds else 0)
        assert plan['route'] == ('lds' if lds else 'workspace'), (C, T, E, D, plan)
        assert need(plan['waves']) <= budget and (plan['waves'] == min(E, 8) or need(plan['waves'] + 1) > budget), (C, T, E, D, plan)
        assert plan['groups'] == -(-E // plan['waves']) and (plan['workspace_bytes'] == 0) == lds
        routes.add((plan['route'], plan['waves']))
    assert ('lds', 1) in routes and ('workspace', 3) in routes and ('lds', 8) in routes


def test_abi_symbols_are_declared():
    symbols = _lib.exported_symbols()
    header = open(os.path.join(ROOT, 'include', 'twog_gcn.h')).read()
    for name, n_args in (('twog_segdecode_limits', 3), ('twog_segdecode_plan', 7), ('twog_segdecode', 17),
                         ('twog_duration_counts', 10)):
        assert name in symbols and f'int {name}(' in header and len(_lib.SIGNATURES[name]) == n_args
    assert f'#define TWOG_SEGDEC_MAX_DURATION {_lib.SEGDEC_MAX_DURATION}\n' in header
