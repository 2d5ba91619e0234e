"""CPU: the specification of the Viterbi decode (tests/viterbi_ref.py) against brute force and hand cases, the transition
statistics and matrix helpers, and the host layer of 2g-gcn_amd/postprocess.py through the test double."""
import itertools
import os

import numpy as np
import pytest
import torch

import twog_gcn_amd  # noqa: F401
from twog_gcn_amd import _lib
from twog_gcn_amd import kernels as twog_kernels
from twog_gcn_amd import postprocess as pp
from tests import viterbi_cases as VC
from tests import viterbi_ref as V
from tests.helpers import ROOT
from tests.viterbi_fake import ViterbiFakeKernels

OVERLAPS = (0.1, 0.25, 0.5)


@pytest.fixture()
def fake():
    backend = ViterbiFakeKernels()
    twog_kernels._set_backend_for_tests(backend)
    yield backend
    twog_kernels._set_backend_for_tests(None)


# ---------------------------------------------------------------------------------------------------- the specification
def brute_force(logp, A, pi):
    """All C^L paths scored in fp64 (exact on the dyadic inputs); among the best the smallest from the last step backwards."""
    L, C = logp.shape
    best, best_key, best_path = None, None, None
    for path in itertools.product(range(C), repeat=L):
        s = float(pi[path[0]]) + float(logp[0, path[0]])
        for t in range(1, L):
            s += float(A[path[t - 1], path[t]]) + float(logp[t, path[t]])
        key = path[::-1]
        if best is None or s > best or (s == best and key < best_key):
            best, best_key, best_path = s, key, path
    return np.asarray(best_path, dtype=np.int64), best


@pytest.mark.parametrize('forbid', (0.0, 0.3))
def test_specification_equals_brute_force_on_dyadic_inputs(forbid):
    ties = 0
    for C in (1, 2, 3):
        for L in range(1, 7):
            for seed in range(6):
                logp, A, pi = VC.dyadic_batch(1000 * C + 10 * L + seed, 1, C, L, 1, forbid)
                # a coarse grid makes equal scores the rule, not the exception
                logp, A, pi = np.round(logp), np.where(np.isinf(A), A, np.round(A / 4)), np.round(pi)
                seq = logp[0, :, :, 0].T
                want, want_score = brute_force(seq, A, pi)
                for decode in (V.decode_sequence, V.decode_sequence_fast):
                    y, score = decode(seq, A, pi)
                    assert np.array_equal(y, want), (C, L, seed, y, want)
                    assert score.dtype == np.float32 and float(score) == want_score
                scores = sorted((sum(float(A[p[t - 1], p[t]]) for t in range(1, L)) + sum(float(seq[t, p[t]]) for t in range(L))
                                 + float(pi[p[0]]) for p in itertools.product(range(C), repeat=L)), reverse=True)
                ties += len(scores) > 1 and scores[0] == scores[1]
    assert ties >= 20, ties          # the tie-break was really asked for


@pytest.mark.parametrize('case', VC.hand_cases(), ids=lambda c: c.name)
def test_specification_hand_cases(case):
    logp, lengths = VC.hand_batch(case)
    for fast in (False, True):
        labels, score = V.viterbi_labels(logp, case.A, case.pi, lengths, fast=fast)
        T = logp.shape[2]
        want = list(case.path) + [case.path[-1] if case.path else 0] * (T - case.length)   # the last label fills the tail
        assert labels[0, :, 0].tolist() == want and float(score[0, 0]) == case.score and score.dtype == np.float32


def test_zero_transitions_are_the_per_step_argmax():
    logp, _, _ = VC.dyadic_batch(3, 3, 5, 40, 2)
    zero = np.zeros((5, 5), dtype=np.float32)
    for ds, T_out in ((1, 40), (3, 100), (3, 130)):
        labels, score = V.viterbi_labels(logp, zero, None, None, ds, T_out, fast=True)
        steps = np.minimum(np.arange(T_out) // ds, 39)
        assert np.array_equal(labels, logp.argmax(1)[:, steps])                       # np.argmax: the first maximum
        assert np.array_equal(score, logp.max(1).astype(np.float64).sum(1).astype(np.float32))   # exact sums
    slow, _ = V.viterbi_labels(logp[:1], zero)
    assert np.array_equal(slow, logp[:1].argmax(1))


def test_lengths_and_upsampling_of_the_specification():
    logp, A, pi = VC.random_batch(4, 4, 3, 7, 2)
    lengths = np.asarray([7, 0, 3, 99])
    labels, score = V.viterbi_labels(logp, A, pi, lengths, 2, 17)
    assert labels.shape == (4, 17, 2) and labels.dtype == np.int64 and score.shape == (4, 2)
    assert not labels[1].any() and not score[1].any()                                   # length 0
    assert np.array_equal(labels[3], V.viterbi_labels(logp[3:], A, pi, None, 2, 17)[0][0])   # clamped to T
    y, s = V.decode_sequence(logp[2, :, :3, 1].T, A, pi)
    assert labels[2, :, 1].tolist() == [y[min(t // 2, 2)] for t in range(17)] and score[2, 1] == s


# ---------------------------------------------------------------------------------------------------- statistics
@pytest.mark.parametrize('stride', (1, 2, 3))
def test_transition_counts_against_the_double_loop(fake, stride):
    for name, targets, C, ignore in VC.count_cases():
        want = VC.double_loop_counts(targets, C, stride, ignore)
        assert np.array_equal(V.transition_counts(targets, C, stride, ignore), want), name
        got = pp.transition_counts(torch.from_numpy(targets), C, stride=stride, ignore_index=ignore)
        assert got.dtype == torch.int64 and np.array_equal(got.numpy(), want), name
        again = pp.transition_counts(torch.from_numpy(targets), C, stride=stride, ignore_index=ignore, out=got)
        assert again is got and np.array_equal(got.numpy(), 2 * want), name            # a second pass accumulates
    assert VC.double_loop_counts(VC.count_cases()[0][1], 4, 1, -1).sum() == 3 * 2 * 18
    assert VC.double_loop_counts(VC.count_cases()[3][1], 4, stride, -1).sum() > 0   # the other entity still counts
    assert VC.double_loop_counts(VC.count_cases()[6][1], 4, stride, -1).sum() == 0


def test_transition_counts_host_checks(fake):
    two_d = pp.transition_counts(torch.tensor([[0, 0, 1, 1, 2]]), 3)
    assert two_d.tolist() == [[1, 1, 0], [0, 1, 1], [0, 0, 0]]
    with pytest.raises(ValueError, match='up to 64 classes'):
        pp.transition_counts(torch.zeros(1, 4, 1, dtype=torch.int64), 65)
    with pytest.raises(ValueError, match='stride'):
        pp.transition_counts(torch.zeros(1, 4, 1, dtype=torch.int64), 3, stride=0)
    assert fake.calls == ['transition_counts']


def test_transition_log_probs():
    counts = np.asarray([[6, 2, 0], [0, 0, 0], [1, 0, 3]], dtype=np.int64)
    for s in (1.0, 0.5):
        got = pp.transition_log_probs(torch.from_numpy(counts), smoothing=s)
        assert got.dtype == torch.float32 and got.shape == (3, 3)
        want = [[np.float32(np.log((float(n) + s) / (float(sum(row)) + 3 * s))) for n in row] for row in counts.tolist()]
        assert np.array_equal(got.numpy(), np.asarray(want, dtype=np.float32))
        assert np.array_equal(got.numpy(), V.transition_log_probs(counts, s))
    hard = pp.transition_log_probs(counts, smoothing=0).numpy()
    assert hard[0, 2] == -np.inf and hard[2, 1] == -np.inf                              # unseen: forbidden
    assert hard[0, 0] == np.float32(np.log(6.0 / 8.0)) and hard[2, 2] == np.float32(np.log(3.0 / 4.0))
    assert not hard[1].any() and not np.isnan(hard).any()                               # the empty row: all zeros
    assert np.array_equal(hard, V.transition_log_probs(counts, 0))


def test_switch_penalty():
    got = pp.switch_penalty(4, 2.5)
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), V.switch_penalty(4, 2.5))
    assert got.diagonal().tolist() == [0.0] * 4 and (got + torch.eye(4) * -2.5 == -2.5).all()


# ---------------------------------------------------------------------------------------------------- the host layer
def test_decoder_returns_what_predict_labels_returns(fake):
    logp, A, pi = VC.random_batch(8, 3, 5, 9, 2)
    out = torch.from_numpy(logp)
    target = torch.zeros(3, 20, 2, dtype=torch.int64)
    decoder = pp.ViterbiDecoder(A.astype(np.float64), pi)            # any dtype comes in, fp32 is kept
    assert decoder.transitions.dtype == torch.float32 and decoder.initial.dtype == torch.float32 and decoder.last_score is None
    for tgt, ds, lengths in ((None, 1, None), (target, 2, None), (None, 2, None), (target, 1, None),
                             (target, 3, torch.tensor([9, 0, 4]))):
        plain = pp.predict_labels(out, tgt, ds)
        got = decoder(out, tgt, ds, lengths)
        assert got.shape == plain.shape and got.dtype == plain.dtype == torch.int64
        want, want_score = V.viterbi_labels(logp, A, pi, None if lengths is None else lengths.numpy(), ds, plain.shape[1])
        assert np.array_equal(got.numpy(), want) and np.array_equal(decoder.last_score.numpy(), want_score)
    assert fake.viterbi_args[-1] == ([9, 0, 4], 3, 20)
    labels, score = pp.viterbi_labels(out, torch.from_numpy(A), torch.from_numpy(pi), target, 2)     # the functional form
    want, want_score = V.viterbi_labels(logp, A, pi, None, 2, 20)
    assert np.array_equal(labels.numpy(), want) and np.array_equal(score.numpy(), want_score)
    zero = pp.ViterbiDecoder(np.zeros((5, 5)))
    dyadic = torch.from_numpy(VC.dyadic_batch(2, 3, 5, 9, 2)[0])
    assert torch.equal(zero(dyadic, target, 2), pp.predict_labels(dyadic, target, 2))
    with pytest.raises(RuntimeError, match='Number of dimensions'):
        decoder(out[0])
    with pytest.raises(ValueError, match='5 classes'):
        pp.ViterbiDecoder(np.zeros((4, 4)))(out)
    with pytest.raises(ValueError, match=r'\(C, C\)'):
        pp.ViterbiDecoder(np.zeros((4, 5)))
    with pytest.raises(ValueError, match='initial'):
        pp.ViterbiDecoder(np.zeros((4, 4)), np.zeros(5))


def test_process_output_with_a_decoder(fake):
    batches = [VC.random_batch(20 + n, 2, 4, 6, 3)[0] for n in range(2)]
    A = V.switch_penalty(4, 1.0)
    outputs = [[torch.from_numpy(b), torch.from_numpy(b[:, :, :, :1].copy())] for b in batches]
    targets = [[torch.zeros(2, 11, 3), torch.zeros(2, 11, 1)] for _ in batches]
    lengths = [torch.tensor([6, 2]), torch.tensor([0, 5])]
    plain = pp.process_output(outputs, 2, targets)
    assert fake.calls == []                                                              # the default path asks no decoder
    got = pp.process_output(outputs, 2, targets, decoder=pp.ViterbiDecoder(A), lengths=lengths)
    assert fake.calls == ['viterbi_decode'] * 4
    for i in (0, 1):
        want = np.concatenate([V.viterbi_labels(o[i].numpy(), A, None, l.numpy(), 2, 11)[0] for o, l in zip(outputs, lengths)])
        assert got[i].shape == plain[i].shape and np.array_equal(got[i].numpy(), want)
    named = pp.process_output(outputs, 2, targets, index_to_name=['h', 'o'], decoder={'o': pp.ViterbiDecoder(A)})
    assert torch.equal(named['h'], plain[0]) and not torch.equal(named['o'], plain[1])   # only 'o' is decoded
    assert np.array_equal(named['o'].numpy(), np.concatenate([V.viterbi_labels(o[1].numpy(), A, None, None, 2, 11)[0]
                                                              for o in outputs]))


def run(acc, batches, step_index=None, device='cpu'):
    for logp, tgt, lengths in batches:
        out, target = torch.from_numpy(logp).to(device), torch.from_numpy(tgt).to(device)
        acc.update([out] * len(acc.names), [target] * len(acc.names), step_index=step_index,
                   lengths=None if lengths is None else torch.from_numpy(lengths).to(device))
    return acc


@pytest.mark.parametrize('route', ('thread', 'workgroup'))
def test_accumulator_with_a_decoder_is_its_kernels_on_the_specification_labels(fake, route):
    batches = VC.accumulator_batches()
    _, A, pi = VC.random_batch(1, 1, 5, 1, 1)
    kwargs = dict(downsampling=2, overlaps=OVERLAPS, f1_route=route, edit=True)
    index = pp.segment_step_index([[0, 3, 4, 9], [1, 2], [], [5, 6, 7, 8, 16, 17, 40]])     # two entries beyond the targets
    for step_index in (None, index):
        fake.calls.clear()
        acc = run(pp.EvaluationAccumulator(['a', 'b'], 5, decoder=pp.ViterbiDecoder(A, pi), **kwargs), batches, step_index)
        f1_calls = ['segment_f1', 'segment_f1_accumulate'] if route == 'workgroup' else ['f1_at_k'] * len(OVERLAPS)
        assert fake.calls == (['viterbi_decode', 'confusion_counts', 'segment_edit', 'segment_f1_accumulate'] + f1_calls) * 4
        assert fake.viterbi_args[-1] == ([9, 1, 7, 0], 2, 17)                              # target steps, whatever the index
        spec = run(pp.EvaluationAccumulator(['a', 'b'], 5, decoder=VC.SpecDecoder(A, pi), **kwargs), batches, step_index)
        assert torch.equal(acc._state, spec._state)
        # and the counts are those of the specification's labels, counted in numpy
        want = np.zeros((5, 5), dtype=np.int64)
        for logp, tgt, lengths in batches:
            labels, _ = V.viterbi_labels(logp, A, pi, lengths, 2, 17, fast=True)
            for b, t, e in itertools.product(*(range(n) for n in tgt.shape)):
                if step_index is not None and t not in [s for s in index[b].tolist() if 0 <= s < 17]:
                    continue
                if tgt[b, t, e] != -1:
                    want[tgt[b, t, e], labels[b, t, e]] += 1
        assert np.array_equal(acc._counts[0].numpy(), want) and np.array_equal(acc._counts[1].numpy(), want)
        if step_index is None:
            assert np.array_equal(acc.result()['a']['confusion'], want)
        else:
            assert acc._flags[0].tolist() == [0, 2 * 2 * len(batches)]                     # 2 entries x E positions per batch
            with pytest.raises(ValueError, match='beyond the last target step'):           # as after eval_update
                acc.result()


def test_accumulator_with_zero_transitions_counts_what_the_plain_one_counts(fake):
    batches = [(l, t, None) for l, t, _ in VC.accumulator_batches(dyadic=True)]
    kwargs = dict(downsampling=2, overlaps=OVERLAPS, f1_route='workgroup', edit=True)
    for step_index in (None, pp.segment_step_index([[0, 3, 4, 9], [1, 2], [], [5, 6, 7, 8, 16]])):
        plain = run(pp.EvaluationAccumulator(['a'], 5, **kwargs), batches, step_index)
        zero = run(pp.EvaluationAccumulator(['a'], 5, decoder=pp.ViterbiDecoder(np.zeros((5, 5))), **kwargs), batches, step_index)
        assert torch.equal(plain._state, zero._state)


def test_accumulator_defaults_are_what_they_were(fake):
    batches = VC.accumulator_batches()
    acc = run(pp.EvaluationAccumulator(['a'], 5, downsampling=2, overlaps=OVERLAPS, f1_route='workgroup'), batches)
    assert acc.decoders == [None] and fake.calls == ['eval_update', 'segment_f1', 'segment_f1_accumulate'] * 2
    mixed = run(pp.EvaluationAccumulator(['a', 'b'], 5, downsampling=2, overlaps=(), decoder=[None, pp.ViterbiDecoder(np.zeros((5, 5)))]),
                batches)
    assert mixed.decoders[0] is None and sorted(mixed.result()) == ['a', 'b']
    with pytest.raises(ValueError, match='one decoder or one'):
        pp.EvaluationAccumulator(['a', 'b'], 5, decoder=[None])
    with pytest.raises(ValueError, match='transition model 4'):
        pp.EvaluationAccumulator(['a'], 5, decoder=pp.ViterbiDecoder(np.zeros((4, 4))))


def test_refusals_above_the_limits_come_before_the_backend(fake):
    assert fake.viterbi_limits() == (64, 4096) == twog_kernels.viterbi_limits()
    decoder = pp.ViterbiDecoder(np.zeros((65, 65)))
    with pytest.raises(ValueError, match='up to 64 classes and 4096 model steps'):
        decoder(torch.zeros(1, 65, 3, 1))
    with pytest.raises(ValueError, match='up to 64 classes and 4096 model steps'):
        pp.ViterbiDecoder(np.zeros((2, 2)))(torch.zeros(1, 2, 4097, 1))
    acc = pp.EvaluationAccumulator(['a'], 2, decoder=pp.ViterbiDecoder(np.zeros((2, 2))))
    with pytest.raises(ValueError, match='up to 64 classes and 4096 model steps'):
        acc.update([torch.zeros(1, 2, 4097, 1)], [torch.zeros(1, 4097, 1, dtype=torch.int64)])
    assert fake.calls == [] and fake.viterbi_args == []
    assert pp.ViterbiDecoder(np.zeros((2, 2)))(torch.zeros(1, 2, 4096, 1)).shape == (1, 4096, 1)


def test_the_ctypes_layer_refuses_before_any_launch():
    """HipKernels.viterbi_decode with the library loaded and no device: beyond the limits it raises before it touches one."""
    K = twog_kernels.HipKernels()
    assert K.viterbi_limits() == (V.MAX_CLASSES, V.MAX_STEPS)
    for shape in ((1, 65, 3, 1), (1, 2, 4097, 1)):
        with pytest.raises(ValueError, match='up to 64 classes and 4096 model steps'):
            K.viterbi_decode(torch.zeros(*shape), torch.zeros(shape[1], shape[1]))
    with pytest.raises(ValueError):
        K.viterbi_route(1, 65, 8, 1)
    assert K.viterbi_route(2, 64, 64, 3) == ('lds', 0)
    route, nbytes = K.viterbi_route(64, 64, 4096, 1)
    assert route == 'workspace' and nbytes == 64 * 64 * 4096                       # one byte per (sequence, t, c)


def test_abi_symbols_are_declared():
    symbols = _lib.exported_symbols()
    header = open(os.path.join(ROOT, 'include', 'twog_gcn.h')).read()
    for name, n_args in (('twog_viterbi_limits', 2), ('twog_viterbi_workspace', 5), ('twog_viterbi_decode', 15),
                         ('twog_transition_counts', 9)):
        assert name in symbols and f'int {name}(' in header and len(_lib.SIGNATURES[name]) == n_args
    assert f'#define TWOG_VITERBI_CHUNK {_lib.VITERBI_CHUNK}\n' in header
