"""CPU: the segmental edit score (twog_segment_edit). The reference project has no such metric, so the numpy specification
(tests/segment_edit_ref.py) is the contract: it is checked here against its hand-computed cases and against a memoised
recursive distance, its row-vectorised second form against the double loop, and then the host layer
(2g-gcn_amd/postprocess.py) through the kernel-interface test double. Integers are compared exactly and per-sequence
scores bit for bit: every operation behind them is an integer count or one correctly rounded fp64 operation."""
import functools
import math
import os

import numpy as np
import pytest
import torch

import twog_gcn_amd  # noqa: F401
from twog_gcn_amd import _lib
from twog_gcn_amd import kernels as twog_kernels
from twog_gcn_amd import postprocess as pp
from tests import evaluation_ref as E
from tests import segment_edit_ref as D
from tests.helpers import ROOT
from tests.segment_edit_fake import SegmentEditFakeKernels
from tests.segment_metrics_fake import SegmentMetricsFakeKernels
from tests.test_evaluation_cpu import OVERLAPS, cases
from tests.test_segment_metrics_cpu import run_accumulator, same_bits


@pytest.fixture()
def fake():
    backend = SegmentEditFakeKernels()
    twog_kernels._set_backend_for_tests(backend)
    yield backend
    twog_kernels._set_backend_for_tests(None)


def recursive_distance(a, b):
    """The textbook recursion on prefixes, memoised: a third statement of the distance."""
    a, b = tuple(a), tuple(b)

    @functools.lru_cache(maxsize=None)
    def d(i, j):
        if i == 0 or j == 0:
            return i + j
        return min(d(i - 1, j) + 1, d(i, j - 1) + 1, d(i - 1, j - 1) + (a[i - 1] != b[j - 1]))
    return d(len(a), len(b))


def random_pairs(count, seed, longest=14):
    rng = np.random.RandomState(seed)
    for _ in range(count):
        alphabet = rng.randint(1, 5)
        yield (rng.randint(0, alphabet, size=rng.randint(0, longest + 1)).tolist(),
               rng.randint(0, alphabet, size=rng.randint(0, longest + 1)).tolist())


def mean_tolerance(n_seq):
    """Two fp64 sums of at most n_seq scores in [0, 100] that differ only in their order: each is within
    (n_seq - 1) * 2^-53 * sum|v| of the exact sum, and the division by the valid count scales the sum and its error alike
    to at most 100; one more rounding for the division itself on either side."""
    return 2 * (n_seq + 1) * 2.0 ** -53 * 100.0


def test_distance_hand_cases_and_recursion():
    for a, b, want in D.LIST_CASES:
        assert D.levenshtein(a, b) == want == recursive_distance(a, b), (a, b)
    for a, b in random_pairs(300, seed=0):
        d = D.levenshtein(a, b)
        assert d == recursive_distance(a, b) == D.levenshtein(b, a), (a, b)
        assert abs(len(a) - len(b)) <= d <= max(len(a), len(b))


def test_row_vectorised_distance_equals_the_double_loop():
    for a, b, want in D.LIST_CASES:
        assert D.levenshtein_rows(a, b) == want, (a, b)
    for a, b in random_pairs(400, seed=1, longest=40):
        assert D.levenshtein_rows(a, b) == D.levenshtein(a, b), (a, b)
    wide = np.int64(1) << 32                       # labels that agree in their low 32 bits stay different
    assert D.levenshtein_rows([5, 5 + wide, 5], [5, 5, 5]) == D.levenshtein([5, 5 + wide, 5], [5, 5, 5]) == 1


@pytest.mark.parametrize('case', D.HAND_CASES, ids=[c[0] for c in D.HAND_CASES])
def test_specification_hand_cases(case):
    _, yt, yp, ignore, bg, (dist, n_true, n_pred, score, valid) = case
    for entity_minor in (False, True):
        t, p = np.array([yt], dtype=np.int64), np.array([yp], dtype=np.int64)
        if entity_minor:
            t, p = t.reshape(1, -1, 1), p.reshape(1, -1, 1)
        got = D.segment_edit(t, p, ignore, bg, entity_minor)
        assert [int(got[j][0]) for j in (1, 2, 3, 4)] == [dist, n_true, n_pred, valid]
        assert same_bits(got[0], [score]) and got[0].dtype == np.float64
        assert all(g.dtype == np.int32 for g in got[1:])
        rows = D.segment_edit(t, p, ignore, bg, entity_minor, distance=D.levenshtein_rows)
        assert all(np.array_equal(a, b) for a, b in zip(got, rows))


def test_specification_mean_and_layouts():
    yt, yp = label_batch(6, 40, 3, seed=3)
    yt[2] = -1
    sm = D.segment_edit(yt.transpose(0, 2, 1).reshape(-1, 40), yp.transpose(0, 2, 1).reshape(-1, 40), -1, None)
    em = D.segment_edit(yt, yp, -1, None, entity_minor=True)
    assert all(np.array_equal(a, b) for a, b in zip(sm, em))
    assert sm[4].tolist() == [1] * 6 + [0] * 3 + [1] * 9 and not sm[0][6:9].any() and not sm[2][6:9].any()
    assert D.mean_edit(sm[0], sm[4]) == sum(float(v) for v in sm[0][sm[4] != 0]) / 15.0
    assert math.isnan(D.mean_edit(np.zeros(3), np.zeros(3, dtype=np.int32)))


def test_packed_layout():
    for n_seq in (0, 1, 2, 5, 8):
        assert twog_kernels.segment_edit_words(n_seq) == 3 * n_seq           # n_seq fp64 and 4 * n_seq int32
        packed = torch.zeros(twog_kernels.segment_edit_words(n_seq), dtype=torch.int64)
        score, distance, n_true, n_pred, valid = twog_kernels.unpack_segment_edit(packed, n_seq)
        assert score.dtype == torch.float64 and score.shape == (n_seq,)
        assert all(v.dtype == torch.int32 and v.shape == (n_seq,) for v in (distance, n_true, n_pred, valid))
        base = packed.data_ptr()
        assert score.data_ptr() % 8 == 0 and (n_seq == 0 or score.data_ptr() == base)
        if n_seq:
            for j, v in enumerate((distance, n_true, n_pred, valid)):
                assert v.data_ptr() == base + 8 * n_seq + 4 * n_seq * j       # consecutive, none overlaps another
            score.fill_(1.5)
            for j, v in enumerate((distance, n_true, n_pred, valid)):
                v.fill_(j + 1)
            assert packed.view(torch.float64)[:n_seq].tolist() == [1.5] * n_seq
            assert packed[n_seq:].view(torch.int32).tolist() == [j + 1 for j in range(4) for _ in range(n_seq)]


def label_batch(bs, steps, E_, seed, classes=4):
    """int64 (bs, steps, E) targets and predictions in runs of 1 to 6 steps; the targets carry a ragged ignored tail and, in
    every second clip, an ignored stretch in the middle."""
    rng = np.random.RandomState(seed)
    runs = lambda: np.repeat(rng.randint(0, classes, size=steps), rng.randint(1, 7, size=steps))[:steps]
    yt = np.stack([np.stack([runs() for _ in range(E_)], 1) for _ in range(bs)]).astype(np.int64)
    yp = np.stack([np.stack([runs() for _ in range(E_)], 1) for _ in range(bs)]).astype(np.int64)
    yp[::3] = yt[::3]
    yp[::3, ::5] = (yp[::3, ::5] + 1) % classes
    for b in range(bs):
        yt[b, steps - rng.randint(0, steps // 3 + 1):] = -1
        if b % 2:
            yt[b, steps // 3:steps // 3 + rng.randint(1, 6), rng.randint(0, E_)] = -1
    return yt, yp


def test_edit_score_per_example_on_both_ranks_and_inputs(fake):
    yt, yp = label_batch(5, 30, 2, seed=4)
    seq_t, seq_p = yt.transpose(0, 2, 1).reshape(-1, 30), yp.transpose(0, 2, 1).reshape(-1, 30)
    for ignore, bg in ((-1.0, None), (None, None), (-1, 0), (None, 2)):
        fake.calls.clear()
        want = D.segment_edit(seq_t, seq_p, None if ignore is None else -1, bg)
        res = pp.edit_score_per_example(seq_t, torch.from_numpy(seq_p), ignore, bg_label=bg)     # numpy and torch input
        assert isinstance(res, pp.SegmentEdit) and res._fields == ('score', 'distance', 'n_true', 'n_pred', 'valid')
        assert fake.calls == ['segment_edit'] and res.score.dtype == torch.float64
        assert same_bits(res.score.numpy(), want[0])
        assert all(g.dtype == torch.int32 and np.array_equal(g.numpy(), w) for g, w in zip(res[1:], want[1:]))
        mean = pp.edit_score(torch.from_numpy(seq_t), seq_p, ignore_value=ignore, bg_label=bg)
        assert mean == D.mean_edit(want[0], want[4])
    # a rank-3 stack of sequence-major matrices is flattened like f1_at_k_per_example flattens it
    res = pp.edit_score_per_example(seq_t.reshape(2, 5, 30), torch.from_numpy(seq_p.reshape(2, 5, 30)), -1.0)
    assert same_bits(res.score.numpy(), D.segment_edit(seq_t, seq_p, -1, None)[0])
    # ignoring matters in these sequences, in the tail and in the middle, and so does the background label
    plain, ignored, bg = (D.segment_edit(seq_t, seq_p, i, b) for i, b in ((None, None), (-1, None), (-1, 0)))
    assert not np.array_equal(plain[1], ignored[1]) and not np.array_equal(ignored[2], bg[2])
    inside = [s for s in range(seq_t.shape[0])
              if np.flatnonzero(seq_t[s] == -1).min(initial=30) < np.flatnonzero(seq_t[s] != -1).max(initial=-1)]
    assert inside and (seq_t[:, -1] == -1).any() and ignored[4][inside].all()


def test_all_invalid_is_nan(fake):
    nothing = torch.full((3, 7), -1)
    pred = torch.arange(21).reshape(3, 7)
    res = pp.edit_score_per_example(nothing, pred, -1.0)
    assert not res.valid.any() and not res.score.any() and not res.distance.any() and not res.n_pred.any()
    assert math.isnan(pp.edit_score(nothing, pred, ignore_value=-1.0))
    assert math.isnan(pp.edit_score(torch.zeros(2, 4), torch.zeros(2, 4), bg_label=0))      # nothing but background
    got = pp.evaluate_edit_score({'sub-activity_recognition': nothing}, {'sub-activity_recognition': pred})
    assert list(got) == ['sub-activity_recognition'] and math.isnan(got['sub-activity_recognition'])


def test_evaluate_edit_score_one_launch_per_index(fake):
    yt3, yp3 = label_batch(4, 25, 3, seed=5)
    yt2, yp2 = label_batch(6, 25, 1, seed=6)
    targets = {'affordance_recognition': torch.from_numpy(yt3), 'sub-activity_recognition': torch.from_numpy(yt2[:, :, 0])}
    outputs = {'affordance_recognition': torch.from_numpy(yp3), 'sub-activity_recognition': torch.from_numpy(yp2[:, :, 0])}
    for bg in (None, 1):
        fake.calls.clear()
        fake.edit_args.clear()
        got = pp.evaluate_edit_score(targets, outputs, bg_label=bg)
        assert fake.calls == ['segment_edit'] * 2 and fake.edit_args == [(-1, bg, True)] * 2     # in place, entity-minor
        assert sorted(got) == sorted(targets)
        for index, (t, p) in {'affordance_recognition': (yt3, yp3), 'sub-activity_recognition': (yt2, yp2)}.items():
            want = D.segment_edit(t, p, -1, bg, entity_minor=True)
            assert got[index] == D.mean_edit(want[0], want[4]), (index, bg)
    with pytest.raises(ValueError, match='equal shape'):
        pp.evaluate_edit_score({'a': torch.zeros(2, 3)}, {'a': torch.zeros(2, 4)})


def accumulator_batches(seed=7, bs=4, C=5, T=9, E_=2, ds=2, T_tgt=17, n_batches=3):
    """[(logp, target)] whose second batch has no target step at all; the targets come in runs."""
    rng = np.random.RandomState(seed)
    batches = []
    for b in range(n_batches):
        logp = torch.log_softmax(torch.from_numpy(rng.randn(bs, C, T, E_).astype(np.float32)), 1).numpy()
        tgt = np.repeat(rng.randint(0, C, size=(bs, T_tgt, E_)), 3, axis=1)[:, :T_tgt].astype(np.int64)
        tgt[rng.rand(bs, T_tgt, E_) < 0.1] = -1
        tgt[0, T_tgt - 4:] = -1
        if b == 1:
            tgt[:] = -1
        batches.append((logp, tgt))
    return batches, ds


def reference_edit_mean(batches, ds, bg_label=None, step_index=None):
    """(the specification's mean over all the sequences of all the batches, their number)."""
    scores, valids = [], []
    for logp, tgt in batches:
        _, _, labels, kept = E.eval_update(logp, ds, tgt, step_index)
        score, _, _, _, valid = D.segment_edit(kept, labels, -1, bg_label, entity_minor=True)
        scores.append(score)
        valids.append(valid)
    scores, valids = np.concatenate(scores), np.concatenate(valids)
    return D.mean_edit(scores, valids), scores.size, valids


@pytest.mark.parametrize('bg_label', (None, 0))
def test_accumulator_with_edit_matches_the_specification_mean(fake, bg_label):
    batches, ds = accumulator_batches()
    acc = pp.EvaluationAccumulator(['a', 'b'], 5, downsampling=ds, overlaps=OVERLAPS, f1_route='workgroup', edit=True,
                                   bg_label=bg_label)
    plain = pp.EvaluationAccumulator(['a', 'b'], 5, downsampling=ds, overlaps=OVERLAPS, f1_route='workgroup')
    for logp, tgt in batches:
        fake.calls.clear()
        fake.edit_args.clear()
        acc.update([torch.from_numpy(logp)] * 2, [torch.from_numpy(tgt)] * 2)
        assert fake.calls == ['eval_update', 'segment_edit', 'segment_f1_accumulate', 'segment_f1', 'segment_f1_accumulate'] * 2
        assert fake.edit_args == [(-1, bg_label, True)] * 2                   # on the labels eval_update wrote, in place
        plain.update([torch.from_numpy(logp)] * 2, [torch.from_numpy(tgt)] * 2)
    want, n_seq, valids = reference_edit_mean(batches, ds, bg_label)
    assert 0 < valids.sum() < n_seq and not valids[n_seq // 3:2 * n_seq // 3].any()               # the all-invalid batch
    n_words = sum(c * c + 2 for c in acc.num_classes) + 2 * len(OVERLAPS) * 2
    assert plain._state.numel() == n_words and acc._state.numel() == n_words + 2 * 2
    assert torch.equal(acc._state[:n_words], plain._state)                    # the new words lie behind the old ones
    assert acc._floats.numel() == 2 * len(OVERLAPS) * 2 + 4 and acc._floats.data_ptr() == plain._floats.data_ptr() - \
        plain._state.data_ptr() + acc._state.data_ptr()                       # inside _floats: all_reduce covers them
    res, res_plain = acc.result(), plain.result()
    for name in ('a', 'b'):
        assert abs(res[name]['edit'] - want) <= mean_tolerance(n_seq), (name, res[name]['edit'], want)
        assert sorted(res[name]) == sorted(list(res_plain[name]) + ['edit'])
        assert res[name]['f1@k'] == res_plain[name]['f1@k']
    acc.all_reduce()                                                          # no process group: the only rank


def test_accumulator_with_edit_and_nothing_valid_is_nan(fake):
    batches, ds = accumulator_batches()
    logp, tgt = batches[1]
    acc = pp.EvaluationAccumulator(['a'], 5, downsampling=ds, overlaps=(), edit=True)
    acc.update([torch.from_numpy(logp)], [torch.from_numpy(tgt)])
    assert fake.calls == ['eval_update', 'segment_edit', 'segment_f1_accumulate']
    res = acc.result()['a']
    assert math.isnan(res['edit']) and res['f1@k'] == {}


def test_accumulator_with_a_step_index(fake):
    batches, ds = accumulator_batches(n_batches=1)
    index = pp.segment_step_index([[0, 3, 4, 9], [1, 2], [], [5, 6, 7, 8, 16]])
    acc = pp.EvaluationAccumulator(['a'], 5, downsampling=ds, edit=True)
    acc.update([torch.from_numpy(batches[0][0])], [torch.from_numpy(batches[0][1])], step_index=index)
    want, n_seq, _ = reference_edit_mean(batches, ds, step_index=index.numpy())
    assert abs(acc.result()['a']['edit'] - want) <= mean_tolerance(n_seq)


def test_accumulator_without_edit_is_what_it_was(fake):
    case = next(c for c in cases() if c.name == 'cad120')
    n_words = sum(h[1] * h[1] + 2 for h in case.heads) + 2 * len(OVERLAPS) * len(case.heads)     # _allocate's formula
    for kwargs, per_output in (({}, ['eval_update'] + ['f1_at_k'] * len(OVERLAPS)),
                               ({'f1_route': 'workgroup'}, ['eval_update', 'segment_f1', 'segment_f1_accumulate'])):
        states = []
        for extra in ({}, {'edit': False}, {'edit': False, 'bg_label': 0}):
            fake.calls.clear()
            acc = run_accumulator(case, 'cpu', overlaps=OVERLAPS, **kwargs, **extra)
            assert acc.edit is False and fake.calls == per_output * (len(case.heads) * len(case.batches))
            assert acc._state.numel() == n_words and acc._floats.numel() == 2 * len(OVERLAPS) * len(case.heads)
            res = acc.result()
            assert all(sorted(r) == ['confusion', 'f1@k', 'macro', 'micro', 'report'] and 'edit' not in r for r in res.values())
            states.append(acc._state.clone())
        # and on the double that has no edit entry point at all: the same state, bit for bit
        twog_kernels._set_backend_for_tests(SegmentMetricsFakeKernels())
        assert not hasattr(twog_kernels.get_kernels(), 'segment_edit')
        states.append(run_accumulator(case, 'cpu', overlaps=OVERLAPS, **kwargs)._state.clone())
        twog_kernels._set_backend_for_tests(fake)
        assert all(torch.equal(states[0], s) for s in states[1:])


def test_a_batch_over_the_limit_is_a_value_error(fake):
    assert fake.segment_edit_limits() == 4096 == fake.segment_f1_limits()[0]
    yt = torch.zeros(2, 4097, dtype=torch.int64)
    with pytest.raises(RuntimeError, match='twog_segment_edit failed with code -2'):          # the entry point refuses
        pp.edit_score_per_example(yt, yt)
    assert pp.edit_score_per_example(yt[:, :4096], yt[:, :4096]).valid.all()
    fake.EDIT_MAX_STEPS = 8
    case = next(c for c in cases() if c.name == 'plain')
    assert case.want(0, 'labels').shape[1] > 8
    for route in ('thread', 'workgroup'):
        fake.calls.clear()
        with pytest.raises(ValueError, match='up to 8 steps'):
            run_accumulator(case, 'cpu', overlaps=OVERLAPS, f1_route=route, edit=True)
        assert fake.calls == []                                               # raised in update, before anything was added
    fake.calls.clear()
    run_accumulator(case, 'cpu', overlaps=OVERLAPS, f1_route='workgroup')     # without the metric the limit is not asked
    assert 'segment_edit' not in fake.calls and fake.calls[0] == 'eval_update'
    # the step index decides how long the batch is
    fake.EDIT_MAX_STEPS = 3
    batches, ds = accumulator_batches(n_batches=1)
    acc = pp.EvaluationAccumulator(['a'], 5, downsampling=ds, edit=True)
    args = [torch.from_numpy(batches[0][0])], [torch.from_numpy(batches[0][1])]
    acc.update(*args, step_index=pp.segment_step_index([[0, 3, 4], [1, 2], [], [5]]))
    with pytest.raises(ValueError, match='up to 3 steps'):
        acc.update(*args, step_index=pp.segment_step_index([[0, 3, 4, 9], [1, 2], [], [5]]))


def test_abi_symbols_are_declared():
    symbols = _lib.exported_symbols()
    header = open(os.path.join(ROOT, 'include', 'twog_gcn.h')).read()
    for name in ('twog_segment_edit', 'twog_segment_edit_limits'):
        assert name in symbols and f'int {name}(' in header
    assert len(_lib.SIGNATURES['twog_segment_edit']) == 15 and len(_lib.SIGNATURES['twog_segment_edit_limits']) == 1
