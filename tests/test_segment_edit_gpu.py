"""GPU: twog_segment_edit through the C ABI against the numpy specification (tests/segment_edit_ref.py) -- its hand cases,
seeded random sequences in both label layouts at every length where the kernel changes what it does (one wave, one
trip of the workgroup, more, the longest it takes), tables far from square, labels that differ only above bit 32, the
background rule, the refusals, guard words, run-to-run identity -- and EvaluationAccumulator(edit=True) on the device.
Everything is compared exactly: integers with array_equal, the score bit for bit. The shapes are the smallest at which
the table can go wrong, not evaluation shapes."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import twog_gcn_amd  # noqa: F401
from twog_gcn_amd import kernels as twog_kernels
from twog_gcn_amd import postprocess as pp
from tests import evaluation_ref as E
from tests import segment_edit_ref as D
from tests.test_evaluation_cpu import OVERLAPS
from tests.test_segment_edit_cpu import mean_tolerance
from tests.test_segment_metrics_cpu import same_bits
from tests.test_segment_metrics_gpu import DEV, K, accumulator_case, dev, entity_minor

pytestmark = pytest.mark.gpu
STEPS = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 4096)
N_SEQ = 6            # a multiple of 3, and the most the longest case may have


def host(res):
    """(score, distance, n_true, n_pred, valid) of K().segment_edit as numpy arrays."""
    return [t.cpu().numpy() for t in res[:5]]


def check_against(got, want, what):
    score, distance, n_true, n_pred, valid = got
    assert np.array_equal(valid, want[4]), what
    assert np.array_equal(n_true, want[2]) and np.array_equal(n_pred, want[3]), what
    assert np.array_equal(distance, want[1]), (what, distance, want[1])
    assert score.dtype == np.float64 and same_bits(score, want[0]), what
    assert all(g.dtype == np.int32 for g in got[1:])


def specification(yt, yp, ignore, bg):
    """The double loop where it is quick, its row-vectorised form (proven equal in tests/test_segment_edit_cpu.py) beyond."""
    distance = D.levenshtein if yt.shape[1] <= 65 else D.levenshtein_rows
    return D.segment_edit(yt, yp, ignore, bg, distance=distance)


def with_segments(rng, n_steps, m):
    """n_steps labels in exactly m runs; neighbouring runs differ, and with 7 labels many cells of the table match."""
    starts = np.sort(rng.choice(np.arange(1, n_steps), size=m - 1, replace=False)) if m > 1 else np.zeros(0, dtype=np.int64)
    labels = np.cumsum(rng.randint(1, 6, size=m)) % 7
    return labels[np.searchsorted(starts, np.arange(n_steps), side='right')].astype(np.int64)


def random_sequences(n_steps, regime, seed):
    """N_SEQ target and prediction sequences. 'runs': 2 or 5 classes in long runs, few segments. 'flicker': a new label at
    every step. Sequences 0 and 1 keep every step; the others have a ragged ignored tail, 3 and 4 ignored steps in the
    middle as well, and 5 is ignored altogether."""
    rng = np.random.RandomState(seed)
    if regime == 'runs':
        def runs():
            classes = (2, 5)[rng.randint(2)]
            return np.repeat(rng.randint(0, classes, size=n_steps), rng.randint(1, 40, size=n_steps))[:n_steps]
        yt = np.stack([runs() for _ in range(N_SEQ)]).astype(np.int64)
        yp = np.stack([runs() for _ in range(N_SEQ)]).astype(np.int64)
        yp[::2] = yt[::2]
        yp[::2, ::11] = (yp[::2, ::11] + 1) % 5                  # the prediction flickers
    else:
        yt = np.stack([with_segments(rng, n_steps, n_steps) for _ in range(N_SEQ)])
        yp = np.stack([with_segments(rng, n_steps, n_steps) for _ in range(N_SEQ)])
    for s in range(2, N_SEQ):
        yt[s, n_steps - rng.randint(0, n_steps // 2 + 1):] = -1
    for s in (3, 4):
        yt[s, rng.rand(n_steps) < 0.15] = -1
    yt[5] = -1
    return yt, yp


@pytest.mark.parametrize('case', range(len(D.HAND_CASES)), ids=[c[0] for c in D.HAND_CASES])
def test_hand_cases_through_the_abi(case):
    _, yt, yp, ignore, bg, (dist, n_true, n_pred, score, valid) = D.HAND_CASES[case]
    t, p = np.array([yt, yt], dtype=np.int64), np.array([yp, yp], dtype=np.int64)
    for got in (host(K().segment_edit(dev(t), dev(p), ignore, bg)),
                host(K().segment_edit(dev(entity_minor(t, 2)), dev(entity_minor(p, 2)), ignore, bg, entity_minor=True))):
        assert [g.tolist() for g in got[1:]] == [[dist] * 2, [n_true] * 2, [n_pred] * 2, [valid] * 2]
        assert same_bits(got[0], [score, score])
    res = pp.edit_score_per_example(dev(t), dev(p), ignore, bg_label=bg)          # the host layer on the device
    assert res.score.device.type == 'cuda' and same_bits(res.score.cpu().numpy(), [score, score])
    mean = pp.edit_score(dev(t), dev(p), ignore_value=ignore, bg_label=bg)
    assert (mean == score) if valid else math.isnan(mean)


@pytest.mark.parametrize('regime', ('runs', 'flicker'))
@pytest.mark.parametrize('n_steps', STEPS)
def test_random_sequences_vs_specification(n_steps, regime):
    max_steps = K().segment_edit_limits()
    assert max_steps == 4096 == K().segment_f1_limits()[0] and max(STEPS) == max_steps
    yt, yp = random_sequences(n_steps, regime, seed=n_steps)
    for bg in (None, 1) if regime == 'runs' else (None,):
        want = specification(yt, yp, -1, bg)
        assert want[4][5] == 0 and (bg is not None or want[4][:3].all())
        if regime == 'flicker':                 # the whole table: diagonals up to n_steps + 1 cells, every buffer phase
            assert want[2][:2].tolist() == want[3][:2].tolist() == [n_steps] * 2
        check_against(host(K().segment_edit(dev(yt), dev(yp), -1, bg)), want, (n_steps, regime, bg, 'sequence-major'))
        for E_ in (1, 3):
            got = K().segment_edit(dev(entity_minor(yt, E_)), dev(entity_minor(yp, E_)), -1, bg, entity_minor=True)
            check_against(host(got), want, (n_steps, regime, bg, 'entity-minor', E_))
    if n_steps <= 257:                          # no ignore value: -1 is a label like any other
        want = specification(yt, yp, None, None)
        assert want[4].all()
        check_against(host(K().segment_edit(dev(yt), dev(yp))), want, (n_steps, regime, 'no ignore value'))


def test_lopsided_tables():
    rng = np.random.RandomState(11)
    for n_steps, shapes in ((4096, ((1, 4096), (4096, 1), (2, 4096), (4096, 3))),          # m + n odd, odd, even, odd
                            (257, ((255, 257), (257, 255), (255, 256), (1, 257), (256, 256)))):
        yt = np.stack([with_segments(rng, n_steps, m) for m, _ in shapes])
        yp = np.stack([with_segments(rng, n_steps, n) for _, n in shapes])
        want = D.segment_edit(yt, yp, None, None, distance=D.levenshtein_rows)
        assert list(zip(want[2].tolist(), want[3].tolist())) == list(shapes)
        check_against(host(K().segment_edit(dev(yt), dev(yp))), want, n_steps)


def test_labels_are_compared_as_int64():
    yt, yp = random_sequences(65, 'flicker', seed=3)
    yt, yp = yt[:5], yp[:5]                                      # without the sequence that is ignored altogether
    high = np.int64(1) << 32
    wide = lambda y: y * high + 7 - (np.int64(1) << 50)          # negative, different above bit 32 only
    want = specification(wide(yt), wide(yp), None, None)
    assert np.array_equal(want[1], specification(yt, yp, None, None)[1]) and want[1].min() > 0
    check_against(host(K().segment_edit(dev(wide(yt)), dev(wide(yp)))), want, 'wide')
    # equal low words: a kernel that compared 32 bits would find distance 0
    same_low = yt + high * (np.arange(65) % 3 == 0)
    want = specification(yt, same_low, -1, None)
    assert (want[1][:2] > 0).all() and not specification(yt, yt, -1, None)[1].any()
    check_against(host(K().segment_edit(dev(yt), dev(same_low), -1)), want, 'equal low words')
    # negative labels that are not the ignore value, and an ignore value that is not -1
    neg = np.where(yt == -1, -1, -2 - yt)
    want = specification(neg, -2 - yp, -1, -3)
    check_against(host(K().segment_edit(dev(neg), dev(-2 - yp), -1, -3)), want, 'negative')
    want = specification(neg, -2 - yp, -4, None)
    assert not np.array_equal(want[2], specification(neg, -2 - yp, None, None)[2])
    check_against(host(K().segment_edit(dev(neg), dev(-2 - yp), -4)), want, 'ignore -4')


def raw_call(yt, yp, n_seq, n_steps, entities, outputs):
    """twog_segment_edit itself, on the outputs the caller laid out."""
    k = K()
    code = k.lib.twog_segment_edit(yt.data_ptr(), yp.data_ptr(), n_seq, n_steps, entities, -1, 1, 0, 0,
                                   *[o.data_ptr() for o in outputs], k._stream())
    torch.cuda.synchronize()
    return code


def guarded_outputs(n_seq):
    """One buffer of 0x5a bytes and five outputs inside it, each with 64 guard bytes on either side."""
    sizes = [8 * n_seq] + [4 * n_seq] * 4
    span = [(s + 63) // 64 * 64 for s in sizes]
    buf = torch.full((64 * 6 + sum(span),), 0x5a, dtype=torch.uint8, device=DEV)
    outputs, keep, at = [], torch.ones(buf.numel(), dtype=torch.bool), 64
    for size, sp, dtype in zip(sizes, span, [torch.float64] + [torch.int32] * 4):
        outputs.append(buf[at:at + size].view(dtype))
        keep[at:at + size] = False
        at += sp + 64
    return buf, outputs, keep.to(DEV)


def test_refusals_and_guard_words():
    yt, yp = random_sequences(65, 'flicker', seed=5)
    t, p = dev(yt), dev(yp)
    with pytest.raises(RuntimeError, match='twog_segment_edit failed with code -2'):
        K().segment_edit(torch.zeros(2, 4097, dtype=torch.int64, device=DEV), torch.zeros(2, 4097, dtype=torch.int64, device=DEV))
    buf, outputs, keep = guarded_outputs(N_SEQ)
    before = buf.clone()
    assert raw_call(t, p, N_SEQ, 4097, 0, outputs) == -2
    assert raw_call(t, p, 5, 65, 3, outputs) == -1               # n_seq is no multiple of entities
    assert raw_call(t, p, -1, 65, 0, outputs) == -1 and raw_call(t, p, N_SEQ, -1, 0, outputs) == -1
    assert raw_call(t, p, N_SEQ, 65, -1, outputs) == -1
    assert raw_call(t, p, 0, 65, 0, outputs) == 0                # nothing to do, nothing launched
    assert torch.equal(buf, before)                              # and none of them wrote anything
    # a launch writes its five outputs and nothing around them
    for entities, (a, b) in ((0, (t, p)), (3, (dev(entity_minor(yt, 3)), dev(entity_minor(yp, 3))))):
        buf.copy_(before)
        assert raw_call(a, b, N_SEQ, 65, entities, outputs) == 0
        assert torch.equal(buf[keep], before[keep])
        check_against([o.cpu().numpy() for o in outputs], specification(yt, yp, -1, None), ('guarded', entities))
    # no steps at all: every sequence is empty, all-zero rows
    empty = torch.zeros(N_SEQ, 0, dtype=torch.int64, device=DEV)
    got = host(K().segment_edit(empty, empty, -1))
    assert all(g.shape == (N_SEQ,) and not g.any() for g in got)


def test_repeated_runs_are_bit_identical():
    yt, yp = random_sequences(1000, 'flicker', seed=8)
    t, p = dev(entity_minor(yt, 3)), dev(entity_minor(yp, 3))
    first = None
    for _ in range(3):
        packed = K().segment_edit(t, p, -1, 2, entity_minor=True)[5].cpu().numpy().tobytes()
        first = packed if first is None else first
        assert packed == first


def test_accumulator_with_edit_does_not_synchronise_and_matches_the_specification_mean():
    logp, tgt, index, outs, tgts, si = accumulator_case()
    acc = pp.EvaluationAccumulator(['a', 'b'], 13, downsampling=3, overlaps=OVERLAPS, f1_route='workgroup', edit=True)
    bg = pp.EvaluationAccumulator(['a', 'b'], 13, downsampling=3, overlaps=(), edit=True, bg_label=0)
    plain = pp.EvaluationAccumulator(['a', 'b'], 13, downsampling=3, overlaps=OVERLAPS, f1_route='workgroup')
    for a in (acc, bg):
        a.update(outs, tgts, si)                                  # allocation and library load happen here
    probe = torch.ones(1, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(RuntimeError):                         # the mode is live in this build
            probe.item()
        for a in (acc, bg):
            a.update(outs, tgts, si)
            a.update(outs, tgts)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    for step_index in (si, si, None):
        plain.update(outs, tgts, step_index)
    scores = {None: [], 0: []}
    valids = {None: [], 0: []}
    for idx in (index, index, None):
        _, _, labels, kept = E.eval_update(logp, 3, tgt, idx)
        for bg_label in (None, 0):
            score, _, _, _, valid = D.segment_edit(kept, labels, -1, bg_label, entity_minor=True)
            scores[bg_label].append(score)
            valids[bg_label].append(valid)
    res, res_bg, res_plain = acc.result(), bg.result(), plain.result()
    for got, bg_label in ((res, None), (res_bg, 0)):
        s, v = np.concatenate(scores[bg_label]), np.concatenate(valids[bg_label])
        want = D.mean_edit(s, v)
        assert 0 < v.sum() < v.size and 0.0 < want < 100.0
        for name in ('a', 'b'):
            assert abs(got[name]['edit'] - want) <= mean_tolerance(s.size), (name, bg_label, got[name]['edit'], want)
    assert res['a']['edit'] != res_bg['a']['edit']
    # the other numbers are those of an accumulator without the metric, whose result has no such key
    n_words = plain._state.numel()
    assert acc._state.numel() == n_words + 4 and torch.equal(acc._state[:n_words], plain._state)
    for name in ('a', 'b'):
        assert 'edit' not in res_plain[name] and sorted(res[name]) == sorted(list(res_plain[name]) + ['edit'])
    with pytest.raises(ValueError, match='up to 4096 steps'):
        acc.update([torch.zeros(1, 13, 2, 2, device=DEV)] * 2, [torch.zeros(1, 4097, 2, dtype=torch.int64, device=DEV)] * 2)
    assert torch.equal(acc._state[:n_words], plain._state)
