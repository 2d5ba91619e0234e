"""Inputs shared by tests/test_segdecode_cpu.py and tests/test_segdecode_gpu.py: the hand cases (each computed by hand
below), the dyadic tie cases, random models, the duration-count double loop and a decoder that returns the specification's
labels."""
from collections import namedtuple

import numpy as np
import torch

from tests import segdecode_ref as S

NEG = -np.inf
Hand = namedtuple('Hand', 'name logp A pi dur length path score')   # logp (L, C) of ONE sequence


def _f(rows):
    return np.asarray(rows, dtype=np.float32)


def hand_cases():
    cases = []
    # A minimum duration of 2 by dur[c][0] = -inf, no segment follows one of its own class, D = 3, L = 4. The per-step argmax
    # is 0 1 0 0. Every segment lasts 2 or 3 steps and 4 = 2 + 2 only (one segment of 4 is longer than D): classes (0, 1)
    # score (0 - 1) + (-1 - 1) = -3, classes (1, 0) score (-1 + 0) + (0 + 0) = -1.
    steps = _f([[0, -1], [-1, 0], [0, -1], [0, -1]])
    no_self = _f([[NEG, 0], [0, NEG]])
    cases.append(Hand('a minimum duration by -inf', steps, no_self, None, _f([[NEG, 0, 0], [NEG, 0, 0]]), 4, [1, 1, 0, 0], -1.0))
    # A run longer than D = 2: class 0 wins every one of 5 steps (class 1 costs 8 a step), so the run is composed of three
    # segments of class 0 (2 + 2 + 1 in some order) joined by A[0][0] = -0.5 twice: -1. Four or five segments pay more.
    cases.append(Hand('a run longer than D composed through A[c][c]', _f([[0, -8]] * 5), _f([[-0.5, -4], [-4, -0.5]]), None,
                      np.zeros((2, 2), dtype=np.float32), 5, [0, 0, 0, 0, 0], -1.0))
    # A tie between one segment of two steps and two segments of one step, D = 2, A[0][0] = -inf. d[0] = (-1, 0).
    # e[1][0] = max(-1 - inf, 0 - 1) = -1 from class 1. For class 0 at t = 1: cand_1 = (e[1][0] + 0) + 0 = -1 and
    # cand_2 = (e[0][0] + 0) + (0 - 1) = -1: not strictly greater, the shorter segment stays: path 1 0, not 0 0.
    # Class 1 at t = 1 scores -8 either way. Score -1.
    cases.append(Hand('a tie goes to the shorter segment', _f([[-1, 0], [0, -8]]), _f([[NEG, 0], [-1, 0]]), None,
                      np.zeros((2, 2), dtype=np.float32), 2, [1, 0], -1.0))
    # Everything zero: every segmentation scores 0; the end takes class 0, every length is 1, every prev is 0.
    cases.append(Hand('a tie goes to the smaller class', np.zeros((3, 3), dtype=np.float32), np.zeros((3, 3), dtype=np.float32),
                      None, np.zeros((3, 2), dtype=np.float32), 3, [0, 0, 0], 0.0))
    # Nothing is allowed: e, every candidate and d are -inf, so len = 1 and prev = 0 throughout and the end takes class 0.
    rng = np.random.default_rng(3)
    cases.append(Hand('an all -inf model', -rng.random((4, 3)).astype(np.float32), np.full((3, 3), NEG, dtype=np.float32),
                      np.full(3, NEG, dtype=np.float32), np.full((3, 2), NEG, dtype=np.float32), 4, [0, 0, 0, 0], NEG))
    # A one-step flicker (argmax 0 0 1 0 0) under dur = (-2, 0, 0): a one-step segment costs 2, transitions are free. Keeping
    # the flicker: emissions -1, durations 0 - 2 + 0: -3. Class 0 throughout in segments of 2 + 3: emissions -2, nothing else:
    # -2. Class 1 over steps 2..3: emissions -3 and a one-step segment of class 0 at the end, -2 more. So the flicker goes.
    flicker = _f([[0, -2], [0, -2], [-2, -1], [0, -2], [0, -2]])
    cases.append(Hand('a duration score removes a flicker', flicker, np.zeros((2, 2), dtype=np.float32), None,
                      _f([[-2, 0, 0], [-2, 0, 0]]), 5, [0, 0, 0, 0, 0], -2.0))
    # pi decides the first segment: flat emissions, no segment follows one of its own class, D = 2 = L. One segment of class c
    # scores pi[c] - 2; two segments pay a transition of -1 on top. pi = (-1, 0): class 1, -2.
    cases.append(Hand('pi decides the first segment', _f([[-1, -1], [-1, -1]]), _f([[NEG, -1], [-1, NEG]]), _f([-1, 0]),
                      np.zeros((2, 2), dtype=np.float32), 2, [1, 1], -2.0))
    return cases


def hand_batch(case, E=1):
    """A hand case as (logp (1, C, T, E), lengths (1,)); the entities repeat the sequence."""
    logp = np.ascontiguousarray(np.repeat(case.logp.T[None, :, :, None], E, axis=3))
    return logp, np.asarray([case.length], dtype=np.int64)


def eighths(rng, shape, lowest=4):
    """Multiples of 1/8 in [-lowest, 0] as fp32: every fp32 sum the decode makes of them is exact, so ties are real ties."""
    return (-rng.integers(0, 8 * lowest + 1, size=shape).astype(np.float64) / 8.0).astype(np.float32)


def dyadic_batch(seed, bs, C, T, E, D, forbid=0.0, no_self=False, lowest=4):
    """(logp, A, pi, dur) in eighths. `forbid`: the share of off-diagonal entries of A and of the entries of dur beyond
    l = 1 set to -inf (dur[:, 0] stays finite, and so does the diagonal of A unless `no_self`, so a finite path exists: with
    no_self the off-diagonal entries stay finite instead when C > 1)."""
    rng = np.random.default_rng(seed)
    logp, A, pi, dur = (eighths(rng, (bs, C, T, E), lowest), eighths(rng, (C, C), lowest), eighths(rng, (C,), lowest),
                        eighths(rng, (C, D), lowest))
    if forbid:
        mask = rng.random((C, C)) < forbid
        np.fill_diagonal(mask, False)
        if not (no_self and C > 1):
            A[mask] = NEG
        dmask = rng.random((C, D)) < forbid
        dmask[:, 0] = False
        dur[dmask] = NEG
    if no_self and C > 1:
        np.fill_diagonal(A, NEG)
    return logp, A, pi, dur


def random_batch(seed, bs, C, T, E, D):
    """(logp, A, pi, dur): fp32 log_softmax of normal scores over the class axis, a random A whose diagonal is unfavoured (a
    segment model), random pi, and duration scores that favour a class-dependent length, some durations forbidden."""
    rng = np.random.default_rng(seed)
    logp = torch.log_softmax(torch.from_numpy(rng.standard_normal((bs, C, T, E)).astype(np.float32)), 1).numpy()
    A = (rng.standard_normal((C, C)) - 1.0).astype(np.float32)
    A[np.arange(C), np.arange(C)] -= np.float32(1.5)
    mode = rng.integers(1, max(2, min(D, 12)) + 1, size=(C, 1))
    dur = (-0.3 * np.abs(np.arange(1, D + 1)[None, :] - mode) + 0.1 * rng.standard_normal((C, D))).astype(np.float32)
    forbidden = rng.random((C, D)) < 0.05
    forbidden[:, 0] = False
    dur[forbidden] = NEG
    return logp, A, rng.standard_normal(C).astype(np.float32), dur


def count_cases():
    """(name, targets (bs, T_tgt, E), C, D, ignore_index) for duration_counts; every one is run at strides 1, 2, 3."""
    rng = np.random.default_rng(11)
    C, D = 4, 5
    runs = np.repeat(rng.integers(0, C, size=(3, 8, 2)), 3, axis=1)[:, :19]          # T_tgt = 19: no multiple of 2 or 3
    inside = runs.copy()
    inside[0, 4:7, 0] = -1
    inside[1, 9, 1] = -1
    tail = runs.copy()
    tail[:, 15:, :] = -1
    entity = runs.copy()
    entity[:, :, 1] = -1
    beyond = runs.copy()
    beyond[2, 3:6, 0] = C          # labels >= C
    beyond[0, 10, 1] = C + 3
    beyond[1, 2, 0] = -7           # and below 0, not the ignore value
    other = runs.copy()
    other[1, 5:8, :] = 2           # ignore_index 2: a real class is ignored
    short = runs[:, :1].copy()     # one step: every run has length 1
    long_runs = np.repeat(rng.integers(0, C, size=(2, 3, 2)), 9, axis=1)             # runs of 9 and more: capped at D
    return [('runs', runs, C, D, -1), ('ignored inside', inside, C, D, -1), ('ignored tail', tail, C, D, -1),
            ('an all-ignored entity', entity, C, D, -1), ('labels outside', beyond, C, D, -1),
            ('a class ignored', other, C, D, 2), ('one step', short, C, D, -1), ('capped', long_runs, C, D, -1),
            ('D = 1', runs, C, 1, -1)]


def double_loop_counts(targets, C, D, stride, ignore_index):
    """The python double loop the counts are defined by, written independently of tests/segdecode_ref.py: the strided labels
    are cut into maximal runs with itertools.groupby."""
    import itertools
    counts = np.zeros((C, D), dtype=np.int64)
    bs, T_tgt, E = targets.shape
    for b in range(bs):
        for e in range(E):
            steps = [int(v) for v in targets[b, ::stride, e]]
            keyed = [(v if (v != ignore_index and 0 <= v < C) else None) for v in steps]
            for label, group in itertools.groupby(keyed):
                if label is not None:
                    counts[label, min(len(list(group)), D) - 1] += 1
    return counts


class SpecDecoder:
    """Stands where a `SegmentalDecoder` stands in an EvaluationAccumulator and returns the SPECIFICATION's labels
    (computed on the host, moved to the output's device): the accumulator's own kernels fed the specification's labels."""

    def __init__(self, transitions, durations, initial=None):
        self.A = np.asarray(transitions, dtype=np.float32)
        self.dur = np.asarray(durations, dtype=np.float32)
        self.pi = None if initial is None else np.asarray(initial, dtype=np.float32)
        self.num_classes = self.A.shape[0]

    def decode(self, output, downsampling, steps, lengths=None):
        labels, _ = S.segment_labels(output.cpu().numpy(), self.A, self.dur, self.pi,
                                     None if lengths is None else lengths.cpu().numpy(), downsampling, steps, fast=True)
        return torch.from_numpy(labels).to(output.device)
