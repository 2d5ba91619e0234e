"""Inputs shared by tests/test_viterbi_cpu.py and tests/test_viterbi_gpu.py: the hand cases (each computed by hand below),
the dyadic tie cases, the transition-count cases and a decoder that returns the specification's labels."""
from collections import namedtuple

import numpy as np
import torch

from tests import viterbi_ref as V

NEG = -np.inf
Hand = namedtuple('Hand', 'name logp A pi length path score')   # logp (L_total, C) of ONE sequence, path over `length` steps


def _f(rows):
    return np.asarray(rows, dtype=np.float32)


def hand_cases():
    cases = []
    # A one-step flicker. Per-step argmax: 0 0 1 0 0. With a switch penalty of 1 the path 0 0 1 0 0 scores
    # 0 + 0 - 1 + 0 + 0 - 2 * 1 = -3 and the constant path 0 0 0 0 0 scores 0 + 0 - 2 + 0 + 0 = -2: the flicker goes.
    flicker = _f([[0, -2], [0, -2], [-2, -1], [0, -2], [0, -2]])
    cases.append(Hand('switch penalty removes a flicker', flicker, V.switch_penalty(2, 1.0), None, 5, [0, 0, 0, 0, 0], -2.0))
    # With a penalty of 0.25 the flicker path scores -1 - 2 * 0.25 = -1.5 > -2: it stays.
    cases.append(Hand('a small penalty keeps it', flicker, V.switch_penalty(2, 0.25), None, 5, [0, 0, 1, 0, 0], -1.5))
    # A forbidden transition 0 -> 1. Freely the best path is 0 0 1 (0 - 1 + 0 = -1), which uses 0 -> 1 at the last step.
    # Paths that end in 1 must now come from 1 or 2: 0 2 1 scores 0 - 3 + 0 = -3; 1 1 1 and 2 1 1 score -8 - 2 + 0 = -10;
    # 1 2 1 and 2 2 1 score -8 - 3 = -11. Paths that end in 0 or 2 pay -8 at the last step: at best 0 0 0 = 0 - 1 - 8 = -9.
    # So the detour through 2 wins with -3.
    detour = _f([[0, -8, -8], [-1, -2, -3], [-8, 0, -8]])
    forbid = np.zeros((3, 3), dtype=np.float32)
    forbid[0, 1] = NEG
    cases.append(Hand('a forbidden transition forces a detour', detour, forbid, None, 3, [0, 2, 1], -3.0))
    cases.append(Hand('the same steps without it', detour, np.zeros((3, 3), dtype=np.float32), None, 3, [0, 0, 1], -1.0))
    # L = 1: no transition is read; classes 1 and 2 tie at -1, the smaller wins.
    cases.append(Hand('one step', _f([[-2, -1, -1], [0, -8, -8]]), forbid, None, 1, [1], -1.0))
    # L = 0: label 0 everywhere, score 0.0.
    cases.append(Hand('no step', _f([[-2, -1, -1], [0, -8, -8]]), forbid, None, 0, [], 0.0))
    # pi decides the first label. Every logp is -1 and a switch costs 1. Without pi: d[0] = (-1, -1); d[1][0] = max(-1 + 0,
    # -1 - 1) - 1 = -2 from 0, d[1][1] = max(-1 - 1, -1 + 0) - 1 = -2 from 1; the tie at the last step takes 0: path 0 0.
    flat = _f([[-1, -1], [-1, -1]])
    cases.append(Hand('flat scores tie towards 0', flat, V.switch_penalty(2, 1.0), None, 2, [0, 0], -2.0))
    # With pi = (-1, 0): d[0] = (-2, -1); d[1][0] = max(-2 + 0, -1 - 1) - 1 = -3, d[1][1] = max(-2 - 1, -1 + 0) - 1 = -2 from 1:
    # path 1 1, score -2.
    cases.append(Hand('pi decides the first label', flat, V.switch_penalty(2, 1.0), _f([-1, 0]), 2, [1, 1], -2.0))
    return cases


def hand_batch(case, E=1):
    """A hand case as (logp (1, C, T, E), lengths (1,)); the entities repeat the sequence."""
    logp = np.ascontiguousarray(np.repeat(case.logp.T[None, :, :, None], E, axis=3))
    return logp, np.asarray([case.length], dtype=np.int64)


def dyadic_batch(seed, bs, C, T, E, forbid=0.0):
    """(logp, A, pi) of multiples of 2^-7 in [-8, 0]: ties are frequent and every fp32 sum is exact. `forbid`: the share
    of off-diagonal entries of A set to -inf (the diagonal stays finite, so a finite path always exists)."""
    rng = np.random.default_rng(seed)
    logp, A, pi = V.dyadic(rng, (bs, C, T, E)), V.dyadic(rng, (C, C)), V.dyadic(rng, (C,))
    if forbid:
        mask = rng.random((C, C)) < forbid
        np.fill_diagonal(mask, False)
        A[mask] = NEG
    return logp, A, pi


def random_batch(seed, bs, C, T, E):
    """(logp, A, pi): fp32 log_softmax of normal scores over the class axis, a random A with a favoured diagonal, random pi."""
    rng = np.random.default_rng(seed)
    logp = torch.log_softmax(torch.from_numpy(rng.standard_normal((bs, C, T, E)).astype(np.float32)), 1).numpy()
    A = (rng.standard_normal((C, C)) - 1.0).astype(np.float32)
    A[np.arange(C), np.arange(C)] += np.float32(1.5)
    return logp, A, rng.standard_normal(C).astype(np.float32)


def count_cases():
    """(name, targets (bs, T_tgt, E), C, ignore_index) for transition_counts; every one is run at strides 1, 2, 3."""
    rng = np.random.default_rng(11)
    C = 4
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
    short = runs[:, :1].copy()     # one step: no pair at all
    return [('runs', runs, C, -1), ('ignored inside', inside, C, -1), ('ignored tail', tail, C, -1),
            ('an all-ignored entity', entity, C, -1), ('labels outside', beyond, C, -1), ('a class ignored', other, C, 2),
            ('one step', short, C, -1)]


def double_loop_counts(targets, C, stride, ignore_index):
    """The python double loop the counts are defined by, written independently of tests/viterbi_ref.py."""
    counts = np.zeros((C, C), dtype=np.int64)
    bs, T_tgt, E = targets.shape
    for b in range(bs):
        for e in range(E):
            steps = [int(v) for v in targets[b, ::stride, e]]
            for a, z in zip(steps[:-1], steps[1:]):
                if a == ignore_index or z == ignore_index or not (0 <= a < C) or not (0 <= z < C):
                    continue
                counts[a, z] += 1
    return counts


class SpecDecoder:
    """Stands where a `ViterbiDecoder` stands in an EvaluationAccumulator and returns the SPECIFICATION's labels (computed
    on the host, moved to the output's device): the accumulator's own kernels fed the specification's labels."""

    def __init__(self, transitions, initial=None):
        self.A = np.asarray(transitions, dtype=np.float32)
        self.pi = None if initial is None else np.asarray(initial, dtype=np.float32)
        self.num_classes = self.A.shape[0]

    def decode(self, output, downsampling, steps, lengths=None):
        labels, _ = V.viterbi_labels(output.cpu().numpy(), self.A, self.pi, None if lengths is None else lengths.cpu().numpy(),
                                     downsampling, steps, fast=True)
        return torch.from_numpy(labels).to(output.device)


def accumulator_batches(seed=5, bs=4, C=5, T=9, E=2, ds=2, T_tgt=17, n_batches=2, dyadic=False):
    """[(logp, target, lengths)]: targets in runs with ignored steps, ragged lengths in the second batch."""
    rng = np.random.default_rng(seed)
    batches = []
    for n in range(n_batches):
        logp = dyadic_batch(seed + n, bs, C, T, E)[0] if dyadic else random_batch(seed + n, bs, C, T, E)[0]
        tgt = np.repeat(rng.integers(0, C, size=(bs, T_tgt, E)), 3, axis=1)[:, :T_tgt].astype(np.int64)
        tgt[rng.random((bs, T_tgt, E)) < 0.1] = -1
        tgt[0, T_tgt - 4:] = -1
        lengths = None if n == 0 else np.asarray([T, 1, T - 2, 0][:bs] + [T] * max(0, bs - 4), dtype=np.int64)
        batches.append((logp, tgt, lengths))
    return batches
