"""The numpy specification of the segmental decode (twog_segdecode), of the duration counts (twog_duration_counts) and of
the two model helpers `duration_log_probs` and `segment_transition_log_probs` of 2g-gcn_amd/postprocess.py. The reference
project decodes with a per-step argmax only, so this file is the contract.

One sequence = one (clip b, entity e). logp[t, c] is read at the model's own step rate, L is the decoded length, A the
fp32 (C, C) scores between consecutive segments (row = from, column = to), pi an optional fp32 (C,) initial score (all
zero when absent), dur fp32 (C, D): dur[c, l-1] is the score of a class-c segment that lasts l steps. All arithmetic is
fp32, each add rounds once in the order written, nothing is fused or reordered, and a candidate replaces the running
best only when it is strictly greater:

    e[0][c] = pi[c]
    e[t][c] = max over c' = 0..C-1 of (d[t-1][c'] + A[c',c]),  prev[t][c] = the smallest c' attaining it     (t >= 1)
    for l = 1 .. min(D, t+1), ascending:   acc_l = acc_(l-1) + logp[t-l+1,c]   (acc_0 = 0)
                                           cand_l = (e[t-l+1][c] + dur[c,l-1]) + acc_l
    d[t][c] = max over l of cand_l,        len[t][c] = the smallest l attaining it (the running best starts as cand_1)
    end:  c = the smallest class attaining max d[L-1][.];  score = that maximum;  t = L-1
    back: l = len[t][c];  y[t-l+1 .. t] = c;  stop if t-l+1 == 0;  c = prev[t-l+1][c];  t = t - l

The diagonal of A is used like any other entry. -inf in A, pi and dur is in contract; NaN is not.

lengths[b] is in model steps, clamped to [0, T]; None means T. A length of 0 gives label 0 everywhere and score 0.0.
Output: out[b, t', e] = y[min(t' // downsampling, L - 1)] for t' < T_out, int64 (bs, T_out, E); score fp32 (bs, E)."""
import math

import numpy as np

MAX_CLASSES, MAX_STEPS, MAX_DURATION = 64, 4096, 128

F = np.float32


def _backtrace(L, length, prev, c):
    y = np.zeros(L, dtype=np.int64)
    t = L - 1
    while True:
        l = int(length[t, c])
        y[t - l + 1:t + 1] = c
        if t - l + 1 == 0:
            return y
        c = int(prev[t - l + 1, c])
        t -= l


def decode_sequence(logp, A, dur, pi=None):
    """logp fp32 (L, C) with L >= 1 -> (y int64 (L,), score np.float32). Explicit np.float32 operations, strict '>'."""
    L, C = logp.shape
    logp, A, dur = np.asarray(logp, dtype=F), np.asarray(A, dtype=F), np.asarray(dur, dtype=F)
    D = dur.shape[1]
    pi = np.zeros(C, dtype=F) if pi is None else np.asarray(pi, dtype=F)
    e = np.empty((L, C), dtype=F)
    d = np.empty((L, C), dtype=F)
    prev = np.zeros((L, C), dtype=np.int64)
    length = np.zeros((L, C), dtype=np.int64)
    with np.errstate(invalid='ignore', over='ignore'):
        for t in range(L):
            for c in range(C):
                if t == 0:
                    e[0, c] = pi[c]
                else:
                    best, arg = F(d[t - 1, 0] + A[0, c]), 0
                    for cp in range(1, C):
                        cand = F(d[t - 1, cp] + A[cp, c])
                        if cand > best:
                            best, arg = cand, cp
                    e[t, c], prev[t, c] = best, arg
            for c in range(C):
                acc = F(0.0)
                best, arg = None, 0
                for l in range(1, min(D, t + 1) + 1):
                    acc = F(acc + logp[t - l + 1, c])
                    cand = F(F(e[t - l + 1, c] + dur[c, l - 1]) + acc)
                    if l == 1 or cand > best:
                        best, arg = cand, l
                d[t, c], length[t, c] = best, arg
    top, c_last = d[L - 1, 0], 0
    for c in range(1, C):
        if d[L - 1, c] > top:
            top, c_last = d[L - 1, c], c
    return _backtrace(L, length, prev, c_last), F(top)


def decode_sequence_fast(logp, A, dur, pi=None):
    """`decode_sequence` with the loops over c, c' and l as numpy array operations: the same fp32 adds in the same order
    (np.cumsum accumulates one element after the other in the array's dtype, starting here from the explicit acc_0 = 0),
    the same strict comparisons (np.argmax returns the first maximum), so the same bits. For the long sequences of the GPU
    tests."""
    L, C = logp.shape
    logp, A, dur = np.asarray(logp, dtype=F), np.asarray(A, dtype=F), np.asarray(dur, dtype=F)
    D = dur.shape[1]
    pi = np.zeros(C, dtype=F) if pi is None else np.asarray(pi, dtype=F)
    dur_t = np.ascontiguousarray(dur.T)                # (D, C): row l - 1
    e = np.empty((L, C), dtype=F)
    prev = np.zeros((L, C), dtype=np.int64)
    length = np.zeros((L, C), dtype=np.int64)
    cols = np.arange(C)
    zero = np.zeros((1, C), dtype=F)
    d = None
    with np.errstate(invalid='ignore', over='ignore'):
        for t in range(L):
            if t == 0:
                e[0] = pi
            else:
                cand = d[:, None] + A                  # cand[c', c], fp32
                arg = np.argmax(cand, axis=0)          # the first (smallest) c' among the maxima
                prev[t] = arg
                e[t] = cand[arg, cols]
            n = min(D, t + 1)
            back = slice(t, None, -1) if n == t + 1 else slice(t, t - n, -1)       # steps t, t-1, .., t-n+1: l = 1 .. n
            acc = np.cumsum(np.concatenate([zero, logp[back]]), axis=0, dtype=F)[1:]
            cand = (e[back] + dur_t[:n]) + acc
            arg = np.argmax(cand, axis=0)              # the first (smallest) l - 1 among the maxima
            length[t] = arg + 1
            d = cand[arg, cols]
    c_last = int(np.argmax(d))
    return _backtrace(L, length, prev, c_last), F(d[c_last])


def segment_labels(logp, A, dur, pi=None, lengths=None, downsampling=1, T_out=None, fast=False):
    """logp fp32 (bs, C, T, E) -> (labels int64 (bs, T_out, E), score fp32 (bs, E)): the contract in the module docstring.
    T_out defaults to T * downsampling."""
    logp = np.asarray(logp, dtype=F)
    bs, C, T, E = logp.shape
    ds = max(1, int(downsampling))
    T_out = T * ds if T_out is None else int(T_out)
    labels = np.zeros((bs, T_out, E), dtype=np.int64)
    score = np.zeros((bs, E), dtype=F)
    one = decode_sequence_fast if fast else decode_sequence
    for b in range(bs):
        L = T if lengths is None else min(max(int(lengths[b]), 0), T)
        if L == 0:
            continue
        steps = np.minimum(np.arange(T_out) // ds, L - 1)
        for e in range(E):
            y, s = one(logp[b, :, :L, e].T, A, dur, pi)
            score[b, e] = s
            labels[b, :, e] = y[steps]
    return labels, score


def duration_counts(targets, num_classes, max_duration, stride=1, ignore_index=-1):
    """int64 (C, D): the labels of a sequence are targets[b, k * stride, e], k = 0, 1, .. while k * stride < T_tgt; a maximal
    run of n equal labels c, each in [0, C) and != ignore_index, adds one to [c, min(n, D) - 1]. A label that does not count
    ends a run and starts none."""
    targets = np.asarray(targets)
    bs, T_tgt, E = targets.shape
    counts = np.zeros((num_classes, max_duration), dtype=np.int64)
    for b in range(bs):
        for e in range(E):
            current, n = None, 0
            k = 0
            while k * stride < T_tgt:
                y = int(targets[b, k * stride, e])
                kept = y != ignore_index and 0 <= y < num_classes
                if current is not None and (not kept or y != current):
                    counts[current, min(n, max_duration) - 1] += 1
                    current, n = None, 0
                if kept:
                    current, n = y, n + 1
                k += 1
            if current is not None:
                counts[current, min(n, max_duration) - 1] += 1
    return counts


def duration_log_probs(counts, smoothing=1.0, scheme='empirical'):
    """fp32 (C, D) in fp64, rounded once. empirical: log((n + s) / (row sum + D * s)), an unseen duration without smoothing
    is -inf. poisson: l * log(lambda) - lambda - lgamma(l + 1), lambda the mean run length of the row. A row without runs is
    all zeros."""
    counts = np.asarray(counts)
    C, D = counts.shape
    out = np.zeros((C, D), dtype=np.float64)
    for c in range(C):
        total = float(counts[c].sum())
        if total == 0.0:
            continue
        lam = sum(float(counts[c, l - 1]) * l for l in range(1, D + 1)) / total
        for l in range(1, D + 1):
            if scheme == 'empirical':
                num = float(counts[c, l - 1]) + float(smoothing)
                out[c, l - 1] = np.log(num / (total + D * float(smoothing))) if num > 0.0 else -np.inf
            else:
                out[c, l - 1] = l * np.log(lam) - lam - math.lgamma(l + 1.0)
    return out.astype(F)


def segment_transition_log_probs(counts, smoothing=1.0, self_transition=None):
    """fp32 (C, C): off the diagonal log((n + s) / (row sum without the diagonal + (C - 1) * s)) in fp64, rounded once (a row
    with a zero denominator is all zeros); the diagonal is self_transition, -inf when None."""
    counts = np.asarray(counts)
    C = counts.shape[0]
    out = np.zeros((C, C), dtype=np.float64)
    for a in range(C):
        den = float(sum(counts[a, z] for z in range(C) if z != a)) + (C - 1) * float(smoothing)
        for z in range(C):
            if z == a:
                out[a, z] = -np.inf if self_transition is None else float(self_transition)
            elif den > 0.0:
                num = float(counts[a, z]) + float(smoothing)
                out[a, z] = np.log(num / den) if num > 0.0 else -np.inf
    return out.astype(F)
