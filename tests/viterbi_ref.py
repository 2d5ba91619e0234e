"""The numpy specification of the Viterbi decode (twog_viterbi_decode), of the transition counts (twog_transition_counts)
and of the two transition-matrix helpers of 2g-gcn_amd/postprocess.py. The reference project decodes with a per-step
argmax only, so this file is the contract.

One sequence = one (clip b, entity e). logp[t, c] is read at the model's own step rate, L is the decoded length, A the
fp32 (C, C) transition scores (row = from, column = to), pi an optional fp32 (C,) initial score (all zero when absent).
All arithmetic is fp32 with one rounding per add; no operation is fused or reordered:

    d[0][c] = logp[0,c] + pi[c]
    m[t][c] = max over c' of (d[t-1][c'] + A[c',c])      psi[t][c] = the SMALLEST c' that attains it
    d[t][c] = m[t][c] + logp[t,c]                        (t = 1 .. L-1)
    y[L-1]  = the smallest c attaining max d[L-1][.]     y[t-1] = psi[t][y[t]]      score = max d[L-1][.]

A candidate replaces the running best only when it is strictly greater: that is the tie-break, and it decides what -inf
does (-inf entries of A, forbidden transitions, are in contract; NaN is not). Among paths of equal score the result is the
smallest one compared from the last step backwards.

lengths[b] is in model steps, clamped to [0, T]; None means T. A length of 0 gives label 0 everywhere and score 0.0.
Output: out[b, t', e] = y[min(t' // downsampling, L - 1)] for t' < T_out, int64 (bs, T_out, E); score fp32 (bs, E)."""
import numpy as np

MAX_CLASSES, MAX_STEPS = 64, 4096

F = np.float32


def decode_sequence(logp, A, pi=None):
    """logp fp32 (L, C) with L >= 1 -> (y int64 (L,), score np.float32). Explicit np.float32 operations, strict '>'."""
    L, C = logp.shape
    logp, A = np.asarray(logp, dtype=F), np.asarray(A, dtype=F)
    pi = np.zeros(C, dtype=F) if pi is None else np.asarray(pi, dtype=F)
    d = np.empty(C, dtype=F)
    for c in range(C):
        d[c] = F(logp[0, c] + pi[c])
    psi = np.zeros((L, C), dtype=np.int64)
    with np.errstate(invalid='ignore', over='ignore'):
        for t in range(1, L):
            new = np.empty(C, dtype=F)
            for c in range(C):
                best, arg = F(d[0] + A[0, c]), 0
                for cp in range(1, C):
                    cand = F(d[cp] + A[cp, c])
                    if cand > best:
                        best, arg = cand, cp
                psi[t, c] = arg
                new[c] = F(best + logp[t, c])
            d = new
    top, y_last = d[0], 0
    for c in range(1, C):
        if d[c] > top:
            top, y_last = d[c], c
    y = np.zeros(L, dtype=np.int64)
    y[L - 1] = y_last
    for t in range(L - 1, 0, -1):
        y[t - 1] = psi[t, y[t]]
    return y, F(top)


def decode_sequence_fast(logp, A, pi=None):
    """`decode_sequence` with the loop over c and c' as numpy array operations: the same fp32 adds, the same strict
    comparisons (np.argmax returns the first maximum), so the same bits. For the long sequences of the GPU tests."""
    L, C = logp.shape
    logp, A = np.asarray(logp, dtype=F), np.asarray(A, dtype=F)
    pi = np.zeros(C, dtype=F) if pi is None else np.asarray(pi, dtype=F)
    d = logp[0] + pi
    psi = np.zeros((L, C), dtype=np.int64)
    cols = np.arange(C)
    with np.errstate(invalid='ignore', over='ignore'):
        for t in range(1, L):
            cand = d[:, None] + A                 # cand[c', c], fp32
            arg = np.argmax(cand, axis=0)         # the first (smallest) c' among the maxima
            psi[t] = arg
            d = cand[arg, cols] + logp[t]
    y = np.zeros(L, dtype=np.int64)
    y[L - 1] = int(np.argmax(d))
    for t in range(L - 1, 0, -1):
        y[t - 1] = psi[t, y[t]]
    return y, F(d[y[L - 1]])


def viterbi_labels(logp, A, pi=None, lengths=None, downsampling=1, T_out=None, fast=False):
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
        for e in range(E):
            y, s = one(logp[b, :, :L, e].T, A, pi)
            score[b, e] = s
            for tp in range(T_out):
                labels[b, tp, e] = y[min(tp // ds, L - 1)]
    return labels, score


def transition_counts(targets, num_classes, stride=1, ignore_index=-1):
    """int64 (C, C): one for every (b, e, k) where targets[b, k * stride, e] and targets[b, (k + 1) * stride, e] are both in
    [0, C) and neither equals ignore_index. targets (bs, T_tgt, E)."""
    targets = np.asarray(targets)
    bs, T_tgt, E = targets.shape
    counts = np.zeros((num_classes, num_classes), dtype=np.int64)
    for b in range(bs):
        for e in range(E):
            k = 0
            while (k + 1) * stride < T_tgt:
                a, z = int(targets[b, k * stride, e]), int(targets[b, (k + 1) * stride, e])
                if a != ignore_index and z != ignore_index and 0 <= a < num_classes and 0 <= z < num_classes:
                    counts[a, z] += 1
                k += 1
    return counts


def transition_log_probs(counts, smoothing=1.0):
    """fp32 (C, C): log((n + s) / (row sum + C * s)) in fp64, rounded once. smoothing 0: an unseen transition is -inf, and a
    row without any count (where the ratio is 0 / 0) is all zeros."""
    counts = np.asarray(counts)
    C = counts.shape[0]
    out = np.zeros((C, C), dtype=np.float64)
    for a in range(C):
        den = float(counts[a].sum()) + C * float(smoothing)
        if den == 0.0:
            continue
        for z in range(C):
            num = float(counts[a, z]) + float(smoothing)
            out[a, z] = np.log(num / den) if num > 0.0 else -np.inf
    return out.astype(F)


def switch_penalty(num_classes, penalty):
    """fp32 (C, C): 0 on the diagonal, -penalty elsewhere."""
    out = np.full((num_classes, num_classes), -F(penalty), dtype=F)
    for c in range(num_classes):
        out[c, c] = F(0.0)
    return out


def dyadic(rng, shape):
    """Multiples of 2^-7 in [-8, 0] as fp32: every fp32 sum of fewer than 4096 of them is exact, so ties are real ties."""
    return (-rng.integers(0, 8 * 128 + 1, size=shape).astype(np.float64) / 128.0).astype(F)
