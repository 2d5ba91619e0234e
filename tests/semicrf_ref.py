"""The semi-Markov CRF loss in numpy: the definition that include/twog_gcn.h (twog_semicrf_nll_fwd) and
losses.semi_crf_loss restate, and what the kernels of csrc/semicrf.hip are held to. It is the sum-product twin of the
segmental decode of tests/segdecode_ref.py and shares its conventions: A fp32 (C, C) scores between consecutive segments
(row = from; the diagonal is an entry like any other), pi fp32 (C,), dur fp32 (C, D) with dur[c, l-1] the score of a class-c
segment of l steps.

`semicrf_nll(..., dtype=np.float64)` is the specification. `dtype=np.float32` is the same recurrences in the log domain with
the maximum subtracted, one fp32 rounding per operation, in the order the kernels take them; it exists only to measure what
fp32 costs (profiles/semicrf_loss_fp64.json, from which the gates of tests/test_semicrf_gpu.py are derived). In both, the
sums over sequences (nll_seq, K, dA, dpi, ddur) are carried in fp64 and rounded to `dtype` once, as the kernels carry them.

For one sequence = (clip b, entity e) with kept steps t_0 < ... < t_{K-1} (0 <= target < C and target != ignore_index),
x_k[c] = input[b, c, t_k, e], y_k = target[b, t_k, e], S_c(s, l) = x_s[c] + ... + x_{s+l-1}[c]:

    e_0[c]   = pi[c]
    e_k[c]   = logsumexp_{c'} (d_{k-1}[c'] + A[c', c])                                   k >= 1
    d_k[c]   = logsumexp_{l = 1 .. min(D, k+1)} (e_{k-l+1}[c] + dur[c, l-1] + S_c(k-l+1, l))
    logZ     = logsumexp_c d_{K-1}[c]
    gold     = the score of the gold segmentation (`gold_pieces`): the maximal runs of equal y; a run of n > D steps is cut
               into pieces of D steps from its start with the remainder (1 .. D steps) last, consecutive pieces joined by
               A[c, c]:  pi[c_1] + sum_j (dur[c_j, l_j - 1] + S_{c_j}(s_j, l_j)) + sum_{j >= 2} A[c_{j-1}, c_j]
    bd_{K-1}[c] = 0;   bd_k[c] = logsumexp_{c'} (A[c, c'] + be_{k+1}[c'])
    be_s[c]     = logsumexp_{l = 1 .. min(D, K-s)} (dur[c, l-1] + S_c(s, l) + bd_{s+l-1}[c])
    mu(s, l, c) = exp(e_s[c] + dur[c, l-1] + S_c(s, l) + bd_{s+l-1}[c] - logZ)
    End_k[c]    = exp(d_k[c] + bd_k[c] - logZ),  Start_k[c] = exp(e_k[c] + be_k[c] - logZ)
    cov_k       = cov_{k+1} + End_k - Start_{k+1}      (cov_K = Start_K = 0): the sum of mu over the segments that cover k

A logsumexp whose terms are all -inf is -inf. -inf in A, pi and dur is in contract as long as the sequence's own gold score
is finite; such an entry gets gradient exactly 0."""
import itertools
from collections import namedtuple

import numpy as np

MAX_CLASSES, MAX_STEPS, MAX_DURATION = 64, 4096, 128   # twog_semicrf_limits

Chain = namedtuple('Chain', 'e d bd be logZ gold cov start end sum_dur sum_A')
SemiCrfResult = namedtuple('SemiCrfResult', 'nll logZ gold K loss count dinput dA dpi ddur')


def kept_steps(target_seq, num_classes, ignore_index=-1):
    """Indices t of the kept steps of one sequence's labels (T,), under the NLL terms' rule."""
    y = np.asarray(target_seq)
    return np.nonzero((y != ignore_index) & (y >= 0) & (y < num_classes))[0]


def gold_pieces(y, D):
    """The gold segmentation of the labels y (K,) of the kept steps: [(start, length, class)] in order. A maximal run of n
    equal labels gives n // D pieces of D steps from its start, then the remainder if there is one."""
    y = [int(v) for v in y]
    out, s = [], 0
    while s < len(y):
        n = 1
        while s + n < len(y) and y[s + n] == y[s]:
            n += 1
        at = s
        while at < s + n:
            l = min(D, s + n - at)
            out.append((at, l, y[s]))
            at += l
        s += n
    return out


def _lse(v, axis, dt):
    """(logsumexp along the axis, the maximum it subtracted); all -inf gives (-inf, 0)."""
    m = v.max(axis=axis)
    ms = np.where(np.isneginf(m), dt(0), m).astype(dt)
    with np.errstate(divide='ignore'):
        return (ms + np.log(np.exp(v - np.expand_dims(ms, axis)).sum(axis=axis, dtype=dt))).astype(dt), ms


def gold_score(x, y, A, pi, dur, dt):
    """The gold score in `dt`, added up in step order: at the first step of a piece the closed piece's duration score and
    the join (pi for the very first), every step its emission, the last piece's duration score at the end."""
    D = dur.shape[1]
    starts = {s for s, _, _ in gold_pieces(y, D)}
    gold, pos = dt(0), 0
    for k in range(len(y)):
        if k in starts:
            if k > 0:
                gold = dt(gold + dur[y[k - 1], pos - 1])
                gold = dt(gold + A[y[k - 1], y[k]])
            else:
                gold = dt(gold + pi[y[0]])
            pos = 0
        pos += 1
        gold = dt(gold + x[k, y[k]])
    return dt(gold + dur[y[-1], pos - 1])


def chain(x, y, A, pi, dur, dtype=np.float64):
    """One compacted sequence: x (K, C) emissions of the kept steps, y (K,) their labels, K >= 1. Returns Chain(e, d, bd, be
    (K, C), logZ, gold, cov, start, end (K, C), sum_dur (C, D) = sum_s mu(s, l, c), sum_A (C, C) = the expected joins), all
    in `dtype` and without the gold counts."""
    dt = np.dtype(dtype).type
    x, A, pi, dur = (np.asarray(a, dt) for a in (x, A, pi, dur))
    K, C = x.shape
    D = dur.shape[1]
    dur_t = np.ascontiguousarray(dur.T)                    # (D, C): row l - 1
    zero = np.zeros((1, C), dt)
    e, d, bd, be = (np.empty((K, C), dt) for _ in range(4))
    with np.errstate(invalid='ignore'):
        for k in range(K):
            e[k] = pi if k == 0 else _lse(d[k - 1][:, None] + A, 0, dt)[0]
            n = min(D, k + 1)
            back = slice(k, None, -1) if n == k + 1 else slice(k, k - n, -1)       # steps k, k-1, .., k-n+1: l = 1 .. n
            acc = np.cumsum(np.concatenate([zero, x[back]]), axis=0, dtype=dt)[1:]
            d[k] = _lse((e[back] + dur_t[:n]) + acc, 0, dt)[0]
        logZ = dt(_lse(d[K - 1], 0, dt)[0])
        sum_dur_t, sum_A = np.zeros((D, C), dt), np.zeros((C, C), dt)
        for k in range(K - 1, -1, -1):
            if k == K - 1:
                bd[k] = 0
            else:
                w = A + be[k + 1][None, :]                  # w[c, c'] = A[c, c'] + be_{k+1}[c']
                bd[k], ms = _lse(w, 1, dt)
                sum_A += np.exp(w - ms[:, None]) * np.exp((d[k] + ms) - logZ)[:, None]
            n = min(D, K - k)
            acc = np.cumsum(np.concatenate([zero, x[k:k + n]]), axis=0, dtype=dt)[1:]
            cand = (bd[k:k + n] + dur_t[:n]) + acc          # l = 1 .. n
            be[k], ms = _lse(cand, 0, dt)
            sum_dur_t[:n] += np.exp(cand - ms[None, :]) * np.exp((e[k] + ms) - logZ)[None, :]
        end, start = np.exp((d + bd) - logZ), np.exp((e + be) - logZ)
    cov = np.empty((K, C), dt)
    run, nxt = np.zeros(C, dt), np.zeros(C, dt)
    for k in range(K - 1, -1, -1):
        run = (run + end[k]) - nxt
        cov[k], nxt = run, start[k]
    return Chain(e, d, bd, be, logZ, gold_score(x, y, A, pi, dur, dt), cov, start, end,
                 np.ascontiguousarray(sum_dur_t.T), sum_A)


def segment_marginals(x, A, pi, dur):
    """mu (K, D, C) of one compacted sequence in fp64: mu[s, l-1, c], zero where the segment does not fit."""
    x, A, pi, dur = (np.asarray(a, np.float64) for a in (x, A, pi, dur))
    K, C = x.shape
    D = dur.shape[1]
    ch = chain(x, np.zeros(K, np.int64), A, pi, dur)
    mu = np.zeros((K, D, C))
    for s in range(K):
        for l in range(1, min(D, K - s) + 1):
            with np.errstate(invalid='ignore'):
                mu[s, l - 1] = np.exp(ch.e[s] + dur[:, l - 1] + x[s:s + l].sum(0) + ch.bd[s + l - 1] - ch.logZ)
    return mu


def semicrf_nll(input, target, A, pi, dur, ignore_index=-1, dtype=np.float64, g=None):
    """input (bs, C, T, E), target int (bs, T, E), A (C, C), pi (C,), dur (C, D). Returns SemiCrfResult: per sequence nll,
    logZ, gold (bs, E) in `dtype` and K (bs, E) int64 (zeros where K = 0); loss = sum nll / sum K (0 when nothing is kept) and
    count = sum K; the gradients dinput (bs, C, T, E), dA (C, C), dpi (C,), ddur (C, D) of the loss, i.e. with the factor
    g = 1 / count (0 for count 0); a given `g` replaces that factor (g = 1: the gradients before the factor)."""
    dt = np.dtype(dtype).type
    x_all, A, pi, dur = (np.asarray(a, dt) for a in (input, A, pi, dur))
    target = np.asarray(target)
    bs, C, T, E = x_all.shape
    D = dur.shape[1]
    assert target.shape == (bs, T, E) and A.shape == (C, C) and pi.shape == (C,) and dur.shape == (C, D)
    nll, logZ, gold = (np.zeros((bs, E), dt) for _ in range(3))
    Ks = np.zeros((bs, E), np.int64)
    raw = np.zeros((bs, C, T, E), dt)          # cov - indicator at the kept steps, 0 elsewhere
    sum_A, sum_pi, sum_dur = np.zeros((C, C), np.float64), np.zeros(C, np.float64), np.zeros((C, D), np.float64)
    for b in range(bs):
        for e in range(E):
            ts = kept_steps(target[b, :, e], C, ignore_index)
            if ts.size == 0:
                continue
            y = target[b, ts, e].astype(np.int64)
            ch = chain(x_all[b][:, ts, e].T, y, A, pi, dur, dt)
            with np.errstate(invalid='ignore'):
                Ks[b, e], logZ[b, e], gold[b, e], nll[b, e] = ts.size, ch.logZ, ch.gold, dt(ch.logZ - ch.gold)
            dx = ch.cov.copy()
            dx[np.arange(ts.size), y] -= dt(1)
            raw[b][:, ts, e] = dx.T
            acc_A, acc_dur, first = ch.sum_A.copy(), ch.sum_dur.copy(), ch.start[0].copy()
            pieces = gold_pieces(y, D)
            for j, (s, l, c) in enumerate(pieces):
                acc_dur[c, l - 1] -= dt(1)
                if j > 0:
                    acc_A[pieces[j - 1][2], c] -= dt(1)
            first[pieces[0][2]] -= dt(1)
            sum_A += acc_A.astype(np.float64)
            sum_pi += first.astype(np.float64)
            sum_dur += acc_dur.astype(np.float64)
    count = float(Ks.sum())
    total = float(nll.astype(np.float64).sum())
    loss = dt(total / count) if count > 0 else dt(0)
    if g is None:
        g = dt(dt(1) / dt(count)) if count > 0 else dt(0)
    g = dt(g)
    return SemiCrfResult(nll, logZ, gold, Ks, loss, count, (g * raw).astype(dt), (np.float64(g) * sum_A).astype(dt),
                         (np.float64(g) * sum_pi).astype(dt), (np.float64(g) * sum_dur).astype(dt))


QUANTITIES = ('loss', 'nll', 'dinput', 'dA', 'dpi', 'ddur')


def errors(got, spec):
    """The largest error per compared quantity of a SemiCrfResult `got` against the fp64 SemiCrfResult `spec` of the same
    inputs: loss and per-sequence nll in absolute terms relative to max(1, |logZ|) (the sequence's own logZ for nll, the
    largest for the loss); the four gradients in absolute terms -- evaluate both with g = 1 to have them before the factor."""
    scale = np.maximum(1.0, np.abs(spec.logZ.astype(np.float64)))
    f64 = lambda a: np.asarray(a, np.float64)
    out = dict(loss=float(abs(float(got.loss) - float(spec.loss)) / scale.max()),
               nll=float((np.abs(f64(got.nll) - f64(spec.nll)) / scale).max()))
    for q in ('dinput', 'dA', 'dpi', 'ddur'):
        out[q] = float(np.abs(f64(getattr(got, q)) - f64(getattr(spec, q))).max())
    return out


def segmentations(K, D):
    """Every way to cut K steps into consecutive segments of 1 .. D steps: lists of (start, length)."""
    if K == 0:
        return [[]]
    out = []
    for l in range(1, min(D, K) + 1):
        out += [rest + [(K - l, l)] for rest in segmentations(K - l, D)]
    return out


def segmentation_score(x, segs, classes, A, pi, dur):
    """The score of one labelled segmentation: segs [(start, length)], classes one per segment."""
    total = pi[classes[0]]
    for j, ((s, l), c) in enumerate(zip(segs, classes)):
        total = total + dur[c, l - 1] + x[s:s + l, c].sum()
        if j > 0:
            total = total + A[classes[j - 1], c]
    return total


def brute_force(x, A, pi, dur):
    """One compacted sequence by enumeration of all labelled segmentations, in fp64: dict(logZ, mu (K, D, C), cov (K, C),
    E_dur (C, D), E_A (C, C), E_pi (C,)): the marginals and the expected counts, i.e. the gradients of logZ."""
    x, A, pi, dur = (np.asarray(a, np.float64) for a in (x, A, pi, dur))
    K, C = x.shape
    D = dur.shape[1]
    paths = [(segs, cls) for segs in segmentations(K, D) for cls in itertools.product(range(C), repeat=len(segs))]
    with np.errstate(invalid='ignore'):
        scores = np.array([segmentation_score(x, segs, cls, A, pi, dur) for segs, cls in paths])
    m = scores.max()
    weights = np.exp(scores - m)
    Z = weights.sum()
    mu, cov = np.zeros((K, D, C)), np.zeros((K, C))
    E_dur, E_A, E_pi = np.zeros((C, D)), np.zeros((C, C)), np.zeros(C)
    for (segs, cls), wgt in zip(paths, weights / Z):
        E_pi[cls[0]] += wgt
        for j, ((s, l), c) in enumerate(zip(segs, cls)):
            mu[s, l - 1, c] += wgt
            cov[s:s + l, c] += wgt
            E_dur[c, l - 1] += wgt
            if j > 0:
                E_A[cls[j - 1], c] += wgt
    return dict(logZ=m + np.log(Z), mu=mu, cov=cov, E_dur=E_dur, E_A=E_A, E_pi=E_pi)
