"""The linear-chain CRF loss in numpy: the definition that include/twog_gcn.h (twog_crf_nll_fwd) and losses.crf_loss
restate, and what the kernels of csrc/crf.hip are held to.

`crf_nll(..., dtype=np.float64)` is the specification. `dtype=np.float32` is the same recurrences in the log domain with
the maximum subtracted, one fp32 rounding per operation; it exists only to measure what fp32 costs a T-step recursion
(profiles/crf_loss_fp64.json, from which the gates of tests/test_crf_gpu.py are derived). In both, the sums over sequences
(nll_seq, K, dA, dpi) are carried in fp64 and rounded to `dtype` once, as the kernels carry them.

For one sequence = (clip b, entity e) with kept steps t_0 < ... < t_{K-1} (0 <= target < C and target != ignore_index),
x_k[c] = input[b, c, t_k, e], y_k = target[b, t_k, e]:

    alpha_0[c] = pi[c] + x_0[c]
    alpha_k[c] = x_k[c] + logsumexp_{c'} (alpha_{k-1}[c'] + A[c', c])
    logZ       = logsumexp_c alpha_{K-1}[c]
    gold       = pi[y_0] + x_0[y_0] + sum_{k>=1} (A[y_{k-1}, y_k] + x_k[y_k])
    beta_{K-1} = 0,  beta_k[c'] = logsumexp_c (A[c', c] + x_{k+1}[c] + beta_{k+1}[c])
    gamma_k[c]  = exp(alpha_k[c] + beta_k[c] - logZ)
    xi_k[c', c] = exp(alpha_{k-1}[c'] + A[c', c] + x_k[c] + beta_k[c] - logZ)          k = 1 .. K-1
"""
from collections import namedtuple

import numpy as np

MAX_CLASSES, MAX_STEPS = 64, 4096   # twog_crf_limits

Chain = namedtuple('Chain', 'alpha beta logZ gold gamma xi')
CrfResult = namedtuple('CrfResult', 'nll logZ gold K loss count dinput dA dpi')


def kept_steps(target_seq, num_classes, ignore_index=-1):
    """Indices t of the kept steps of one sequence's labels (T,), under the NLL terms' rule."""
    y = np.asarray(target_seq)
    return np.nonzero((y != ignore_index) & (y >= 0) & (y < num_classes))[0]


def _lse(v, axis, dt):
    m = v.max(axis=axis)
    return m + np.log(np.exp(v - np.expand_dims(m, axis)).sum(axis=axis, dtype=dt))


def chain(x, y, A, pi, dtype=np.float64):
    """One compacted sequence: x (K, C) emissions of the kept steps, y (K,) their labels, K >= 1. Returns Chain(alpha (K, C),
    beta (K, C), logZ, gold, gamma (K, C), xi (K - 1, C, C) with xi[k - 1] = xi_k), everything in `dtype`."""
    dt = np.dtype(dtype).type
    x, A, pi = np.asarray(x, dt), np.asarray(A, dt), np.asarray(pi, dt)
    K, C = x.shape
    alpha, beta = np.empty((K, C), dt), np.zeros((K, C), dt)
    alpha[0] = pi + x[0]
    gold = dt(pi[y[0]] + x[0, y[0]])
    for k in range(1, K):
        alpha[k] = x[k] + _lse(alpha[k - 1][:, None] + A, 0, dt)
        gold = dt(gold + dt(A[y[k - 1], y[k]] + x[k, y[k]]))
    logZ = dt(_lse(alpha[K - 1], 0, dt))
    xi = np.empty((max(K - 1, 0), C, C), dt)
    for k in range(K - 2, -1, -1):
        u = x[k + 1] + beta[k + 1]
        beta[k] = _lse(A + u[None, :], 1, dt)
        xi[k] = np.exp(((alpha[k][:, None] + A) + u[None, :]) - logZ)
    gamma = np.exp((alpha + beta) - logZ)
    return Chain(alpha, beta, logZ, gold, gamma, xi)


def crf_nll(input, target, A, pi, ignore_index=-1, dtype=np.float64, g=None):
    """input (bs, C, T, E), target int (bs, T, E), A (C, C), pi (C,). Returns CrfResult: per sequence nll, logZ, gold (bs, E)
    in `dtype` and K (bs, E) int64 (zeros where K = 0); loss = sum nll / sum K (0 when nothing is kept) and count = sum K;
    the gradients dinput (bs, C, T, E), dA (C, C), dpi (C,) of the loss, i.e. with the factor g = 1 / count (0 for count 0);
    a given `g` replaces that factor (g = 1: the gradients before the factor)."""
    dt = np.dtype(dtype).type
    x_all, A, pi = np.asarray(input, dt), np.asarray(A, dt), np.asarray(pi, dt)
    target = np.asarray(target)
    bs, C, T, E = x_all.shape
    assert target.shape == (bs, T, E) and A.shape == (C, C) and pi.shape == (C,)
    nll, logZ, gold = (np.zeros((bs, E), dt) for _ in range(3))
    Ks = np.zeros((bs, E), np.int64)
    raw = np.zeros((bs, C, T, E), dt)          # gamma - indicator at the kept steps, 0 elsewhere
    sum_A, sum_pi = np.zeros((C, C), np.float64), np.zeros(C, np.float64)
    for b in range(bs):
        for e in range(E):
            ts = kept_steps(target[b, :, e], C, ignore_index)
            if ts.size == 0:
                continue
            y = target[b, ts, e].astype(np.int64)
            ch = chain(x_all[b][:, ts, e].T, y, A, pi, dt)
            Ks[b, e], logZ[b, e], gold[b, e], nll[b, e] = ts.size, ch.logZ, ch.gold, dt(ch.logZ - ch.gold)
            d = ch.gamma.copy()
            d[np.arange(ts.size), y] -= dt(1)
            raw[b][:, ts, e] = d.T
            acc = np.zeros((C, C), dt)             # the sequence's own sum, in `dtype`, from the last pair to the first
            for k in range(ts.size - 2, -1, -1):
                acc += ch.xi[k]
                acc[y[k], y[k + 1]] -= dt(1)
            sum_A += acc.astype(np.float64)
            sum_pi += d[0].astype(np.float64)
    count = float(Ks.sum())
    total = float(nll.astype(np.float64).sum())
    loss = dt(total / count) if count > 0 else dt(0)
    if g is None:
        g = dt(dt(1) / dt(count)) if count > 0 else dt(0)
    g = dt(g)
    return CrfResult(nll, logZ, gold, Ks, loss, count, (g * raw).astype(dt), (np.float64(g) * sum_A).astype(dt),
                     (np.float64(g) * sum_pi).astype(dt))


QUANTITIES = ('loss', 'nll', 'dinput', 'dA', 'dpi')


def errors(got, spec):
    """The largest error per compared quantity of a CrfResult `got` against the fp64 CrfResult `spec` of the same inputs: loss
    and per-sequence nll in absolute terms relative to max(1, |logZ|) (the sequence's own logZ for nll, the largest for the
    loss); the three gradients in absolute terms -- evaluate both with g = 1 to have them before the factor g."""
    scale = np.maximum(1.0, np.abs(spec.logZ.astype(np.float64)))
    f64 = lambda a: np.asarray(a, np.float64)
    return dict(loss=float(abs(float(got.loss) - float(spec.loss)) / scale.max()),
                nll=float((np.abs(f64(got.nll) - f64(spec.nll)) / scale).max()),
                dinput=float(np.abs(f64(got.dinput) - f64(spec.dinput)).max()),
                dA=float(np.abs(f64(got.dA) - f64(spec.dA)).max()),
                dpi=float(np.abs(f64(got.dpi) - f64(spec.dpi)).max()))


def brute_force(x, A, pi):
    """One compacted sequence by enumeration of all C^K paths, in fp64: (logZ, gamma (K, C), xi (K - 1, C, C))."""
    import itertools
    x, A, pi = np.asarray(x, np.float64), np.asarray(A, np.float64), np.asarray(pi, np.float64)
    K, C = x.shape
    paths = list(itertools.product(range(C), repeat=K))
    scores = np.array([pi[p[0]] + x[0, p[0]] + sum(A[p[k - 1], p[k]] + x[k, p[k]] for k in range(1, K)) for p in paths])
    m = scores.max()
    weights = np.exp(scores - m)
    Z = weights.sum()
    gamma, xi = np.zeros((K, C)), np.zeros((max(K - 1, 0), C, C))
    for p, wgt in zip(paths, weights):
        for k in range(K):
            gamma[k, p[k]] += wgt / Z
            if k >= 1:
                xi[k - 1, p[k - 1], p[k]] += wgt / Z
    return m + np.log(Z), gamma, xi
