"""The temporal smoothing loss (truncated MSE between the log-probabilities of adjacent steps) as a numpy SPECIFICATION:
the definition at twog_smooth_loss_t in include/twog_gcn.h restated with its arithmetic spelled out -- the difference in
fp32 (one rounding), its square and the clamp in fp64 (the product of two fp32 numbers is exact there), the sum in fp64, the
gradient in fp32 with every product rounded once. tests/test_smooth_loss_gpu.py holds the HIP kernels to it, the test double
tests/smooth_loss_fake.py states the kernel interface through it."""
import numpy as np

F32, F64 = np.float32, np.float64


def _pairs(x, y, tau, ignore):
    """(kept pairs [outer][T-1][E], fp32 differences [outer][C][T-1][E], their exact squares in fp64, tau^2 in fp64)."""
    x, y = np.asarray(x), np.asarray(y)
    assert x.dtype == F32 and y.dtype == np.int64 and x.ndim == 4 and y.shape == (x.shape[0], x.shape[2], x.shape[3])
    kept = (y != int(ignore)) & (y >= 0) & (y < x.shape[1])          # the NLL term's own rule
    pair = kept[:, 1:] & kept[:, :-1]
    d = x[:, :, 1:] - x[:, :, :-1]                                   # fp32 operands: one fp32 rounding
    assert d.dtype == F32
    sq = d.astype(F64) * d.astype(F64)
    return pair, d, sq, F64(F32(tau)) * F64(F32(tau))


def forward(x, y, weight=1.0, tau=4.0, ignore=-1):
    """-> (loss fp32, stats = (sum, count) fp64)."""
    pair, _, sq, tau2 = _pairs(x, y, tau, ignore)
    s = F64(np.where(pair[:, None], np.minimum(sq, tau2), 0.0).sum(dtype=F64))
    count = F64(int(pair.sum()) * x.shape[1])
    loss = F32(weight) * F32(s / count) if count > 0 else F32(0.0)
    return F32(loss), (s, count)


def gradient(x, y, weight=1.0, tau=4.0, ignore=-1, dloss=1.0, count=None):
    """d(loss_total) / d(x) for an upstream gradient dloss, fp32: fl(g * 2 D) on step t of every kept pair whose D^2 <= tau^2
    (boundary included), 0 elsewhere -- the predecessor is a constant. count: the count the loss was normalised by (default:
    the term's own; a count reducer may have replaced it)."""
    pair, d, sq, tau2 = _pairs(x, y, tau, ignore)
    if count is None:
        count = F64(int(pair.sum()) * x.shape[1])
    g = (F32(weight) * F32(dloss)) / F32(F64(count)) if count > 0 else F32(0.0)
    assert np.asarray(g).dtype == F32
    grad = np.zeros(x.shape, F32)
    grad[:, :, 1:] = np.where(pair[:, None] & (sq <= tau2), F32(g) * (F32(2.0) * d), F32(0.0))
    return grad


def smooth_loss(x, y, weight=1.0, tau=4.0, ignore=-1, dloss=1.0):
    """-> (loss, (sum, count), gradient)."""
    loss, stats = forward(x, y, weight, tau, ignore)
    return loss, stats, gradient(x, y, weight, tau, ignore, dloss, stats[1])
