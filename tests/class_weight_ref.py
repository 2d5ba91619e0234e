"""The criterion with class weights (NLL terms) and the positive-class weight (BCE terms) as a numpy SPECIFICATION: the
definition at twog_wloss_t in include/twog_gcn.h restated operation by operation -- the sums in fp64 (the product of a
class weight and an input, both fp32, is exact there), the loss as w * (float)(sum / den), the gradient in fp32 with every
product and quotient rounded once and no multiplication fused with an addition. tests/test_class_weight_gpu.py holds the HIP
kernels to it, the test double tests/class_weight_fake.py states the kernel interface through it.

`real=F64` evaluates the same formulas in fp64 (the "fp64 form"), which tools/make_golden_class_weights.py and the golden
test compare with the reference: there the only difference left is the reference's own fp32 rounding."""
import numpy as np

F32, F64 = np.float32, np.float64
NLL, BCE, BUDGET = 0, 1, 2


def kept_nll(x, y, ignore):
    """The NLL term's rule: y != ignore && 0 <= y < C."""
    return (y != int(ignore)) & (y >= 0) & (y < x.shape[1])


def _nll_parts(x, y, ignore, class_weight):
    """(kept [outer][inner...], the input at the target class, the class weight at the target class), the last two where kept."""
    x, y = np.asarray(x), np.asarray(y)
    assert y.dtype == np.int64 and x.ndim >= 2 and y.shape == x.shape[:1] + x.shape[2:]
    kept = kept_nll(x, y, ignore)
    ys = np.where(kept, y, 0)
    picked = np.take_along_axis(x, ys[:, None], 1)[:, 0]
    cw = np.ones(x.shape[1], x.dtype) if class_weight is None else np.asarray(class_weight)
    assert cw.shape == (x.shape[1],)
    return kept, picked, cw[ys]


def _clamped_log(v):
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.maximum(np.log(v), v.dtype.type(-100.0))


def _positive(t, p, ignore):
    return (t == 1.0) & (p > 1) & (t != ignore)


def forward(kind, x, y, weight=1.0, ignore=-1, class_weight=None, positive_class_weight=1.0, real=F32):
    """-> (loss in `real`, (sum, den) fp64)."""
    x = np.asarray(x).astype(real)
    if kind == NLL:
        cw = None if class_weight is None else np.asarray(class_weight).astype(real)
        kept, picked, cwy = _nll_parts(x, y, ignore, cw)
        s = F64(np.where(kept, cwy.astype(F64) * (-picked).astype(F64), 0.0).sum(dtype=F64))
        den = F64(np.where(kept, cwy.astype(F64), 0.0).sum(dtype=F64))
        with np.errstate(divide='ignore', invalid='ignore'):
            return real(weight) * real(s / den), (s, den)                      # 0 / 0 -> NaN, as torch
    t = np.asarray(y).astype(real)
    kept = t != real(ignore)
    if kind == BUDGET:
        term = x
    else:
        p, one = real(positive_class_weight), real(1.0)
        plain = -(t * _clamped_log(x) + (one - t) * _clamped_log(one - x))    # every operation rounded on its own
        with np.errstate(divide='ignore', invalid='ignore'):
            pos = -np.maximum(p * np.log(x), real(-100.0))
        term = np.where(_positive(t, p, real(ignore)), pos, plain)
    assert term.dtype == real
    s = F64(np.where(kept, term.astype(F64), 0.0).sum(dtype=F64))
    den = F64(int(kept.sum()))
    return (real(weight) * real(s / den) if den > 0 else real(0.0)), (s, den)


def gradient(kind, x, y, weight=1.0, ignore=-1, class_weight=None, positive_class_weight=1.0, dloss=1.0, den=None, real=F32):
    """d(loss_total) / d(x) for an upstream gradient dloss, in `real`. den: what the loss was normalised by (default: the
    term's own; a count reducer may have replaced it)."""
    x = np.asarray(x).astype(real)
    if den is None:
        den = forward(kind, x, y, weight, ignore, class_weight, positive_class_weight, real)[1][1]
    g = (real(weight) * real(dloss)) / real(F64(den)) if den > 0 else real(0.0)
    assert np.asarray(g).dtype == real
    if kind == NLL:
        cw = None if class_weight is None else np.asarray(class_weight).astype(real)
        kept, _, cwy = _nll_parts(x, y, ignore, cw)
        v = np.where(kept, -(g * cwy), real(0.0)).astype(real)
        grad = np.zeros(x.shape, real)
        np.put_along_axis(grad, np.where(kept, y, 0)[:, None], v[:, None], 1)
        return grad
    t = np.asarray(y).astype(real)
    kept = t != real(ignore)
    if kind == BUDGET:
        return np.where(kept, g, real(0.0)).astype(real)
    p, one = real(positive_class_weight), real(1.0)
    d0 = (g * (x - t)) / np.maximum((one - x) * x, real(1e-12))               # torch's binary_cross_entropy backward
    d = np.where(_positive(t, p, real(ignore)), d0 * p, d0)
    assert d.dtype == real
    return np.where(kept, d, real(0.0)).astype(real)
