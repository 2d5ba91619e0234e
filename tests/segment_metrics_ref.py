"""Executable specification (test infrastructure only) of twog_segment_f1 / twog_segment_f1_accumulate: the sequential
greedy matching of pyrutils/metrics.py:30-44 for tp / fp / fn, and oracle.postprocess_ref.f1_at_k_single_example for the
F1 value. Deliberately NOT the order-free form the kernel uses: the predicted segments are visited in order against a
`used` array, with the IoU against every target segment. Pinned to the reference by golden G17
(tools/make_golden_segment_metrics.py)."""
import numpy as np

from oracle import postprocess_ref as R

MAX_STEPS = 4096      # what twog_segment_f1_limits reports
MAX_OVERLAPS = 8


def counts_single_example(y_true, y_pred, num_classes, overlap):
    """(tp, fp, fn) of one filtered, non-empty pair of label sequences."""
    tgt_ids, tgt_iv = R._rle(list(y_true))
    out_ids, out_iv = R._rle(list(y_pred))
    tp = fp = 0
    used = np.zeros(len(tgt_ids), dtype=bool)
    for (o0, o1), oid in zip(out_iv, out_ids):
        inter = np.minimum(o1, tgt_iv[:, 1]) - np.maximum(o0, tgt_iv[:, 0])
        union = np.maximum(o1, tgt_iv[:, 1]) - np.minimum(o0, tgt_iv[:, 0])
        iou = (inter / union) * (oid == tgt_ids)
        idx = int(np.argmax(iou))
        if oid >= num_classes:
            continue
        if iou[idx] >= overlap and not used[idx]:
            tp += 1
            used[idx] = True
        else:
            fp += 1
    return tp, fp, int(len(used) - used.sum())


def sequences(y_true, y_pred, entity_minor=False):
    """Label arrays -> sequence-major (n_seq, n_steps): (bs, S, E) with entity_minor gives sequence b * E + e."""
    y_true, y_pred = np.asarray(y_true), np.asarray(y_pred)
    if entity_minor:
        steps = y_true.shape[1]
        return y_true.transpose(0, 2, 1).reshape(-1, steps), y_pred.transpose(0, 2, 1).reshape(-1, steps)
    return y_true, y_pred


def segment_f1(y_true, y_pred, num_classes, overlaps, ignore_value=None, entity_minor=False):
    """f1 float64 (n_seq, K), tp, fp, fn int32 (n_seq, K), valid int32 (n_seq,)."""
    y_true, y_pred = sequences(y_true, y_pred, entity_minor)
    n_seq, K = y_true.shape[0], len(overlaps)
    f1 = np.zeros((n_seq, K), dtype=np.float64)
    tp, fp, fn = (np.zeros((n_seq, K), dtype=np.int32) for _ in range(3))
    valid = np.zeros(n_seq, dtype=np.int32)
    for s, (yt, yp) in enumerate(zip(y_true, y_pred)):
        if ignore_value is not None:
            keep = yt != ignore_value
            yt, yp = yt[keep], yp[keep]
        if yt.size == 0:
            continue
        valid[s] = 1
        for k, overlap in enumerate(overlaps):
            tp[s, k], fp[s, k], fn[s, k] = counts_single_example(yt, yp, num_classes, overlap)
            f1[s, k] = R.f1_at_k_single_example(yt, yp, num_classes, overlap)
    return f1, tp, fp, fn, valid


def mean_f1(f1, valid):
    """The batch metric of metrics.py:70-81: the per-sequence values added in sequence order, over the valid count."""
    out = []
    for k in range(f1.shape[1]):
        total = 0.0
        for v in f1[valid != 0, k]:
            total += float(v)
        out.append(total / float(valid.sum()) if valid.sum() else float('nan'))
    return out
