"""Executable specification (test infrastructure only) of the prediction evaluation: a numpy restatement of the two
entry points twog_eval_update / twog_confusion_counts and of the metrics computed from their confusion counts. It is
pinned to the reference's own functions and to scikit-learn by golden G15 (tools/make_golden_evaluation.py)."""
import numpy as np


def eval_update(logp, downsampling, target, step_index=None):
    """logp (bs, C, T, E), target int (bs, T_tgt, E), step_index int (bs, S) or None ->
    counts int64 (C, C), flags int64 (2,), labels int64 (bs, S, E), targets int64 (bs, S, E)."""
    bs, C, T, E = logp.shape
    T_tgt = target.shape[1]
    if step_index is None:
        step_index = np.tile(np.arange(T_tgt), (bs, 1))
    S = step_index.shape[1]
    counts, flags = np.zeros((C, C), dtype=np.int64), np.zeros(2, dtype=np.int64)
    labels, targets = np.zeros((bs, S, E), dtype=np.int64), np.full((bs, S, E), -1, dtype=np.int64)
    for b in range(bs):
        for s in range(S):
            tp = int(step_index[b, s])
            if tp < 0:
                continue                                   # padding: label 0, target -1, nothing counted
            if tp >= T_tgt:
                flags[1] += E                              # never read
                continue
            t = min(tp // downsampling, T - 1)
            for e in range(E):
                label = int(np.argmax(logp[b, :, t, e]))   # first maximum
                tgt = int(target[b, tp, e])
                labels[b, s, e], targets[b, s, e] = label, tgt
                if tgt == -1:
                    continue
                if tgt < -1 or tgt >= C:
                    flags[0] += 1
                    continue
                counts[tgt, label] += 1
    return counts, flags, labels, targets


def confusion_counts(y_true, y_pred, C):
    counts, flags = np.zeros((C, C), dtype=np.int64), np.zeros(2, dtype=np.int64)
    for t, p in zip(np.asarray(y_true).reshape(-1).tolist(), np.asarray(y_pred).reshape(-1).tolist()):
        t, p = int(t), int(p)
        if t == -1:
            continue
        if t < -1 or t >= C or p < 0 or p >= C:
            flags[0] += 1
            continue
        counts[t, p] += 1
    return counts, flags


def _div(a, b):
    return a / b if b else 0.0


def _class_rows(counts, labels):
    """[(precision, recall, f1, support)] of the classes in `labels`; a class beyond the matrix has no counts."""
    C = counts.shape[0]
    rows = []
    for c in labels:
        tp = int(counts[c, c]) if c < C else 0
        pred = int(counts[:, c].sum()) if c < C else 0
        true = int(counts[c, :].sum()) if c < C else 0
        rows.append((_div(tp, pred), _div(tp, true), _div(2 * tp, pred + true), true))
    return rows


def precision_recall_f1(counts, average):
    """sklearn precision_recall_fscore_support(average=..., labels=None) from counts."""
    counts = np.asarray(counts, dtype=np.int64)
    C = counts.shape[0]
    if average == 'micro':
        tp, total = int(np.trace(counts)), int(counts.sum())
        return {'precision': _div(tp, total), 'recall': _div(tp, total), 'f1': _div(2 * tp, 2 * total)}
    present = [c for c in range(C) if counts[c, :].sum() + counts[:, c].sum() > 0]
    rows = _class_rows(counts, present)
    if not rows:
        return {'precision': float('nan'), 'recall': float('nan'), 'f1': float('nan')}
    return {k: float(np.mean([r[i] for r in rows])) for i, k in enumerate(('precision', 'recall', 'f1'))}


def classification_report(counts, target_names):
    """sklearn classification_report(labels=range(len(target_names)), target_names=..., output_dict=True) from counts."""
    counts = np.asarray(counts, dtype=np.int64)
    C, L = counts.shape[0], len(target_names)
    rows = _class_rows(counts, range(L))
    rep = {str(n): {'precision': r[0], 'recall': r[1], 'f1-score': r[2], 'support': r[3]}
           for n, r in zip(target_names, rows)}
    support = sum(r[3] for r in rows)
    tp = sum(int(counts[c, c]) for c in range(min(L, C)))
    pred = sum(int(counts[:, c].sum()) for c in range(min(L, C)))
    covered = all(counts[c, :].sum() + counts[:, c].sum() == 0 for c in range(L, C))
    if covered:
        rep['accuracy'] = _div(tp, support)
    else:
        rep['micro avg'] = {'precision': _div(tp, pred), 'recall': _div(tp, support),
                            'f1-score': _div(2 * tp, pred + support), 'support': support}
    for name, weights in (('macro avg', None), ('weighted avg', [r[3] for r in rows] if support else None)):
        rep[name] = {k: float(np.average([r[i] for r in rows], weights=weights)) if rows else float('nan')
                     for i, k in enumerate(('precision', 'recall', 'f1-score'))}
        rep[name]['support'] = support
    return rep
