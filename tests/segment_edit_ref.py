"""Executable specification (test infrastructure only) of twog_segment_edit: the segmental edit score of action
segmentation. The reference project does not compute it, so this file IS the contract:

  per sequence, drop the steps whose target equals the ignore value from both sequences; run-length encode both into
  lists of segment labels; with a background label remove the segments of that label from both lists WITHOUT merging the
  neighbours this brings together (A bg A is [A, A]); distance = Levenshtein(true list, predicted list) with unit
  insertion, deletion and substitution; score = (1.0 - distance / max(m, n)) * 100.0 in fp64. A sequence with no kept
  step, or with both lists empty, is not valid: all five of its outputs are zero and the mean skips it.

`levenshtein` is the plain double loop over the full table, deliberately NOT the anti-diagonal order the kernel uses.
`levenshtein_rows` is a second, row-vectorised form for the long cases (tests/test_segment_edit_cpu.py proves the two
equal before anything relies on it). HAND_CASES pins the definition with values worked out by hand."""
import numpy as np

from tests.segment_metrics_ref import sequences

MAX_STEPS = 4096      # what twog_segment_edit_limits reports: the max_steps of twog_segment_f1_limits


def levenshtein(a, b):
    """Unit-cost edit distance between two sequences of labels: D[i][j] over the full (m + 1) x (n + 1) table."""
    m, n = len(a), len(b)
    D = [[0] * (n + 1) for _ in range(m + 1)]
    for i in range(m + 1):
        D[i][0] = i
    for j in range(n + 1):
        D[0][j] = j
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            D[i][j] = min(D[i - 1][j] + 1, D[i][j - 1] + 1, D[i - 1][j - 1] + (0 if a[i - 1] == b[j - 1] else 1))
    return D[m][n]


def levenshtein_rows(a, b):
    """The same distance, one numpy row at a time. Row i is min(x[j], row[j - 1] + 1) with x[j] = min(prev[j] + 1,
    prev[j - 1] + cost) the part that does not depend on the row itself; the insertion chain row[j] = min_k<=j (x[k] + j - k)
    is j + the running minimum of x[k] - k."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    n = b.size
    index = np.arange(n + 1, dtype=np.int64)
    row = index.copy()
    for i in range(1, a.size + 1):
        x = np.empty(n + 1, dtype=np.int64)
        x[0] = i
        x[1:] = np.minimum(row[1:] + 1, row[:-1] + (a[i - 1] != b))
        row = np.minimum.accumulate(x - index) + index
    return int(row[n])


def rle_labels(y):
    """The labels of the runs of a 1-d array, in order."""
    y = np.asarray(y)
    if y.size == 0:
        return y[:0]
    return y[np.concatenate([[True], y[1:] != y[:-1]])]


def segment_lists(yt, yp, ignore_value=None, bg_label=None):
    """(true list, predicted list, number of kept steps) of one sequence."""
    yt, yp = np.asarray(yt), np.asarray(yp)
    if ignore_value is not None:
        keep = yt != ignore_value
        yt, yp = yt[keep], yp[keep]
    tl, pl = rle_labels(yt), rle_labels(yp)
    if bg_label is not None:
        tl, pl = tl[tl != bg_label], pl[pl != bg_label]
    return tl, pl, yt.size


def score_value(distance, longer):
    """Three fp64 operations, each rounded once."""
    ratio = float(distance) / float(longer)
    kept = 1.0 - ratio
    return kept * 100.0


def segment_edit(y_true, y_pred, ignore_value=None, bg_label=None, entity_minor=False, distance=levenshtein):
    """score float64 (n_seq,), distance, n_true, n_pred, valid int32 (n_seq,)."""
    y_true, y_pred = sequences(y_true, y_pred, entity_minor)
    n_seq = y_true.shape[0]
    score = np.zeros(n_seq, dtype=np.float64)
    dist, n_true, n_pred, valid = (np.zeros(n_seq, dtype=np.int32) for _ in range(4))
    for s, (yt, yp) in enumerate(zip(y_true, y_pred)):
        tl, pl, n_kept = segment_lists(yt, yp, ignore_value, bg_label)
        longer = max(len(tl), len(pl))
        if n_kept == 0 or longer == 0:
            continue
        d = distance(tl.tolist(), pl.tolist())
        score[s], dist[s], n_true[s], n_pred[s], valid[s] = score_value(d, longer), d, len(tl), len(pl), 1
    return score, dist, n_true, n_pred, valid


def mean_edit(score, valid):
    """The batch metric: the scores of the valid sequences added in sequence order, over their number."""
    total = 0.0
    for v in np.asarray(score)[np.asarray(valid) != 0]:
        total += float(v)
    return total / float(np.sum(valid)) if np.sum(valid) else float('nan')


def _letters(word):
    return [ord(c) for c in word]


# Pairs of LISTS with their distance, worked out by hand: the textbook pair (k->s, e->i, +g), an empty list against n.
LIST_CASES = [
    (_letters('kitten'), _letters('sitting'), 3),
    (_letters('sitting'), _letters('kitten'), 3),
    ([], [4, 5, 6, 4], 4),
    ([4, 5, 6, 4], [], 4),
    ([], [], 0),
    ([1, 2, 3, 4, 5], [3], 4),          # keep the 3, insert the other four
    ([1, 2, 3, 4, 5], [9], 5),          # substitute it, insert four
    ([1, 2, 3], [1, 2, 3], 0),
]

# (name, y_true, y_pred, ignore_value, bg_label, (distance, n_true, n_pred, score, valid)), worked out by hand. The two
# sequences of a case have one length; the scores are written as the three operations of the definition.
HAND_CASES = [
    # identical sequences: nothing to edit
    ('identical', [3, 3, 5, 5, 5, 2, 7, 7], [3, 3, 5, 5, 5, 2, 7, 7], None, None, (0, 4, 4, 100.0, 1)),
    # one constant prediction against m = 5 true segments that contain its label: m - 1
    ('constant prediction, label present', [1, 1, 2, 2, 3, 3, 4, 4, 5, 5], [3] * 10, None, None,
     (4, 5, 1, (1.0 - 4.0 / 5.0) * 100.0, 1)),
    # ... that do not contain it: m
    ('constant prediction, label absent', [1, 1, 2, 2, 3, 3, 4, 4, 5, 5], [9] * 10, None, None, (5, 5, 1, 0.0, 1)),
    # the textbook pair as segment lists: a background step keeps the double t apart and is then removed without merging
    ('kitten / sitting', _letters('kit') + [0] + _letters('tenn'), _letters('sit') + [0] + _letters('ting'), None, 0,
     (3, 6, 7, (1.0 - 3.0 / 7.0) * 100.0, 1)),
    # an empty list against n = 3 (every true step is background): n, and score 0
    ('empty true list against three', [0, 0, 0, 0, 0, 0], [1, 1, 2, 2, 3, 3], None, 0, (3, 0, 3, 0.0, 1)),
    ('three against an empty predicted list', [1, 1, 2, 2, 3, 3], [0, 0, 0, 0, 0, 0], None, 0, (3, 3, 0, 0.0, 1)),
    # both lists emptied by the background rule: not valid
    ('both lists empty', [0, 0, 0, 0], [0, 0, 0, 0], None, 0, (0, 0, 0, 0.0, 0)),
    # no kept step: not valid
    ('all ignored', [-1, -1, -1], [4, 5, 6], -1, None, (0, 0, 0, 0.0, 0)),
    # A bg A stays [A, A]: against a prediction of one A that is one insertion
    ('background neighbours not merged', [7, 7, 0, 0, 7, 7], [7, 7, 7, 7, 7, 7], None, 0, (1, 2, 1, 50.0, 1)),
    # ... whereas an IGNORED stretch between two runs of one label makes them one segment, in both sequences
    ('ignored stretch merges', [7, 7, -1, -1, 7, 7], [7, 7, 3, 3, 7, 7], -1, None, (0, 1, 1, 100.0, 1)),
    # an ignored tail hides what the prediction does there; without the ignore value -1 is a label like any other
    ('ignored tail', [1, 1, 2, 2, -1, -1], [1, 1, 2, 2, 5, 6], -1, None, (0, 2, 2, 100.0, 1)),
    ('tail not ignored', [1, 1, 2, 2, -1, -1], [1, 1, 2, 2, 5, 6], None, None, (2, 3, 4, 50.0, 1)),
    # over-segmentation: one flicker inserts two segments
    ('flicker', [1, 1, 1, 1, 2, 2, 2, 2], [1, 1, 2, 1, 2, 2, 2, 2], None, None, (2, 2, 4, 50.0, 1)),
]
