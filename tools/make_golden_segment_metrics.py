#!/usr/bin/env python3
"""Generate tests/golden/g17_segment_metrics.npz: the reference's per-example segmental F1@k on seeded label matrices.

Runs only where the reference checkout is present (never on the GPU machine). pyrutils.metrics imports cleanly;
predict.py imports omegaconf and the data loaders at module level, so dump_f1_scores_per_example is loaded by slicing its
source at run time, the way G15 loads its functions (tools/make_golden_evaluation.py); none of that text is kept here.
The fixture holds, per label matrix, the labels, num_classes, f1_at_k_single_example of every sequence with a kept step
at 0.10 / 0.25 / 0.50 (fp64; 0 and valid 0 for a sequence the reference skips) and f1_at_k of the matrix; and for a case
with two problem types of (N, T, E) labels the text dump_f1_scores_per_example wrote at each overlap.
Usage:  python tools/make_golden_segment_metrics.py [--out FILE | --check]
(--check regenerates in memory and compares every array with the committed fixture, bit for bit.)
"""
import argparse
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('TWOG_REFERENCE', '/root/reference')
sys.path.insert(0, REF)
from pyrutils.metrics import f1_at_k, f1_at_k_single_example  # noqa: E402

OVERLAPS = (0.1, 0.25, 0.5)


def load_dump_function():
    src = open(os.path.join(REF, 'predict.py')).read()
    ns = {'os': os, 'f1_at_k_single_example': f1_at_k_single_example}
    first, after = 'def dump_f1_scores_per_example(', 'def to_dict('
    exec(compile(src[src.index(first):src.index(after)], 'predict_slice', 'exec'), ns)
    return ns['dump_f1_scores_per_example']


def runs(rng, n_steps, n_labels, longest):
    """A label sequence of n_steps whose labels hold for 1..longest steps."""
    return np.repeat(rng.randint(0, n_labels, size=n_steps), rng.randint(1, longest + 1, size=n_steps))[:n_steps]


def pad(rows, width):
    return np.array([list(r) + [-1] * (width - len(r)) for r in rows], dtype=np.int64)


def build_matrices():
    rng = np.random.RandomState(17)
    m = {}
    # hand-written situations, 3 classes (label 3 and above is not a class), padded to 14 steps with -1
    true = [[-1] * 14,                                   # fully ignored
            [2],                                         # one step
            [0, 0, 1, 0, 0],                             # exact IoU tie between the two 0-segments: the first must win
            [0, 0, 1, 1, 2, 2, 0, 0, 1, 1, 2, 2],        # one predicted segment over many target segments
            [0, 0, -1, -1, 0, 1, 1, -1, 2, 2],           # -1 inside (the two 0-runs join) and at the end
            [0, 0, 0, 1, 1, 1, 2, 2, 2],                 # predictions at or above num_classes
            [1, 1, 1, 1, 2, 2, 2, 2],                    # two predicted segments on one target segment, both over 0.25
            [0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1]]  # a new label every step
    pred = [[0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1],
            [2],
            [0, 0, 0, 0, 0],
            [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1],
            [0, 0, 2, 1, 0, 0, 1, 1, 2, 2],
            [0, 0, 3, 3, 1, 1, 4, 2, 2],
            [1, 1, 0, 1, 1, 2, 2, 2],
            [0, 1, 1, 1, 0, 0, 0, 1, 0, 1, 0, 0, 0, 1]]
    m['edge'] = (pad(true, 14), pad(pred, 14), 3)
    # longer than 256 steps: six sequences, labels 0..5 of which 5 is not a class, -1 inside and a padded tail
    n_seq, n_steps = 6, 300
    yt = np.stack([runs(rng, n_steps, 6, 9) for _ in range(n_seq)]).astype(np.int64)
    yp = np.stack([runs(rng, n_steps, 6, 9) for _ in range(n_seq)]).astype(np.int64)
    yp[:4] = yt[:4]
    yp[:4, ::11] = (yp[:4, ::11] + 1) % 6
    yp[1] = np.roll(yt[1], 3)
    yt[rng.rand(n_seq, n_steps) < 0.05] = -1
    for s in range(n_seq):
        yt[s, n_steps - rng.randint(0, 60):] = -1
    m['over256'] = (yt, yp, 5)
    # longer than 1 024 steps
    n_seq, n_steps = 3, 1100
    yt = np.stack([runs(rng, n_steps, 4, 25) for _ in range(n_seq)]).astype(np.int64)
    yp = np.stack([np.roll(yt[s], rng.randint(-8, 9)) for s in range(n_seq)]).astype(np.int64)
    yp[:, ::37] = (yp[:, ::37] + 1) % 4
    yp[2] = runs(rng, n_steps, 4, 3)
    yt[rng.rand(n_seq, n_steps) < 0.02] = -1
    yt[0, 1000:] = -1
    m['over1024'] = (yt, yp, 4)
    return m


def build_dump_case():
    """{problem_type: (target, output) of (N, T, E) labels}: one human for the sub-activity, three objects for the
    affordance of which some have no target step at all."""
    rng = np.random.RandomState(171)
    N, T = 4, 40
    case = {}
    for name, E, n_names in (('sub-activity_recognition', 1, 5), ('affordance_recognition', 3, 4)):
        tgt = np.stack([np.stack([runs(rng, T, n_names, 8) for _ in range(E)], -1) for _ in range(N)]).astype(np.int64)
        out = np.where(rng.rand(N, T, E) < 0.8, tgt, rng.randint(0, n_names + 1, size=(N, T, E))).astype(np.int64)
        for n in range(N):
            tgt[n, T - rng.randint(0, 12):] = -1
        if E > 1:
            tgt[1, :, 2] = -1                              # an object that does not exist in this clip
            tgt[3, :, 0] = -1
        case[name] = (tgt, out, n_names)
    return case, ['task1_vid07', 'task1_vid11', 'task3_vid02', 'task9_vid30']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'g17_segment_metrics.npz'))
    ap.add_argument('--check', action='store_true', help='compare with the existing fixture instead of writing it')
    args = ap.parse_args()
    out = {'overlaps': np.array(OVERLAPS, dtype=np.float64)}
    matrices = build_matrices()
    out['matrices'] = np.array(list(matrices))
    for name, (yt, yp, ncls) in matrices.items():
        f1 = np.zeros((yt.shape[0], len(OVERLAPS)), dtype=np.float64)
        valid = np.zeros(yt.shape[0], dtype=np.int32)
        for s in range(yt.shape[0]):
            keep = yt[s] != -1.0                            # the filter of metrics.py:73-76
            if not keep.any():
                continue
            valid[s] = 1
            for k, ov in enumerate(OVERLAPS):
                f1[s, k] = f1_at_k_single_example(yt[s][keep], yp[s][keep], ncls, overlap=ov)
        out[f'{name}_true'], out[f'{name}_pred'], out[f'{name}_ncls'] = yt, yp, np.array(ncls)
        out[f'{name}_f1'], out[f'{name}_valid'] = f1, valid
        out[f'{name}_mean'] = np.array([f1_at_k(yt, yp, ncls, overlap=ov, ignore_value=-1.0) for ov in OVERLAPS], dtype=np.float64)
    dump = load_dump_function()
    case, test_ids = build_dump_case()
    out['dump_types'], out['dump_test_ids'] = np.array(list(case)), np.array(test_ids)
    outputs, targets = {k: v[1] for k, v in case.items()}, {k: v[0] for k, v in case.items()}
    for name, (tgt, pred, n_names) in case.items():
        out[f'dump_{name}_target'], out[f'dump_{name}_output'], out[f'dump_{name}_n_names'] = tgt, pred, np.array(n_names)
    sub = {i: f'sub{i}' for i in range(case['sub-activity_recognition'][2])}
    aff = {i: f'aff{i}' for i in range(case['affordance_recognition'][2])}
    with tempfile.TemporaryDirectory() as tmp:
        for k, ov in enumerate(OVERLAPS):
            dump(tmp, outputs, targets, test_ids, sub, aff, ov)
            out[f'dump_text_{k}'] = np.array(open(os.path.join(tmp, f'f1_scores_{ov:.2f}.txt')).read())
    if args.check:
        have = np.load(args.out)
        assert sorted(have.files) == sorted(out), sorted(set(have.files) ^ set(out))
        for k, v in out.items():
            v = np.asarray(v)
            assert have[k].dtype == v.dtype and have[k].shape == v.shape and have[k].tobytes() == v.tobytes(), k
        print('g17:', len(out), 'arrays identical to', args.out)
        return
    np.savez_compressed(args.out, **out)
    print('g17:', len(out), 'arrays,', os.path.getsize(args.out), 'bytes')


if __name__ == '__main__':
    main()
