#!/usr/bin/env python3
"""Generate tests/golden/g15_evaluation.npz: the reference's frame-wise evaluation on seeded cases.

Runs only where the reference checkout and scikit-learn are present (never on the GPU machine). predict.py imports
omegaconf and the data loaders at module level, so the functions used here -- match_shape, downsample_bad_bimanual_videos,
summarize_frames_into_segments, process_output, evaluate_predictions -- are loaded by slicing its source at run time, the
way G8 loads match_shape (tools/make_golden.py); none of that text is kept here. The fixture holds the inputs (log-
probabilities, targets, the 15-fps flags / segment starts), the labels and targets the reference's pipeline ends with,
scikit-learn's confusion matrix, what evaluate_predictions returned, classification_report(output_dict=True) and
pyrutils.metrics.f1_at_k. Usage:  python tools/make_golden_evaluation.py [--out FILE | --check]
(--check regenerates in memory and compares every array with the committed fixture, bit for bit; the file itself carries
the zip member timestamps of the run that wrote it.)
"""
import argparse
from collections import defaultdict
import contextlib
import io
import os
import sys
import warnings

import numpy as np
import torch
from sklearn.metrics import classification_report, confusion_matrix, precision_recall_fscore_support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('TWOG_REFERENCE', '/root/reference')
sys.path.insert(0, REF)
from pyrutils.metrics import f1_at_k  # noqa: E402

OVERLAPS = (0.1, 0.25, 0.5)


def load_reference_functions():
    src = open(os.path.join(REF, 'predict.py')).read()
    ns = {'torch': torch, 'np': np, 'defaultdict': defaultdict, 'classification_report': classification_report,
          'precision_recall_fscore_support': precision_recall_fscore_support}
    for first, after in (('def match_shape(out, tgt):', 'def match_att_shape'),
                         ('def downsample_bad_bimanual_videos(', 'def evaluate_f1_at_k(')):
        exec(compile(src[src.index(first):src.index(after)], 'predict_slice', 'exec'), ns)
    return ns


def make_case(rng, heads, batches, T, T_tgt, ds, pad_tail=True):
    """heads: [(name, C, E, n_names)]; batches: clips per batch -> [[(logp, target) per head] per batch]."""
    data = []
    for bs in batches:
        lengths = rng.randint(max(1, T_tgt // 2), T_tgt + 1, size=bs) if pad_tail else np.full(bs, T_tgt)
        lengths[0] = T_tgt
        per_head = []
        for _, C, E, _ in heads:
            logp = torch.log_softmax(torch.from_numpy(rng.randn(bs, C, T, E).astype(np.float32) * 2.0), 1)
            tgt = rng.randint(0, C, size=(bs, T_tgt, E)).astype(np.int64)
            agree = rng.rand(bs, T_tgt, E) < 0.6          # make most targets agree with the prediction
            steps = np.minimum(np.arange(T_tgt) // ds, T - 1)
            tgt = np.where(agree, logp.numpy().argmax(1)[:, steps], tgt)
            for b, n in enumerate(lengths):
                tgt[b, n:] = -1                            # trailing padding
            per_head.append([logp, torch.from_numpy(tgt)])
        data.append(per_head)
    return data


def suppress_class(logp, c):
    logp[:, c] = logp.min() - 5.0   # class c is never predicted


def build_cases():
    rng = np.random.RandomState(15)
    cases = {}
    # a class never true (4), never predicted (3), absent from both (2); a logit tie; trailing padding; E > 1
    heads = [('sub-activity_recognition', 5, 2, 5)]
    d = make_case(rng, heads, [3], T=10, T_tgt=10, ds=1)
    logp, tgt = d[0][0]
    suppress_class(logp, 3)
    suppress_class(logp, 2)
    tgt[tgt == 4] = 0
    tgt[tgt == 2] = 1
    tgt[0, :3, 0] = 3
    logp[0, 1, 0, 0] = logp[0, 4, 0, 0] = logp[0].max() + 1.0   # tie: the first index wins
    cases['plain'] = dict(heads=heads, data=d, ds=1)
    # predicted labels beyond len(target_names): 6 classes, 4 names; E = 1; T_tgt shorter than T * ds
    heads = [('sub-activity_recognition', 6, 1, 4)]
    d = make_case(rng, heads, [4], T=7, T_tgt=19, ds=3)
    tgt = d[0][0][1]
    tgt[tgt >= 4] = 1
    cases['beyond_names'] = dict(heads=heads, data=d, ds=3)
    # ds 4 with T_tgt longer than T * ds, two batches
    heads = [('sub-activity_recognition', 12, 3, 12), ('sub-activity_prediction', 12, 3, 12)]
    cases['ds4_long'] = dict(heads=heads, data=make_case(rng, heads, [2, 3], T=6, T_tgt=26, ds=4), ds=4)
    # an output whose every target is -1
    heads = [('sub-activity_recognition', 4, 2, 4), ('sub-activity_prediction', 4, 2, 4)]
    d = make_case(rng, heads, [3], T=8, T_tgt=8, ds=1)
    d[0][1][1][:] = -1
    cases['all_ignored'] = dict(heads=heads, data=d, ds=1)
    # Bimanual: two 15-fps clips among normal ones, odd and even T_tgt
    heads = [('sub-activity_recognition', 14, 2, 14), ('sub-activity_prediction', 14, 2, 14)]
    for name, T_tgt in (('bimanual_odd', 23), ('bimanual_even', 22)):
        d = make_case(rng, heads, [5], T=8, T_tgt=T_tgt, ds=3)
        cases[name] = dict(heads=heads, data=d, ds=3, is_15fps=[False, True, False, False, True])
    # CAD-120: sub-activity heads over one human, affordance heads over the objects
    heads = [('sub-activity_recognition', 10, 1, 10), ('sub-activity_prediction', 10, 1, 10),
             ('affordance_recognition', 12, 5, 12), ('affordance_prediction', 12, 5, 12)]
    cases['cad120'] = dict(heads=heads, data=make_case(rng, heads, [3, 2], T=9, T_tgt=9, ds=1), ds=1)
    # frame -> segment level
    heads = [('sub-activity_recognition', 6, 2, 6), ('sub-activity_prediction', 6, 2, 6)]
    d = make_case(rng, heads, [3], T=12, T_tgt=12, ds=1, pad_tail=False)
    cases['segments'] = dict(heads=heads, data=d, ds=1, segment_starts=[[0, 3, 7], [0, 5], [0, 2, 4, 6, 11]])
    return cases


def run_reference(ref, case):
    heads, ds = case['heads'], case['ds']
    outputs, targets = [], []
    for per_head in case['data']:
        output = [lp.clone() for lp, _ in per_head]
        target = [t.clone() for _, t in per_head]
        if ds > 1:                                     # the loop of predict.py:64-70
            for i, (out, tgt) in enumerate(zip(output, target)):
                output[i] = ref['match_shape'](torch.repeat_interleave(out, repeats=ds, dim=-2), tgt)
        outputs.append(output)
        targets.append(target)
    if 'is_15fps' in case:
        ids = [f'v{i}' for i in range(len(case['is_15fps']))]
        fps = {v: 15 if f else 30 for v, f in zip(ids, case['is_15fps'])}
        outputs, targets = ref['downsample_bad_bimanual_videos'](outputs, targets, ids, fps)
    if 'segment_starts' in case:
        segmentations = [[(s, s) for s in starts] for starts in case['segment_starts']]
        outputs = ref['summarize_frames_into_segments'](outputs, segmentations, is_ground_truth=False)
        targets = ref['summarize_frames_into_segments'](targets, segmentations, is_ground_truth=True)
    index_to_name = {i: h[0] for i, h in enumerate(heads)}
    labels = ref['process_output'](outputs, is_ground_truth=False, index_to_name=index_to_name)
    truths = ref['process_output'](targets, is_ground_truth=True, index_to_name=index_to_name)
    return labels, truths


def row(d):
    return np.array([d['precision'], d['recall'], d['f1-score'], d['support']], dtype=np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'g15_evaluation.npz'))
    ap.add_argument('--check', action='store_true', help='compare with the existing fixture instead of writing it')
    args = ap.parse_args()
    ref = load_reference_functions()
    out = {}
    cases = build_cases()
    out['cases'] = np.array(list(cases))
    for cname, case in cases.items():
        heads = case['heads']
        out[f'{cname}_heads'] = np.array([h[0] for h in heads])
        out[f'{cname}_cfg'] = np.array([case['ds'], len(case['data'])] + [v for h in heads for v in h[1:]])
        for bi, per_head in enumerate(case['data']):
            for hi, (logp, tgt) in enumerate(per_head):
                out[f'{cname}_b{bi}_h{hi}_logp'] = logp.numpy().copy()
                out[f'{cname}_b{bi}_h{hi}_target'] = tgt.numpy().copy()
        if 'is_15fps' in case:
            out[f'{cname}_is_15fps'] = np.array(case['is_15fps'])
        if 'segment_starts' in case:
            width = max(len(s) for s in case['segment_starts'])
            out[f'{cname}_segment_starts'] = np.array([s + [-1] * (width - len(s)) for s in case['segment_starts']])
        labels, truths = run_reference(ref, case)
        sub_names = [f'sub{i}' for i in range(next((h[3] for h in heads if 'affordance' not in h[0]), 0))]
        aff_names = [f'aff{i}' for i in range(next((h[3] for h in heads if 'affordance' in h[0]), 0))]
        with warnings.catch_warnings(), contextlib.redirect_stdout(io.StringIO()):
            warnings.simplefilter('ignore')
            results = ref['evaluate_predictions'](truths, labels, print_report=True, subactivity_names=sub_names,
                                                  affordance_names=aff_names or None)
        for hi, (name, C, E, n_names) in enumerate(heads):
            y_pred, y_true = labels[name].astype(np.int64), truths[name].astype(np.int64)
            out[f'{cname}_h{hi}_labels'], out[f'{cname}_h{hi}_targets'] = y_pred, y_true
            keep = y_true.reshape(-1) != -1
            yt, yp = y_true.reshape(-1)[keep], y_pred.reshape(-1)[keep]
            out[f'{cname}_h{hi}_counts'] = confusion_matrix(yt, yp, labels=list(range(C))).astype(np.int64)
            for average in ('micro', 'macro'):
                r = results[f'{name}-{average}']
                out[f'{cname}_h{hi}_{average}'] = np.array([r['precision'], r['recall'], r['f1']], dtype=np.float64)
            names = aff_names if 'affordance' in name else sub_names
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                rep = classification_report(yt, yp, labels=list(range(n_names)), target_names=names, digits=4,
                                            output_dict=True)
            out[f'{cname}_h{hi}_report_classes'] = np.stack([row(rep[n]) for n in names])
            out[f'{cname}_h{hi}_report_accuracy'] = np.array(rep['accuracy'] if 'accuracy' in rep else np.nan)
            out[f'{cname}_h{hi}_report_micro'] = row(rep['micro avg']) if 'micro avg' in rep else np.full(4, np.nan)
            out[f'{cname}_h{hi}_report_macro'] = row(rep['macro avg'])
            out[f'{cname}_h{hi}_report_weighted'] = row(rep['weighted avg'])
            seq_t, seq_p = np.swapaxes(y_true, 1, 2), np.swapaxes(y_pred, 1, 2)   # the layout of evaluate_f1_at_k
            steps = seq_p.shape[-1]
            f1 = []
            for ov in OVERLAPS:
                try:
                    f1.append(f1_at_k(seq_t.reshape(-1, steps), seq_p.reshape(-1, steps), n_names, overlap=ov,
                                      ignore_value=-1.0))
                except ZeroDivisionError:              # no sequence with a counted step
                    f1.append(np.nan)
            out[f'{cname}_h{hi}_f1_at_k'] = np.array(f1, dtype=np.float64)
    if args.check:
        have = np.load(args.out)
        assert sorted(have.files) == sorted(out), sorted(set(have.files) ^ set(out))
        for k, v in out.items():
            v = np.asarray(v)
            assert have[k].dtype == v.dtype and have[k].shape == v.shape and have[k].tobytes() == v.tobytes(), k
        print('g15:', len(out), 'arrays identical to', args.out)
        return
    np.savez_compressed(args.out, **out)
    print('g15:', len(out), 'arrays,', os.path.getsize(args.out), 'bytes')


if __name__ == '__main__':
    main()
