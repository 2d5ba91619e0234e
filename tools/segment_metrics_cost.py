#!/usr/bin/env python3
"""Cost of the segmental F1@k inside EvaluationAccumulator.update, four routes alternated in one process on one device:

  thread       update(f1_route='thread'): twog_eval_update, two transposed copies of the labels and, per overlap,
               twog_f1_at_k (one thread per sequence) with its sums -- the route the accumulator had before.
  workgroup    update(f1_route='workgroup'): twog_eval_update, one twog_segment_f1 (a workgroup per sequence, all overlaps),
               one twog_segment_f1_accumulate: three launches per output.
  counts_only  update with no overlaps: the confusion counts alone.
  host         what a caller had before the accumulator: predict_labels, .cpu() of the labels, numpy.bincount, and
               scikit-learn's micro + macro where it imports (no F1@k at all).

After a warm-up the routes take turns in windows of --seconds each, --windows times round; inside a window every call is
timed by device events and by a host clock that ends in a synchronise. Per route: the median over all its windows, and
the medians of its single windows, whose range is the spread a difference between two routes has to exceed. The shapes
are those of tools/evaluation_cost.py. Kernel times come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/segment_metrics_cost.py --rounds 20 --out /dev/null` run.
Writes profiles/segment_metrics_cost.json.   python tools/segment_metrics_cost.py [--seconds 3] [--windows 2]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from evaluation_cost import synthetic_head  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seconds', type=float, default=3.0, help='one window of one route')
    ap.add_argument('--windows', type=int, default=2, help='windows per route and shape')
    ap.add_argument('--rounds', type=int, default=0, help='fixed number of calls per window instead of a duration')
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'segment_metrics_cost.json'))
    args = ap.parse_args()
    import twog_gcn_amd  # noqa: F401
    from twog_gcn_amd import postprocess as pp
    from twog_gcn_amd.hostcpu import limit_host_threads
    from twog_gcn_amd.kernels import get_kernels
    limit_host_threads()
    try:
        from sklearn.metrics import precision_recall_fscore_support
    except ImportError:
        precision_recall_fscore_support = None
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    dev = torch.device('cuda', 0)
    K = get_kernels()
    assert K.name == 'hip'
    _, per_trip = K.eval_limits()
    max_steps, max_overlaps = K.segment_f1_limits()
    bs, ds = 128, 3
    long_T_tgt = per_trip // (bs * 2) + 37
    shapes = {'predict_batch': dict(T=120, T_tgt=360, heads=[(13, 2)]),
              'cad120_two_heads': dict(T=120, T_tgt=360, heads=[(10, 1), (12, 5)]),
              'long': dict(T=(long_T_tgt + ds - 1) // ds, T_tgt=long_T_tgt, heads=[(13, 2)]),
              'predict_batch_unstructured': dict(T=120, T_tgt=360, heads=[(13, 2)], runs=False)}
    overlaps = (0.1, 0.25, 0.5)
    res = dict(device=torch.cuda.get_device_name(0), clips=bs, downsampling=ds, overlaps=overlaps,
               scikit_learn=precision_recall_fscore_support is not None, segment_f1_max_steps=max_steps,
               segment_f1_max_overlaps=max_overlaps, window_seconds=args.seconds, windows_per_route=args.windows, shapes={})
    for name, sh in shapes.items():
        rng = np.random.RandomState(0)
        outs, tgts_host = [], []
        for C, E in sh['heads']:
            logp, tgt = synthetic_head(rng, bs, C, sh['T'], E, sh['T_tgt'], ds, sh.get('runs', True))
            outs.append(torch.from_numpy(logp).to(dev))
            tgts_host.append(torch.from_numpy(tgt))
        tgts = [t.to(dev) for t in tgts_host]
        names = [f'head{i}' for i in range(len(outs))]
        classes = [C for C, _ in sh['heads']]
        accs = {'thread': pp.EvaluationAccumulator(names, classes, downsampling=ds, overlaps=overlaps, f1_route='thread'),
                'workgroup': pp.EvaluationAccumulator(names, classes, downsampling=ds, overlaps=overlaps, f1_route='workgroup'),
                'counts_only': pp.EvaluationAccumulator(names, classes, downsampling=ds, overlaps=())}

        def host_route():
            for out, tgt, C in zip(outs, tgts_host, classes):
                labels = pp.predict_labels(out, tgt, ds).cpu().numpy().reshape(-1)
                truth = tgt.numpy().reshape(-1)
                keep = truth != -1
                np.bincount(truth[keep] * C + labels[keep], minlength=C * C).reshape(C, C)
                if precision_recall_fscore_support is not None:
                    for average in ('micro', 'macro'):
                        precision_recall_fscore_support(truth[keep], labels[keep], average=average, zero_division=0)

        routes = {k: (lambda a=a: a.update(outs, tgts)) for k, a in accs.items()}
        routes['host'] = host_route
        for _ in range(args.warmup):
            for fn in routes.values():
                fn()
        torch.cuda.synchronize()
        assert accs['workgroup'].last_f1_route == 'workgroup' and accs['thread'].last_f1_route == 'thread'
        event_ms = {k: [] for k in routes}     # per route: one list per window
        wall_ms = {k: [] for k in routes}
        for _ in range(args.windows):
            for k, fn in routes.items():
                ev, wall = [], []
                t_end = time.perf_counter() + args.seconds
                while (len(wall) < args.rounds) if args.rounds else (time.perf_counter() < t_end):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0 = time.perf_counter()
                    a.record()
                    fn()
                    b.record()
                    torch.cuda.synchronize()
                    wall.append((time.perf_counter() - t0) * 1e3)
                    ev.append(a.elapsed_time(b))
                event_ms[k].append(ev)
                wall_ms[k].append(wall)
        med = statistics.median
        summary = lambda windows: dict(median_ms=med([v for w in windows for v in w]), window_medians_ms=[med(w) for w in windows],
                                       calls=sum(len(w) for w in windows))
        launches = 3 * len(outs)               # eval_update, segment_f1, segment_f1_accumulate per output
        wg_events = med([v for w in event_ms['workgroup'] for v in w])
        # the two routes agree (fp32 per-sequence values on the thread route)
        f1 = {k: accs[k].result() for k in ('thread', 'workgroup')}
        agree = max(abs(f1['thread'][n]['f1@k'][ov] - f1['workgroup'][n]['f1@k'][ov]) for n in names for ov in overlaps)
        res['shapes'][name] = dict(
            T=sh['T'], T_tgt=sh['T_tgt'], label_runs=sh.get('runs', True), heads=[dict(classes=C, entities=E) for C, E in sh['heads']],
            sequences=sum(bs * E for _, E in sh['heads']),
            device_events={k: summary(v) for k, v in event_ms.items() if k != 'host'},
            host_clock_with_sync={k: summary(v) for k, v in wall_ms.items()},
            workgroup_launches_per_update=launches, workgroup_us_per_launch_device_events=1e3 * wg_events / launches,
            max_abs_f1_difference_thread_vs_workgroup=agree)
    if args.out != '/dev/null':
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
    print(json.dumps({k: {r: s['median_ms'] for r, s in v['host_clock_with_sync'].items()} for k, v in res['shapes'].items()}))


if __name__ == '__main__':
    main()
