#!/usr/bin/env python3
"""Cost of the segmental edit score inside EvaluationAccumulator.update, two accumulators alternated in one process on one
device, both on the workgroup F1 route:

  edit_off   update(edit=False): twog_eval_update, twog_segment_f1, twog_segment_f1_accumulate -- three launches per
             output, what the accumulator does without the metric.
  edit_on    update(edit=True): the same plus twog_segment_edit and a second twog_segment_f1_accumulate: five launches.

After a warm-up the two take turns in windows of --seconds each, --windows times round; inside a window every call is
timed by device events and by a host clock that ends in a synchronise. Per route: the median over all its windows, and the
medians of its single windows, whose range is the spread a difference between the two has to exceed. The shapes are those
of tools/segment_metrics_cost.py. Then twog_segment_edit alone: on the labels of each shape (back-to-back launches between
two events, divided by their number: typical tables of a few dozen segments, where the barrier per diagonal is what is
paid), and one launch at a time of its worst case, 64 sequences of max_steps steps with a new label at every step in both
sequences (m = n = max_steps: 2 * max_steps diagonals of up to max_steps + 1 cells).
Writes profiles/segment_edit_cost.json.   python tools/segment_edit_cost.py [--seconds 2] [--windows 3]
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


def events_ms(fn, launches):
    """Device time of `launches` back-to-back calls of fn, per call."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seconds', type=float, default=2.0, help='one window of one route')
    ap.add_argument('--windows', type=int, default=3, help='windows per route and shape')
    ap.add_argument('--rounds', type=int, default=0, help='fixed number of calls per window instead of a duration')
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--worst-launches', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'segment_edit_cost.json'))
    args = ap.parse_args()
    import twog_gcn_amd  # noqa: F401
    from twog_gcn_amd import postprocess as pp
    from twog_gcn_amd.hostcpu import limit_host_threads
    from twog_gcn_amd.kernels import get_kernels
    limit_host_threads()
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    dev = torch.device('cuda', 0)
    K = get_kernels()
    assert K.name == 'hip'
    max_steps = K.segment_edit_limits()
    bs, ds = 128, 3
    shapes = {'predict_batch': dict(T=120, T_tgt=360, heads=[(13, 2)]),
              'cad120_two_heads': dict(T=120, T_tgt=360, heads=[(10, 1), (12, 5)]),
              'predict_batch_unstructured': dict(T=120, T_tgt=360, heads=[(13, 2)], runs=False)}
    overlaps = (0.1, 0.25, 0.5)
    res = dict(device=torch.cuda.get_device_name(0), clips=bs, downsampling=ds, overlaps=overlaps,
               segment_edit_max_steps=max_steps, window_seconds=args.seconds, windows_per_route=args.windows, shapes={})
    med = statistics.median
    for name, sh in shapes.items():
        rng = np.random.RandomState(0)
        outs, tgts = [], []
        for C, E in sh['heads']:
            logp, tgt = synthetic_head(rng, bs, C, sh['T'], E, sh['T_tgt'], ds, sh.get('runs', True))
            outs.append(torch.from_numpy(logp).to(dev))
            tgts.append(torch.from_numpy(tgt).to(dev))
        names = [f'head{i}' for i in range(len(outs))]
        classes = [C for C, _ in sh['heads']]
        accs = {'edit_off': pp.EvaluationAccumulator(names, classes, downsampling=ds, overlaps=overlaps, f1_route='workgroup'),
                'edit_on': pp.EvaluationAccumulator(names, classes, downsampling=ds, overlaps=overlaps, f1_route='workgroup',
                                                    edit=True)}
        routes = {k: (lambda a=a: a.update(outs, tgts)) for k, a in accs.items()}
        for _ in range(args.warmup):
            for fn in routes.values():
                fn()
        torch.cuda.synchronize()
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
        summary = lambda windows: dict(median_ms=med([v for w in windows for v in w]), window_medians_ms=[med(w) for w in windows],
                                       calls=sum(len(w) for w in windows))
        # the kernel alone, on the labels eval_update writes for this shape
        alone, segments = [], []
        for out, tgt, C in zip(outs, tgts, classes):
            state = K.zeros(C * C + 2, dtype=torch.int64, device=dev)
            labels, kept = K.eval_update(out, ds, tgt, None, state[:-2].view(C, C), state[-2:], want_labels=True)
            edit = lambda: K.segment_edit(kept, labels, -1, None, entity_minor=True)
            f1 = lambda: K.segment_f1(kept, labels, C, overlaps, -1, entity_minor=True)
            edit(), f1()
            torch.cuda.synchronize()
            _, _, n_true, n_pred, valid, _ = edit()
            segments.append(dict(sequences=int(valid.numel()), mean_true_segments=float(n_true.double().mean()),
                                 mean_predicted_segments=float(n_pred.double().mean()),
                                 most_diagonals=int((n_true + n_pred).max())))
            alone.append(dict(segment_edit_us=1e3 * med([events_ms(edit, 200) for _ in range(5)]),
                              segment_f1_us=1e3 * med([events_ms(f1, 200) for _ in range(5)])))
        result = {'edit_on': accs['edit_on'].result()}
        res['shapes'][name] = dict(
            T=sh['T'], T_tgt=sh['T_tgt'], label_runs=sh.get('runs', True), heads=[dict(classes=C, entities=E) for C, E in sh['heads']],
            sequences=sum(bs * E for _, E in sh['heads']),
            device_events={k: summary(v) for k, v in event_ms.items()},
            host_clock_with_sync={k: summary(v) for k, v in wall_ms.items()},
            launches_per_update={'edit_off': 3 * len(outs), 'edit_on': 5 * len(outs)},
            kernel_alone_back_to_back=alone, tables=segments,
            edit_score={n: result['edit_on'][n]['edit'] for n in names})
    # the worst case: a new label at every step of both sequences
    rng = np.random.RandomState(1)
    flicker = lambda: torch.from_numpy((np.cumsum(rng.randint(1, 6, size=(64, max_steps)), axis=1) % 7).astype(np.int64)).to(dev)
    yt, yp = flicker(), flicker()
    worst = lambda: K.segment_edit(yt, yp, -1, None)
    _, distance, n_true, n_pred, _, _ = worst()
    torch.cuda.synchronize()
    assert int(n_true.min()) == int(n_pred.min()) == max_steps
    times = [events_ms(worst, 1) for _ in range(args.worst_launches)]
    res['worst_case'] = dict(sequences=64, steps=max_steps, true_segments=max_steps, predicted_segments=max_steps,
                             diagonals=2 * max_steps + 1, launch_ms_median=med(times), launch_ms_min=min(times),
                             launch_ms_max=max(times), launches=len(times), mean_distance=float(distance.double().mean()))
    if args.out != '/dev/null':
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
    print(json.dumps({**{k: {r: s['median_ms'] for r, s in v['device_events'].items()} for k, v in res['shapes'].items()},
                      'worst_case_ms': res['worst_case']['launch_ms_median']}))


if __name__ == '__main__':
    main()
