#!/usr/bin/env python3
"""Cost of the segmental decode (twog_segdecode) beside the Viterbi decode and the per-step argmax, in one process on one
device.

  labels     per output head of one evaluation batch (128 clips of 120 model steps; the MPHOI and the CAD-120 output shapes
             of bench.py's configurations): `predict_labels` (twog_predict_labels), `ViterbiDecoder` and `SegmentalDecoder`
             at D = 32 and at D = 120 on the same tensors, taking turns in windows of --seconds each, --windows times
             round (tools/viterbi_cost.py's `alternate`); every call timed by device events and by a host clock that ends
             in a synchronise. Reported: the median over all windows of a route, the medians of its single windows (their
             range is the spread a difference has to exceed), and the ratios to the Viterbi launch and to the argmax.
             The model is made the way a user makes it: duration_counts -> duration_log_probs, transition_counts ->
             segment_transition_log_probs of the batch's own targets.
  worst      the worst case the limits admit, alone: 64 sequences of max_classes classes, max_steps model steps and the
             longest duration, the back-pointers in the caller's workspace; one launch at a time, beside the Viterbi
             decode of the same tensor.

Writes profiles/segment_decode_cost.json.   python tools/segment_decode_cost.py [--seconds 1] [--windows 3]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from evaluation_cost import synthetic_head  # noqa: E402
from viterbi_cost import alternate, ratio  # noqa: E402

med = statistics.median


def launches(fn, n):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return dict(launch_ms_median=med(times), launch_ms_min=min(times), launch_ms_max=max(times), launches=len(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seconds', type=float, default=1.0, help='one window of one route')
    ap.add_argument('--windows', type=int, default=3, help='windows per route and shape')
    ap.add_argument('--rounds', type=int, default=0, help='fixed number of calls per window instead of a duration')
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--worst-launches', type=int, default=10)
    ap.add_argument('--self-transition', type=float, default=-2.0, help='A[c][c] of the segment model')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'segment_decode_cost.json'))
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
    max_classes, max_steps, max_duration = K.segdecode_limits()
    bs, ds, T, T_tgt = 128, 3, 120, 360
    durations = (32, 120)
    shapes = {'mphoi': [(13, 2)], 'cad120': [(10, 1), (12, 5)]}
    res = dict(device=torch.cuda.get_device_name(0), clips=bs, downsampling=ds, T=T, T_tgt=T_tgt, durations=durations,
               self_transition=args.self_transition, segdecode_limits=[max_classes, max_steps, max_duration],
               window_seconds=args.seconds, windows_per_route=args.windows, shapes={})
    for name, heads in shapes.items():
        rng = np.random.RandomState(0)
        rows = []
        for C, E in heads:
            logp, tgt = synthetic_head(rng, bs, C, T, E, T_tgt, ds, True)
            out, tgt = torch.from_numpy(logp).to(dev), torch.from_numpy(tgt).to(dev)
            frames = pp.transition_counts(tgt, C, stride=ds)
            A = pp.segment_transition_log_probs(frames, 1.0, self_transition=args.self_transition)
            decoders = {'viterbi': pp.ViterbiDecoder(pp.transition_log_probs(frames, 1.0))}
            plans = {}
            for D in durations:
                dur = pp.duration_log_probs(pp.duration_counts(tgt, C, D, stride=ds), 1.0)
                decoders[f'segmental_D{D}'] = pp.SegmentalDecoder(A, dur)
                plans[f'segmental_D{D}'] = K.segdecode_plan(bs, C, T, E, D)
            routes = {'argmax': lambda out=out, tgt=tgt: pp.predict_labels(out, tgt, ds)}
            routes.update({k: (lambda out=out, tgt=tgt, dec=dec: dec(out, tgt, ds)) for k, dec in decoders.items()})
            timed = alternate(routes, args.seconds, args.windows, args.rounds, args.warmup)
            plain = routes['argmax']()
            rows.append(dict(classes=C, entities=E, sequences=bs * E, plans=plans, **timed,
                             over_viterbi={k: ratio(timed, k, 'viterbi') for k in plans},
                             over_argmax={k: ratio(timed, k, 'argmax') for k in decoders},
                             share_of_labels_changed={k: float((routes[k]() != plain).double().mean()) for k in decoders}))
        res['shapes'][name] = rows
    # the worst case the limits admit
    rng = np.random.RandomState(1)
    logp = torch.log_softmax(torch.from_numpy(rng.randn(64, max_classes, max_steps, 1).astype(np.float32)), 1).to(dev)
    A = rng.randn(max_classes, max_classes).astype(np.float32)
    segmental = pp.SegmentalDecoder(A, rng.randn(max_classes, max_duration).astype(np.float32))
    viterbi = pp.ViterbiDecoder(A)
    plan = K.segdecode_plan(64, max_classes, max_steps, 1, max_duration)
    assert plan['route'] == 'workspace'
    worst = launches(lambda: segmental(logp), args.worst_launches)
    beside = launches(lambda: viterbi(logp), args.worst_launches)
    res['worst_case'] = dict(sequences=64, classes=max_classes, steps=max_steps, duration=max_duration, plan=plan, **worst,
                             ns_per_step=1e6 * worst['launch_ms_median'] / max_steps,
                             ns_per_step_and_duration=1e6 * worst['launch_ms_median'] / max_steps / max_duration,
                             viterbi=beside, over_viterbi=worst['launch_ms_median'] / beside['launch_ms_median'])
    if args.out != '/dev/null':
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
    print(json.dumps({**{k: [dict(ms={r: h[r]['device_events']['median_ms'] for r in ('argmax', 'viterbi', 'segmental_D32',
                                                                                     'segmental_D120')},
                                  over_viterbi=h['over_viterbi']) for h in v] for k, v in res['shapes'].items()},
                      'worst_case_ms': res['worst_case']['launch_ms_median'],
                      'worst_case_viterbi_ms': res['worst_case']['viterbi']['launch_ms_median']}))


if __name__ == '__main__':
    main()
