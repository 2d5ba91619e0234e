#!/usr/bin/env python3
"""Cost of the Viterbi decode (twog_viterbi_decode) beside the per-step argmax it replaces, in one process on one device.

  labels     per output head of one evaluation batch (128 clips; the MPHOI and the CAD-120 output shapes of bench.py's
             configurations): `predict_labels` (twog_predict_labels) and `ViterbiDecoder` on the same tensors, taking
             turns in windows of --seconds each, --windows times round; every call timed by device events and by a host
             clock that ends in a synchronise. Reported: the median over all windows of a route, the medians of its
             single windows (their range is the spread a difference has to exceed), and the ratio decode / argmax.
  update     EvaluationAccumulator.update (workgroup F1 route, edit score on) without and with a decoder, the same way.
  worst      the worst case the limits admit, alone: 64 sequences of max_classes classes and max_steps model steps, the
             back-pointers in the caller's workspace; one launch at a time.

Writes profiles/viterbi_cost.json.   python tools/viterbi_cost.py [--seconds 2] [--windows 3]
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

med = statistics.median


def alternate(routes, seconds, windows, rounds, warmup):
    """{route: {'device_events': summary, 'host_clock_with_sync': summary}} of callables that take turns in windows."""
    for _ in range(warmup):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    event_ms, wall_ms = {k: [] for k in routes}, {k: [] for k in routes}
    for _ in range(windows):
        for k, fn in routes.items():
            ev, wall = [], []
            t_end = time.perf_counter() + seconds
            while (len(wall) < rounds) if rounds else (time.perf_counter() < t_end):
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
    summary = lambda ws: dict(median_ms=med([v for w in ws for v in w]), window_medians_ms=[med(w) for w in ws],
                              calls=sum(len(w) for w in ws))
    return {k: dict(device_events=summary(event_ms[k]), host_clock_with_sync=summary(wall_ms[k])) for k in routes}


def ratio(res, num, den, clock='device_events'):
    return res[num][clock]['median_ms'] / res[den][clock]['median_ms']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seconds', type=float, default=2.0, help='one window of one route')
    ap.add_argument('--windows', type=int, default=3, help='windows per route and shape')
    ap.add_argument('--rounds', type=int, default=0, help='fixed number of calls per window instead of a duration')
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--worst-launches', type=int, default=10)
    ap.add_argument('--penalty', type=float, default=2.0, help='the switch penalty of the transition model')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'viterbi_cost.json'))
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
    max_classes, max_steps = K.viterbi_limits()
    bs, ds = 128, 3
    shapes = {'mphoi': dict(T=120, T_tgt=360, heads=[(13, 2)]),
              'cad120': dict(T=120, T_tgt=360, heads=[(10, 1), (12, 5)])}
    overlaps = (0.1, 0.25, 0.5)
    res = dict(device=torch.cuda.get_device_name(0), clips=bs, downsampling=ds, overlaps=overlaps, switch_penalty=args.penalty,
               viterbi_limits=[max_classes, max_steps], window_seconds=args.seconds, windows_per_route=args.windows, shapes={})
    for name, sh in shapes.items():
        rng = np.random.RandomState(0)
        outs, tgts = [], []
        for C, E in sh['heads']:
            logp, tgt = synthetic_head(rng, bs, C, sh['T'], E, sh['T_tgt'], ds, True)
            outs.append(torch.from_numpy(logp).to(dev))
            tgts.append(torch.from_numpy(tgt).to(dev))
        names = [f'head{i}' for i in range(len(outs))]
        classes = [C for C, _ in sh['heads']]
        decoders = [pp.ViterbiDecoder(pp.switch_penalty(C, args.penalty)) for C in classes]
        heads = []
        for out, tgt, dec, (C, E) in zip(outs, tgts, decoders, sh['heads']):
            routes = {'argmax': lambda out=out, tgt=tgt: pp.predict_labels(out, tgt, ds),
                      'viterbi': lambda out=out, tgt=tgt, dec=dec: dec(out, tgt, ds)}
            timed = alternate(routes, args.seconds, args.windows, args.rounds, args.warmup)
            changed = float((routes['argmax']() != routes['viterbi']()).double().mean())
            heads.append(dict(classes=C, entities=E, sequences=bs * E, route=K.viterbi_route(bs, C, sh['T'], E)[0], **timed,
                              viterbi_over_argmax=ratio(timed, 'viterbi', 'argmax'), share_of_labels_changed=changed))
        kwargs = dict(downsampling=ds, overlaps=overlaps, f1_route='workgroup', edit=True)
        accs = {'argmax': pp.EvaluationAccumulator(names, classes, **kwargs),
                'viterbi': pp.EvaluationAccumulator(names, classes, decoder=decoders, **kwargs)}
        timed = alternate({k: (lambda a=a: a.update(outs, tgts)) for k, a in accs.items()}, args.seconds, args.windows,
                          args.rounds, args.warmup)
        result = {k: a.result() for k, a in accs.items()}
        res['shapes'][name] = dict(
            T=sh['T'], T_tgt=sh['T_tgt'], labels=heads,
            update=dict(**timed, viterbi_over_argmax=ratio(timed, 'viterbi', 'argmax'),
                        viterbi_over_argmax_host=ratio(timed, 'viterbi', 'argmax', 'host_clock_with_sync'),
                        edit={k: {n: r[n]['edit'] for n in names} for k, r in result.items()},
                        f1_at_50={k: {n: r[n]['f1@k'][0.5] for n in names} for k, r in result.items()}))
    # the worst case the limits admit
    rng = np.random.RandomState(1)
    logp = torch.log_softmax(torch.from_numpy(rng.randn(64, max_classes, max_steps, 1).astype(np.float32)), 1).to(dev)
    worst_decoder = pp.ViterbiDecoder(rng.randn(max_classes, max_classes).astype(np.float32))
    route, ws_bytes = K.viterbi_route(64, max_classes, max_steps, 1)
    assert route == 'workspace'
    worst = lambda: worst_decoder(logp)
    worst()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.worst_launches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        worst()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    res['worst_case'] = dict(sequences=64, classes=max_classes, steps=max_steps, route=route, workspace_bytes=ws_bytes,
                             launch_ms_median=med(times), launch_ms_min=min(times), launch_ms_max=max(times), launches=len(times),
                             ns_per_step=1e6 * med(times) / max_steps)
    if args.out != '/dev/null':
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
    print(json.dumps({**{k: dict(labels=[h['viterbi_over_argmax'] for h in v['labels']], update=v['update']['viterbi_over_argmax'])
                         for k, v in res['shapes'].items()}, 'worst_case_ms': res['worst_case']['launch_ms_median']}))


if __name__ == '__main__':
    main()
