#!/usr/bin/env python3
"""Cost of evaluating one batch of model outputs, two routes alternated in one process on one device:

  accumulator  EvaluationAccumulator.update -- twog_eval_update and, per overlap, twog_f1_at_k; nothing leaves the device.
               Timed by device events, and by a host clock that ends in a synchronise as well (the route is a string of
               small launches, so what the host spends enqueueing them is part of its cost).
  counts_only  the same with no overlaps: the confusion counts alone, which is all the other route computes.
  host         what a caller had before: predict_labels, .cpu() of the labels, confusion counts by numpy.bincount on the
               host (targets already there), and precision_recall_fscore_support micro + macro where scikit-learn
               imports. Host clock ending in a synchronise. host_counts_only stops after the bincount.

Shapes: predict.py's batch (128 clips, C 13, T 120, E 2, downsampling 3), the CAD-120 two-head layout (sub-activity C 10
E 1, affordance C 12 E 5) and a long shape that needs more than one trip of the capped grid, with labels that hold for
5-25 model steps; and predict.py's batch once more with a new label every step. Also records the bytes
crossing PCIe per batch for each route, computed from the shapes. Kernel times come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/evaluation_cost.py --rounds 20 --out /dev/null` run.
Writes profiles/evaluation_cost.json.   python tools/evaluation_cost.py [--seconds 3]
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


def synthetic_head(rng, bs, C, T, E, T_tgt, ds, runs):
    """Log-probabilities and targets of one head. With `runs` the predicted label holds for 5-25 model steps at a time,
    like a trained model's output (a sub-activity lasts seconds), and the target is that labelling with shifted
    boundaries; without, logits and targets are independent noise. Targets end in -1 padding of 0-20 % of the steps."""
    logits = rng.randn(bs, C, T, E).astype(np.float32)
    steps = np.minimum(np.arange(T_tgt) // ds, T - 1)
    if runs:
        lab = np.zeros((bs, T, E), dtype=np.int64)
        for b in range(bs):
            for e in range(E):
                t = 0
                while t < T:
                    n = rng.randint(5, 26)
                    lab[b, t:t + n, e] = rng.randint(0, C)
                    t += n
        np.put_along_axis(logits, lab[:, None], 6.0, axis=1)
        tgt = np.roll(lab[:, steps], rng.randint(-6, 7), axis=1)
    else:
        tgt = rng.randint(0, C, size=(bs, T_tgt, E))
    tgt = tgt.astype(np.int64)
    for b in range(bs):
        tgt[b, T_tgt - rng.randint(0, T_tgt // 5 + 1):] = -1
    return torch.log_softmax(torch.from_numpy(logits), 1).numpy(), tgt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seconds', type=float, default=3.0, help='timed window per shape')
    ap.add_argument('--rounds', type=int, default=0, help='fixed number of rounds per shape instead of a window')
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'evaluation_cost.json'))
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
    bs, ds = 128, 3
    long_T_tgt = per_trip // (bs * 2) + 37
    shapes = {'predict_batch': dict(T=120, T_tgt=360, heads=[(13, 2)]),
              'cad120_two_heads': dict(T=120, T_tgt=360, heads=[(10, 1), (12, 5)]),
              'long': dict(T=(long_T_tgt + ds - 1) // ds, T_tgt=long_T_tgt, heads=[(13, 2)]),
              # the worst case of the F1@k kernel (one thread per sequence, segments x segments): a new label every step
              'predict_batch_unstructured': dict(T=120, T_tgt=360, heads=[(13, 2)], runs=False)}
    overlaps = (0.1, 0.25, 0.5)
    res = dict(device=torch.cuda.get_device_name(0), clips=bs, downsampling=ds, overlaps=overlaps,
               scikit_learn=precision_recall_fscore_support is not None, positions_per_trip=per_trip, shapes={})
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
        acc = pp.EvaluationAccumulator(names, classes, downsampling=ds, overlaps=overlaps)
        acc_counts = pp.EvaluationAccumulator(names, classes, downsampling=ds, overlaps=())

        def host_route(with_sklearn=True):
            for out, tgt, C in zip(outs, tgts_host, classes):
                labels = pp.predict_labels(out, tgt, ds).cpu().numpy().reshape(-1)
                truth = tgt.numpy().reshape(-1)
                keep = truth != -1
                np.bincount(truth[keep] * C + labels[keep], minlength=C * C).reshape(C, C)
                if with_sklearn and precision_recall_fscore_support is not None:
                    for average in ('micro', 'macro'):
                        precision_recall_fscore_support(truth[keep], labels[keep], average=average, zero_division=0)

        routes = {'accumulator': lambda: acc.update(outs, tgts), 'counts_only': lambda: acc_counts.update(outs, tgts),
                  'host_counts_only': lambda: host_route(False), 'host': host_route}
        for _ in range(args.warmup):
            for fn in routes.values():
                fn()
        torch.cuda.synchronize()
        event_ms = {k: [] for k in routes if not k.startswith('host')}
        wall_ms = {k: [] for k in routes}
        t_end = time.perf_counter() + args.seconds
        rounds = 0
        while (rounds < args.rounds) if args.rounds else (time.perf_counter() < t_end):
            for k, fn in routes.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                wall_ms[k].append((time.perf_counter() - t0) * 1e3)
                if k in event_ms:
                    event_ms[k].append(a.elapsed_time(b))
            rounds += 1
        labels_bytes = sum(bs * sh['T_tgt'] * E * 8 for _, E in sh['heads'])
        state_bytes = int(acc._state.numel() * 8)
        med = lambda v: statistics.median(v)
        spread = lambda v: [float(np.percentile(v, 10)), float(np.percentile(v, 90))]
        res['shapes'][name] = dict(
            T=sh['T'], T_tgt=sh['T_tgt'], label_runs=sh.get('runs', True), heads=[dict(classes=C, entities=E) for C, E in sh['heads']],
            positions=sum(bs * sh['T_tgt'] * E for _, E in sh['heads']), rounds=rounds,
            logp_bytes=sum(int(o.numel()) * 4 for o in outs),
            pcie_bytes_per_batch=dict(accumulator=0, counts_only=0, host_counts_only=labels_bytes, host=labels_bytes),
            pcie_bytes_once_per_test_set=dict(accumulator=state_bytes, host=0),
            median_ms_device_events={k: med(v) for k, v in event_ms.items()},
            median_ms_host_clock_with_sync={k: med(v) for k, v in wall_ms.items()},
            p10_p90_ms_host_clock_with_sync={k: spread(v) for k, v in wall_ms.items()})
        acc.result()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: {r: v['median_ms_host_clock_with_sync'][r] for r in v['median_ms_host_clock_with_sync']}
                      for k, v in res['shapes'].items()}))


if __name__ == '__main__':
    main()
