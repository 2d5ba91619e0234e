#!/usr/bin/env python3
"""Cost of the temporal smoothing terms (misc.smoothing_loss) on the fused criterion: forward + backward of the criterion
alone at the bench's output shapes (64 clips, T = 120; the MPHOI term list with 13 sub-activities on 2 humans, the CAD-120
list with 10 sub-activities on 1 human and 12 affordances on 5 objects), the option on and off in alternating windows so
that clock drift falls on both alike, and the two new launches alone. Every window is timed by device events around
`--reps` repetitions and ends in a synchronise. Writes profiles/smooth_loss_cost.json.
    python tools/smooth_loss_cost.py [--pairs 6] [--reps 1000]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BS, T = 64, 120
LAYOUTS = {'mphoi': dict(ents=[2], classes=[13]), 'cad120': dict(ents=[1, 5], classes=[10, 12])}


def outputs(ds, dev, seed=0):
    """Random tensors of the shapes of the model's output list and targets with a ragged tail (-1), as the criterion sees them."""
    lay, g = LAYOUTS[ds], torch.Generator().manual_seed(seed)
    k = len(lay['ents'])
    outs, tgts = [], []
    for i in range(6 * k):
        E, C = lay['ents'][i % k if i < 2 * k else ((i - 2 * k) % (2 * k)) // 2], None
        if i < 2 * k:
            o = torch.rand(BS, T, E, generator=g) * 0.9 + 0.05
            t = (torch.rand(BS, T, E, generator=g) > 0.5).float()
        else:
            C = lay['classes'][((i - 2 * k) % (2 * k)) // 2]
            o = torch.log_softmax(torch.randn(BS, C, T, E, generator=g), 1)
            t = torch.randint(0, C, (BS, T, E), generator=g)
        t[1::2, T - 20:] = -1
        outs.append(o.to(dev))
        tgts.append(t.to(dev))
    return outs, tgts


def window_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=6)
    ap.add_argument('--reps', type=int, default=1000)
    ap.add_argument('--warmup', type=int, default=50)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'smooth_loss_cost.json'))
    args = ap.parse_args()
    import twog_gcn_amd  # noqa: F401
    from twog_gcn_amd.hostcpu import limit_host_threads
    from twog_gcn_amd.kernels import get_kernels
    from twog_gcn_amd.losses import select_loss
    limit_host_threads()
    assert torch.cuda.is_available(), 'a measurement needs the GPU: there is no fallback'
    dev = torch.device('cuda', 0)
    K = get_kernels()
    assert K.name == 'hip'
    misc = dict(budget_loss=dict(add=True), segmentation_loss=dict(add=True, pretrain=False), first_level_loss_weight=0.3)
    res = dict(clips=BS, T=T, pairs=args.pairs, reps_per_window=args.reps, device=torch.cuda.get_device_name(0), lists={})
    for ds in LAYOUTS:
        outs, tgts = outputs(ds, dev)
        leaves = [o.requires_grad_(True) for o in outs]
        steps = {}
        for name, add in (('off', False), ('on', True)):
            crit, names = select_loss('2G-GCN', 'multiple', ds, dict(misc=dict(misc, smoothing_loss=dict(add=add))))

            def step(crit=crit):
                for x in leaves:
                    x.grad = None
                sum(crit(leaves, tgts)).backward()
            steps[name] = (step, names)
        n, n_on = len(steps['off'][1]), len(steps['on'][1])
        # the two new launches alone, on the terms the criterion hands them
        terms = [dict(input=outs[i], target=tgts[i], weight=0.15, tau=4.0, ignore=-1) for i in range(n - (n_on - n), n)]
        m = len(terms)
        loss = torch.empty(m, dtype=torch.float32, device=dev)
        stats = torch.empty(m, 2, dtype=torch.float64, device=dev)
        dl = torch.ones(m, dtype=torch.float32, device=dev)
        dins = [torch.empty_like(t['input']) for t in terms]
        alone = {'smooth_loss_fwd': lambda: K.smooth_loss_fwd(terms, loss, stats),
                 'smooth_loss_bwd': lambda: K.smooth_loss_bwd(terms, stats, dl, dins, [False] * m)}
        for fn in [s for s, _ in steps.values()] + list(alone.values()):
            window_ms(fn, args.warmup)
        ms = {'off': [], 'on': []}
        for _ in range(args.pairs):
            for name in ('off', 'on'):
                ms[name].append(window_ms(steps[name][0], args.reps) / args.reps)
        alone_us = {k: [window_ms(fn, args.reps) / args.reps * 1e3 for _ in range(3)] for k, fn in alone.items()}
        med = {k: statistics.median(v) for k, v in ms.items()}
        nbytes = sum(t['input'].numel() * 4 + t['target'].numel() * 8 for t in terms)
        res['lists'][ds] = dict(terms_off=n, terms_on=n_on, criterion_ms_off=ms['off'], criterion_ms_on=ms['on'],
                                median_ms_off=med['off'], median_ms_on=med['on'], overhead_us=(med['on'] - med['off']) * 1e3,
                                launches_alone_us=alone_us,
                                launches_alone_us_median={k: statistics.median(v) for k, v in alone_us.items()},
                                smoothing_input_bytes=nbytes)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps({ds: {k: v for k, v in r.items() if not isinstance(v, (list, dict))} for ds, r in res['lists'].items()}))


if __name__ == '__main__':
    main()
