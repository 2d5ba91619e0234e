#!/usr/bin/env python3
"""Cost of class weights (misc.class_weights) and the positive-class weight (misc.segmentation_loss.positive_class_weight)
on the fused criterion: forward + backward of the criterion alone at the bench's output shapes (64 clips, T = 120; the MPHOI
term list with 13 sub-activities on 2 humans, the CAD-120 list with 10 sub-activities on 1 human and 12 affordances on 5
objects), the options on and off in alternating windows so that clock drift falls on both alike, and the two new launches
alone next to the two they replace. Off is the plain path (twog_multitask_loss_*), on sends every term through
twog_weighted_loss_*: the same number of launches, one more read of cw[y] per kept element. Every window is timed by device
events around `--reps` repetitions and ends in a synchronise. Writes profiles/class_weight_cost.json.
    python tools/class_weight_cost.py [--pairs 6] [--reps 1000]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from smooth_loss_cost import LAYOUTS, BS, T, outputs, window_ms  # noqa: E402  (the same shapes and the same timing)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=6)
    ap.add_argument('--reps', type=int, default=1000)
    ap.add_argument('--warmup', type=int, default=50)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'class_weight_cost.json'))
    args = ap.parse_args()
    import twog_gcn_amd  # noqa: F401
    from twog_gcn_amd.hostcpu import limit_host_threads
    from twog_gcn_amd.kernels import get_kernels
    from twog_gcn_amd import losses
    limit_host_threads()
    assert torch.cuda.is_available(), 'a measurement needs the GPU: there is no fallback'
    dev = torch.device('cuda', 0)
    K = get_kernels()
    assert K.name == 'hip'
    misc = dict(budget_loss=dict(add=True), segmentation_loss=dict(add=True, pretrain=False), first_level_loss_weight=0.3)
    res = dict(clips=BS, T=T, pairs=args.pairs, reps_per_window=args.reps, device=torch.cuda.get_device_name(0), lists={})
    for ds, lay in LAYOUTS.items():
        outs, tgts = outputs(ds, dev)
        leaves = [o.requires_grad_(True) for o in outs]
        # the weights a user would pass: 'balanced' weights from the class counts of these very targets
        # (the last terms of the list: ... SAR, SAP on the humans [, OAR, OAP on the objects])
        labelled = [tgts[-1]] if len(lay['classes']) == 1 else [tgts[-4], tgts[-2]]
        cw = [losses.class_weights(losses.class_counts(y, C)).cpu().tolist() for y, C in zip(labelled, lay['classes'])]
        on = dict(misc, class_weights=dict(add=True, subactivity=cw[0], affordance=cw[-1]))
        on['segmentation_loss'] = dict(misc['segmentation_loss'], positive_class_weight=2.0)
        steps, launches = {}, {}
        for name, cfg in (('off', misc), ('on', on)):
            crit, names = losses.select_loss('2G-GCN', 'multiple', ds, dict(misc=cfg))

            def step(crit=crit):
                for x in leaves:
                    x.grad = None
                sum(crit(leaves, tgts)).backward()
            steps[name] = step
            # the launches of one criterion call, counted at the kernel interface
            seen = []
            real = {k: getattr(K, k) for k in ('multitask_loss_fwd', 'multitask_loss_bwd', 'weighted_loss_fwd',
                                               'weighted_loss_bwd')}
            for k, fn in real.items():
                setattr(K, k, lambda *a, _k=k, _f=fn, **kw: (seen.append(_k), _f(*a, **kw))[1])
            step()
            for k in real:
                delattr(K, k)
            launches[name] = seen
        n = len(outs)
        kinds = [2] * (n // 6) + [1] * (n // 6) + [0] * (n - n // 3)
        plain = [dict(kind=k, input=o.detach(), target=t, weight=1.0, ignore=-1) for k, o, t in zip(kinds, outs, tgts)]
        cws = losses.select_loss('2G-GCN', 'multiple', ds, dict(misc=on))[0].keywords['class_weights']
        weighted = [dict(p, class_weight=None if c is None else torch.tensor(c, device=dev),
                         positive_class_weight=2.0 if p['kind'] == 1 else 1.0) for p, c in zip(plain, cws)]
        dl = torch.ones(n, dtype=torch.float32, device=dev)
        stats = {'plain': K.multitask_loss_fwd(plain)[1], 'weighted': K.weighted_loss_fwd(weighted)[1]}
        alone = {'multitask_loss_fwd': lambda: K.multitask_loss_fwd(plain),
                 'weighted_loss_fwd': lambda: K.weighted_loss_fwd(weighted),
                 'multitask_loss_bwd': lambda: K.multitask_loss_bwd(plain, stats['plain'], dl, [True] * n),
                 'weighted_loss_bwd': lambda: K.weighted_loss_bwd(weighted, stats['weighted'], dl, [True] * n)}
        for fn in list(steps.values()) + list(alone.values()):
            window_ms(fn, args.warmup)
        ms = {'off': [], 'on': []}
        for _ in range(args.pairs):
            for name in ('off', 'on'):
                ms[name].append(window_ms(steps[name], args.reps) / args.reps)
        alone_us = {k: [] for k in alone}
        for _ in range(3):
            for k, fn in alone.items():
                alone_us[k].append(window_ms(fn, args.reps) / args.reps * 1e3)
        med = {k: statistics.median(v) for k, v in ms.items()}
        res['lists'][ds] = dict(terms=n, launches_off=launches['off'], launches_on=launches['on'],
                                criterion_ms_off=ms['off'], criterion_ms_on=ms['on'], median_ms_off=med['off'],
                                median_ms_on=med['on'], overhead_us=(med['on'] - med['off']) * 1e3,
                                launches_alone_us=alone_us,
                                launches_alone_us_median={k: statistics.median(v) for k, v in alone_us.items()})
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps({ds: {k: v for k, v in r.items() if not isinstance(v, (list, dict))} for ds, r in res['lists'].items()}))


if __name__ == '__main__':
    main()
