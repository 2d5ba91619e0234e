#!/usr/bin/env python3
"""Cost of the linear-chain CRF terms (misc.crf_loss) on the fused criterion: forward + backward of the criterion alone at the
bench's output shapes (64 clips, T = 120; the MPHOI term list with 13 sub-activities on 2 humans, the CAD-120 list with 10
sub-activities on 1 human and 12 affordances on 5 objects), one CRF term per final-level NLL term, the option on and off
in alternating windows so that clock drift falls on both alike; the new launches alone beside the NLL launches alone on the
same inputs; and the worst case the limits admit (64 sequences of 4 096 kept steps over 64 classes). Every window is timed
by device events around `--reps` repetitions and ends in a synchronise. Writes profiles/crf_loss_cost.json.
    python tools/crf_loss_cost.py [--pairs 6] [--reps 500]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.smooth_loss_cost import BS, LAYOUTS, T, outputs, window_ms   # noqa: E402  (the same shapes and windows)

KEYS = {'mphoi': ('SAR', 'SAP'), 'cad120': ('SAR', 'SAP', 'OAR', 'OAP')}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=6)
    ap.add_argument('--reps', type=int, default=500)
    ap.add_argument('--warmup', type=int, default=30)
    ap.add_argument('--worst-reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'crf_loss_cost.json'))
    args = ap.parse_args()
    import twog_gcn_amd  # noqa: F401
    from twog_gcn_amd.hostcpu import limit_host_threads
    from twog_gcn_amd.kernels import get_kernels
    from twog_gcn_amd.losses import LinearChainCRF, select_loss
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
        n = len(outs)
        first = n - len(KEYS[ds])
        crfs = {}
        for j, k in enumerate(KEYS[ds]):
            crfs[k] = LinearChainCRF(outs[first + j].shape[1]).to(dev)
            with torch.no_grad():
                crfs[k].transitions.normal_(generator=None)
        steps = {}
        for name, add in (('off', False), ('on', True)):
            crit, names = select_loss('2G-GCN', 'multiple', ds, dict(misc=dict(misc, crf_loss=dict(add=add))),
                                      crf=crfs if add else None)

            def step(crit=crit):
                for x in leaves:
                    x.grad = None
                for m in crfs.values():
                    m.transitions.grad = m.initial.grad = None
                sum(crit(leaves, tgts)).backward()
            steps[name] = (step, names)
        # the new launches alone, on the terms the criterion hands them, and the NLL launches alone on the same inputs
        terms = [dict(input=outs[first + j].detach(), target=tgts[first + j], weight=1.0, ignore=-1,
                      transitions=crfs[k].transitions.detach(), initial=crfs[k].initial.detach())
                 for j, k in enumerate(KEYS[ds])]
        m = len(terms)
        loss = torch.empty(m, dtype=torch.float32, device=dev)
        stats = torch.empty(m, 2, dtype=torch.float64, device=dev)
        dl = torch.ones(m, dtype=torch.float32, device=dev)
        dins = [torch.empty_like(t['input']) for t in terms]
        nll = [dict(kind=0, input=t['input'], target=t['target'], weight=1.0, ignore=-1) for t in terms]
        K.crf_nll_fwd(terms, loss, stats)
        nll_stats = K.multitask_loss_fwd(nll)[1]
        alone = {'crf_nll_fwd': lambda: K.crf_nll_fwd(terms, loss, stats),
                 'crf_nll_bwd': lambda: K.crf_nll_bwd(terms, stats, dl, dins, [False] * m, [True] * m),
                 'crf_nll_bwd_input_only': lambda: K.crf_nll_bwd(terms, stats, dl, dins, [False] * m, [False] * m),
                 'nll_fwd': lambda: K.multitask_loss_fwd(nll),
                 'nll_bwd': lambda: K.multitask_loss_bwd(nll, nll_stats, dl, [True] * m)}
        for fn in [s for s, _ in steps.values()] + list(alone.values()):
            window_ms(fn, args.warmup)
        ms = {'off': [], 'on': []}
        for _ in range(args.pairs):
            for name in ('off', 'on'):
                ms[name].append(window_ms(steps[name][0], args.reps) / args.reps)
        alone_us = {k: [window_ms(fn, args.reps) / args.reps * 1e3 for _ in range(3)] for k, fn in alone.items()}
        med = {k: statistics.median(v) for k, v in ms.items()}
        ws = [K.crf_workspace(*t['input'].shape) for t in terms]
        res['lists'][ds] = dict(terms_off=len(steps['off'][1]), terms_on=len(steps['on'][1]), crf_terms=m,
                                criterion_ms_off=ms['off'], criterion_ms_on=ms['on'], median_ms_off=med['off'],
                                median_ms_on=med['on'], overhead_us=(med['on'] - med['off']) * 1e3,
                                launches_alone_us=alone_us,
                                launches_alone_us_median={k: statistics.median(v) for k, v in alone_us.items()},
                                crf_input_bytes=sum(t['input'].numel() * 4 + t['target'].numel() * 8 for t in terms),
                                workspace_bytes=dict(alpha=sum(w[0] for w in ws), seq=sum(w[1] for w in ws),
                                                     partials=max(w[2] for w in ws)))
    # the worst case the limits admit: 64 sequences of 4096 kept steps over 64 classes
    bs, C, Tm, E = 64, 64, 4096, 1
    g = torch.Generator().manual_seed(1)
    term = dict(input=torch.log_softmax(torch.randn(bs, C, Tm, E, generator=g), 1).to(dev),
                target=torch.randint(0, C, (bs, Tm, E), generator=g).to(dev), weight=1.0, ignore=-1,
                transitions=torch.randn(C, C, generator=g).to(dev), initial=torch.randn(C, generator=g).to(dev))
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    stats = torch.empty(1, 2, dtype=torch.float64, device=dev)
    dl, din = torch.ones(1, dtype=torch.float32, device=dev), torch.empty_like(term['input'])
    worst = {'crf_nll_fwd': lambda: K.crf_nll_fwd([term], loss, stats),
             'crf_nll_bwd': lambda: K.crf_nll_bwd([term], stats, dl, [din], [False], [True])}
    res['worst_case'] = dict(sequences=bs * E, classes=C, steps=Tm, reps_per_window=args.worst_reps,
                             workspace_bytes=dict(zip(('alpha', 'seq', 'partials'), K.crf_workspace(bs, C, Tm, E))))
    for k, fn in worst.items():
        window_ms(fn, 1)
        res['worst_case'][k + '_ms'] = [window_ms(fn, args.worst_reps) / args.worst_reps for _ in range(3)]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps({ds: {k: v for k, v in r.items() if not isinstance(v, list)} for ds, r in res['lists'].items()}))
    print(json.dumps(res['worst_case']))


if __name__ == '__main__':
    main()
