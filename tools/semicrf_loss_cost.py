#!/usr/bin/env python3
"""Cost of the semi-Markov CRF terms on the fused criterion: forward + backward of the criterion alone at the bench's output
shapes (128 clips, T = 120; the MPHOI term list with 13 sub-activities on 2 humans, the CAD-120 list with 10 sub-activities on
1 human and 12 affordances on 5 objects), one SemiMarkovCRF term per final-level NLL term at D = 32 and D = 120, the option
on and off in alternating windows of about one second so that clock drift falls on both alike; the two new launches alone
beside twog_crf_nll_fwd/bwd and twog_segdecode on the same tensors; and the worst case the limits admit (64 sequences of
4 096 kept steps over 64 classes at D = 128). Every window is timed by device events around its repetitions and ends in a
synchronise. Labels come in runs of 8 steps. Writes profiles/semicrf_loss_cost.json.
    python tools/semicrf_loss_cost.py [--pairs 5] [--window-ms 1000]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.smooth_loss_cost import LAYOUTS, window_ms   # noqa: E402  (the same head layouts and windows)

BS, T, RUN = 128, 120, 8
KEYS = {'mphoi': ('SAR', 'SAP'), 'cad120': ('SAR', 'SAP', 'OAR', 'OAP')}
DURATIONS = (32, 120)


def outputs(ds, dev, seed=0):
    """tools/smooth_loss_cost.outputs at 128 clips, the class labels in runs of RUN steps."""
    lay, g = LAYOUTS[ds], torch.Generator().manual_seed(seed)
    k = len(lay['ents'])
    outs, tgts = [], []
    for i in range(6 * k):
        E = lay['ents'][i % k if i < 2 * k else ((i - 2 * k) % (2 * k)) // 2]
        if i < 2 * k:
            o = torch.rand(BS, T, E, generator=g) * 0.9 + 0.05
            t = (torch.rand(BS, T, E, generator=g) > 0.5).float()
        else:
            C = lay['classes'][((i - 2 * k) % (2 * k)) // 2]
            o = torch.log_softmax(torch.randn(BS, C, T, E, generator=g), 1)
            t = torch.randint(0, C, (BS, T // RUN, E), generator=g).repeat_interleave(RUN, 1)
        t[1::2, T - 20:] = -1
        outs.append(o.to(dev))
        tgts.append(t.to(dev))
    return outs, tgts


def reps_for(fn, target_ms, probe=20):
    """Repetitions that fill a window of about target_ms, from a probe window."""
    window_ms(fn, 3)
    per = window_ms(fn, probe) / probe
    return max(1, int(math.ceil(target_ms / max(per, 1e-3))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=5)
    ap.add_argument('--window-ms', type=float, default=1000.0)
    ap.add_argument('--alone-window-ms', type=float, default=300.0)
    ap.add_argument('--worst-reps', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'semicrf_loss_cost.json'))
    args = ap.parse_args()
    import twog_gcn_amd  # noqa: F401
    from twog_gcn_amd.hostcpu import limit_host_threads
    from twog_gcn_amd.kernels import get_kernels
    from twog_gcn_amd.losses import SemiMarkovCRF, select_loss
    limit_host_threads()
    assert torch.cuda.is_available(), 'a measurement needs the GPU: there is no fallback'
    dev = torch.device('cuda', 0)
    K = get_kernels()
    assert K.name == 'hip'
    misc = dict(budget_loss=dict(add=True), segmentation_loss=dict(add=True, pretrain=False), first_level_loss_weight=0.3)
    res = dict(clips=BS, T=T, label_run=RUN, pairs=args.pairs, window_ms=args.window_ms,
               device=torch.cuda.get_device_name(0), lists={})
    med = statistics.median
    for ds in LAYOUTS:
        outs, tgts = outputs(ds, dev)
        leaves = [o.requires_grad_(True) for o in outs]
        first = len(outs) - len(KEYS[ds])
        res['lists'][ds] = {}
        for D in DURATIONS:
            mods = {}
            for j, k in enumerate(KEYS[ds]):
                mods[k] = SemiMarkovCRF(outs[first + j].shape[1], D).to(dev)
                with torch.no_grad():
                    for p in mods[k].parameters():
                        p.normal_()
            steps = {}
            for name, add in (('off', False), ('on', True)):
                crit, names = select_loss('2G-GCN', 'multiple', ds, dict(misc=dict(misc, crf_loss=dict(add=add))),
                                          crf=mods if add else None)

                def step(crit=crit):
                    for x in leaves:
                        x.grad = None
                    for m in mods.values():
                        for p in m.parameters():
                            p.grad = None
                    sum(crit(leaves, tgts)).backward()
                steps[name] = (step, names)
            # the new launches alone, on the terms the criterion hands them; the CRF launches and the segmental decode on
            # the same tensors
            terms = [dict(input=outs[first + j].detach(), target=tgts[first + j], weight=1.0, ignore=-1,
                          transitions=mods[k].transitions.detach(), initial=mods[k].initial.detach(),
                          durations=mods[k].durations.detach()) for j, k in enumerate(KEYS[ds])]
            m = len(terms)
            loss = torch.empty(m, dtype=torch.float32, device=dev)
            stats = torch.empty(m, 2, dtype=torch.float64, device=dev)
            crf_loss, crf_stats = torch.empty_like(loss), torch.empty_like(stats)
            dl = torch.ones(m, dtype=torch.float32, device=dev)
            dins = [torch.empty_like(t['input']) for t in terms]
            crf_terms = [{k: v for k, v in t.items() if k != 'durations'} for t in terms]
            K.semicrf_nll_fwd(terms, loss, stats)
            K.crf_nll_fwd(crf_terms, crf_loss, crf_stats)
            alone = {'semicrf_nll_fwd': lambda: K.semicrf_nll_fwd(terms, loss, stats),
                     'semicrf_nll_bwd': lambda: K.semicrf_nll_bwd(terms, stats, dl, dins, [False] * m, [True] * m),
                     'semicrf_nll_bwd_input_only': lambda: K.semicrf_nll_bwd(terms, stats, dl, dins, [False] * m, [False] * m),
                     'crf_nll_fwd': lambda: K.crf_nll_fwd(crf_terms, crf_loss, crf_stats),
                     'crf_nll_bwd': lambda: K.crf_nll_bwd(crf_terms, crf_stats, dl, dins, [False] * m, [True] * m),
                     'segdecode': lambda: [K.segment_decode(t['input'], t['transitions'], t['durations'], t['initial'])
                                           for t in terms]}
            reps = {name: reps_for(fn, args.window_ms) for name, (fn, _) in steps.items()}
            ms = {'off': [], 'on': []}
            for _ in range(args.pairs):
                for name in ('off', 'on'):
                    ms[name].append(window_ms(steps[name][0], reps[name]) / reps[name])
            alone_us = {}
            for k, fn in alone.items():
                r = reps_for(fn, args.alone_window_ms)
                alone_us[k] = [window_ms(fn, r) / r * 1e3 for _ in range(3)]
            a = {k: med(v) for k, v in alone_us.items()}
            plans = [K.semicrf_plan(*t['input'].shape, D) for t in terms]
            res['lists'][ds][f'D{D}'] = dict(
                terms_off=len(steps['off'][1]), terms_on=len(steps['on'][1]), semicrf_terms=m, reps_per_window=reps,
                criterion_ms_off=ms['off'], criterion_ms_on=ms['on'], median_ms_off=med(ms['off']), median_ms_on=med(ms['on']),
                overhead_us=(med(ms['on']) - med(ms['off'])) * 1e3, launches_alone_us=alone_us, launches_alone_us_median=a,
                ratio_fwd_to_crf_fwd=a['semicrf_nll_fwd'] / a['crf_nll_fwd'],
                ratio_bwd_to_crf_bwd=a['semicrf_nll_bwd'] / a['crf_nll_bwd'],
                ratio_fwd_to_segdecode=a['semicrf_nll_fwd'] / a['segdecode'],
                ratio_bwd_to_segdecode=a['semicrf_nll_bwd'] / a['segdecode'], plans=plans)
    # the worst case the limits admit: 64 sequences of 4096 kept steps over 64 classes at D = 128
    bs, C, Tm, E, D = 64, 64, 4096, 1, 128
    g = torch.Generator().manual_seed(1)
    term = dict(input=torch.log_softmax(torch.randn(bs, C, Tm, E, generator=g), 1).to(dev),
                target=torch.randint(0, C, (bs, Tm // RUN, E), generator=g).repeat_interleave(RUN, 1).to(dev), weight=1.0,
                ignore=-1, transitions=torch.randn(C, C, generator=g).to(dev), initial=torch.randn(C, generator=g).to(dev),
                durations=torch.randn(C, D, generator=g).to(dev))
    crf_term = {k: v for k, v in term.items() if k != 'durations'}
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    stats = torch.empty(1, 2, dtype=torch.float64, device=dev)
    crf_stats = torch.empty_like(stats)
    dl, din = torch.ones(1, dtype=torch.float32, device=dev), torch.empty_like(term['input'])
    worst = {'semicrf_nll_fwd': lambda: K.semicrf_nll_fwd([term], loss, stats),
             'semicrf_nll_bwd': lambda: K.semicrf_nll_bwd([term], stats, dl, [din], [False], [True]),
             'crf_nll_fwd': lambda: K.crf_nll_fwd([crf_term], loss, crf_stats),
             'crf_nll_bwd': lambda: K.crf_nll_bwd([crf_term], crf_stats, dl, [din], [False], [True]),
             'segdecode': lambda: K.segment_decode(term['input'], term['transitions'], term['durations'], term['initial'])}
    res['worst_case'] = dict(sequences=bs * E, classes=C, steps=Tm, max_duration=D, reps_per_window=args.worst_reps,
                             plan=K.semicrf_plan(bs, C, Tm, E, D))
    for k, fn in worst.items():
        window_ms(fn, 1)
        res['worst_case'][k + '_ms'] = [window_ms(fn, args.worst_reps) / args.worst_reps for _ in range(3)]
    w = {k: med(v) for k, v in res['worst_case'].items() if k.endswith('_ms')}
    res['worst_case'].update(ratio_fwd_to_crf_fwd=w['semicrf_nll_fwd_ms'] / w['crf_nll_fwd_ms'],
                             ratio_bwd_to_crf_bwd=w['semicrf_nll_bwd_ms'] / w['crf_nll_bwd_ms'],
                             ratio_fwd_to_segdecode=w['semicrf_nll_fwd_ms'] / w['segdecode_ms'],
                             ratio_bwd_to_segdecode=w['semicrf_nll_bwd_ms'] / w['segdecode_ms'])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    for ds, by_d in res['lists'].items():
        for d, r in by_d.items():
            print(ds, d, json.dumps({k: v for k, v in r.items() if not isinstance(v, (list, dict))}))
    print(json.dumps({k: v for k, v in res['worst_case'].items() if not isinstance(v, dict)}))


if __name__ == '__main__':
    main()
