#!/usr/bin/env python3
"""Cost of the reference trainer's two training-step options on the headline step (bench.py's c3 workload: 64 clips,
T = 120, h = 512): the plain fused step against the same step with FusedAdam(max_grad_norm=...) and the multi-task loss
learner (DataParallel(extra_modules=[learner])). Two models in one process, their steps alternated, so that clock and
thermal drift fall on both alike; plus the norm kernel alone over the model's gradient slice (HIP events). Writes
profiles/train_options_cost.json.   python tools/train_options_cost.py [--pairs 8]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=8)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'train_options_cost.json'))
    args = ap.parse_args()
    import bench
    import twog_gcn_amd  # noqa: F401
    from twog_gcn_amd.distributed import DataParallel, FusedAdam
    from twog_gcn_amd.hostcpu import limit_host_threads
    from twog_gcn_amd.kernels import get_kernels
    from twog_gcn_amd.losses import select_loss, select_loss_types, select_loss_learning_mask
    from twog_gcn_amd.models import TGGCN
    from twog_gcn_amd.multi_task import MultiTaskLossLearner
    limit_host_threads()
    w = bench.select_workload('c3')
    dev = torch.device('cuda', 0)
    K = get_kernels()
    assert K.name == 'hip'
    crit, _ = select_loss('2G-GCN', 'multiple', 'mphoi', dict(misc={}))
    x_human, x_objects, mask, targets = bench.synthetic_batch(w['bs'], dev, seed=1234)
    seg = torch.ones(w['bs'], bench.T, w['H'], device=dev)
    seg_t = torch.zeros_like(seg)
    tgt = [seg_t, seg_t, targets[0], targets[1], targets[0], targets[1]]

    def build(options):
        torch.manual_seed(0)
        model = TGGCN(input_size=(2048 + 4 * w['N'], 2048), num_classes=(w['classes'], None), **bench.CFG).to(dev).train()
        mtll = MultiTaskLossLearner(select_loss_types('2G-GCN', 'mphoi', {}),
                                    select_loss_learning_mask('2G-GCN', 'mphoi', {})).to(dev) if options else None
        dp = DataParallel(model, extra_modules=[mtll] if options else ())
        opt = FusedAdam(dp.flat, lr=1e-4, max_grad_norm=1.0 if options else 0.0)

        def step():
            dp.zero_grad()
            out = model(x_human, x_objects, mask, human_segmentation=seg)
            losses = crit(out, tgt)
            if mtll is not None:
                losses = mtll(losses)
            sum(losses).backward()
            dp.all_reduce_gradients()
            opt.step(dp.grad_scale)
        return step, dp

    plain, _ = build(False)
    opts, dp = build(True)
    for _ in range(args.warmup):
        plain()
        opts()
    torch.cuda.synchronize()
    times = {'plain': [], 'options': []}
    for _ in range(args.pairs):
        for name, fn in (('plain', plain), ('options', opts)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b))
    # the norm kernel alone (two launches: partial sums + the fixed-order combine) over the model's slice
    b0, e0 = dp.flat.module_ranges[0]
    for _ in range(3):
        K.grad_norm(dp.flat.grad, [(b0, e0)], 1.0, 1.0)
    norm_us = []
    for _ in range(20):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        K.grad_norm(dp.flat.grad, [(b0, e0)], 1.0, 1.0)
        b.record()
        torch.cuda.synchronize()
        norm_us.append(a.elapsed_time(b) * 1e3)
    nbytes = (e0 - b0) * 4
    med = {k: statistics.median(v) for k, v in times.items()}
    res = dict(workload='c3', clips=w['bs'], T=bench.T, hidden=w['h'], pairs=args.pairs,
               step_ms_plain=times['plain'], step_ms_options=times['options'],
               median_ms_plain=med['plain'], median_ms_options=med['options'],
               overhead_ms=med['options'] - med['plain'],
               model_grad_floats=e0 - b0, norm_us_events=norm_us, norm_us_median=statistics.median(norm_us),
               norm_tbs_events=nbytes / (statistics.median(norm_us) * 1e-6) / 1e12,
               device=torch.cuda.get_device_name(0))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if not isinstance(v, list)}))


if __name__ == '__main__':
    main()
