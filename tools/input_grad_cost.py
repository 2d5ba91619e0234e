#!/usr/bin/env python3
"""What the input gradients cost at the bench shape (64 clips, T 120, H 2, O 8, N 34, h 512) on one MI355X.

  backward pass   device events around loss.backward() of bench.py's model and batch, three variants ALTERNATED round by
                  round in one process: no input requires grad (what every training step without a front-end pays),
                  x_objects only (one more GEMM), both (the grouped GEMM of two problems + twog_gcn_input_bwd). Medians.
  kernel          twog_gcn_input_bwd's own time comes from a separate run under the profiler,
                      rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- \\
                          python tools/input_grad_cost.py --rounds 10 --out /dev/null
                  whose kernel-stats CSV is then given to a plain run with --kernel-stats: achieved bytes/s over the
                  algorithmic (256 + 16 + 16) * N bytes per frame (de1 read, x read, dx written; human 0), against the
                  6.29 TB/s float4 copy of the microarchitecture guide.
  bench lines     --bench-this / --bench-parent: files holding the JSON line of `bench.py --gpus 1 --steps 6 --warmup 2` on
                  this tree and on the commit before the feature (which cannot compute the quantity; the comparison that
                  matters is that a step that asks for nothing costs what it did). Both lines are copied into the record.
Writes profiles/input_grad_cost.json.    python tools/input_grad_cost.py [--rounds 30]
"""
import argparse
import csv
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_BW_TBS = 6.29   # MI355X microarchitecture guide: float4 copy, measured
VARIANTS = {'none': (False, False), 'x_objects': (False, True), 'both': (True, True)}


def last_json_line(path):
    lines = [ln for ln in open(path).read().splitlines() if ln.startswith('{')]
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--kernel-stats', help='kernel_stats.csv of the separate rocprofv3 run')
    ap.add_argument('--bench-this', help='file with the bench.py JSON line of this tree')
    ap.add_argument('--bench-parent', help='file with the bench.py JSON line of the commit before the feature')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'input_grad_cost.json'))
    args = ap.parse_args()
    import bench
    import twog_gcn_amd  # noqa: F401
    from twog_gcn_amd.models import TGGCN
    from twog_gcn_amd.kernels import get_kernels
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    dev = torch.device('cuda', 0)
    assert get_kernels().name == 'hip'
    bs, T, H, O, N = bench.BS, bench.T, bench.H, bench.O, bench.N_NODES
    torch.manual_seed(0)
    model = TGGCN(input_size=(2048 + 4 * N, 2048), num_classes=(bench.N_CLASSES, None), **bench.CFG).to(dev).train()
    x_human, x_objects, mask, _ = bench.synthetic_batch(bs, dev, seed=0)
    seg = torch.ones(bs, T, H, device=dev)
    cot = None
    ms = {k: [] for k in VARIANTS}
    for r in range(args.warmup + args.rounds):
        for name, (need_h, need_o) in VARIANTS.items():
            xh, xo = x_human.detach().requires_grad_(need_h), x_objects.detach().requires_grad_(need_o)
            out = model(xh, xo, mask, human_segmentation=seg)
            if cot is None:
                g = torch.Generator(device='cpu').manual_seed(1)
                cot = [torch.randn(o.shape, generator=g).to(dev) for o in out]
            loss = sum((o * c).sum() for o, c in zip(out, cot) if o.requires_grad)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            loss.backward()
            b.record()
            torch.cuda.synchronize()
            assert (xh.grad is not None) == need_h and (xo.grad is not None) == need_o
            model.zero_grad(set_to_none=True)
            if r >= args.warmup:
                ms[name].append(a.elapsed_time(b))
    med = {k: statistics.median(v) for k, v in ms.items()}
    q = lambda v, p: sorted(v)[min(len(v) - 1, int(p * len(v)))]
    n_frames = bs * T
    kernel_bytes = (256 + 16 + 16) * N * n_frames
    res = dict(device=torch.cuda.get_device_name(0),
               shape=dict(clips=bs, T=T, H=H, O=O, N=N, h=bench.CFG['hidden_size']), rounds=args.rounds,
               backward_ms_median_device_events=med,
               backward_ms_p10_p90={k: [q(v, 0.1), q(v, 0.9)] for k, v in ms.items()},
               added_ms_over_none={k: med[k] - med['none'] for k in ('x_objects', 'both')},
               input_gradient_bytes=dict(x_human=int(x_human.numel()) * 4, x_objects=int(x_objects.numel()) * 4),
               twog_gcn_input_bwd=dict(algorithmic_bytes_per_frame=(256 + 16 + 16) * N, frames=n_frames, algorithmic_bytes=kernel_bytes,
                                       zero_fill_bytes_other_humans=16 * N * (H - 1) * n_frames,
                                       kernel_time='not measured (give --kernel-stats)'))
    if args.kernel_stats:
        rows = [r for r in csv.DictReader(open(args.kernel_stats)) if 'input_bwd_kernel' in r['Name']]
        assert len(rows) == 1, [r['Name'] for r in rows]
        avg_ns = float(rows[0]['AverageNs'])
        res['twog_gcn_input_bwd'].update(
            kernel_time=dict(source='rocprofv3 --kernel-trace --stats, separate run', calls=int(rows[0]['Calls']),
                             average_us=avg_ns / 1e3, min_us=float(rows[0]['MinNs']) / 1e3, max_us=float(rows[0]['MaxNs']) / 1e3),
            achieved_TBs_over_algorithmic_bytes=kernel_bytes / avg_ns / 1e3,
            measured_float4_copy_TBs=COPY_BW_TBS,
            share_of_copy_bandwidth=kernel_bytes / avg_ns / 1e3 / COPY_BW_TBS)
    for key, path in (('bench_line_this_tree_nothing_requested', args.bench_this), ('bench_line_parent_commit', args.bench_parent)):
        if path:
            res[key] = last_json_line(path)
    if args.out != '/dev/null':
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
    print(json.dumps({k: res[k] for k in ('backward_ms_median_device_events', 'added_ms_over_none', 'twog_gcn_input_bwd')}))


if __name__ == '__main__':
    main()
