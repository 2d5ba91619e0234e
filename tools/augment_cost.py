#!/usr/bin/env python3
"""Cost of the device-side input augmentation (augment.InputAugmentation -> twog_augment_inputs) at the bench's input shape:
64 clips, T = 120, 2 humans of 2 048 + 4 * 34 channels, 4 objects of 2 048 channels. Four variants in alternating windows, so
that clock drift falls on all alike: the geometry launch alone, the feature launch alone, both, and as the floor the feature
pass is judged against a plain device copy of the same two tensors (torch's copy_ and the library's own twog_copy_blocks; the
faster one is the floor). Every window is timed by device events around `--reps` repetitions and ends in a synchronise; the
median over the windows is reported, with the ratio to the copy and -- given the result line of a bench.py run on the same
box (--bench-json) -- the share of that step time. The augmentation runs in place on the same buffers again and again: the
values drift (to inf, under dropout's rescaling), the work per call does not.
Writes profiles/augment_cost.json.
    python bench.py --gpus 1 --steps 20 --warmup 5 > bench_line.json
    python tools/augment_cost.py --bench-json bench_line.json [--windows 7] [--reps 500]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BS, T, H, O, C, N = 64, 120, 2, 4, 2048, 34
GEOMETRY = dict(max_rotation_deg=15., max_scale=0.1, max_shift=0.05, centre=(0.5, 0.5))
FEATURES = dict(feature_noise_std=0.1, feature_dropout=0.1)


def window_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--reps', type=int, default=500)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--bench-json', default=None, help='file holding the JSON result line of a bench.py run on this box')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'augment_cost.json'))
    args = ap.parse_args()
    import twog_gcn_amd  # noqa: F401
    from twog_gcn_amd.augment import InputAugmentation
    from twog_gcn_amd.hostcpu import limit_host_threads
    from twog_gcn_amd.kernels import get_kernels
    limit_host_threads()
    assert torch.cuda.is_available(), 'a measurement needs the GPU: there is no fallback'
    dev = torch.device('cuda', 0)
    K = get_kernels()
    assert K.name == 'hip'
    g = torch.Generator().manual_seed(0)
    x_human = torch.rand(BS, T, H, C + 4 * N, generator=g).to(dev)
    x_objects = torch.rand(BS, T, O, C, generator=g).to(dev)
    data = [x_human, x_objects, torch.ones(BS, O, device=dev), None, None, None, None, torch.full((BS,), float(T), device=dev)]
    ids = torch.arange(BS, device=dev)
    dst_h, dst_o = torch.empty_like(x_human), torch.empty_like(x_objects)
    augs = {'geometry': InputAugmentation(1, gcn_node=N, **GEOMETRY), 'features': InputAugmentation(1, gcn_node=N, **FEATURES),
            'both': InputAugmentation(1, gcn_node=N, **GEOMETRY, **FEATURES)}
    variants = {name: (lambda a=a: a(data, ids)) for name, a in augs.items()}
    variants['copy_torch'] = lambda: (dst_h.copy_(x_human), dst_o.copy_(x_objects))
    variants['copy_blocks'] = lambda: K.copy_blocks([(x_human, dst_h), (x_objects, dst_o)])
    for fn in variants.values():
        window_ms(fn, args.warmup)
    ms = {name: [] for name in variants}
    for _ in range(args.windows):
        for name, fn in variants.items():
            ms[name].append(window_ms(fn, args.reps))
    med = {name: statistics.median(v) for name, v in ms.items()}
    floor = min(med['copy_torch'], med['copy_blocks'])
    feature_floats = BS * T * (H + O) * C
    res = dict(clips=BS, T=T, humans=H, objects=O, channels=C, gcn_node=N, windows=args.windows, reps_per_window=args.reps,
               device=torch.cuda.get_device_name(0), options=dict(geometry=GEOMETRY, features=FEATURES),
               window_ms=ms, median_ms=med, copy_floor_ms=floor, ratio_to_copy={k: v / floor for k, v in med.items()},
               feature_floats=feature_floats, feature_bytes_read_and_written=8 * feature_floats,
               feature_generator_calls=feature_floats // 2,
               feature_pass_tb_per_s=8 * feature_floats / (med['features'] * 1e-3) / 1e12,
               copy_tb_per_s=8 * (x_human.numel() + x_objects.numel()) / (floor * 1e-3) / 1e12)
    if args.bench_json:
        with open(args.bench_json) as f:
            line = json.loads([ln for ln in f.read().splitlines() if ln.startswith('{')][-1])
        res['bench_ms_per_step'] = line['ms_per_step']
        res['share_of_step'] = {k: v / line['ms_per_step'] for k, v in med.items()}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k in ('median_ms', 'ratio_to_copy', 'share_of_step', 'bench_ms_per_step')}))


if __name__ == '__main__':
    main()
