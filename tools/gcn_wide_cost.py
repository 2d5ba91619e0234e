#!/usr/bin/env python3
"""What the geometric-level GCN block costs beyond 64 nodes (the wide kernel family, csrc/geo_wide.hip) on one MI355X.

  block time     the block's kernels forward + backward -- bn_fold (with the similarity fold), gcn_fused_fwd, gcn_embed1_fwd,
                 gcn_attn2_bwd, gcn_embed1_bwd through HipKernels, which picks the kernel family -- at 8 clips x T 120, H 2:
                 at N = 64 through the tuned kernels and through the wide family (HipKernels' private switch) on the same
                 inputs in ALTERNATING windows, at N = 72, 176 and 256 through the wide family. Device events between
                 device synchronisations; medians. (The strided output GEMM and the two X GEMMs of the backward pass are the
                 same launches in both families and are left out.)
  bytes          achieved bytes/s over the algorithmic T * (16 N + 512 N) bytes per clip of the forward pass
                 (ops.geo_gcn_forward) against the forward kernel's time.
  kernels        per-kernel times come from a separate run under the profiler,
                     rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- \\
                         python tools/gcn_wide_cost.py --rounds 5 --out /dev/null
                 whose kernel-stats CSV is then given to a plain run with --kernel-stats.
Writes profiles/gcn_wide_cost.json. This is a record, not a gate.    python tools/gcn_wide_cost.py [--rounds 20]
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

CLIPS, T, H = 8, 120, 2
COPY_BW_TBS = 6.29   # MI355X microarchitecture guide: float4 copy, measured


def make_case(N, dev):
    g = torch.Generator().manual_seed(N)
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(dev)
    xh = torch.zeros(CLIPS, T, H, 2048 + 4 * N)
    xh[..., 2048:] = torch.randn(CLIPS, T, H, 4 * N, generator=g)
    rows = CLIPS * T * N
    return dict(N=N, xh=xh.to(dev), gamma=r(4 * N).abs() + 0.5, beta=r(4 * N), rm=r(4 * N, scale=0.1), rv=r(4 * N).abs() + 0.5,
                nbt=torch.zeros((), dtype=torch.int64, device=dev), w1=r(64, 4), b1=r(64), w2=r(64, 64, scale=0.2),
                b2=r(64, scale=0.2), wq=r(128, 64, scale=0.02), wk=r(128, 64, scale=0.02), bq=r(128, scale=0.1),
                dz=r(rows, 64), de1=r(rows, 64))


def run_block(K, c, ev):
    """One forward + backward of the block's kernels; ev: three events (start, after the forward, end)."""
    N, xh = c['N'], c['xh']
    ev[0].record()
    ab, mi, md = K.bn_fold(xh, N, c['gamma'], c['beta'], c['rm'], c['rv'], c['nbt'], True, fold=(c['wq'], c['wk'], c['bq']))
    X, adj, Z = K.gcn_fused_fwd(xh, N, ab, c['w1'], c['b1'], c['w2'], c['b2'], md)
    ev[1].record()
    e1 = K.gcn_embed1_fwd(xh, N, ab, c['w1'], c['b1'])
    K.gcn_attn2_bwd(X, md, adj, c['dz'], CLIPS * T, N)
    K.gcn_embed1_bwd(xh, N, ab, mi, c['w1'], c['de1'])
    ev[2].record()
    return e1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--kernel-stats', help='kernel_stats.csv of the separate rocprofv3 run')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gcn_wide_cost.json'))
    args = ap.parse_args()
    import twog_gcn_amd  # noqa: F401
    from twog_gcn_amd.kernels import get_kernels
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    dev = torch.device('cuda', 0)
    K = get_kernels()
    assert K.name == 'hip'
    variants = [('N64_tuned', 64, False), ('N64_wide', 64, True), ('N72_wide', 72, False), ('N176_wide', 176, False),
                ('N256_wide', 256, False)]
    cases = {N: make_case(N, dev) for N in sorted({v[1] for v in variants})}
    ms = {v[0]: dict(block=[], forward=[]) for v in variants}
    for r in range(args.warmup + args.rounds):
        for name, N, forced in variants:     # alternating windows: every variant once per round
            K._force_wide = forced
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            torch.cuda.synchronize()
            run_block(K, cases[N], ev)
            torch.cuda.synchronize()
            K._force_wide = False
            if r >= args.warmup:
                ms[name]['block'].append(ev[0].elapsed_time(ev[2]))
                ms[name]['forward'].append(ev[0].elapsed_time(ev[1]))
    res = dict(device=torch.cuda.get_device_name(0), shape=dict(clips=CLIPS, T=T, H=H), rounds=args.rounds, variants={})
    for name, N, forced in variants:
        fwd, blk = statistics.median(ms[name]['forward']), statistics.median(ms[name]['block'])
        alg = CLIPS * T * (16 * N + 512 * N)
        res['variants'][name] = dict(N=N, family='wide' if forced or N > 64 else 'tuned', block_ms_median=blk, forward_ms_median=fwd,
                                     algorithmic_forward_bytes=alg, achieved_TBs_over_algorithmic_bytes=alg / (fwd * 1e-3) / 1e12,
                                     share_of_float4_copy_bandwidth=alg / (fwd * 1e-3) / 1e12 / COPY_BW_TBS)
    res['kernel_times'] = 'not measured (give --kernel-stats)'
    if args.kernel_stats:
        rows = [r for r in csv.DictReader(open(args.kernel_stats))
                if any(k in r['Name'] for k in ('gcn_wide', 'gcn_fused', 'gcn_attn2', 'bn_stats', 'bn_finalize', 'embed1'))]
        res['kernel_times'] = dict(source='rocprofv3 --kernel-trace --stats, separate run',
                                   kernels=[dict(name=r['Name'], calls=int(r['Calls']), average_us=float(r['AverageNs']) / 1e3,
                                                 min_us=float(r['MinNs']) / 1e3, max_us=float(r['MaxNs']) / 1e3) for r in rows])
    if args.out != '/dev/null':
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
    print(json.dumps({k: dict(block_ms=v['block_ms_median'], forward_ms=v['forward_ms_median']) for k, v in res['variants'].items()}))


if __name__ == '__main__':
    main()
