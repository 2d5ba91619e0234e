#!/usr/bin/env python3
"""What the optimizer step costs with its step state on the device (FusedAdam's device path: twog_optim_prepare +
twog_optim_apply) against the step without it (twog_adam_step, what the commit before the feature ran and what bench.py still
runs), at the headline model's flat size FlatParameters(TGGCN(BASELINE configs[2])).numel, on one MI355X.

Five optimizers over ONE pair of flat parameter / gradient buffers (each with its own moments), stepped in ALTERNATING windows
of --window steps in one process: `legacy` (today's arguments), `neutral` (device_state=True, nothing else), `ema`, `skip`
(skip_nonfinite: one gradient-norm pass more) and `all` (max_grad_norm + skip_nonfinite + ema_decay). A window is timed by two
device events around its steps (no host synchronisation inside); every optimizer is warmed before the first window. Per
optimizer: the per-step median over the windows, p10 / p90, the bytes a step must move (computed from the size: 28 B per element,
+8 with EMA, +4 per norm pass) and the rate that gives, and the ratio to `legacy` of the same run. A record, not a gate.

Kernel times proper come from a separate `rocprofv3 --kernel-trace --stats -- python tools/optim_state_cost.py --windows 2
--out /dev/null` run. Writes profiles/optim_state_cost.json.    python tools/optim_state_cost.py [--windows 10]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = {
    'legacy': (dict(), 28),
    'neutral': (dict(device_state=True), 28),
    'ema': (dict(ema_decay=0.999), 36),
    'skip': (dict(skip_nonfinite=True), 32),
    'all': (dict(max_grad_norm=1.0, skip_nonfinite=True, ema_decay=0.999), 40),
}


def summary(v):
    v = sorted(v)
    q = lambda p: v[min(len(v) - 1, int(p * len(v)))]
    return dict(median=statistics.median(v), p10=q(0.1), p90=q(0.9), n=len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=10, help='windows per optimizer')
    ap.add_argument('--window', type=int, default=20, help='steps per window')
    ap.add_argument('--warmup', type=int, default=5, help='untimed steps per optimizer before the windows')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'optim_state_cost.json'))
    args = ap.parse_args()
    import bench
    import twog_gcn_amd  # noqa: F401
    from twog_gcn_amd.distributed import FlatParameters, FusedAdam
    from twog_gcn_amd.hostcpu import limit_host_threads
    from twog_gcn_amd.kernels import get_kernels
    from twog_gcn_amd.models import TGGCN
    limit_host_threads()
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    dev = torch.device('cuda', 0)
    assert get_kernels().name == 'hip'
    torch.manual_seed(0)
    model = TGGCN(input_size=(2048 + 4 * bench.N_NODES, 2048), num_classes=(bench.N_CLASSES, None), **bench.CFG).to(dev).train()
    flat = FlatParameters(model)
    n = flat.numel
    flat.grad.copy_(torch.randn(n, device=dev) * 1e-3)
    opts = {name: FusedAdam(flat, lr=1e-6, **kw) for name, (kw, _) in VARIANTS.items()}
    for opt in opts.values():
        for _ in range(args.warmup):
            opt.step(1.0)
    torch.cuda.synchronize()
    times = {name: [] for name in opts}
    for _ in range(args.windows):
        for name, opt in opts.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.window):
                opt.step(1.0)
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1) * 1e3 / args.window)   # microseconds per step
    assert bool(torch.isfinite(flat.flat).all()) and all(o.skipped_steps() == 0 for o in opts.values())
    res = dict(device=torch.cuda.get_device_name(0), numel=n, mbytes_per_buffer=n * 4 / 1e6, windows=args.windows,
               steps_per_window=args.window, unit='microseconds per optimizer step (device events around a window of steps)',
               optimizers={})
    base = statistics.median(times['legacy'])
    for name, (kw, bytes_per_el) in VARIANTS.items():
        s = summary(times[name])
        res['optimizers'][name] = dict(options=kw, us=s, bytes_per_step=bytes_per_el * n,
                                       tbytes_per_s=bytes_per_el * n / (s['median'] * 1e-6) / 1e12,
                                       ratio_to_legacy=s['median'] / base)
        print(f"{name:8s} {s['median']:8.1f} us  (p10 {s['p10']:.1f}, p90 {s['p90']:.1f})  x{s['median'] / base:.3f} of legacy, "
              f"{res['optimizers'][name]['tbytes_per_s']:.2f} TB/s")
    if args.out != '/dev/null':
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
