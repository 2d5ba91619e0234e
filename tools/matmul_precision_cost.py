#!/usr/bin/env python3
"""What TGGCN.use_matmul_precision buys per training step: 'highest' (six bf16 chunk products per multiply in the 128x128
GEMM class, the default), 'high' (three) and 'medium' (one), alternated in one process on one device.

Shapes: the headline step of bench.py (64 clips x T 120 x N 34 x h 512: forward + loss + backward + Adam) and its 8-clip
shape (workload c2). After a settling run the three modes take turns in windows of --steps steps, --windows times round
(A/B/C, A/B/C, ...); every step is timed by a host clock that ends in a synchronise. Per mode: the median over all its
steps, and the medians of its single windows, whose range is the spread a difference between two modes has to exceed.
Beside the times: the worst deviation of the outputs (max abs over the log-probabilities) and of the parameter gradients
(max abs over the tensor's max abs) from 'highest', one step from the same parameters, inputs and Gumbel noise. At these
shapes the objects' hard gates are learned: a gate decision that flips moves everything behind it, so these deviations are
those of a training step, not of the arithmetic alone (tests/test_matmul_precision_gpu.py has the arithmetic).
Writes profiles/matmul_precision_cost.json.   python tools/matmul_precision_cost.py [--steps 8] [--windows 4]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the headline workload: its configuration, its synthetic batch; sets OMP_NUM_THREADS before torch)
import torch  # noqa: E402

MODES = ('highest', 'high', 'medium')


def measure(workload, args, device):
    import twog_gcn_amd  # noqa: F401
    from twog_gcn_amd.distributed import DataParallel, FusedAdam
    from twog_gcn_amd.losses import select_loss
    from twog_gcn_amd.models import TGGCN
    bench.select_workload(workload)
    T, H, O, bs = bench.T, bench.H, bench.O, bench.BS
    torch.manual_seed(0)
    model = TGGCN(input_size=(2048 + 4 * bench.N_NODES, 2048), num_classes=(bench.N_CLASSES, None), **bench.CFG).to(device).train()
    dp = DataParallel(model)
    opt = FusedAdam(dp.flat, lr=1e-4)
    criterion, _ = select_loss('2G-GCN', 'multiple', 'mphoi', dict(misc={}))
    x_human, x_objects, mask, targets = bench.synthetic_batch(bs, device, seed=1234)
    seg = torch.ones(bs, T, H, device=device)
    seg_target = torch.zeros(bs, T, H, device=device)
    loss_targets = [seg_target, seg_target, targets[0], targets[1], targets[0], targets[1]]
    flat0 = dp.flat.flat.clone()
    buffers0 = [b.clone() for b in model.buffers()]

    def step(adam=True):
        dp.zero_grad()
        out = model(x_human, x_objects, mask, human_segmentation=seg)
        loss = sum(criterion(out, loss_targets))
        loss.backward()
        if adam:
            dp.all_reduce_gradients()
            opt.step(dp.grad_scale)
        return out

    def timed():
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    hist = []
    for _ in range(40):   # settle as bench.py does: three steps in a row within 3 %
        hist.append(timed())
        if len(hist) >= 4 and max(hist[-3:]) <= 1.03 * min(hist[-3:]):
            break
    for mode in MODES:    # every mode's kernels have run before the first window
        model.use_matmul_precision(mode)
        timed()
    windows = {m: [] for m in MODES}
    for _ in range(args.windows):
        for mode in MODES:
            model.use_matmul_precision(mode)
            timed()   # the switch itself stays outside the window
            windows[mode].append([timed() for _ in range(args.steps)])
    med = statistics.median
    times = {}
    for mode, w in windows.items():
        wm = [med(x) for x in w]
        times[mode] = dict(median_ms=med([v for x in w for v in x]), window_medians_ms=wm, window_spread_ms=max(wm) - min(wm),
                           steps=sum(len(x) for x in w))
    base = times['highest']['median_ms']
    for mode in MODES:
        times[mode]['ratio_to_highest'] = times[mode]['median_ms'] / base

    # deviation of one step from 'highest': same parameters, batch-norm statistics, inputs and noise
    n_gated = O   # the humans' segmentation is given, the objects draw their own
    noise = torch.distributions.gumbel.Gumbel(0.0, 1.0).sample((T * n_gated, bs, 2)).to(device)
    model._gumbel_noise_override = noise
    runs = {}
    for mode in MODES + ('highest',):   # 'highest' a second time: what the comparison itself shows on equal arithmetic
        with torch.no_grad():
            dp.flat.flat.copy_(flat0)
            for b, b0 in zip(model.buffers(), buffers0):
                b.copy_(b0)
        model.use_matmul_precision(mode)
        out = step(adam=False)
        torch.cuda.synchronize()
        runs['highest again' if mode in runs else mode] = ([o.detach().clone() for o in out], {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None})
    model._gumbel_noise_override = None
    model.use_matmul_precision('highest')
    dev = {}
    out0, g0 = runs['highest']
    for mode in MODES[1:] + ('highest again',):
        out1, g1 = runs[mode]
        worst, name, all_d = 0.0, None, []
        for n, g in g0.items():
            d = float((g1[n] - g).abs().max() / g.abs().max().clamp_min(1e-30))
            all_d.append(d)
            if d > worst:
                worst, name = d, n
        dev[mode] = dict(out_max_abs_log_prob=max(float((a - b).abs().max()) for a, b in zip(out1[2:6], out0[2:6])),
                         grad_max_abs_of_scale=worst, worst_gradient=name, grad_median_over_tensors=statistics.median(all_d), finite=bool(all(torch.isfinite(g).all() for g in g1.values())))
    return dict(clips=bs, T=T, H=H, O=O, N=bench.N_NODES, hidden=bench.CFG['hidden_size'], settling_steps=len(hist),
                step_ms=times, deviation_from_highest=dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=8, help='steps of one window of one mode')
    ap.add_argument('--windows', type=int, default=4, help='windows per mode and shape')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'matmul_precision_cost.json'))
    args = ap.parse_args()
    import twog_gcn_amd  # noqa: F401
    from twog_gcn_amd.hostcpu import limit_host_threads
    from twog_gcn_amd.kernels import get_kernels
    limit_host_threads()
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    assert get_kernels().name == 'hip'
    device = torch.device('cuda', 0)
    res = dict(device=torch.cuda.get_device_name(0), steps_per_window=args.steps, windows_per_mode=args.windows,
               step='forward + loss + backward + Adam, host clock ending in a synchronise',
               shapes={'headline_bs64': measure('c3', args, device), 'clips8': measure('c2', args, device)})
    if args.out != '/dev/null':
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
    print(json.dumps({k: {m: (round(t['median_ms'], 2), round(t['window_spread_ms'], 2)) for m, t in v['step_ms'].items()}
                      for k, v in res['shapes'].items()}))
    print(json.dumps({k: v['deviation_from_highest'] for k, v in res['shapes'].items()}))


if __name__ == '__main__':
    main()
