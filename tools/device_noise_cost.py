#!/usr/bin/env python3
"""What the Gumbel noise of the segment-boundary gates costs per training step, drawn on the host (the default: the CPU
default generator, then a copy from pageable memory) against drawn on the device (TGGCN.use_device_noise: one
twog_gumbel_noise_fill), at bench.py's headline shape (64 clips) and at 8 clips, on one MI355X.

  step      bench.py's training step (zero_grad, forward, criterion, backward, fused Adam) with the two routes ALTERNATED in
            windows of --window steps in one process; the first step of a window is dropped (the route just changed). Per
            step: the host time until the step function returns (everything enqueued) and the step time, a host clock
            that ends in a synchronise. Medians over all kept steps of a route, p10 / p90, and the difference of the medians.
            The baseline is the host route of this same tree, which is what the commit before the feature did.
  draw      the two draws alone, alternated: host = Gumbel(0, 1).sample + .to(device), device = the fill; host clock
            ending in a synchronise, and device events around the fill (its two launches).
  accuracy  the largest |noise - g| / max(1, |g|) against the fp64 specification of the same u (tests/gumbel_noise_ref.py) over
            the headline buffer, in units of 2^-22 (the bound of tests/test_device_noise_gpu.py).
Kernel times proper come from a separate `rocprofv3 --kernel-trace --stats -- python tools/device_noise_cost.py --windows 2
--out /dev/null` run. Writes profiles/device_noise_cost.json.    python tools/device_noise_cost.py [--windows 8]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 1234


def summary(v):
    v = sorted(v)
    q = lambda p: v[min(len(v) - 1, int(p * len(v)))]
    return dict(median=statistics.median(v), p10=q(0.1), p90=q(0.9), n=len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=8, help='windows per route and shape')
    ap.add_argument('--window', type=int, default=6, help='steps per window (the first is dropped)')
    ap.add_argument('--settle', type=int, default=12, help='untimed steps per route before the windows')
    ap.add_argument('--draws', type=int, default=200, help='rounds of the draw-alone measurement')
    ap.add_argument('--clips', type=int, nargs='+', default=None, help='shapes (default: the headline batch and 8)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'device_noise_cost.json'))
    args = ap.parse_args()
    import bench
    import twog_gcn_amd  # noqa: F401
    from tests import gumbel_noise_ref as R
    from twog_gcn_amd.distributed import DataParallel, FusedAdam
    from twog_gcn_amd.hostcpu import limit_host_threads
    from twog_gcn_amd.kernels import get_kernels
    from twog_gcn_amd.losses import select_loss
    from twog_gcn_amd.models import TGGCN
    limit_host_threads()
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    dev = torch.device('cuda', 0)
    K = get_kernels()
    assert K.name == 'hip'
    T, H, O, N = bench.T, bench.H, bench.O, bench.N_NODES
    criterion, _ = select_loss('2G-GCN', 'multiple', 'mphoi', dict(misc={}))
    res = dict(device=torch.cuda.get_device_name(0), shape=dict(T=T, H=H, O=O, N=N, h=bench.CFG['hidden_size']),
               windows=args.windows, steps_per_window=args.window, shapes={})
    for bs in (args.clips or [bench.BS, 8]):
        torch.manual_seed(0)
        model = TGGCN(input_size=(2048 + 4 * N, 2048), num_classes=(bench.N_CLASSES, None), **bench.CFG).to(dev).train()
        dp = DataParallel(model)
        opt = FusedAdam(dp.flat, lr=1e-4)
        x_human, x_objects, mask, targets = bench.synthetic_batch(bs, dev, seed=1234)
        seg = torch.ones(bs, T, H, device=dev)
        seg_target = torch.zeros(bs, T, H, device=dev)
        loss_targets = [seg_target, seg_target, targets[0], targets[1], targets[0], targets[1]]

        def step():
            dp.zero_grad()
            out = model(x_human, x_objects, mask, human_segmentation=seg)
            loss = sum(criterion(out, loss_targets))
            loss.backward()
            dp.all_reduce_gradients()
            opt.step(dp.grad_scale)
            return loss.detach()

        routes = {'host': model.use_host_noise, 'device': lambda: model.use_device_noise(*state)}
        state = (SEED, 0)
        # the shape of the noise buffer, as the forward asks for it
        seen = {}
        fill = K.gumbel_noise_fill

        def recording_fill(noise, t, e, b, *a, **k):
            seen.update(T=t, E=e, bs=b)
            return fill(noise, t, e, b, *a, **k)

        K.gumbel_noise_fill = recording_fill
        model.use_device_noise(SEED)
        step()
        del K.gumbel_noise_fill   # (the instance attribute: the method is back)
        state = model.device_noise_state()
        assert seen['T'] == T and seen['bs'] == bs, seen
        E = seen['E']
        for name, select in routes.items():
            select()
            for _ in range(args.settle):
                step()
            if name == 'device':
                state = model.device_noise_state()
        torch.cuda.synchronize()
        host_ms, step_ms = {k: [] for k in routes}, {k: [] for k in routes}
        for _ in range(args.windows):
            for name, select in routes.items():
                select()
                for i in range(args.window):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    step()
                    t1 = time.perf_counter()
                    torch.cuda.synchronize()
                    t2 = time.perf_counter()
                    if i:
                        host_ms[name].append((t1 - t0) * 1e3)
                        step_ms[name].append((t2 - t0) * 1e3)
                if name == 'device':
                    state = model.device_noise_state()   # the next device window continues the sequence
        model.use_host_noise()

        # ---- the draws alone
        st = K.new_noise_state(SEED, 0, device=dev)
        buf = torch.empty(T * E, bs, 2, device=dev)

        def host_draw():
            return torch.distributions.gumbel.Gumbel(0.0, 1.0).sample((T * E, bs, 2)).to(device=dev, non_blocking=True)

        draws = {'host': host_draw, 'device': lambda: K.gumbel_noise_fill(buf, T, E, bs, 0, st)}
        for fn in draws.values():
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        draw_ms, fill_event_ms = {k: [] for k in draws}, []
        for _ in range(args.draws):
            for name, fn in draws.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                draw_ms[name].append((time.perf_counter() - t0) * 1e3)
                if name == 'device':
                    fill_event_ms.append(a.elapsed_time(b))

        # ---- accuracy of the buffer of one more fill against the fp64 specification of the same u
        words = torch.empty(T * E * bs * 4, dtype=torch.int32, device=dev)
        K.gumbel_noise_fill(buf, T, E, bs, 0, st, words)
        w = words.cpu().numpy().view(np.uint32).reshape(T, E, bs, 4)
        want = R.gumbel_of_words(w[..., :2])
        got = buf.cpu().numpy().astype(np.float64).reshape(T, E, bs, 2)
        ratio = np.abs(got - want) / np.maximum(1.0, np.abs(want))

        hs, ss = {k: summary(v) for k, v in host_ms.items()}, {k: summary(v) for k, v in step_ms.items()}
        res['shapes'][f'{bs}_clips'] = dict(
            clips=bs, noise_shape=[T, E, bs, 2], noise_bytes=T * E * bs * 8,
            train_step_host_enqueue_ms=hs, train_step_ms_host_clock_with_sync=ss,
            device_minus_host_median_ms=dict(host_enqueue=hs['device']['median'] - hs['host']['median'],
                                             step=ss['device']['median'] - ss['host']['median']),
            draw_alone_ms_host_clock_with_sync={k: summary(v) for k, v in draw_ms.items()},
            fill_ms_device_events=summary(fill_event_ms),
            noise_max_error_in_units_of_2_pow_minus_22=float(ratio.max() * 2 ** 22), noise_all_finite=bool(np.isfinite(got).all()),
            words_equal_specification=bool(np.array_equal(w, R.noise_words(SEED, st.tolist()[1] - 1, T, E, bs))))
        dp.close()
        del model, dp, opt
    if args.out != '/dev/null':
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
    print(json.dumps({k: dict(step=v['train_step_ms_host_clock_with_sync'], host=v['train_step_host_enqueue_ms'],
                              draw=v['draw_alone_ms_host_clock_with_sync'], fill=v['fill_ms_device_events'])
                      for k, v in res['shapes'].items()}))


if __name__ == '__main__':
    main()
