#!/usr/bin/env python3
"""Training-step time of the two baseline models on the HIP path against the same models composed of PyTorch-ROCm eager
ops (nn.GRU / nn.Linear, written here), alternated in one process. One GPU process; prints one JSON line.

A step is forward + criterion (nll, the baselines' select_loss) + backward + Adam, timed with device events after warm-up.
Sizes: Bimanual H = 2, O = 9, F_h = 2168; CAD-120 H = 1, O = 5, F_h = 2124, classes (10, 12); T = 120; 16 and 64 clips;
hidden_size 128 and 512. At each size the two paths are also checked to agree (same weights, same batch).

Usage: python tools/baseline_bench.py [--steps 10] [--warmup 3] [--out profiles/baselines_bench.json]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import twog_gcn_amd  # noqa: E402,F401
from twog_gcn_amd import baselines  # noqa: E402
from twog_gcn_amd.hostcpu import limit_host_threads  # noqa: E402

KINDS = {'bimanual': dict(H=2, O=9, F=(2168, 2048), classes=(14, None), name='bimanual_baseline'),
         'cad120': dict(H=1, O=5, F=(2124, 2048), classes=(10, 12), name='cad120_baseline')}


class Eager(torch.nn.Module):
    """The baseline forward in eager PyTorch: every entity of a type goes through nn.GRU as one batch row."""

    def __init__(self, hip_model):
        super().__init__()
        self.m = hip_model   # the same parameter containers, called here as modules

    def forward(self, x_h, x_o, mask):
        m = self.m
        bs, T, H, _ = x_h.shape
        O = x_o.shape[2]

        def rnn(x, gru):
            E = x.shape[2]
            y, _ = gru(x.permute(0, 2, 1, 3).reshape(bs * E, T, -1))
            return y.reshape(bs, E, T, -1).permute(0, 2, 1, 3)

        hfr = rnn(m.human_embedding_mlp[1](m.human_embedding_mlp[0](x_h)), m.human_bd_rnn)
        ofr = rnn(m.object_embedding_mlp[1](m.object_embedding_mlp[0](x_o)), m.object_bd_rnn)
        mk = mask[:, None, :, None]
        pool = (ofr * mk).sum(2, keepdim=True) / mk.sum(2, keepdim=True).clamp(min=1.0)
        hin = torch.cat([hfr, pool.expand(-1, -1, H, -1)], -1)
        outs = [F.log_softmax(m.human_recognition_mlp[0](hin), -1).permute(0, 3, 1, 2).contiguous()]
        if hasattr(m, 'object_recognition_mlp'):
            oin = torch.cat([ofr, hfr.sum(2, keepdim=True).expand(-1, -1, O, -1)], -1)
            outs.append(F.log_softmax(m.object_recognition_mlp[0](oin), -1).permute(0, 3, 1, 2).contiguous())
        return outs


def batch(kind, bs, T, dev, seed=0):
    k = KINDS[kind]
    g = torch.Generator().manual_seed(seed)
    x_h = torch.rand(bs, T, k['H'], k['F'][0], generator=g).to(dev)
    x_o = torch.rand(bs, T, k['O'], k['F'][1], generator=g).to(dev)
    mask = torch.ones(bs, k['O'])
    mask[0, -1] = 0.0
    ys = [torch.randint(0, k['classes'][0], (bs, T, k['H']), generator=g).to(dev)]
    if k['classes'][1] is not None:
        ys.append(torch.randint(0, k['classes'][1], (bs, T, k['O']), generator=g).to(dev))
    return x_h, x_o, mask.to(dev), ys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--T', type=int, default=120)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    limit_host_threads()
    dev = 'cuda:0'
    cases = []
    for kind in ('bimanual', 'cad120'):
        for bs in (16, 64):
            for h in (128, 512):
                k = KINDS[kind]
                torch.manual_seed(0)
                model = baselines.select_model(k['name'])(input_size=k['F'], num_classes=k['classes'], hidden_size=h).to(dev)
                eager = Eager(model)
                crit, _ = baselines.select_loss(k['name'], 'multiple', kind, {})
                opt = torch.optim.Adam(model.parameters(), lr=1e-4)
                x_h, x_o, mask, ys = batch(kind, bs, a.T, dev)
                # agreement at the timed size (forward outputs and the first parameter gradients, before any step)
                with torch.no_grad():
                    o_hip, o_eag = model(x_h, x_o, mask), eager(x_h, x_o, mask)
                agree = max(float((p - q).abs().max() / q.abs().max()) for p, q in zip(o_hip, o_eag))
                model.zero_grad()
                sum(crit(model(x_h, x_o, mask), ys)).backward()
                g_hip = [p.grad.clone() for p in model.parameters()]
                model.zero_grad()
                sum(F.nll_loss(o.contiguous(), y, ignore_index=-1) for o, y in zip(eager(x_h, x_o, mask), ys)).backward()
                g_err = max(float((p.grad - q).abs().max() / (p.grad.abs().max() + 1e-30)) for p, q in zip(model.parameters(), g_hip))

                def step_hip():
                    opt.zero_grad()
                    sum(crit(model(x_h, x_o, mask), ys)).backward()
                    opt.step()

                def step_eager():
                    opt.zero_grad()
                    sum(F.nll_loss(o, y, ignore_index=-1) for o, y in zip(eager(x_h, x_o, mask), ys)).backward()
                    opt.step()

                times = {'hip': [], 'eager': []}
                for i in range(a.warmup + a.steps):   # alternated, same process, same weights
                    for tag, fn in (('hip', step_hip), ('eager', step_eager)):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        fn()
                        e1.record()
                        e1.synchronize()
                        if i >= a.warmup:
                            times[tag].append(e0.elapsed_time(e1))
                row = dict(model=kind, bs=bs, T=a.T, hidden=h)
                for tag in ('hip', 'eager'):
                    ms = sorted(times[tag])[len(times[tag]) // 2]
                    row[f'{tag}_ms'] = round(ms, 3)
                    row[f'{tag}_clips_per_s'] = round(bs / ms * 1e3, 1)
                row['speedup'] = round(row['eager_ms'] / row['hip_ms'], 3)
                row['max_rel_output_diff'] = agree
                row['max_rel_grad_diff'] = g_err
                cases.append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
                del model, eager, opt
                torch.cuda.empty_cache()
    line = json.dumps(dict(metric='baseline_step_ms_median', steps=a.steps, warmup=a.warmup, cases=cases))
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
