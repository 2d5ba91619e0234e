#!/usr/bin/env python3
"""Generate the G16 golden vectors (tests/golden/g16_input_grads.npz): the REAL reference's gradients with respect to its
two feature inputs, `x_human.grad` and `x_objects.grad` (build container only; the reference never travels to the GPU box).

For each case below the inputs, weights and Gumbel noise are those of the G4 fixture tests/golden/g4_<case>.npz (the noise
is replayed, so the train-mode run repeats the G4 run); both inputs are autograd leaves; the loss is the G4 loss, the
projection of every differentiable output on its detgen cotangent. Each case runs in train mode (batch statistics in the
GCN's BatchNorm) and in eval mode (running statistics). Stored per case and mode, under '<case>_<mode>_':
    xh_geo     the geometry columns of x_human.grad in full, (bs, T, H, 4N)
    xh_vis     the visual columns of x_human.grad, strided as tests.helpers.sample_grad does, and xh_vis_stride
    xo         x_objects.grad, strided the same way, and xo_stride
    loss       the scalar that was differentiated
Usage:  python tools/make_golden_input_grads.py
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from make_golden import OUT  # noqa: E402  (puts the reference on sys.path)
from vhoi.models import TGGCN  # noqa: E402

from oracle import detgen  # noqa: E402
from tests.helpers import det_state_dict, g4_inputs, load_g4, sample_grad  # noqa: E402
from tests.input_grad_cases import G16_CASES, G16_LIMIT, sample_stride  # noqa: E402


class GumbelReplay:
    """Makes torch.distributions.gumbel.Gumbel.sample hand back recorded noise, draw by draw."""

    def __init__(self, noise):
        self.noise, self.i = noise, 0
        self._orig = torch.distributions.gumbel.Gumbel.sample

    def __enter__(self):
        rep = self

        def sample(self_, sample_shape=torch.Size()):
            g = rep.noise[rep.i]
            rep.i += 1
            assert tuple(g.shape) == tuple(sample_shape), (g.shape, sample_shape)
            return g.clone()

        torch.distributions.gumbel.Gumbel.sample = sample
        return self

    def __exit__(self, *a):
        torch.distributions.gumbel.Gumbel.sample = self._orig


def run(name, mode):
    z, meta = load_g4(name)
    model = TGGCN(input_size=(2048 + 4 * meta['N'], 2048), num_classes=tuple(meta['classes']), **meta['cfg'])
    model.load_state_dict(det_state_dict(meta['state_dict_shapes'], seed=meta['seed'], gain=meta['gain']))
    model.train(mode == 'train')
    kw = g4_inputs(z)
    kw['x_human'].requires_grad_(True)
    kw['x_objects'].requires_grad_(True)
    noise = torch.from_numpy(z['gumbel_noise'])
    with GumbelReplay(noise) as rep:
        out = model(**kw)
    assert rep.i == len(noise), (rep.i, len(noise))
    loss = 0
    for i, o in enumerate(out):
        if o.requires_grad:
            r = torch.from_numpy(detgen.normal(f'{name}.r{i}', tuple(o.shape), seed=meta['seed']))
            loss = loss + (o * r).sum()
    if mode == 'train':   # the replay repeats the G4 run
        got, want = float(loss.detach()), float(z['loss'])
        assert abs(got - want) <= 1e-5 * max(1.0, abs(want)), (got, want)
    loss.backward()
    gh, go = kw['x_human'].grad, kw['x_objects'].grad
    vis = gh[..., :2048].contiguous()
    key = f'{name}_{mode}_'
    return {key + 'xh_geo': gh[..., 2048:].numpy().copy(),
            key + 'xh_vis': sample_grad(vis, G16_LIMIT), key + 'xh_vis_stride': np.array(sample_stride(vis.numel())),
            key + 'xo': sample_grad(go, G16_LIMIT), key + 'xo_stride': np.array(sample_stride(go.numel())),
            key + 'loss': np.array(float(loss.detach()))}


def main():
    save = {}
    for name in G16_CASES:
        for mode in ('train', 'eval'):
            r = run(name, mode)
            save.update(r)
            k = f'{name}_{mode}_'
            geo = r[k + 'xh_geo']
            print(f'g16 {name} {mode}: loss={float(r[k + "loss"]):.5f} |geo h0|max={np.abs(geo[:, :, 0]).max():.3e} '
                  f'|geo h>=1|max={np.abs(geo[:, :, 1:]).max() if geo.shape[2] > 1 else 0.0:.1e} '
                  f'|vis|max={np.abs(r[k + "xh_vis"]).max():.3e} |xo|max={np.abs(r[k + "xo"]).max():.3e}')
    save['meta_json'] = np.array(json.dumps(dict(cases=G16_CASES, modes=['train', 'eval'], limit=G16_LIMIT)))
    path = os.path.join(OUT, 'g16_input_grads.npz')
    np.savez_compressed(path, **save)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
