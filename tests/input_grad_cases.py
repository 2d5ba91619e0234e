"""Shared by the input-gradient tests (tests/test_input_grads_cpu.py, test_input_grads_gpu.py) and by
tools/make_golden_input_grads.py: the G16 cases, the fixture's sampling, the oracle's input gradients and a run of the
product path that asks for them."""
import json
import os

import numpy as np
import torch

from oracle import cpu_ref, detgen
from tests.helpers import GOLDEN, det_state_dict, g4_inputs, load_g4

G16_CASES = ['c1_stage1', 'c1_stage2', 'c2_stage1', 'c2_stage2', 'c5_stage1', 'c2_relational', 'c2_distance', 'c2_concat']
G16_MODES = ['train', 'eval']
G16_LIMIT = 4096


def sample_stride(size, limit=G16_LIMIT):
    """The stride tests.helpers.sample_grad takes through a flat tensor of `size` elements."""
    return 1 if size <= limit else size // limit


def load_g16():
    z = np.load(os.path.join(GOLDEN, 'g16_input_grads.npz'), allow_pickle=False)
    return z, json.loads(str(z['meta_json']))


def g4_loss(name, meta, out):
    """The G4 scalar: every differentiable output projected on its detgen cotangent (tests/test_oracle_golden.py)."""
    loss = 0
    for i, o in enumerate(out):
        if o.requires_grad:
            r = torch.from_numpy(detgen.normal(f'{name}.r{i}', tuple(o.shape), seed=meta['seed'])).to(o.device, o.dtype)
            loss = loss + (o * r).sum()
    return loss


def oracle_run(name, mode, dtype=torch.float32):
    """cpu_ref with both inputs as autograd leaves -> dict(xh=x_human.grad, xo=x_objects.grad, out=outputs, sd=state dict
    whose parameters carry .grad)."""
    z, meta = load_g4(name)
    sd = det_state_dict(meta['state_dict_shapes'], seed=meta['seed'], gain=meta['gain'])
    sd = {k: (v.to(dtype).requires_grad_('running_' not in k) if v.is_floating_point() else v) for k, v in sd.items()}
    kw = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in g4_inputs(z).items()}
    kw['x_human'].requires_grad_(True)
    kw['x_objects'].requires_grad_(True)
    noise = torch.from_numpy(z['gumbel_noise']).to(dtype)
    out = cpu_ref.tggcn_forward(sd, meta['cfg'], training=(mode == 'train'), gumbel_noise=noise if len(noise) else None, **kw)
    g4_loss(name, meta, out).backward()
    return dict(xh=kw['x_human'].grad, xo=kw['x_objects'].grad, out=[o.detach() for o in out], sd=sd)


def build_model(meta, device='cpu'):
    from twog_gcn_amd.models import TGGCN
    m = TGGCN(input_size=(2048 + 4 * meta['N'], 2048), num_classes=tuple(meta['classes']), **meta['cfg'])
    m.load_state_dict(det_state_dict(meta['state_dict_shapes'], seed=meta['seed'], gain=meta['gain']))
    return m.to(device)


def product_forward(name, mode, need=(True, True), device='cpu', model=None):
    """The product model on the G4 inputs of `name`; x_human / x_objects require grad as `need` says.
    -> (model, kwargs, outputs, loss)."""
    z, meta = load_g4(name)
    m = build_model(meta, device) if model is None else model
    m.train(mode == 'train')
    noise = torch.from_numpy(z['gumbel_noise'])
    m._gumbel_noise_override = noise.to(device) if len(noise) else None
    kw = {k: v.to(device) for k, v in g4_inputs(z).items()}
    kw['x_human'].requires_grad_(need[0])
    kw['x_objects'].requires_grad_(need[1])
    out = m(**kw)
    return m, kw, out, g4_loss(name, meta, out)
