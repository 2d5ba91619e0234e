#!/usr/bin/env python3
"""Generate tests/golden/g18_geo_gcn_wide.npz by running the REAL reference's Geo_gcn(N, 4, 128) beyond 64 nodes.

Build container only (imports the reference, like tools/make_golden.py). It is G1's recipe (tools/make_golden.py, g1_geo_gcn:
weights and inputs from oracle/detgen.py, train and eval, outputs + parameter gradients + running statistics) at
N = 65, 72, 176 and 256, bs 2, T 2. The file has to stay small: y is whole for 65 and 72 and sampled with the fixed odd stride
Y_STRIDE for 176 and 256; gradients of more than GRAD_WHOLE elements are sampled with the fixed odd stride GRAD_STRIDE. The
strides are stored in the file; tests/test_gcn_wide_cpu.py samples the oracle's tensors the same way.
Usage:  TWOG_REFERENCE=<checkout of the reference> python tools/make_golden_gcn_wide.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('TWOG_REFERENCE')
if not REF:
    sys.exit('set TWOG_REFERENCE to a checkout of the reference (tanqiu98/2G-GCN)')
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

from oracle import detgen  # noqa: E402
from pyrutils.torch.models_gcn import Geo_gcn  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'g18_geo_gcn_wide.npz')
NODE_COUNTS = (65, 72, 176, 256)
Y_WHOLE = (65, 72)
Y_STRIDE = 17
GRAD_WHOLE = 4096
GRAD_STRIDE = 7
BS, T = 2, 2


def load_det(module, seed):
    shapes = {k: tuple(v.shape) for k, v in module.state_dict().items()}
    vals = detgen.fill_state_dict(shapes, seed=seed, gain=1.0)
    module.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in vals.items()})


def main():
    out = dict(y_stride=np.array(Y_STRIDE), grad_stride=np.array(GRAD_STRIDE), grad_whole=np.array(GRAD_WHOLE))
    for N in NODE_COUNTS:
        for mode in ('train', 'eval'):
            m = Geo_gcn(N, 4, 128)
            load_det(m, seed=100 + N)
            m.train(mode == 'train')
            x = torch.from_numpy(detgen.normal(f'g18.x.{N}', (BS, 4, N, T), std=1.0, seed=1))
            r = torch.from_numpy(detgen.normal(f'g18.r.{N}', (BS, 128, N, T), std=1.0, seed=2))
            y = m(x)
            (y * r).sum().backward()
            key = f'N{N}_{mode}'
            yf = y.detach().numpy()
            out[key + '_y'] = yf.copy() if N in Y_WHOLE else yf.reshape(-1)[::Y_STRIDE].copy()
            for name, p in m.named_parameters():
                g = p.grad.numpy()
                out[f'{key}_grad_{name}'] = g.copy() if g.size <= GRAD_WHOLE else g.reshape(-1)[::GRAD_STRIDE].copy()
                out[f'{key}_gradmax_{name}'] = np.array(np.abs(g).max())
            bn = m.joint_embed.cnn[0].bn
            out[key + '_running_mean'] = bn.running_mean.numpy().copy()
            out[key + '_running_var'] = bn.running_var.numpy().copy()
            out[key + '_nbt'] = np.array(int(bn.num_batches_tracked))
    np.savez_compressed(OUT, **out)
    print('g18:', len(out), 'arrays,', os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
