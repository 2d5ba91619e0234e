#!/usr/bin/env python3
"""Generate golden G19 (tests/golden/g19_class_weights.npz): the reference's `binary_cross_entropy_loss` with
`positive_class_weight` (pyrutils/torch/losses.py:7-21, imported from the REAL reference; build container only) and torch's
`F.nll_loss(weight=, ignore_index=-1)`, values and input gradients, on small inputs:
  BCE  input (3, 17, 2) in [1e-3, 1 - 1e-3], targets 0 / 1 / a smoothed 0.5 / ignored (-1), p in {0.5, 1, 1.5, 2, 3};
  NLL  log-probabilities (3, 13, 17, 2), targets with ignored entries, two weight vectors (one with a zero-weight class, a
       1e-3 and a 1e3).
Prints the largest relative deviation of the fp64 form of the specification (tests/class_weight_ref.py, real=F64) from the
reference, for the loss and for the gradient (element by element, over the non-zero elements): the golden test gates at four
times these. Usage:  python tools/make_golden_class_weights.py  (TWOG_REFERENCE names the reference checkout)
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from make_golden import REF  # noqa: E402,F401  (puts the reference on sys.path, as for every other golden vector)

from pyrutils.torch.losses import binary_cross_entropy_loss  # noqa: E402  (the reference's)

from tests import class_weight_ref as W  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'g19_class_weights.npz')
PS = [0.5, 1.0, 1.5, 2.0, 3.0]


def rel(a, b):
    """Largest |a - b| / |b| over the elements where b != 0; the zeros must coincide."""
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    assert np.array_equal(a == 0, b == 0)
    nz = b != 0
    return float(np.max(np.abs(a[nz] - b[nz]) / np.abs(b[nz]))) if nz.any() else 0.0


def main():
    g = torch.Generator().manual_seed(19)
    out = {}
    # ---- BCE
    x = torch.rand(3, 17, 2, generator=g) * (1 - 2e-3) + 1e-3
    x[0, 0, 0], x[0, 1, 0] = 1e-3, 1 - 1e-3
    t = (torch.rand(3, 17, 2, generator=g) < 0.35).float()
    t[torch.rand(3, 17, 2, generator=g) < 0.2] = -1.0
    t[1, 3, 0], t[2, 5, 1] = 0.5, 0.5
    t[0, 0, 0], t[0, 1, 0] = 1.0, 1.0
    out['bce_x'], out['bce_t'], out['bce_p'] = x.numpy(), t.numpy(), np.asarray(PS, np.float32)
    dev_loss = dev_grad = 0.0
    for p in PS:
        leaf = x.clone().requires_grad_(True)
        loss = binary_cross_entropy_loss(leaf, t, positive_class_weight=p)
        loss.backward()
        out[f'bce_loss_{p}'], out[f'bce_grad_{p}'] = loss.detach().numpy(), leaf.grad.numpy()
        spec, (_, den) = W.forward(W.BCE, x.numpy(), t.numpy(), positive_class_weight=p, real=W.F64)
        grad = W.gradient(W.BCE, x.numpy(), t.numpy(), positive_class_weight=p, den=den, real=W.F64)
        dev_loss, dev_grad = max(dev_loss, rel(spec, float(loss.detach()))), max(dev_grad, rel(grad, leaf.grad.numpy()))
    print(f'BCE: fp64 specification against the reference: loss {dev_loss:.3e}, gradient {dev_grad:.3e}')
    # ---- NLL
    C = 13
    xn = torch.log_softmax(torch.randn(3, C, 17, 2, generator=g) * 3, 1)
    y = torch.randint(0, C, (3, 17, 2), generator=g)
    y[torch.rand(3, 17, 2, generator=g) < 0.2] = -1
    cws = torch.stack([torch.rand(C, generator=g) * 2 + 0.1, torch.rand(C, generator=g) * 2 + 0.1])
    cws[1, 4], cws[1, 7], cws[1, 9] = 0.0, 1e-3, 1e3
    out['nll_x'], out['nll_y'], out['nll_cw'] = xn.numpy(), y.numpy(), cws.numpy()
    dev_loss = dev_grad = 0.0
    for k, cw in enumerate(cws):
        leaf = xn.clone().requires_grad_(True)
        loss = F.nll_loss(leaf, y, weight=cw, ignore_index=-1)
        loss.backward()
        out[f'nll_loss_{k}'], out[f'nll_grad_{k}'] = loss.detach().numpy(), leaf.grad.numpy()
        spec, (_, den) = W.forward(W.NLL, xn.numpy(), y.numpy(), class_weight=cw.numpy(), real=W.F64)
        grad = W.gradient(W.NLL, xn.numpy(), y.numpy(), class_weight=cw.numpy(), den=den, real=W.F64)
        dev_loss, dev_grad = max(dev_loss, rel(spec, float(loss.detach()))), max(dev_grad, rel(grad, leaf.grad.numpy()))
    print(f'NLL: fp64 specification against F.nll_loss(weight=): loss {dev_loss:.3e}, gradient {dev_grad:.3e}')
    np.savez(OUT, **out)
    print(f'wrote {OUT} ({os.path.getsize(OUT)} bytes)')


if __name__ == '__main__':
    main()
