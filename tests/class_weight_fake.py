"""The smoothing-loss test double (tests/smooth_loss_fake.py::SmoothLossFakeKernels) with the weighted criterion entry points
of 2g-gcn_amd/kernels.py (weighted_loss_fwd / weighted_loss_bwd) and class_counts, stated through the specification in
tests/class_weight_ref.py. For the CPU tests of the host layer in 2g-gcn_amd/losses.py. `calls` records, besides the parent's
entries, ('weighted_loss_fwd', n terms, positional arguments after `terms`, keyword arguments) and ('weighted_loss_bwd', need)."""
import math

import numpy as np
import torch

from tests import class_weight_ref as W
from tests.smooth_loss_fake import SmoothLossFakeKernels


class ClassWeightFakeKernels(SmoothLossFakeKernels):
    @staticmethod
    def _term_args(t):
        x, y, cw = t['input'], t['target'], t.get('class_weight')
        p = float(t.get('positive_class_weight', 1.0))
        assert x.is_contiguous() and y.is_contiguous() and x.dtype == torch.float32
        assert y.dtype == (torch.int64 if t['kind'] == W.NLL else torch.float32)
        assert cw is None or t['kind'] == W.NLL
        assert p == 1.0 or t['kind'] == W.BCE
        if cw is not None:
            assert cw.dtype == torch.float32 and cw.is_contiguous() and cw.shape == (x.shape[1],) and cw.device == x.device
            cw = cw.numpy()
        if not (math.isfinite(p) and p >= 0):   # the library's answer to a malformed term
            raise RuntimeError('twog_weighted_loss failed with code -1')
        return (t['kind'], x.numpy(), y.numpy(), t['weight'], t['ignore'], cw, p)

    def weighted_loss_fwd(self, terms, *args, **kwargs):
        self.calls.append(('weighted_loss_fwd', len(terms), args, dict(kwargs)))
        room = kwargs.get('room', args[0] if args else 0)
        n = len(terms)
        losses = torch.full((n + room,), float('nan'), dtype=torch.float32)   # the tail is smooth_loss_fwd's to write
        stats = torch.full((n + room, 2), float('nan'), dtype=torch.float64)
        for i, t in enumerate(terms):
            loss, (s, den) = W.forward(*self._term_args(t))
            losses[i] = torch.tensor(np.float32(loss))
            stats[i, 0], stats[i, 1] = float(s), float(den)
        return losses, stats

    def weighted_loss_bwd(self, terms, stats, dlosses, need):
        self.calls.append(('weighted_loss_bwd', tuple(bool(x) for x in need)))
        assert stats.shape[1:] == (2,) and stats.dtype == torch.float64
        out = []
        for i, (t, nd) in enumerate(zip(terms, need)):
            if not nd:
                out.append(None)
                continue
            g = W.gradient(*self._term_args(t), dloss=np.float32(float(dlosses[i])), den=float(stats[i, 1]))
            out.append(torch.from_numpy(g).reshape(t['input'].shape))
        return out

    def class_counts(self, targets, num_classes, ignore_index, counts):
        self.calls.append(('class_counts', int(num_classes), int(ignore_index)))
        assert targets.dtype == torch.int64 and counts.dtype == torch.int64 and counts.shape == (num_classes,)
        y = targets.numpy().ravel()
        y = y[(y != ignore_index) & (y >= 0) & (y < num_classes)]
        counts += torch.from_numpy(np.bincount(y, minlength=num_classes))
        return counts
