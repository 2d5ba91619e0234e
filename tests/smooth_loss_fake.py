"""The training-options test double (tests/train_options_helpers.py::TrainOptionKernels, a FakeKernels) with the temporal
smoothing entry points of 2g-gcn_amd/kernels.py, stated through the specification in tests/smooth_loss_ref.py. For the CPU
tests of the host layer in 2g-gcn_amd/losses.py. `calls` records every criterion call the host layer made, in order:
('multitask_loss_fwd', n terms, positional arguments after `terms`, keyword arguments), ('multitask_loss_bwd', need),
('smooth_loss_fwd', m), ('smooth_loss_bwd', terms with a buffer, accumulate flags)."""
import torch

from tests import smooth_loss_ref as S
from tests.train_options_helpers import TrainOptionKernels


class SmoothLossFakeKernels(TrainOptionKernels):
    def multitask_loss_fwd(self, terms, *args, **kwargs):
        self.calls.append(('multitask_loss_fwd', len(terms), args, dict(kwargs)))
        room = kwargs.get('room', args[0] if args else 0)
        losses, stats = super().multitask_loss_fwd(terms)
        if not room:
            return losses, stats
        n = len(terms)
        all_losses = torch.full((n + room,), float('nan'), dtype=torch.float32)   # the tail is smooth_loss_fwd's to write
        all_stats = torch.full((n + room, 2), float('nan'), dtype=torch.float64)
        all_losses[:n], all_stats[:n] = losses, stats
        return all_losses, all_stats

    def multitask_loss_bwd(self, terms, stats, dlosses, need):
        self.calls.append(('multitask_loss_bwd', tuple(bool(x) for x in need)))
        return super().multitask_loss_bwd(terms, stats, dlosses, need)

    @staticmethod
    def _check_term(t):
        x, y = t['input'], t['target']
        assert x.is_contiguous() and y.is_contiguous() and x.dtype == torch.float32 and y.dtype == torch.int64
        assert x.dim() == 4 and y.shape == (x.shape[0], x.shape[2], x.shape[3])
        if not t['tau'] > 0:   # the library's answer to a malformed term
            raise RuntimeError('twog_smooth_loss failed with code -1')

    def smooth_loss_fwd(self, terms, losses_out, stats_out):
        self.calls.append(('smooth_loss_fwd', len(terms)))
        assert losses_out.shape == (len(terms),) and stats_out.shape == (len(terms), 2)
        for j, t in enumerate(terms):
            self._check_term(t)
            loss, (s, c) = S.forward(t['input'].numpy(), t['target'].numpy(), t['weight'], t['tau'], t['ignore'])
            losses_out[j] = float(loss)
            stats_out[j, 0], stats_out[j, 1] = float(s), float(c)

    def smooth_loss_bwd(self, terms, stats, dlosses, dins, accumulate):
        self.calls.append(('smooth_loss_bwd', tuple(d is not None for d in dins), tuple(bool(a) for a in accumulate)))
        assert stats.shape == (len(terms), 2) and dlosses.shape == (len(terms),)
        ptrs = [d.data_ptr() for d in dins if d is not None]
        assert len(set(ptrs)) == len(ptrs)
        for j, (t, d) in enumerate(zip(terms, dins)):
            if d is None:
                continue
            self._check_term(t)
            g = torch.from_numpy(S.gradient(t['input'].numpy(), t['target'].numpy(), t['weight'], t['tau'], t['ignore'],
                                            dloss=float(dlosses[j]), count=float(stats[j, 1])))
            if accumulate[j]:
                d.copy_(torch.where(g != 0, d + g, d))
            else:
                d.copy_(g)
