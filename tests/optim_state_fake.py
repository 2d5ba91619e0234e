"""The kernel test double of Adam with its step state on the device: tests.train_options_helpers.TrainOptionKernels plus
new_optim_state / optim_prepare / optim_apply from the numpy specification (tests/optim_state_ref.py), on CPU tensors. The state
block is the same uint8 [64] tensor the HIP backend keeps on the device. Records every call in `calls`."""
import numpy as np
import torch

from tests import optim_state_ref as R
from tests.train_options_helpers import TrainOptionKernels
from twog_gcn_amd.kernels import optim_state_block


class OptimStateKernels(TrainOptionKernels):
    STREAM_OPTIM = 13
    OPTIM_CLIP, OPTIM_DECOUPLED, OPTIM_SKIP_NONFINITE = R.CLIP, R.DECOUPLED, R.SKIP_NONFINITE

    def new_optim_state(self, step, skipped, beta1, beta2, device, powers=None):
        self.calls.append(('new_optim_state', int(step), int(skipped)))
        return optim_state_block(step, skipped, beta1, beta2, powers).to(device)

    @staticmethod
    def _scalar(t):
        return None if t is None else t.detach().reshape(-1)[0].item()

    def optim_prepare(self, state, hyper, lr, norms=(), coef=None, flags=0):
        self.calls.append(('optim_prepare', len(norms), coef is not None, int(flags)))
        s = R.unpack(state.numpy())
        R.prepare(s, hyper, self._scalar(lr) if torch.is_tensor(lr) else lr, [self._scalar(n) for n in norms], self._scalar(coef),
                  int(flags))
        state.copy_(torch.from_numpy(R.pack(s)))

    def optim_apply(self, param, grad, exp_avg, exp_avg_sq, ema, hyper, flags, state):
        self.calls.append(('optim_apply', param.numel(), ema is not None, int(flags)))
        if ema is not None and not 0.0 < hyper['ema_decay'] < 1.0:
            raise RuntimeError('twog_optim_apply failed with code -2')
        views = [None if t is None else t.detach().numpy() for t in (param, grad, exp_avg, exp_avg_sq, ema)]   # share the memory
        R.apply(*views, hyper, int(flags), R.unpack(state.numpy()), dtype=views[0].dtype.type)


def state_fields(state):
    """The fields of a state block (CPU or device tensor) with the floats as raw bits: what two backends must agree on."""
    s = R.unpack(state.detach().cpu().numpy())
    return {k: (np.asarray(v).tobytes().hex() if isinstance(v, np.floating) else int(v)) for k, v in s.items()}
