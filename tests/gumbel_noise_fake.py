"""The kernel-interface test double (tests/fake_kernels.py) with the device-noise entry points, `gumbel_noise_fill` and
`new_noise_state`, stated through the specification in tests/gumbel_noise_ref.py. For the CPU tests of the host layer in
2g-gcn_amd/models.py and distributed.py. `noise_calls` records (T, noise_entities, bs, clip_offset) of every fill."""
import torch

from tests import gumbel_noise_ref as R
from tests.fake_kernels import FakeKernels


class GumbelNoiseFakeKernels(FakeKernels):
    def __init__(self):
        super().__init__()
        self.noise_calls = []

    def new_noise_state(self, seed, calls=0, device=None):
        to_signed = lambda v: (int(v) % 2 ** 64) - (2 ** 64 if int(v) % 2 ** 64 >= 2 ** 63 else 0)
        return torch.tensor([to_signed(seed), to_signed(calls)], dtype=torch.int64, device=device)

    def gumbel_noise_fill(self, noise, T, noise_entities, bs, clip_offset, state, words=None):
        assert self._tape is None, 'the fill is not a recordable call'
        assert state.dtype == torch.int64 and state.numel() == 2
        assert noise.dtype == torch.float32 and noise.numel() == T * noise_entities * bs * 2
        self.noise_calls.append((T, noise_entities, bs, clip_offset))
        seed, calls = state.tolist()
        w = R.noise_words(seed, calls, T, noise_entities, bs, clip_offset)
        noise.view(-1).copy_(torch.from_numpy(R.gumbel_of_words(w[..., :2])).reshape(-1))   # fp64 rounded to fp32
        if words is not None:
            words.view(-1).copy_(torch.from_numpy(w.view('int32')).reshape(-1))
        state[1] += 1   # (int64 wraps like the device's unsigned add)
        return noise
