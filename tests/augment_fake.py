"""The kernel-interface test double (tests/fake_kernels.py) with the augmentation entry points, `augment_inputs` and
`augment_grid`, stated through the specification in tests/augment_ref.py. For the CPU tests of the host layer in
2g-gcn_amd/augment.py and data_loading.DevicePrefetcher. `augment_calls` records (bs, launches) of every call, where
launches names the parts the library would launch for the options ('geometry', 'features'): a neutral call records nothing."""
import torch

from tests import augment_ref as R
from tests.fake_kernels import FakeKernels


class AugmentFakeKernels(FakeKernels):
    def __init__(self):
        super().__init__()
        self.augment_calls = []

    def augment_grid(self, work):
        assert work >= 0, work
        return min(max(int(work), 1), 2048)   # twog_augment_grid: one workgroup per item up to the cap

    def augment_inputs(self, x_human, x_objects, clip_ids, state, opts, steps=None, objects_mask=None, params_out=None):
        assert self._tape is None, 'the augmentation is not a recordable call'
        assert state.dtype == torch.int64 and state.numel() == 2 and clip_ids.dtype == torch.int64
        for t in (x_human, x_objects, steps, objects_mask, params_out):
            if t is not None:
                assert t.dtype == torch.float32
                if not t.is_contiguous():
                    raise ValueError('augment_inputs writes in place and does not copy: a tensor is not contiguous')
        launches = tuple(n for n, on in (('geometry', R.geometry_on(opts)), ('features', R.features_on(opts))) if on)
        if launches:
            self.augment_calls.append((x_human.shape[0], launches))
        seed, epoch = state.tolist()
        np_of = lambda t: None if t is None else t.numpy()   # (shares the tensor's memory: the specification writes in place)
        params = R.augment(np_of(x_human), np_of(x_objects), clip_ids.numpy(), seed, epoch, opts, np_of(steps),
                           np_of(objects_mask))
        if params_out is not None:
            params_out.view(-1, 4).copy_(torch.from_numpy(params))
        return x_human, x_objects
