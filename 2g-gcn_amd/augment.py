"""Input augmentation on the device (kernels.augment_inputs / twog_augment_inputs in include/twog_gcn.h).

The reference trainer has none: its loaders hand the stored features over unchanged. SGN, the model Geo_gcn is taken from,
rotates its skeletons at random in its loader; here the same kind of regulariser runs on the device, because a resident
split never leaves HBM and the staged route is already bound by the host.

Two parts, both in place on the fetched batch:
  geometry  one random rotation (at most `max_rotation_deg`), scale (1 +- `max_scale`) and shift (+- `max_shift` per axis)
            per clip, about `centre`, of the (x, y, vx, vy) skeleton / box nodes at the end of every x_human row;
  features  uniform jitter of standard deviation `feature_noise_std` and inverted dropout of probability `feature_dropout`
            on the visual channels of humans and objects.
The distance tensors of a batch (human-human, human-object, object-object) are NOT transformed: they are normalised by the
image size per axis, so no similarity transform of the image plane maps onto them.

A clip's draw is a function of (seed, epoch, the clip's index in its data set) only -- not of the batch it sits in, the batch
size, the rank or the launch geometry. (seed, epoch) live in device memory: set_epoch / next_epoch are device-side writes.
"""
import math

import torch

from .kernels import _as_int64, _f32, get_kernels

_OPTIONS = ('max_rotation_deg', 'max_scale', 'max_shift', 'centre', 'feature_noise_std', 'feature_dropout', 'gcn_node')


class InputAugmentation:
    def __init__(self, seed, *, max_rotation_deg=0., max_scale=0., max_shift=0., centre=(0., 0.), feature_noise_std=0.,
                 feature_dropout=0., gcn_node, epoch=0):
        self.seed, self.epoch = int(seed) % 2 ** 64, int(epoch) % 2 ** 64
        self._state = None   # int64 [seed, epoch] on the device of the first batch
        self._set_options(max_rotation_deg=max_rotation_deg, max_scale=max_scale, max_shift=max_shift, centre=centre,
                          feature_noise_std=feature_noise_std, feature_dropout=feature_dropout, gcn_node=gcn_node)

    def _set_options(self, **o):
        o['centre'] = tuple(float(v) for v in o['centre'])
        o['gcn_node'] = int(o['gcn_node'])
        for k in ('max_rotation_deg', 'max_scale', 'max_shift', 'feature_noise_std', 'feature_dropout'):
            o[k] = float(o[k])
            if not math.isfinite(o[k]):
                raise ValueError(f'{k} = {o[k]}')
        if not 0. <= o['max_rotation_deg'] <= 90.:
            raise ValueError(f"max_rotation_deg {o['max_rotation_deg']} outside [0, 90]")
        if not 0. <= o['max_scale'] < 1.:
            raise ValueError(f"max_scale {o['max_scale']} outside [0, 1)")
        if not 0. <= o['feature_dropout'] < 1.:
            raise ValueError(f"feature_dropout {o['feature_dropout']} outside [0, 1)")
        if o['feature_noise_std'] < 0. or o['max_shift'] < 0.:
            raise ValueError('feature_noise_std and max_shift must not be negative')
        if len(o['centre']) != 2 or o['gcn_node'] < 0:
            raise ValueError(f"centre {o['centre']}, gcn_node {o['gcn_node']}")
        self.options = {k: o[k] for k in _OPTIONS}
        p = o['feature_dropout']
        # everything the kernels take, made once in fp64 and rounded to the fp32 the C ABI passes
        self.kernel_options = dict(
            tan_half_max=_f32(math.tan(math.radians(o['max_rotation_deg']) / 2.)), scale_max=_f32(o['max_scale']),
            shift_max=_f32(o['max_shift']), cx=_f32(o['centre'][0]), cy=_f32(o['centre'][1]),
            amp=_f32(o['feature_noise_std'] * math.sqrt(3.)), keep_scale=_f32(1. / (1. - p)),
            drop_threshold=min(int(round(p * 2 ** 24)), 2 ** 24 - 1), gcn_node=o['gcn_node'])

    # ------------------------------------------------------------------ state
    def state(self, device):
        """The device words [seed, epoch] on `device`: made on first use (one small host-to-device copy) and again only when
        the batches move to another device. 'cuda' without an index means the current device."""
        device = torch.device(device)
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        if self._state is None or self._state.device != device:
            self._state = self._words().to(device)
        return self._state

    def _words(self):
        return torch.tensor([_as_int64(self.seed), _as_int64(self.epoch)], dtype=torch.int64)

    def set_epoch(self, n):
        self.epoch = int(n) % 2 ** 64
        if self._state is not None:
            self._state[1].fill_(_as_int64(self.epoch))   # a device-side write in stream order: nothing waits
        return self

    def next_epoch(self):
        self.epoch = (self.epoch + 1) % 2 ** 64
        if self._state is not None:
            self._state[1].add_(1)                        # (int64 wraps like the unsigned value it stands for)
        return self

    def state_dict(self):
        return dict(seed=self.seed, epoch=self.epoch, **self.options)

    def load_state_dict(self, sd):
        self._set_options(**{k: sd[k] for k in _OPTIONS})
        self.seed, self.epoch = int(sd['seed']) % 2 ** 64, int(sd['epoch']) % 2 ** 64
        if self._state is not None:
            self._state.copy_(self._words())   # into the existing words: a captured launch goes on reading this tensor
        return self

    # ------------------------------------------------------------------ the call
    def __call__(self, data, clip_ids, params_out=None):
        """data: the fetched list of data_loading.gcn_fetcher (x_human, x_objects, objects_mask, ..., steps_per_example at 7);
        clip_ids: int64 tensor on the batch's device, the clips' indices in their data set. Augments data[0] and data[1] in
        place and returns data. Tensors that are not contiguous raise (the write is in place, so no silent copy)."""
        x_human, x_objects, mask, steps = data[0], data[1], data[2], data[7]
        if x_objects is not None and x_objects.numel() == 0:
            x_objects = None
        get_kernels().augment_inputs(x_human, x_objects, clip_ids, self.state(x_human.device), self.kernel_options, steps=steps,
                                     objects_mask=mask if x_objects is not None else None, params_out=params_out)
        return data
