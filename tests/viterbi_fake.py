"""The segment-edit test double (tests/segment_edit_fake.py) with the Viterbi entry points, stated through the
specification in tests/viterbi_ref.py. For the CPU tests of the host layer in 2g-gcn_amd/postprocess.py. `calls` records
the name of every kernel-interface method the host layer used, in order; `viterbi_args` the (lengths, downsampling,
target_steps) of every viterbi_decode."""
import numpy as np
import torch

from tests import viterbi_ref as V
from tests.segment_edit_fake import SegmentEditFakeKernels


class ViterbiFakeKernels(SegmentEditFakeKernels):
    VITERBI_MAX_CLASSES = V.MAX_CLASSES
    VITERBI_MAX_STEPS = V.MAX_STEPS

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.viterbi_args = []

    def viterbi_limits(self):
        return self.VITERBI_MAX_CLASSES, self.VITERBI_MAX_STEPS

    def viterbi_route(self, bs, num_classes, T, E):
        if num_classes > self.VITERBI_MAX_CLASSES or T > self.VITERBI_MAX_STEPS:
            raise ValueError('beyond the limits')
        return 'lds', 0

    def viterbi_decode(self, logp, transitions, initial=None, lengths=None, downsampling=1, target_steps=None):
        bs, Cn, T, E = logp.shape
        if Cn > self.VITERBI_MAX_CLASSES or T > self.VITERBI_MAX_STEPS:   # the ctypes layer refuses before any launch
            raise ValueError(f'viterbi_decode takes up to {self.VITERBI_MAX_CLASSES} classes and {self.VITERBI_MAX_STEPS} '
                             f'model steps, not {Cn} and {T}')
        self.calls.append('viterbi_decode')
        assert logp.dtype == torch.float32 and transitions.dtype == torch.float32 and transitions.shape == (Cn, Cn)
        assert initial is None or (initial.dtype == torch.float32 and initial.shape == (Cn,))
        assert lengths is None or (lengths.dtype == torch.int64 and lengths.shape == (bs,))
        self.viterbi_args.append((None if lengths is None else lengths.tolist(), int(downsampling), target_steps))
        labels, score = V.viterbi_labels(logp.numpy(), transitions.numpy(), None if initial is None else initial.numpy(),
                                         None if lengths is None else lengths.numpy(), int(downsampling), target_steps,
                                         fast=True)
        return torch.from_numpy(labels), torch.from_numpy(score)

    def transition_counts(self, targets, num_classes, stride, ignore_index, counts):
        self.calls.append('transition_counts')
        assert targets.dtype == torch.int64 and targets.dim() == 3 and counts.dtype == torch.int64
        if num_classes > self.VITERBI_MAX_CLASSES:
            raise RuntimeError('twog_transition_counts failed with code -2')
        counts += torch.from_numpy(V.transition_counts(targets.numpy(), int(num_classes), int(stride), int(ignore_index)))
        return counts

    def confusion_counts(self, *args, **kwargs):
        self.calls.append('confusion_counts')
        return super().confusion_counts(*args, **kwargs)
