"""The Viterbi test double (tests/viterbi_fake.py) with the segmental-decode entry points, stated through the
specification in tests/segdecode_ref.py. For the CPU tests of the host layer in 2g-gcn_amd/postprocess.py. `calls` records
the name of every kernel-interface method the host layer used, in order; `segdecode_args` the (lengths, downsampling,
target_steps, D) of every segment_decode."""
import torch

from tests import segdecode_ref as S
from tests.viterbi_fake import ViterbiFakeKernels


class SegdecodeFakeKernels(ViterbiFakeKernels):
    SEGDEC_MAX_DURATION = S.MAX_DURATION

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.segdecode_args = []

    def segdecode_limits(self):
        return self.VITERBI_MAX_CLASSES, self.VITERBI_MAX_STEPS, self.SEGDEC_MAX_DURATION

    def _refuse(self, what, Cn, T, D):
        if Cn > self.VITERBI_MAX_CLASSES or T > self.VITERBI_MAX_STEPS or D > self.SEGDEC_MAX_DURATION:
            raise ValueError(f'{what} takes up to {self.VITERBI_MAX_CLASSES} classes, {self.VITERBI_MAX_STEPS} model steps and '
                             f'durations up to {self.SEGDEC_MAX_DURATION}, not {Cn}, {T} and {D}')

    def segdecode_plan(self, bs, num_classes, T, E, D):
        self._refuse('segdecode_plan', num_classes, T, D)
        return {'class_template': 64, 'waves': 1, 'groups': E, 'route': 'lds', 'workspace_bytes': 0}

    def segment_decode(self, logp, transitions, durations, initial=None, lengths=None, downsampling=1, target_steps=None):
        bs, Cn, T, E = logp.shape
        assert durations.dim() == 2 and durations.shape[0] == Cn and durations.dtype == torch.float32
        self._refuse('segment_decode', Cn, T, durations.shape[1])     # the ctypes layer refuses before any launch
        self.calls.append('segment_decode')
        assert logp.dtype == torch.float32 and transitions.dtype == torch.float32 and transitions.shape == (Cn, Cn)
        assert initial is None or (initial.dtype == torch.float32 and initial.shape == (Cn,))
        assert lengths is None or (lengths.dtype == torch.int64 and lengths.shape == (bs,))
        self.segdecode_args.append((None if lengths is None else lengths.tolist(), int(downsampling), target_steps,
                                    durations.shape[1]))
        labels, score = S.segment_labels(logp.numpy(), transitions.numpy(), durations.numpy(),
                                         None if initial is None else initial.numpy(),
                                         None if lengths is None else lengths.numpy(), int(downsampling), target_steps, fast=True)
        return torch.from_numpy(labels), torch.from_numpy(score)

    def duration_counts(self, targets, num_classes, max_duration, stride, ignore_index, counts):
        self.calls.append('duration_counts')
        assert targets.dtype == torch.int64 and targets.dim() == 3 and counts.dtype == torch.int64
        assert counts.shape == (num_classes, max_duration)
        if num_classes > self.VITERBI_MAX_CLASSES or max_duration > self.SEGDEC_MAX_DURATION:
            raise RuntimeError('twog_duration_counts failed with code -2')
        counts += torch.from_numpy(S.duration_counts(targets.numpy(), int(num_classes), int(max_duration), int(stride),
                                                     int(ignore_index)))
        return counts
