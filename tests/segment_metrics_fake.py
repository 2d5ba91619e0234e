"""The evaluation test double (tests/evaluation_fake.py) with the segment-F1 entry points, stated through the specification
in tests/segment_metrics_ref.py. For the CPU tests of the host layer in 2g-gcn_amd/postprocess.py. `calls` records the
name of every kernel-interface method the host layer used, in order."""
import numpy as np
import torch

from tests import segment_metrics_ref as S
from tests.evaluation_fake import EvaluationFakeKernels
from twog_gcn_amd.kernels import segment_f1_words, unpack_segment_f1


class SegmentMetricsFakeKernels(EvaluationFakeKernels):
    MAX_STEPS = S.MAX_STEPS
    MAX_OVERLAPS = S.MAX_OVERLAPS

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.calls = []

    def segment_f1_limits(self):
        return self.MAX_STEPS, self.MAX_OVERLAPS

    def segment_f1(self, y_true, y_pred, num_classes, overlaps, ignore_value=None, entity_minor=False):
        self.calls.append('segment_f1')
        assert y_true.dtype == torch.int64 and y_pred.dtype == torch.int64
        overlaps = [float(o) for o in overlaps]
        if not 1 <= len(overlaps) <= self.MAX_OVERLAPS or not all(o > 0 for o in overlaps):
            raise RuntimeError('twog_segment_f1 failed with code -1')
        if y_true.shape[1] > self.MAX_STEPS:
            raise RuntimeError('twog_segment_f1 failed with code -2')
        got = S.segment_f1(y_true.numpy(), y_pred.numpy(), num_classes, overlaps, ignore_value, entity_minor)
        n_seq, K = got[0].shape
        packed = torch.zeros(segment_f1_words(n_seq, K), dtype=torch.int64)
        views = unpack_segment_f1(packed, n_seq, K)
        for view, value in zip(views, got):
            view.copy_(torch.from_numpy(np.ascontiguousarray(value)))
        return (*views, packed)

    def segment_f1_accumulate(self, f1, valid, f1_sums, valid_sums):
        self.calls.append('segment_f1_accumulate')
        f1_sums += f1.sum(0, dtype=torch.float64)
        valid_sums += valid.sum().to(torch.float64)

    def eval_update(self, *args, **kwargs):
        self.calls.append('eval_update')
        return super().eval_update(*args, **kwargs)

    def f1_at_k(self, *args, **kwargs):
        self.calls.append('f1_at_k')
        return super().f1_at_k(*args, **kwargs)
