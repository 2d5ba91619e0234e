"""The segment-metrics test double (tests/segment_metrics_fake.py) with the edit-score entry points, stated through the
specification in tests/segment_edit_ref.py. For the CPU tests of the host layer in 2g-gcn_amd/postprocess.py. `calls`
records the name of every kernel-interface method the host layer used, in order; `edit_args` the (ignore_value, bg_label,
entity_minor) of every segment_edit."""
import numpy as np
import torch

from tests import segment_edit_ref as D
from tests.segment_metrics_fake import SegmentMetricsFakeKernels
from twog_gcn_amd.kernels import segment_edit_words, unpack_segment_edit


class SegmentEditFakeKernels(SegmentMetricsFakeKernels):
    EDIT_MAX_STEPS = D.MAX_STEPS

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.edit_args = []

    def segment_edit_limits(self):
        return self.EDIT_MAX_STEPS

    def segment_edit(self, y_true, y_pred, ignore_value=None, bg_label=None, entity_minor=False):
        self.calls.append('segment_edit')
        self.edit_args.append((ignore_value, bg_label, entity_minor))
        assert y_true.dtype == torch.int64 and y_pred.dtype == torch.int64 and y_true.shape == y_pred.shape
        assert y_true.dim() == (3 if entity_minor else 2), tuple(y_true.shape)
        if y_true.shape[1] > self.EDIT_MAX_STEPS:
            raise RuntimeError('twog_segment_edit failed with code -2')
        got = D.segment_edit(y_true.numpy(), y_pred.numpy(), None if ignore_value is None else int(ignore_value),
                             None if bg_label is None else int(bg_label), entity_minor)
        n_seq = got[0].shape[0]
        packed = torch.zeros(segment_edit_words(n_seq), dtype=torch.int64)
        views = unpack_segment_edit(packed, n_seq)
        for view, value in zip(views, got):
            view.copy_(torch.from_numpy(np.ascontiguousarray(value)))
        return (*views, packed)
