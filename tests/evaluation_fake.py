"""The kernel-interface test double (tests/fake_kernels.py) with the two evaluation entry points, stated through the
specification in tests/evaluation_ref.py. For the CPU tests of the host layer in 2g-gcn_amd/postprocess.py."""
import torch

from tests import evaluation_ref as E
from tests.fake_kernels import FakeKernels


class EvaluationFakeKernels(FakeKernels):
    MAX_CLASSES = 64

    def eval_limits(self):
        return self.MAX_CLASSES, 1 << 18

    def eval_update(self, logp, downsampling, target, step_index, counts, flags, want_labels=False):
        if logp.shape[1] > self.MAX_CLASSES:
            raise RuntimeError('twog_eval_update failed with code -2')
        c, f, labels, targets = E.eval_update(logp.numpy(), int(downsampling), target.numpy(),
                                              None if step_index is None else step_index.numpy())
        counts += torch.from_numpy(c).view_as(counts)
        flags += torch.from_numpy(f)
        return (torch.from_numpy(labels), torch.from_numpy(targets)) if want_labels else None

    def confusion_counts(self, y_true, y_pred, num_classes, counts, flags):
        if num_classes > self.MAX_CLASSES:
            raise RuntimeError('twog_confusion_counts failed with code -2')
        c, f = E.confusion_counts(y_true.to(torch.int64).numpy(), y_pred.to(torch.int64).numpy(), int(num_classes))
        counts += torch.from_numpy(c).view_as(counts)
        flags += torch.from_numpy(f)
        return counts
