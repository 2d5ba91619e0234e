"""The class-weight test double (tests/class_weight_fake.py::ClassWeightFakeKernels: the plain, smoothing and weighted
criterion entry points) and the Viterbi one (tests/viterbi_fake.py) with the linear-chain CRF entry points of
2g-gcn_amd/kernels.py (crf_limits, crf_nll_fwd, crf_nll_bwd), stated through the specification in tests/crf_ref.py at fp32. For
the CPU tests of the host layer in 2g-gcn_amd/losses.py. `calls` records, besides the parents' entries, ('crf_nll_fwd', m) and
('crf_nll_bwd', terms with a d(input) buffer, accumulate flags, terms whose parameters are asked for)."""
import numpy as np
import torch

from tests import crf_ref as R
from tests.class_weight_fake import ClassWeightFakeKernels
from tests.viterbi_fake import ViterbiFakeKernels


class CrfFakeKernels(ClassWeightFakeKernels, ViterbiFakeKernels):
    def crf_limits(self):
        return R.MAX_CLASSES, R.MAX_STEPS

    def _check_crf_term(self, t):
        x, y, A, pi = t['input'], t['target'], t['transitions'], t['initial']
        assert x.is_contiguous() and y.is_contiguous() and x.dtype == torch.float32 and y.dtype == torch.int64
        assert x.dim() == 4 and y.shape == (x.shape[0], x.shape[2], x.shape[3])
        Cn = x.shape[1]
        if Cn > R.MAX_CLASSES or x.shape[2] > R.MAX_STEPS:   # the ctypes layer refuses before any launch
            raise ValueError(f'the CRF loss takes up to {R.MAX_CLASSES} classes and {R.MAX_STEPS} model steps')
        assert A.shape == (Cn, Cn) and pi.shape == (Cn,) and A.dtype == pi.dtype == torch.float32
        assert A.is_contiguous() and pi.is_contiguous() and not A.requires_grad and not pi.requires_grad

    @staticmethod
    def _spec(t, g=None):
        return R.crf_nll(t['input'].numpy(), t['target'].numpy(), t['transitions'].numpy(), t['initial'].numpy(),
                         int(t['ignore']), np.float32, g=g)

    def crf_nll_fwd(self, terms, losses_out, stats_out):
        for t in terms:
            self._check_crf_term(t)
        self.calls.append(('crf_nll_fwd', len(terms)))
        assert losses_out.shape == (len(terms),) and stats_out.shape == (len(terms), 2)
        for j, t in enumerate(terms):
            r = self._spec(t)
            t['alpha'], t['seq'] = 'written', 'written'   # the workspaces the backward reads
            losses_out[j] = float(np.float32(t['weight']) * r.loss)
            stats_out[j, 0], stats_out[j, 1] = float(r.nll.astype(np.float64).sum()), r.count

    def crf_nll_bwd(self, terms, stats, dlosses, dins, accumulate, need_params):
        self.calls.append(('crf_nll_bwd', tuple(d is not None for d in dins), tuple(bool(a) for a in accumulate),
                           tuple(bool(p) for p in need_params)))
        assert stats.shape == (len(terms), 2) and dlosses.shape == (len(terms),)
        ptrs = [d.data_ptr() for d in dins if d is not None]
        assert len(set(ptrs)) == len(ptrs)
        out = []
        for j, (t, d) in enumerate(zip(terms, dins)):
            if d is None and not need_params[j]:
                out.append(None)
                continue
            assert t.get('alpha') == 'written' and t.get('seq') == 'written'
            cnt = float(stats[j, 1])
            g = np.float32(t['weight']) * np.float32(float(dlosses[j])) / np.float32(cnt) if cnt > 0 else np.float32(0)
            r = self._spec(t, g=g)
            if d is not None:
                grad = torch.from_numpy(r.dinput)
                d.copy_(d + grad if accumulate[j] else grad)
            out.append((torch.from_numpy(r.dA), torch.from_numpy(r.dpi)) if need_params[j] else None)
        return out
