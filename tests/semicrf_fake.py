"""The CRF test double (tests/crf_fake.py: the criterion entry points, the Viterbi decode and the linear-chain CRF loss) and
the segmental-decode one (tests/segdecode_fake.py) with the semi-Markov CRF entry points of 2g-gcn_amd/kernels.py
(semicrf_limits, semicrf_plan, semicrf_nll_fwd, semicrf_nll_bwd), stated through the specification in tests/semicrf_ref.py at
fp32. For the CPU tests of the host layer in 2g-gcn_amd/losses.py. `calls` records, besides the parents' entries,
('semicrf_nll_fwd', m) and ('semicrf_nll_bwd', terms with a d(input) buffer, accumulate flags, terms whose parameters are
asked for)."""
import numpy as np
import torch

from tests import semicrf_ref as R
from tests.crf_fake import CrfFakeKernels
from tests.segdecode_fake import SegdecodeFakeKernels


class SemiCrfFakeKernels(CrfFakeKernels, SegdecodeFakeKernels):
    def semicrf_limits(self):
        return R.MAX_CLASSES, R.MAX_STEPS, R.MAX_DURATION

    def semicrf_plan(self, bs, num_classes, T, E, D):
        self._refuse('semicrf_plan', num_classes, T, D)
        n = bs * E
        return {'class_template': 64, 'fwd_waves': 1, 'fwd_groups': E, 'bwd_waves': 1, 'bwd_groups': E,
                'ed_bytes': 8 * n * T * num_classes, 'marks_bytes': 4 * n * T, 'seq_bytes': 16 * n,
                'partial_bytes': 4 * n * num_classes * (num_classes + 1 + min(D, T))}

    def _check_semicrf_term(self, t):
        x, y, A, pi, dur = t['input'], t['target'], t['transitions'], t['initial'], t['durations']
        assert x.is_contiguous() and y.is_contiguous() and x.dtype == torch.float32 and y.dtype == torch.int64
        assert x.dim() == 4 and y.shape == (x.shape[0], x.shape[2], x.shape[3])
        Cn = x.shape[1]
        assert dur.dim() == 2 and dur.shape[0] == Cn
        self._refuse('the semi-Markov CRF loss', Cn, x.shape[2], dur.shape[1])   # the ctypes layer refuses before any launch
        assert A.shape == (Cn, Cn) and pi.shape == (Cn,) and A.dtype == pi.dtype == dur.dtype == torch.float32
        for p in (A, pi, dur):
            assert p.is_contiguous() and not p.requires_grad

    @staticmethod
    def _semicrf_spec(t, g=None):
        return R.semicrf_nll(t['input'].numpy(), t['target'].numpy(), t['transitions'].numpy(), t['initial'].numpy(),
                             t['durations'].numpy(), int(t['ignore']), np.float32, g=g)

    def semicrf_nll_fwd(self, terms, losses_out, stats_out):
        for t in terms:
            self._check_semicrf_term(t)
        self.calls.append(('semicrf_nll_fwd', len(terms)))
        assert losses_out.shape == (len(terms),) and stats_out.shape == (len(terms), 2)
        for j, t in enumerate(terms):
            r = self._semicrf_spec(t)
            t['ed'], t['marks'], t['seq'] = 'written', 'written', 'written'   # the workspaces the backward reads
            losses_out[j] = float(np.float32(t['weight']) * r.loss)
            stats_out[j, 0], stats_out[j, 1] = float(r.nll.astype(np.float64).sum()), r.count

    def semicrf_nll_bwd(self, terms, stats, dlosses, dins, accumulate, need_params):
        self.calls.append(('semicrf_nll_bwd', tuple(d is not None for d in dins), tuple(bool(a) for a in accumulate),
                           tuple(bool(p) for p in need_params)))
        assert stats.shape == (len(terms), 2) and dlosses.shape == (len(terms),)
        ptrs = [d.data_ptr() for d in dins if d is not None]
        assert len(set(ptrs)) == len(ptrs)
        out = []
        for j, (t, d) in enumerate(zip(terms, dins)):
            if d is None and not need_params[j]:
                out.append(None)
                continue
            assert t.get('ed') == 'written' and t.get('marks') == 'written' and t.get('seq') == 'written'
            cnt = float(stats[j, 1])
            g = np.float32(t['weight']) * np.float32(float(dlosses[j])) / np.float32(cnt) if cnt > 0 else np.float32(0)
            r = self._semicrf_spec(t, g=g)
            if d is not None:
                grad = torch.from_numpy(r.dinput)
                d.copy_(d + grad if accumulate[j] else grad)
            out.append((torch.from_numpy(r.dA), torch.from_numpy(r.dpi), torch.from_numpy(r.ddur)) if need_params[j] else None)
        return out
