"""GPU: the general single-relation kernels (csrc/relation.hip) over the cases of tests/relation_cases.py: the entity limit
R = S = 16 for every score mode x message mode, rectangular and degenerate relations, widths around and far beyond the 64-lane
stride, one and eight instances, every row operand as a column block and as a 3-D view, every feature-gradient branch.

Every floating-point output (out, att, dmsg, dp_r, dp_s, dq, dk, da_r, dc_s and dscore_sum per instance) is judged by
tests.entity_envelope.judge against the specification run in fp64, with the fp32 specification's own error as the yardstick
(e_hip <= 8 x e_ref + 4 x 2^-24, tensor-wide and per row, zero rows exactly zero). The backing buffer of every written operand
is pre-filled with seeded values and compared outside the written view bit for bit; dq / dk of the modes without scores are
exact (zeros, or untouched when they accumulate). The weights obey the structure rules of relation_cases.att_structure_failures.
Multi-descriptor calls are bit-equal to single-descriptor calls, a repeated call is bit-equal to itself, and descriptors beyond
the limits are refused before any launch. tests/test_relation_kernels_cpu.py checks the case list and the specification.

TWOG_RELATION_RECORD=<file>: e_hip, e_ref and their ratio of every (case, tensor) are written there as JSON
(profiles/relation_kernels_fp64.json is such a record)."""
import json
import os

import pytest
import torch

import twog_gcn_amd  # noqa: F401
from twog_gcn_amd import kernels as twog_kernels
from tests import entity_envelope as EE
from tests import relation_cases as RC
from tests.relation_cases import F, EXACT, JUDGE

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32, F64 = torch.float32, torch.float64
RECORDS = {}


@pytest.fixture(scope='module')
def K():
    twog_kernels._set_backend_for_tests(None)
    k = twog_kernels.get_kernels()
    assert k.name == 'hip'
    yield k
    dst = os.environ.get('TWOG_RELATION_RECORD')
    if dst and RECORDS:
        fin = lambda v: (float(f'{v:.4g}') if v == v and abs(v) != float('inf') else str(v)) if isinstance(v, float) else v
        with open(dst, 'w') as f:
            json.dump({k_: {a: fin(b) for a, b in r.items()} for k_, r in sorted(RECORDS.items())}, f, indent=0)


class Verdict:
    """Collects the judgement of every tensor of one case: all of them are measured (and recorded) before the case fails."""

    def __init__(self, case):
        self.case, self.fails, self.worst = case, [], (0.0, '')

    def add(self, name, hip, s32, s64, row_factor=None):
        rec, fails = EE.judge(hip, s32, s64, EE.FACTOR, row_factor)
        RECORDS[f'{self.case}/{name}'] = dict(rec, factor=EE.FACTOR, row_factor=row_factor or EE.FACTOR)
        self.fails += [f'{name}: {f}' for f in fails]
        self.worst = max(self.worst, (max(rec['ratio'], rec['row_ratio']), name))

    def exact(self, name, hip, s32):
        hip = hip.detach().cpu()
        if hip.shape != s32.shape or hip.dtype != s32.dtype:
            self.fails.append(f'{name}: shape / dtype {tuple(hip.shape)} {hip.dtype}, specification {tuple(s32.shape)} {s32.dtype}')
        elif not torch.equal(hip, s32):
            bad = hip != s32
            self.fails.append(f'{name}: not bit-equal to the fp32 specification in {int(bad.sum())} of {bad.numel()} places, the first at '
                              f'{torch.nonzero(bad)[0].tolist()}')

    def all(self, hip, s32, s64, row_factors):
        assert set(hip) == set(s32) == set(s64)
        for k, (v, how) in s32.items():
            if how == EXACT:
                self.exact(k, hip[k][0], v)
            else:
                self.add(k, hip[k][0], v, s64[k][0], row_factors.get(k))

    def check(self):
        print(f'{self.case}: worst e_hip / e_ref {self.worst[0]:.2f} ({self.worst[1]})')
        assert not self.fails, f'{self.case}:\n  ' + '\n  '.join(self.fails)


# ------------------------------------------------------------------------------------------------ every case against fp64
@pytest.mark.parametrize('c', RC.CASES, ids=lambda c: c['id'])
def test_relation_forward_and_backward(K, c):
    s32, s64 = RC.run(F, c, 'cpu', F32), RC.run(F, c, 'cpu', F64)
    hip = RC.run(K, c, DEV, F32)
    torch.cuda.synchronize()
    V = Verdict(c['id'])
    V.all(hip, s32, s64, c['row_factors'])
    V.fails += [f'att: {f}' for f in RC.att_structure_failures(hip['att'][0], c)]
    if c['R'] == c['S'] == 1 and c['excl']:   # no valid sender anywhere: exactly zero, nothing NaN
        for k in ('out', 'att', 'dmsg', 'dp_r', 'dp_s'):
            if k in hip and not bool((hip[k][0] == 0).all()):
                V.fails.append(f'{k}: not exactly zero without any valid sender')
    if c['zero_dist_recv'] and float(hip['att'][0][:, c['R'] // 2].abs().max()) != 0.0:
        V.fails.append('att: the receiver whose distances are all 0 has a non-zero weight')
    V.check()


# ----------------------------------------------------------------------------------- several descriptors per launch
def _build_all(entries):
    return [RC.build(RC.case(i, **o), DEV, F32) for i, o in entries]


def _same_words(entries, many, single):
    for (id, o), (_, _, wm), (_, _, ws) in zip(entries, many, single):
        if o.get('desc_R') == 0:   # no receivers: every buffer still holds what it was filled with
            ws = RC.build(RC.case(id, **o), 'cpu', F32)[2]
        for k in wm:
            assert torch.equal(wm[k][0].cpu(), ws[k][0].cpu()), f'{id} {o}: {k} differs from the single-descriptor call'


@pytest.mark.parametrize('n', [len(RC.MANY_FWD), RC.MANY_FWD_SHORT])
def test_forward_of_many_descriptors_equals_the_single_calls_bit_for_bit(K, n):
    """Two launches (8 + 3 descriptors, and 8 + 1): n_inst between 1 and 8 within a launch, the largest never first, one R = 0
    descriptor in the middle. The same device function runs in the same order in both forms, so every word is equal."""
    entries = RC.MANY_FWD[:n]
    many, single = _build_all(entries), _build_all(entries)
    K.relation_fwd_many([d for d, _, _ in many])
    for d, _, _ in single:
        K.relation_fwd(d)
    torch.cuda.synchronize()
    _same_words(entries, many, single)


@pytest.mark.parametrize('n', [len(RC.MANY_BWD), RC.MANY_BWD_SHORT])
def test_backward_of_many_descriptors_equals_the_single_calls_bit_for_bit(K, n):
    """Two launches (6 + 2 descriptors, and 6 + 1). No two descriptors share a buffer (the contract of twog_relation_bwd_n)."""
    entries = RC.MANY_BWD[:n]
    many, single = _build_all(entries), _build_all(entries)
    K.relation_bwd_many([b for _, b, _ in many])
    for _, b, _ in single:
        K.relation_bwd(b)
    torch.cuda.synchronize()
    _same_words(entries, many, single)


def test_the_largest_backward_case_gives_the_same_words_twice(K):
    c = max((c for c in RC.CASES if c['score'] == RC.DOT), key=lambda c: c['n_inst'] * c['R'] * c['S'] * (c['hidden'] + c['D']))
    assert c['R'] == c['S'] == RC.MAXE
    runs = [RC.run(K, c, DEV, F32) for _ in range(2)]
    torch.cuda.synchronize()
    for k in runs[0]:
        assert torch.equal(runs[0][k][0], runs[1][k][0]), k


# ------------------------------------------------------------------------------------------------------------ rejection
def _bad_descriptors():
    """(what, case id, backward only, change of (d, b)): each fails a host-side check (-2) before any launch."""
    def three_d(d, b):
        backing = torch.zeros(d['n_inst'], d['R'] + 1, d['hidden'] + 3, device=DEV)
        d['out'] = backing[:, :, :d['hidden']]   # inner = R + 1
    return [('R = 17', 'lim_dot_sender', False, lambda d, b: d.update(R=17)),
            ('S = 17', 'lim_dot_sender', False, lambda d, b: d.update(S=17)),
            ('hidden = 0', 'lim_add_pair', False, lambda d, b: d.update(hidden=0)),
            ('a 3-D row set with inner != R', 'w_dot_sender_D63_h63', False, three_d),
            ('DOT without k', 'lim_dot_pair', False, lambda d, b: d.update(k=None)),
            ('PAIR backward without dp_s', 'lim_dot_pair', True, lambda d, b: b.update(dp_s=None))]


def test_descriptors_beyond_the_limits_are_refused_before_any_launch(K):
    """Host-side checks only: nothing is launched, every pre-filled output stays as it was, also the outputs of a valid
    descriptor that shares a multi-descriptor call with the refused one; the device stays usable."""
    for what, id, bwd_only, change in _bad_descriptors():
        c = RC.case(id)
        d, b, w = RC.build(c, DEV, F32)
        good = RC.build(RC.case('inst_n1'), DEV, F32)
        change(d, b)
        calls = [lambda: K.relation_bwd(b), lambda: K.relation_bwd_many([good[1], b])]
        if not bwd_only:
            calls += [lambda: K.relation_fwd(d), lambda: K.relation_fwd_many([good[0], d])]
        for call in calls:
            with pytest.raises(RuntimeError, match='failed with code -2'):
                call()
        torch.cuda.synchronize()
        for built, cc in ((w, c), (good[2], RC.case('inst_n1'))):
            fresh = RC.build(cc, 'cpu', F32)[2]
            for k in fresh:
                assert torch.equal(built[k][0].cpu(), fresh[k][0]), f'{what}: {k} was written'
    x = torch.ones(4, device=DEV)
    assert float((x + 1).sum()) == 8.0
