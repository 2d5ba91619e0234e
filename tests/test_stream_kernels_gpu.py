"""GPU: the small streaming kernels of every training step (csrc/gate.hip, misc.hip, posfeat.hip, ssp.hip) over the cases of
tests/stream_cases.py: gates, column sums, rank-1 update, ReLU backward, row add, grouped row operations, mul, row scaling, Adam,
reorder, filter, label heads, position features, sender-side projection glue, zero fill, packed-weight copies.

Every floating-point result is judged by tests.entity_envelope.judge against the specification run in fp64, with the fp32
specification's own error as the yardstick (e_hip <= 8 x e_ref + 4 x 2^-24, tensor-wide and per row; one tensor of one case has
a row factor of 32, stated with its reason and the measured 28.3 at HEAD_CASES of stream_cases.py); copies, selections, single
additions and the memory around a written view must be bit-equal to the fp32 specification. The first test proves from the
library's launch-free grid plan (HipKernels.stream_grid) that the cases written for a capped grid make their stride loops turn.
tests/test_stream_kernels_cpu.py checks the case list and the specification themselves.

TWOG_STREAM_RECORD=<file>: e_hip, e_ref and their ratio of every (case, tensor) are written there as JSON
(profiles/stream_kernels_fp64.json is such a record)."""
import json
import os

import pytest
import torch

import twog_gcn_amd  # noqa: F401
from twog_gcn_amd import kernels as twog_kernels
from tests import entity_envelope as EE
from tests import stream_cases as SC
from tests.stream_cases import F, EXACT, JUDGE

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
    dst = os.environ.get('TWOG_STREAM_RECORD')
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

    def all(self, hip, s32, s64, row_factors=None):
        """row_factors: {tensor: factor of the row-wise rule} where a case states one with its reason (stream_cases.py)."""
        for k, v in s32.items():
            if not isinstance(v, tuple):
                if hip[k] != v:
                    self.fails.append(f'{k}: {hip[k]} on the device, {v} in the specification')
            elif v[1] == EXACT:
                self.exact(k, hip[k][0], v[0])
            elif v[1] == JUDGE:
                self.add(k, hip[k][0], v[0], s64[k][0], (row_factors or {}).get(k))

    def check(self):
        print(f'{self.case}: worst e_hip / e_ref {self.worst[0]:.2f} ({self.worst[1]})')
        assert not self.fails, f'{self.case}:\n  ' + '\n  '.join(self.fails)


def three(K, run, *a):
    """-> (HIP result, fp32 specification, fp64 specification) of one case."""
    s32, s64 = run(F, *a, 'cpu', F32), run(F, *a, 'cpu', F64)
    hip = run(K, *a, DEV, F32)
    torch.cuda.synchronize()
    return hip, s32, s64


def close(a, b, rtol, atol, what):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    err = (a - b).abs().max().item() if a.numel() else 0.0
    tol = atol + rtol * b.abs().max().item() if b.numel() else atol
    assert err <= tol, f'{what}: max err {err:.3e} > tol {tol:.3e}'


# ------------------------------------------------------------------------------------------- the case list against the plan
def _plans():
    ps = [(c['id'], c['plan']) for c in SC.EW_CASES + SC.ADAM_CASES if c['plan']]
    return ps + [('rowops', SC.ROWOPS_PLAN), ('fill_zero', SC.FILL_BIG_PLAN), ('copy_blocks', SC.COPY_BIG_PLAN)]


def test_capped_cases_make_a_second_trip_by_the_library_s_own_grid(K):
    """No launch. grid x threads x items per thread < work - slack (the work sure to reach the strided loop: head bytes of the
    zero fill and incomplete groups of four left out) for every case written for a capped grid, with a ragged remainder; fails
    when a cap is raised so that such a case silently becomes a single-trip launch again."""
    seen = set()
    for name, plan in _plans():
        one_trip, work = SC.second_trip(K, plan)
        assert one_trip < work and work % one_trip != 0, f'{name}: one trip covers {one_trip} of {work} items'
        seen.add(getattr(K, plan[0]))
    assert seen == set(range(K.STREAM_REORDER)), 'a capped kernel has no case beyond its cap'
    for c in SC.REORDER_CASES:
        assert K.stream_grid(K.STREAM_REORDER, c['bs'] * c['E'], c['cols']) == c['chunks'], c['id']
    assert K.lib.twog_stream_grid(99, 1, 0) == -2


# ---------------------------------------------------------------------------------------------------------------- gates
@pytest.mark.parametrize('c', SC.GATE_CASES, ids=lambda c: c['id'])
def test_gate_forward_and_backward(K, c):
    s32 = SC.gate_run(F, c, 'cpu', F32)
    s64 = SC.gate_run(F, c, 'cpu', F64, saved=s32)
    hip = SC.gate_run(K, c, DEV, F32, saved=s32)
    torch.cuda.synchronize()
    V = Verdict('gate_' + c['id'])
    V.all(hip, s32, s64)
    ok = SC.hard_comparable(c, s64['soft'][0])
    assert int((~ok).sum()) <= 1
    hard = hip['hard'][0].cpu()
    if not torch.equal(hard[ok], s64['hard'][0][ok]):
        V.fails.append('hard: a decision outside the margin differs from the fp64 specification')
    if not set(hard.unique().tolist()) <= {0.0, 1.0}:
        V.fails.append('hard: values other than 0 and 1')
    if c['force_last'] and not bool((hard.view(c['bs'], c['T'], c['E'])[:, -1] == 1).all()):
        V.fails.append('hard: the last step is not forced to 1')
    V.check()


def test_gate_with_saturated_logits_against_the_fp32_specification(K):
    """|logit| > 20 on some rows: p rounds to 0 or 1 in fp32, where fp32 and fp64 legitimately part ways (log(p + 1e-20)): the
    fp32 specification alone, at the tolerances of the omnibus test."""
    c = SC.GATE_SATURATED
    s32 = SC.gate_run(F, c, 'cpu', F32)
    hip = SC.gate_run(K, c, DEV, F32, saved=s32)
    torch.cuda.synchronize()
    p = hip['p_save'][0]
    assert int(((p == 0) | (p == 1)).sum()) >= 4
    for k in ('soft', 'p_save', 'dlogit', 'dlogit_hard_only', 'dlogit_soft_only'):
        assert bool(torch.isfinite(hip[k][0]).all()), k
        close(hip[k][0], s32[k][0], rtol=1e-4, atol=1e-6, what=k)
    hard = hip['hard'][0].cpu()
    assert set(hard.unique().tolist()) <= {0.0, 1.0}
    safe = (s32['soft'][0] - c['thr']).abs() > SC.HARD_MARGIN
    assert torch.equal(hard[safe], s32['hard'][0][safe])


# ---------------------------------------------------------------------------------------------------------- column sums
@pytest.mark.parametrize('c', SC.COLSUM_CASES, ids=lambda c: c['id'])
def test_column_sums(K, c):
    assert SC.vec_ok(SC.colsum_problem(c, DEV, F32)[0]) == c['vec'], 'the case does not reach the form it was written for'
    V = Verdict('colsum_' + c['id'])
    V.all(*three(K, SC.colsum_run, c))
    V.check()


def test_grouped_column_sums_of_every_case_equal_the_single_calls_bit_for_bit(K):
    """More than 16 problems, 16-byte and scalar forms mixed in one pair of launches."""
    many = SC.colsum_many_run(K, DEV, F32)
    single = [SC.colsum_run(K, c, DEV, F32)['out'][0] for _ in range(2) for c in SC.COLSUM_CASES]
    torch.cuda.synchronize()
    assert len(many) == len(single) > 16
    for k, (a, b) in enumerate(zip(many, single)):
        assert torch.equal(a, b), SC.COLSUM_CASES[k % len(SC.COLSUM_CASES)]['id']


# --------------------------------------------------------------------------------------------- element-wise, capped grids
@pytest.mark.parametrize('c', SC.EW_CASES, ids=lambda c: c['id'])
def test_elementwise_kernels(K, c):
    V = Verdict('ew_' + c['id'])
    hip, s32, s64 = three(K, SC.ew_run, c)
    assert c['op'] == 'mul' or hip['vec'] == c['vec'], 'the case does not reach the form it was written for'
    V.all(hip, s32, s64)
    V.check()


def test_grouped_row_operations_of_very_different_sizes_in_two_launches(K):
    assert len(SC.ROWOPS_SHAPES) == 17
    V = Verdict('rowops')
    V.all(*three(K, SC.rowops_run))
    V.check()


@pytest.mark.parametrize('c', SC.ADAM_CASES, ids=lambda c: c['id'])
def test_adam_against_fp64_adam(K, c):
    """weight_decay != 0, grad_scale != 1, step numbers 1, 2, 1000, non-zero moments (the comparison with torch.optim.Adam stays
    in tests/test_kernels_gpu.py)."""
    V = Verdict('adam_' + c['id'])
    V.all(*three(K, SC.adam_run, c))
    V.check()


# -------------------------------------------------------------------------------------------- reorder / filter / heads
@pytest.mark.parametrize('c', SC.REORDER_CASES, ids=lambda c: c['id'])
def test_reorder_forward_and_backward(K, c):
    V = Verdict('reorder_' + c['id'])
    V.all(*three(K, SC.reorder_run, c))
    V.check()


@pytest.mark.parametrize('c', SC.FILTER_CASES, ids=lambda c: c['id'])
def test_filter_on_ties_and_values_on_the_threshold(K, c):
    V = Verdict('filter_' + c['id'])
    V.all(*three(K, SC.filter_run, c))
    V.check()


@pytest.mark.parametrize('c', SC.HEAD_CASES, ids=lambda c: c['id'])
def test_label_heads(K, c):
    """Log-softmax with the permuted store into a NaN-poisoned buffer (every position written, nothing behind the last), and its
    backward pass on the specification's saved output. dlogits of C64_scale80: row factor 32, see stream_cases.HEAD_CASES."""
    s32 = SC.head_run(F, c, 'cpu', F32)
    s64 = SC.head_run(F, c, 'cpu', F64, saved=s32)
    hip = SC.head_run(K, c, DEV, F32, saved=s32)
    torch.cuda.synchronize()
    V = Verdict('head_' + c['id'])
    if bool(torch.isnan(hip['out'][0]).any()):
        V.fails.append(f"out: {int(torch.isnan(hip['out'][0]).sum())} positions were not written")
    if not bool(torch.isnan(hip['guard'][0]).all()):
        V.fails.append('out: the call wrote behind its last element')
    V.all(hip, s32, s64, row_factors=dict(dlogits=c['dlogits_row_factor']))
    V.check()


# ---------------------------------------------------------------------------------------------------- position features
@pytest.mark.parametrize('c', SC.POS_CASES, ids=lambda c: c['id'])
def test_position_embeddings(K, c):
    V = Verdict('pos_' + c['id'])
    V.all(*three(K, SC.pos_run, c))
    V.check()


@pytest.mark.parametrize('c', SC.SEGLEN_CASES, ids=lambda c: c['id'])
def test_segment_lengths(K, c):
    V = Verdict('seglen_' + c['id'])
    V.all(*three(K, SC.seglen_run, c))
    V.check()


# ------------------------------------------------------------------------------------------- sender-side projection glue
@pytest.mark.parametrize('c', SC.SSP_CASES, ids=lambda c: c['id'])
def test_sender_side_projection_at_its_limits(K, c):
    hip, s32, s64 = three(K, SC.ssp_run, c)
    V = Verdict('ssp_' + c['id'])
    V.all(hip, s32, s64)
    if c['mask'] and c['ph'] and float(hip['dw'][0][:SC.SSP_IPC].abs().max()) != 0.0:
        V.fails.append('dw: not exactly 0 in the fully masked clip')
    V.check()


def test_sender_side_gather_with_both_leading_dimensions_larger_than_dense(K):
    V = Verdict('ssp_gather_strided')
    V.all(*three(K, SC.ssp_gather_run))
    V.check()


# ----------------------------------------------------------------------------------------------- zero fill / block copies
def test_fill_zero_clears_exactly_the_requested_bytes_at_every_alignment(K):
    """Offsets 0 .. 17 and lengths 0 .. 48 from a 16-byte boundary: head bytes, 16-byte body and tail bytes in every
    combination; one synchronisation, then every byte of the buffer is compared."""
    got = SC.fill_run(K, DEV)
    torch.cuda.synchronize()
    got, want = got.cpu(), SC.fill_expected()
    bad = got != want
    assert not bool(bad.any()), f'(offset, length) {SC.FILL_PAIRS[int(torch.nonzero(bad)[0][0])]}: byte {int(torch.nonzero(bad)[0][1]) - 16}'


def test_fill_zero_beyond_one_trip_of_the_capped_grid(K):
    off, n = SC.FILL_BIG
    head = -off % 16
    assert (n - head) // 16 > K.stream_grid(K.STREAM_FILL_ZERO, n) * K.STREAM_THREADS, 'the 16-byte body fits one trip'
    buf = torch.full((n + 64,), SC.FILL_BYTE, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    K.fill_zero(buf[off:off + n])
    torch.cuda.synchronize()
    assert int(buf[off:off + n].count_nonzero()) == 0
    assert bool((buf[:off] == SC.FILL_BYTE).all()) and bool((buf[off + n:] == SC.FILL_BYTE).all())


def test_copy_blocks_at_every_alignment_with_guards(K):
    """Sizes with and without a tail, source and destination 0 .. 3 floats off a 16-byte boundary, 99 pairs (seven launches of
    the wrapper, aligned and unaligned pairs side by side), three blocks beyond one trip of the capped grid; every float of the
    destination buffer, guards included, is compared."""
    got = SC.copy_run(K, DEV)
    torch.cuda.synchronize()
    got, want = got.cpu(), SC.copy_expected()
    bad = got != want
    assert not bool(bad.any()), f'{int(bad.sum())} floats differ, the first at {int(torch.nonzero(bad)[0])}'
