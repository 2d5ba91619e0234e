"""CPU companion of tests/test_stream_kernels_gpu.py: the case lists of tests/stream_cases.py and the specification themselves.

  builds   every case runs through the specification in fp32 and in fp64; what the GPU test demands bit for bit of the kernels is
           the same value in both runs, what it judges agrees to within the fp32 rounding of the operation;
  gates    at most one hard decision per case lies within the margin of the threshold, and outside it the fp32 and the fp64
           specification decide alike (a condition on the chosen seeds, proven here);
  filter   the inputs do contain ties with a neighbour and soft == threshold;
  reach    the list reaches every branch it names: 16-byte and scalar forms (from the launchers' host-side conditions on the
           very tensors a run builds), column chunks and second trips (from the library's launch-free plan twog_stream_grid, which
           the specification passes on -- host arithmetic, no device is opened);
  guards   the doubles of fill_zero / copy_blocks pass the byte-exact checks the kernels get."""
import pytest
import torch

import twog_gcn_amd  # noqa: F401
from twog_gcn_amd import _lib
from tests import stream_cases as SC
from tests.entity_envelope import EPS, reference_error, sqrt_k_bound
from tests.stream_cases import F, EXACT, JUDGE

F32, F64 = torch.float32, torch.float64
# the fp32 specification against the fp64 one, relative to the tensor's largest value: a random walk over the longest sum of any
# case (4096 products of the widest gate) with the head room of entity_envelope.sqrt_k_bound
AGREE = sqrt_k_bound(4096)


def _agree(name, s32, s64):
    for k, v in s32.items():
        if not isinstance(v, tuple):
            assert v == s64[k], (name, k)
            continue
        a, how = v
        b = s64[k][0]
        assert a.shape == b.shape, (name, k)
        if how == EXACT:
            e = reference_error(a, b)   # copies and selections: 0; a single fp32 addition: its rounding, under the rule's floor
            assert e <= 4 * EPS, f'{name}/{k}: demanded bit for bit of the kernel, but fp32 and fp64 specification differ by {e:.3e}'
        elif how == JUDGE:
            assert torch.isfinite(a).all() and torch.isfinite(b.double()).all(), (name, k)
            e = reference_error(a, b)
            assert e <= AGREE, f'{name}/{k}: fp32 and fp64 specification differ by {e:.3e} of the largest value'


def _both(run, *a, **kw):
    return run(F, *a, 'cpu', F32, **kw), run(F, *a, 'cpu', F64, **kw)


FAMILIES = [('colsum', SC.COLSUM_CASES, SC.colsum_run), ('ew', SC.EW_CASES, SC.ew_run), ('adam', SC.ADAM_CASES, SC.adam_run),
            ('reorder', SC.REORDER_CASES, SC.reorder_run), ('filter', SC.FILTER_CASES, SC.filter_run),
            ('pos', SC.POS_CASES, SC.pos_run), ('seglen', SC.SEGLEN_CASES, SC.seglen_run), ('ssp', SC.SSP_CASES, SC.ssp_run)]


@pytest.mark.parametrize('name,cases,run', FAMILIES, ids=[f[0] for f in FAMILIES])
def test_every_case_builds_and_the_two_specification_runs_agree(name, cases, run):
    assert len({c['id'] for c in cases}) == len(cases)
    for c in cases:
        assert c['why']
        _agree(f"{name}/{c['id']}", *_both(run, c))


def test_single_cases_build_and_agree():
    _agree('rowops', *_both(SC.rowops_run))
    _agree('ssp_gather', *_both(SC.ssp_gather_run))
    for a, b in zip(SC.colsum_many_run(F, 'cpu', F32), SC.colsum_many_run(F, 'cpu', F64)):
        assert reference_error(a, b) <= AGREE
    assert len(SC.COLSUM_CASES) * 2 > 16


def test_head_cases_build_agree_and_leave_the_guard():
    for c in SC.HEAD_CASES:
        s32 = SC.head_run(F, c, 'cpu', F32)
        s64 = SC.head_run(F, c, 'cpu', F64, saved=s32)
        _agree(f"head/{c['id']}", s32, s64)
        assert torch.isnan(s32['guard'][0]).all() and s32['guard'][0].numel() == SC.HEAD_GUARD
        if c['C'] == 1:
            assert float(s32['out'][0].abs().max()) == 0.0 and float(s32['dlogits'][0].abs().max()) == 0.0
    assert {c['C'] for c in SC.HEAD_CASES} == {1, 13, 64} and all(c['bs'] * c['T'] * c['E'] == 402 for c in SC.HEAD_CASES)


def test_the_stated_row_factor_of_the_head_backward_is_a_property_of_fp32_summation_order():
    """The reason given in stream_cases.py for dlogits_row_factor, executed: the formula of the backward kernel in plain fp32
    torch, with the 64-term sum in another order than the specification's, misses factor 8 row-wise on C64_scale80 (and only
    there), stays far inside it tensor-wide, and is within a few half-ulps of the row's largest value."""
    from tests.entity_envelope import judge
    for c in SC.HEAD_CASES:
        s32 = SC.head_run(F, c, 'cpu', F32)
        s64 = SC.head_run(F, c, 'cpu', F64, saved=s32)
        for chains in (1, 4):
            rec, _ = judge(SC.head_bwd_in_plain_fp32(c, s32['out'][0], chains), s32['dlogits'][0], s64['dlogits'][0])
            assert rec['ratio'] < 1, (c['id'], chains, rec)
            if c['dlogits_row_factor']:
                assert rec['row_ratio'] > 8 and rec['row_e_hip'] < 16 * EPS and rec['row_e_ref'] < EPS, (c['id'], chains, rec)
            else:
                assert rec['row_ratio'] <= 8, (c['id'], chains, rec)
    assert [c['id'] for c in SC.HEAD_CASES if c['dlogits_row_factor']] == ['C64_scale80']


# ---------------------------------------------------------------------------------------------------------------- gates
@pytest.mark.parametrize('c', SC.GATE_CASES, ids=lambda c: c['id'])
def test_gate_cases_agree_and_at_most_one_hard_decision_is_within_the_margin(c):
    s32 = SC.gate_run(F, c, 'cpu', F32)
    s64 = SC.gate_run(F, c, 'cpu', F64, saved=s32)
    _agree(c['id'], s32, s64)
    ok = SC.hard_comparable(c, s64['soft'][0])
    assert int((~ok).sum()) <= 1, f"{c['id']}: {int((~ok).sum())} decisions within {SC.HARD_MARGIN} of the threshold: choose another seed"
    assert torch.equal(s32['hard'][0][ok], s64['hard'][0][ok])
    hard = s32['hard'][0].view(c['bs'], c['T'], c['E'])
    assert set(hard.unique().tolist()) <= {0.0, 1.0}
    if c['force_last']:
        assert bool((hard[:, -1] == 1).all())
    if c['T'] > 1 or not c['force_last']:
        assert 0 < float(hard.mean()) < 1, 'the case decides nothing'


def test_saturated_gate_case_saturates():
    c = SC.GATE_SATURATED
    s32 = SC.gate_run(F, c, 'cpu', F32)
    p = s32['p_save'][0]
    assert int(((p == 0) | (p == 1)).sum()) >= 4, 'no row saturates in fp32'
    for k in ('soft', 'p_save', 'dlogit', 'dlogit_hard_only', 'dlogit_soft_only'):
        assert torch.isfinite(s32[k][0]).all(), k


def test_gate_case_list_reaches_the_named_branches():
    cs = SC.GATE_CASES
    assert {c['bs'] * c['T'] * c['E'] % 4 for c in cs} == {0, 1, 2, 3}
    assert {c['hidden'] for c in cs} >= {32, 64, 72, 512} and {c['n_seg'] for c in cs} >= {1, 5, 8}
    assert {(c['noise'], c['noise_offset']) for c in cs} >= {(True, 0), (True, 2), (False, 0)}
    assert {c['force_last'] for c in cs} == {0, 1} and {c['thr'] for c in cs} == {0.3, 0.5}
    assert any(not c['bias'] for c in cs) and any(c['c0'] % 4 for c in cs)
    for c in cs:   # the segments' columns are no identity layout: a wrong weight block or column offset changes the result
        i = SC.gate_inputs(c['id'])
        assert len(i['seg_col']) == c['n_seg'] and (c['n_seg'] == 1 or i['seg_col'] != sorted(i['seg_col']))


# --------------------------------------------------------------------------------------------------------------- filter
def test_filter_inputs_contain_ties_and_values_on_the_threshold():
    assert {c['T'] for c in SC.FILTER_CASES} == {1, 2, 9} and any(c['bs'] * c['T'] * c['E'] > 256 for c in SC.FILTER_CASES)
    for c in SC.FILTER_CASES:
        soft = SC.filter_soft(c)
        assert torch.equal(soft * 16, (soft * 16).round())
        if c['T'] > 1:
            assert bool((soft[:, 1:] == soft[:, :-1]).any()), 'no tie with a neighbour'
        for thr in SC.FILTER_THRESHOLDS:
            assert bool((soft == thr).any()), f'no value equal to the threshold {thr}'
            hard, gmask = F.filter_fwd(soft, thr)
            assert 0 < float(hard.mean()) < 1 and (c['T'] == 1 or 0 < float(gmask.mean()) < 1)
    big = SC.filter_soft(SC.FILTER_CASES[0])
    tie_peak = (big[:, 1:-1] == big[:, :-2]) & (big[:, 1:-1] > big[:, 2:]) & (big[:, 1:-1] >= 0.5)
    assert bool(tie_peak.any()), 'no tie that decides: > and >= would give the same result'


# ---------------------------------------------------------------------------------------------------------------- reach
def test_launch_free_grid_plan_of_the_library():
    """Host arithmetic only, no device is opened: at least one workgroup, never fewer for more work, a cap that is reached (the
    same grid for 2^40 and 2^41 items), exactly enough workgroups below it; the reorder chunks keep 64 columns and aim at 512
    workgroups; the documented error codes."""
    lib = _lib.load()
    works = sorted({0, 1, 3, 4, 5, 15, 16, 17, 255, 256, 257, 1023, 1024, 1025} | {2 ** k + d for k in range(8, 27) for d in (-1, 0, 1, 77)})
    per = {F.STREAM_RELU_BWD_VEC: 4, F.STREAM_RANK1_VEC: 4, F.STREAM_COPY_BLOCKS: 4, F.STREAM_FILL_ZERO: 16}
    for kernel in range(F.STREAM_REORDER):
        grids = [lib.twog_stream_grid(kernel, w, 0) for w in works]
        cap = lib.twog_stream_grid(kernel, 2 ** 40, 0)
        assert cap == lib.twog_stream_grid(kernel, 2 ** 41, 0) and grids[0] == 1 and grids == sorted(grids) and grids[-1] <= cap
        for w, g in zip(works, grids):
            assert g == F.stream_grid(kernel, w)
            if g < cap:   # below the cap one trip covers the work (up to the incomplete group the strided loop leaves out)
                assert g * F.STREAM_THREADS * per.get(kernel, 1) >= w - SC.STREAM_SLACK[per.get(kernel, 1)], (kernel, w, g)
    for pairs in (0, 1, 2, 7, 10, 32, 64, 511, 512, 513, 4000):
        for cols in (1, 63, 64, 70, 127, 128, 192, 200, 1024, 4096):
            n = lib.twog_stream_grid(F.STREAM_REORDER, pairs, cols)
            assert 1 <= n <= max(cols // 64, 1) and (n == 1 or pairs * (n - 1) < 512), (pairs, cols, n)
    assert lib.twog_stream_grid(F.STREAM_REORDER, 8 * 4, 1024) == 16    # the product: 8 clips x 4 entities at 2h = 1024
    assert lib.twog_stream_grid(12, 1, 0) == -2 and lib.twog_stream_grid(0, -1, 0) == -2
    assert lib.twog_stream_grid(11, -1, 64) == -2 and lib.twog_stream_grid(11, 1, -1) == -2 and lib.twog_stream_grid(11, 2 ** 31, 64) == -2


def _plans():
    ps = [(c['id'], c['plan']) for c in SC.EW_CASES + SC.ADAM_CASES if c['plan']]
    return ps + [('rowops', SC.ROWOPS_PLAN), ('fill_zero', SC.FILL_BIG_PLAN), ('copy_blocks', SC.COPY_BIG_PLAN)]


def test_capped_cases_make_a_second_ragged_trip_and_every_capped_kernel_has_one():
    for name, plan in _plans():
        one_trip, work = SC.second_trip(F, plan)
        assert one_trip < work and work % one_trip != 0, (name, one_trip, work)
    assert {p[0] for _, p in _plans()} == {n for n in dir(F) if n.startswith('STREAM_') and n not in ('STREAM_THREADS', 'STREAM_REORDER')}


def test_vector_and_scalar_forms_are_reached_as_the_cases_say():
    for c in SC.EW_CASES:
        if c['op'] != 'mul':
            assert SC.ew_run(F, c, 'cpu', F32)['vec'] == c['vec'], c['id']
    for op in ('relu_bwd', 'rank1'):
        assert {(c['vec'], bool(c['plan'])) for c in SC.EW_CASES if c['op'] == op} == {(True, True), (True, False), (False, True), (False, False)}
    for c in SC.COLSUM_CASES:
        assert SC.vec_ok(SC.colsum_problem(c, 'cpu', F32)[0]) == c['vec'], c['id']
    cs = SC.COLSUM_CASES
    assert {c['rows'] for c in cs} >= {0, 1, 3, 4, 17, 64 * 3 + 5}
    assert any(not c['vec'] and c['cols'] > 64 for c in cs) and any(c['vec'] and c['cols'] > 256 for c in cs)
    assert any(c['acc'] and c['cols'] > 256 for c in cs) and {c['scaled'] for c in cs} == {True, False}
    assert {(c['cols'], c['vec']) for c in cs} >= {(260, True), (260, False), (516, True), (516, False), (33, False)}
    # the three reasons for the scalar form
    assert any(c['cols'] % 4 for c in cs) and any(c['ld'] % 4 and not c['cols'] % 4 for c in cs) and any(c['c0'] % 4 for c in cs)


def test_reorder_cases_reach_the_chunkings_they_name():
    for c in SC.REORDER_CASES:
        assert F.stream_grid(F.STREAM_REORDER, c['bs'] * c['E'], c['cols']) == c['chunks'], c['id']
        assert (c['cols'] % 4 == 0) == c['vec']
    cs = {c['id']: c for c in SC.REORDER_CASES}
    assert {c['cols'] for c in cs.values()} >= {64, 70, 192, 200, 1024} and {c['T'] for c in cs.values()} >= {1, 7, 300}
    u = cs['c200_T7']
    assert (u['cols'] // 4) % u['chunks'] != 0, 'the chunks are even'
    assert cs['c1024_pairs513']['bs'] * cs['c1024_pairs513']['E'] > 512
    g = SC.reorder_gate(5, 7, 2, 801)
    assert float(g[0].sum()) == 0 and float(g[1].min()) == 1 and float(g[2].sum()) == 2 == float(g[2, -1].sum())
    assert float(g[3].sum()) == 2 == float(g[3, 0].sum()) and 0 < float(g[4].mean()) < 1


def test_position_and_projection_lists_reach_the_named_sizes():
    per = [c for c in SC.POS_CASES if c['periodic']]
    assert {c['hidden'] for c in per} >= {2, 32, 70, 256, 258, 510, 512} and all(c['hidden'] % 2 == 0 for c in per)
    assert any(c['hidden'] % 2 for c in SC.POS_CASES if not c['periodic'])
    assert {c['T'] for c in SC.POS_CASES} >= {1, 7, 120} and {c['divide'] for c in SC.POS_CASES} == {True, False}
    assert any(c['c0'] for c in SC.POS_CASES)
    assert {c['bs'] * c['E'] for c in SC.SEGLEN_CASES} >= {297} and {c['T'] for c in SC.SEGLEN_CASES} >= {1, 7, 120}
    assert {(c['H'], c['O']) for c in SC.SSP_CASES} >= {(4, 16), (1, 1), (4, 1)} and {c['cols'] for c in SC.SSP_CASES} >= {4, 512, 1028}
    assert any(c['ph'] and not c['ps'] for c in SC.SSP_CASES) and any(c['ps'] and not c['ph'] for c in SC.SSP_CASES)
    assert any(not c['mask'] for c in SC.SSP_CASES)
    for c in SC.SSP_CASES:
        i = SC.ssp_inputs(c)
        assert i['off'] > 0 and i['off'] + c['H'] * c['O'] < i['natt']
        if c['mask'] and c['ph']:
            dw = SC.ssp_run(F, c, 'cpu', F32)['dw'][0]
            assert float(dw[:SC.SSP_IPC].abs().max()) == 0.0 and float(dw[SC.SSP_IPC:].abs().max()) > 0


# --------------------------------------------------------------------------------------------------------------- guards
def test_fill_zero_double_clears_exactly_the_requested_bytes():
    assert len(SC.FILL_PAIRS) == 18 * 49
    got, want = SC.fill_run(F, 'cpu'), SC.fill_expected()
    assert torch.equal(got, want)
    assert int((want == 0).sum()) == sum(n for _, n in SC.FILL_PAIRS) and int((want == SC.FILL_BYTE).sum()) == want.numel() - int((want == 0).sum())
    small = [(3, 100)]
    assert torch.equal(SC.fill_run(F, 'cpu', small, 256), SC.fill_expected(small, 256))


def test_copy_blocks_double_leaves_every_guard_float():
    got, want = SC.copy_run(F, 'cpu'), SC.copy_expected()
    assert torch.equal(got, want)
    assert len(SC.COPY_PAIRS) > 17 and {n for n, _, _ in SC.COPY_PAIRS} >= set(SC.COPY_SIZES)
    assert {(so, do) for _, so, do in SC.COPY_PAIRS} >= {(a, b) for a in range(4) for b in range(4)}
    n_guard = int((want == SC.COPY_SENTINEL).sum())
    assert n_guard >= 2 * SC.COPY_GUARD * len(SC.COPY_PAIRS) and n_guard + sum(n for n, _, _ in SC.COPY_PAIRS) == want.numel()
