"""CPU companion of tests/test_relation_kernels_gpu.py: the case list of tests/relation_cases.py and the specification themselves.

  builds     every case runs through the specification in fp32 and in fp64, finite and in agreement; what the GPU test demands
             bit for bit is the same in both runs;
  margin     DOT with relu_scores: no pair of any such case lies within 16 x 2^-24 x (scale <|q|, |k|> + |bias|) of zero, so the
             ReLU decisions do not depend on the summation order (a condition on the seeds, proven here);
  reach      the coverage the list claims, asserted from the list: widths, the entity limit for every mode pair, views of every
             row operand, feature-gradient branches, the shape of the multi-descriptor lists. This is also the argument for the
             one fault the GPU test must not provoke: an early return of relation_bwd_n_kernel that compared with the chunk's
             largest n_inst would run workgroups beyond the buffers of the smaller descriptors -- MANY_BWD has such descriptors in
             both chunks, and every bit of their buffers is compared with the single-descriptor calls;
  structure  the specification's weights obey the rules the kernel's are held to;
  R = 0      no receivers: the specification reads and writes nothing, like the library."""
import pytest
import torch

from tests import relation_cases as RC
from tests.entity_envelope import EPS, reference_error, sqrt_k_bound
from tests.relation_cases import F, EXACT, JUDGE

F32, F64 = torch.float32, torch.float64
# fp32 against fp64 specification, relative to the tensor's largest value: a random walk over the longest sum of any case
# (512 products per pair, 16 pairs per receiver) with the head room of entity_envelope.sqrt_k_bound
AGREE = sqrt_k_bound(512 * 16)
IDS = [c['id'] for c in RC.CASES]


def _dot_relu(c):
    return c['score'] == RC.DOT and c['relu']


@pytest.mark.parametrize('c', RC.CASES, ids=IDS)
def test_every_case_builds_and_the_two_specification_runs_agree(c):
    assert c['why']
    s32, s64 = RC.run(F, c, 'cpu', F32), RC.run(F, c, 'cpu', F64)
    assert set(s32) == set(s64) and 'out' in s32 and 'att' in s32
    for k, (a, how) in s32.items():
        b = s64[k][0]
        assert a.shape == b.shape and a.dtype == F32 and b.dtype == F64, k
        assert torch.isfinite(a).all() and torch.isfinite(b).all(), k
        e = reference_error(a, b)
        assert e <= (4 * EPS if how == EXACT else AGREE), f'{k}: fp32 and fp64 specification differ by {e:.3e} of the largest value'
    assert not RC.att_structure_failures(s32['att'][0], c)
    assert not RC.att_structure_failures(s64['att'][0], c)
    if c['R'] == c['S'] == 1 and c['excl']:   # no valid sender anywhere
        for k in ('out', 'att', 'dmsg', 'dp_r', 'dp_s'):
            assert k not in s32 or float(s32[k][0].abs().max()) == 0.0, k
    if c['score'] not in RC.SCORED and c['grads'] is not None:
        _, b0, _ = RC.build(c, 'cpu', F32)
        for k, acc in zip(('dq', 'dk'), c['grads']):
            assert torch.equal(s32[k][0], b0[k] if acc else torch.zeros_like(b0[k])), k


def test_ids_are_unique():
    assert len(set(IDS)) == len(IDS)


@pytest.mark.parametrize('c', [c for c in RC.CASES if _dot_relu(c)], ids=lambda c: c['id'])
def test_relu_decisions_of_the_dot_scores_do_not_depend_on_summation_order(c):
    m = RC.relu_margin(c)
    assert m > RC.RELU_BAND, f'a pair lies {m:.2e} x mag from zero, inside the band of {RC.RELU_BAND:.2e}'
    # both branches of the ReLU are well populated: a bias within 2 x BIAS_SCALE of zero against scores of about N(0, 1) gives a
    # share between 0.31 and 0.69, and the smallest case (90 pairs) adds a sampling noise of 2 x sqrt(0.25 / 90) = 0.1
    share = RC.relu_positive_share(c)
    assert 0.2 <= share <= 0.8, f'{share:.2f} of the valid pairs have a positive raw score'
    # the fp32 and the fp64 specification therefore decide alike: their ReLU masks on the raw scores are equal
    raws = []
    for dtype in (F32, F64):
        d, _, _ = RC.build(c, 'cpu', dtype)
        q, k = F._rel_rows(d['q'], c['n_inst'], c['R']), F._rel_rows(d['k'], c['n_inst'], c['S'])
        raws.append(torch.einsum('nrd,nsd->nrs', q, k) * d['scale'] + d['score_bias'] > 0)
    assert torch.equal(*raws)


def test_per_instance_score_gradients_add_up_to_the_specification_s_total():
    for c in (c for c in RC.CASES if _dot_relu(c)):
        for dtype in (F32, F64):
            d, b, w = RC.build(c, 'cpu', dtype)
            F.relation_bwd(b)
            total = float(w['dscore_sum'][1][0])
            assert float(w['dscore_sum'][1][1:].abs().sum()) == 0.0 or c['n_inst'] == 1
            per = RC.per_instance_dscore(d, b)
            assert per.shape == (c['n_inst'],) and per.dtype == dtype
            assert abs(float(per.double().sum()) - total) <= sqrt_k_bound(c['n_inst'] * 256) * max(float(per.abs().max()), 1e-30), c['id']


# ------------------------------------------------------------------------------------------------ what the list reaches
def test_every_listed_width_appears_in_a_case_whose_mode_uses_that_loop():
    """Every case runs forward and backward (relation_cases.run). hidden: the weight-gradient loop runs in the scored modes only, once per message mode; D: wdot runs for DOT only."""
    for msg in (RC.SENDER, RC.PAIR):
        seen = {c['hidden'] for c in RC.CASES if c['score'] in RC.SCORED and c['msg'] == msg}
        assert set(RC.HIDDEN_WIDTHS) <= seen, (msg, sorted(set(RC.HIDDEN_WIDTHS) - seen))
    seen = {c['D'] for c in RC.CASES if c['score'] == RC.DOT}
    assert set(RC.D_WIDTHS) <= seen, sorted(set(RC.D_WIDTHS) - seen)
    # dq / dk of DOT at D with a ragged tail, at the limit and with more rows x columns than one pass of 256 threads
    assert any(c['score'] == RC.DOT and c['R'] == c['S'] == RC.MAXE and c['D'] % 64 and c['R'] * c['D'] > 256 for c in RC.CASES)


def test_the_entity_limit_appears_for_every_mode_pair_the_host_composes():
    at_limit = {(c['score'], c['msg'], bool(c['relu'])) for c in RC.CASES if c['R'] == c['S'] == RC.MAXE}
    want = {(RC.SUM, RC.PAIR, False), (RC.MEAN, RC.PAIR, False), (RC.DOT, RC.SENDER, False), (RC.DOT, RC.PAIR, False),
            (RC.DOT, RC.SENDER, True), (RC.ADDITIVE, RC.SENDER, False), (RC.ADDITIVE, RC.PAIR, False),
            (RC.DISTANCE, RC.SENDER, False), (RC.MEAN, RC.SENDER, False)}
    assert want <= at_limit, want - at_limit
    lim = [c for c in RC.CASES if c['R'] == c['S'] == RC.MAXE]
    assert all(c['excl'] for c in lim), 'exclude_self on the square relations'
    assert any(c['smask'] for c in lim) and all(c['rmask'] for c in lim if c['msg'] == RC.SENDER and not c['self_rel'])
    for c in lim:
        if c['smask']:   # an all-masked clip and a clip with exactly one valid sender
            counts = (RC.send_mask_of(c) != 0).sum(1).tolist()
            assert 0 in counts and 1 in counts and max(counts) > 1, (c['id'], counts)
    import twog_gcn_amd  # noqa: F401
    from twog_gcn_amd import _lib
    assert _lib.load().twog_relation_limits() == RC.MAXE   # host arithmetic, no device is opened


def test_rectangular_degenerate_and_instance_shapes_are_listed():
    shapes = {(c['R'], c['S']) for c in RC.CASES}
    assert {(16, 1), (1, 16), (13, 16), (5, 3)} <= shapes
    assert any((c['R'], c['S'], c['excl']) == (1, 1, 1) for c in RC.CASES)
    assert any(c['n_inst'] == 1 and c['ipc'] == 1 for c in RC.CASES) and any(c['n_inst'] == 8 and c['ipc'] == 4 for c in RC.CASES)
    assert all(c['n_inst'] <= 8 and c['n_inst'] % c['ipc'] == 0 for c in RC.CASES)
    assert all(c['R'] <= RC.MAXE and c['S'] <= RC.MAXE for c in RC.CASES)


def test_every_row_operand_arrives_once_as_a_column_block_and_once_as_a_3d_view():
    from twog_gcn_amd.kernels import rows_of
    for views in ('cols', '3d'):
        seen = set()
        for c in (c for c in RC.CASES if c['views'] == views):
            d, b, _ = RC.build(c, 'cpu', F32)
            for k, t in list(d.items()) + list(b.items()):
                if k not in RC.ROW_OPERANDS or t is None:
                    continue
                seen.add(k)
                r = rows_of(t)
                if views == 'cols':
                    assert t.dim() == 2 and t.storage_offset() % 4 != 0 and r.ld_outer > t.shape[1], (c['id'], k)
                else:
                    n = c['R'] if k in ('q', 'p_r', 'out', 'dout', 'dp_r', 'dq') else c['S']
                    assert t.dim() == 3 and not t.is_contiguous(), (c['id'], k)
                    assert (r.inner == n and r.ld_inner > t.shape[2]) or (n == 1 and r.inner == 1), (c['id'], k)
        assert seen == set(RC.ROW_OPERANDS), (views, sorted(set(RC.ROW_OPERANDS) - seen))
    for c in (c for c in RC.CASES if c['score'] == RC.DISTANCE):
        d, _, _ = RC.build(c, 'cpu', F32)
        assert d['dist'].shape == (c['n_inst'], c['R'], c['S']) and d['dist'].stride(2) == c['R'] > 1, c['id']


def test_feature_gradient_branches_are_listed():
    dot = {tuple(c['grads']) for c in RC.CASES if c['score'] == RC.DOT}
    assert dot == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert any(c['self_rel'] and c['R'] == c['S'] == RC.MAXE and c['D'] == 65 and c['grads'] == (1, 1) for c in RC.CASES)
    for mode in (RC.SUM, RC.DISTANCE, RC.MEAN):   # written as zeros / left alone, for dq and for dk
        seen = {tuple(c['grads']) for c in RC.CASES if c['score'] == mode and c['grads'] is not None}
        assert {g[0] for g in seen} == {0, 1} and {g[1] for g in seen} == {0, 1}, (mode, seen)
    # accumulated buffers and every other written buffer are pre-filled with values, not zeros
    for c in RC.CASES:
        for k, (backing, _) in RC.build(c, 'cpu', F32)[2].items():
            assert float(backing.abs().min()) > 0.0, (c['id'], k)


def test_distance_cases_hold_zero_distances_and_a_receiver_without_any_sender():
    cs = [c for c in RC.CASES if c['score'] == RC.DISTANCE]
    for c in cs:
        dist = RC.dist_of(c)
        assert bool((dist == 0).any()) and float(dist[dist != 0].min()) >= 0.05, c['id']
    c = next(c for c in cs if c['zero_dist_recv'])
    s32 = RC.run(F, c, 'cpu', F32)
    att = s32['att'][0]
    assert float(att[:, c['R'] // 2].abs().max()) == 0.0 and float(att.abs().max()) > 0.0


def test_multi_descriptor_lists_exceed_one_chunk_with_uneven_instance_counts():
    for entries, per, short in ((RC.MANY_FWD, RC.MAXREL_F, RC.MANY_FWD_SHORT), (RC.MANY_BWD, RC.MAXREL_B, RC.MANY_BWD_SHORT)):
        assert len(entries) == {RC.MAXREL_F: 11, RC.MAXREL_B: 8}[per] > per
        assert len(RC.chunks(entries[:short], per)[-1]) == 1, 'the short form ends in a chunk of one descriptor'
        zero = [i for i, (_, o) in enumerate(entries) if o.get('desc_R') == 0]
        assert len(zero) == 1 and 0 < zero[0] % per < per - 1 and zero[0] < per, 'one R = 0 descriptor in the middle of a chunk'
        assert RC.case(entries[zero[0]][0])['views'] == 'dense'   # a 3-D row set with inner != R is refused, not skipped
        for ch in RC.chunks(entries, per):
            n = [RC.case(i, **o)['n_inst'] if o.get('desc_R') != 0 else 0 for i, o in ch]
            assert n.index(max(n)) != 0 and len(set(n)) > 1 and min(x for x in n if x) < max(n), n
    # backward: a descriptor of the scored and of the unscored branch, one that accumulates, none sharing a buffer (build() makes
    # fresh buffers per descriptor)
    modes = {RC.case(i)['score'] for i, _ in RC.MANY_BWD}
    assert RC.DOT in modes and RC.SUM in modes and RC.ADDITIVE in modes


# -------------------------------------------------------------------------------------------------------------- R = 0
@pytest.mark.parametrize('id', ['lim_dot_sender', 'lim_sum_pair', 'inst_n8_ipc4', 'rect_5x3_dot_relu_pair'])
def test_no_receivers_means_no_buffer_is_read_or_written(id):
    c = RC.case(id, desc_R=0)
    d, b, w = RC.build(c, 'cpu', F32)
    _, _, w0 = RC.build(c, 'cpu', F32)
    assert d['R'] == 0 and b['f'] is d
    F.relation_fwd(d)
    F.relation_bwd(b)
    F.relation_fwd_many([d])
    F.relation_bwd_many([b])
    for k in w:
        assert torch.equal(w[k][0], w0[k][0]), k
