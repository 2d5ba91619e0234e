"""CPU companion of tests/test_gru_persist_gpu.py: the case lists of tests/gru_persist_cases.py against the library's launch-free
report of the persistent BiGRU partition (twog_bigru_persistent_plan with the compute-unit count given: host arithmetic, no device
is opened), and the specification on every case.

  claims     at 256 compute units the report equals what every case claims: forward instance <NKB, TWC>, the multiset of (tiles per
             chunk, tiles per wave), whether the backward serves it;
  partition  the combinations tile [0, row tiles) of every (type, direction) group without gap or overlap, tw = ceil(tiles / 4),
             grid = combinations x h / 16 <= 256, LDS <= 160 KB;
  coverage   the twelve forward instances and the four backward widths are claimed by some case; the default list holds the edges
             the kernels' index arithmetic has (chunks of 1 .. 4 tiles, one row, four types, rows % 16 in {1, 15}, no bias, T in
             {1, 2}); the refused shapes are refused;
  index      the kernels' row -> clip expression (a float reciprocal) equals the integer division for every E and row of a served shape;
  builds     the specification in fp32 against fp64 on every case: finite, and e_ref > 0 for every judged tensor, so the yardstick
             of the GPU rule is never 0 by accident."""
import pytest
import torch

import twog_gcn_amd  # noqa: F401
from twog_gcn_amd import _lib
from tests import gru_cases as GC
from tests import gru_persist_cases as PC
from tests.entity_envelope import reference_error, sqrt_k_bound
from tests.gru_cases import F, JUDGE

F32, F64 = torch.float32, torch.float64
AGREE = sqrt_k_bound(2048)   # as tests/test_gru_kernels_cpu.py: the longest sum is the 1 536 products of the carried gradient


def report(Es, bs, h, n_cus=PC.N_CUS):
    return _lib.bigru_persistent_plan(_lib.load(), Es, bs, h, n_cus)


def test_ids_are_unique_and_every_case_names_its_branch():
    ids = [c['id'] for c in PC.LAUNCHED]
    assert len(set(ids)) == len(ids) and all(c['why'] for c in PC.LAUNCHED)
    assert not set(ids) & {c['id'] for c in GC.REC_ALL}, 'the persistent cases are registered beside REC_ALL, not in it'
    assert all(GC.REC_BY_ID[c['id']] is c for c in PC.LAUNCHED)
    assert all(c['nd'] == 2 and c['bwd'] == (c['inst'][1] == 1) for c in PC.LAUNCHED)
    assert all(c['inst'][1] == 1 for c in PC.DEFAULT) and all(c['inst'][1] > 1 for c in PC.FORCED)


@pytest.mark.parametrize('c', PC.LAUNCHED, ids=lambda c: c['id'])
def test_the_report_at_256_compute_units_equals_the_claims(c):
    p = report(c['Es'], c['bs'], c['h'])
    assert p['served'] and p['n_cus'] == PC.N_CUS, p
    assert PC.claimed(p) == PC.claims(c), f"{c['id']} no longer reaches its branch ({c['why']}): change the shape, not the claim"
    assert p['nkb'] == c['h'] // 32 and sum(c['chunks'].values()) == p['n_combos'] == len(p['combos'])


@pytest.mark.parametrize('c', PC.LAUNCHED, ids=lambda c: c['id'])
def test_the_combinations_tile_every_group_and_the_launch_fits_the_device(c):
    p = report(c['Es'], c['bs'], c['h'])
    by_group = {}
    for g, rt0, rt1, tw in p['combos']:
        assert 0 <= rt0 < rt1 and tw == (rt1 - rt0 + 3) // 4 and 1 <= tw <= 4, (g, rt0, rt1, tw)
        by_group.setdefault(g, []).append((rt0, rt1))
    assert sorted(by_group) == list(range(2 * len(c['Es'])))
    for g, spans in by_group.items():
        tiles = (PC.type_rows(c)[g // 2] + 15) // 16
        spans.sort()
        assert spans[0][0] == 0 and spans[-1][1] == tiles, (g, spans, tiles)
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:])), f'group {g}: gap or overlap in {spans}'
    assert p['grid'] == p['n_combos'] * c['h'] // 16 <= PC.N_CUS
    assert 0 < p['lds_fwd'] <= PC.LDS_LIMIT and 0 < p['lds_bwd'] <= PC.LDS_LIMIT
    most = max(tw for _, _, _, tw in p['combos'])
    assert p['twc'] == {1: 1, 2: 2, 3: 4, 4: 4}[most] and p['bwd_served'] == (most == 1)


def test_every_forward_instance_and_every_backward_width_is_claimed():
    assert {c['inst'] for c in PC.LAUNCHED} == PC.INSTANCES and len(PC.INSTANCES) == 12
    assert {c['h'] for c in PC.DEFAULT if c['bwd']} == PC.BWD_WIDTHS
    assert not any(c['bwd'] for c in PC.FORCED)
    # within the TWC = 4 instances: three tiles per wave (the fourth slot idle) and four
    assert {tw for c in PC.FORCED for (_, tw) in c['chunks']} == {1, 2, 3, 4}


def test_the_default_list_holds_the_edges():
    D = PC.DEFAULT
    assert {tiles for c in D for (tiles, _) in c['chunks']} == {1, 2, 3, 4}
    assert any(PC.type_rows(c) == [1] for c in D), 'a one-row problem'
    assert {c['T'] for c in D if PC.type_rows(c) == [1]} == {1, 2, 3}
    assert max(c['T'] for c in D) >= 33
    four = [c for c in D if len(c['Es']) == 4 and c['h'] == 512]
    assert four and report(four[0]['Es'], four[0]['bs'], 512)['grid'] == PC.N_CUS, 'four types at h = 512: every compute unit'
    assert {r % 16 for c in D for r in PC.type_rows(c)} >= {1, 15}
    assert any(not c['bias'] for c in D)
    assert {E for c in D for E in c['Es']} >= {1, 2, 3, 5, 7, 9, 11, 12, 13}
    # the MAXC bound: 32 combinations on half the device, one group with a single two-tile chunk among one-tile chunks
    c = GC.REC_BY_ID['persist_h64_maxc']
    p = report(c['Es'], c['bs'], c['h'])
    assert p['n_combos'] == _lib.BIGRU_PLAN_MAX_COMBOS and p['grid'] < PC.N_CUS
    sizes = {}
    for g, rt0, rt1, _ in p['combos']:
        sizes.setdefault(g, []).append(rt1 - rt0)
    assert any(sorted(s)[-2:] == [1, 2] and len(s) > 2 for s in sizes.values()), sizes


@pytest.mark.parametrize('id,why,Es,bs,h,n_cus', PC.REFUSED, ids=[r[0] for r in PC.REFUSED])
def test_refused_shapes_are_not_served(id, why, Es, bs, h, n_cus):
    p = report(Es, bs, h, n_cus)
    assert not p['served'] and p['n_combos'] == -1 and p['combos'] == [] and p['n_cus'] == n_cus, (why, p)
    assert (p['nkb'], p['twc'], p['grid'], p['lds_fwd'], p['lds_bwd'], p['bwd_served']) == (0, 0, 0, 0, 0, False)


def test_the_refusals_are_of_the_stated_kind():
    """Each refused shape is one step from a served one: the refusal is the stated reason's, not another's."""
    assert report((1, 1, 1, 1), 3, 64)['served'] and report((2, 3, 1), 3, 128)['served'] and report((2, 3), 3, 64)['served']
    assert report((2, 8, 1), 64, 512)['served'], 'a chunk of 16 tiles is served'
    assert max(rt1 - rt0 for _, rt0, rt1, _ in report((2, 8, 1), 64, 512)['combos']) == 16
    assert report((2, 3, 1), 3, 512, 192)['served'] and not report((2, 3, 1), 3, 512, 191)['served']


def test_the_float_reciprocal_of_the_row_index_is_exact_over_the_whole_range():
    """Both kernels find the clip of a row as (int)((row + 0.5f) * (1.0f / E)). In IEEE fp32 (numpy: the same three roundings, no
    contraction possible) that equals row // E for every E and every row a served shape can have: at most MAXC combinations of at
    most 16 tiles of 16 rows per launch. The cases only sample nine values of E; this covers the rest of the expression's range."""
    import numpy as np
    most = _lib.BIGRU_PLAN_MAX_COMBOS * 16 * 16
    row = np.arange(most, dtype=np.int32)
    half = row.astype(np.float32) + np.float32(0.5)
    for E in range(1, most + 1):
        b = (half * (np.float32(1.0) / np.float32(E))).astype(np.int32)
        assert np.array_equal(b, row // E), E


@pytest.mark.parametrize('c', PC.LAUNCHED, ids=lambda c: c['id'])
def test_every_case_builds_in_both_precisions(c):
    s32 = GC.rec_run(F, c, 'cpu', F32)
    s64 = GC.rec_run(F, c, 'cpu', F64, saved=s32)
    judged = [k for k, (_, how) in s32.items() if how == JUDGE]
    assert len(judged) == 4 * len(c['Es'])
    for k in judged:
        a, b = s32[k][0], s64[k][0]
        assert a.dtype == F32 and b.dtype == F64 and a.shape == b.shape and a.numel(), (c['id'], k)
        assert torch.isfinite(a).all() and torch.isfinite(b).all(), (c['id'], k)
        e = reference_error(a, b)
        assert 0 < e <= AGREE, f"{c['id']}/{k}: e_ref = {e:.3e}"
    if not c['bias']:
        for k in range(len(c['Es'])):
            rows = PC.first_step_hn_rows(c, k)
            assert len(rows) == 2 * c['bs'] * c['Es'][k]
            assert float(s32[f'save{k}'][0][rows].abs().max()) == 0.0 and float(s64[f'save{k}'][0][rows].abs().max()) == 0.0
            assert int((s32[f'save{k}'][0].abs().amax(1) == 0).sum()) == len(rows), 'no other row of save is zero'
