"""CPU companion of tests/test_seg_persist_gpu.py: the case lists of tests/seg_persist_cases.py against the library's launch-free
report of the persistent segment launches (twog_segrnn_persistent_plan with the compute-unit count given: host arithmetic, no device
is opened), the specification on every case, and the judgement against planted faults.

  claims      at 256 compute units the report equals what every case claims -- (mh, mo), x3q1, cpc, n_chunks, clips of the last
              chunk, pair mask -- for the launched cases and for the pinned shapes of the older tests; the refused shapes are refused,
              each for its stated reason;
  plan        for every served case: grid = 2 x n_chunks x 4 x h / 16 <= 256 and a multiple of 8; both LDS sizes in (80 KB, 160 KB]
              (more than half: one workgroup per compute unit); the counters end below the error word; the chunks tile [0, bs);
              cpc x H <= 16, cpc x O <= 32; the pair mask equals one recomputed from "which tiles hold two rows of a clip"; dw_pad;
              the reported scratch bytes equal the formula of twog_segrnn_bwd_persistent_scratch_bytes on the reported numbers;
  coverage    the launched and pinned cases claim all eight (h, mo) cells -- both launches, so both x3q1 values for both mo --, the
              three pair masks, cpc in {1, 2, 3, 8, 16}, a ragged last chunk with mo = 1 and with mo = 2, T in {1, 2, 3};
  builds      the specification in fp32 against fp64 on every case: finite, within sqrt_k_bound of the longest sum, e_ref > 0 for
              every judged tensor that is not exactly zero or an exact copy by construction (the case says which: `zero`, `exact`),
              and the exact zeros are zeros;
  judgement   entity_envelope.judge at the GPU test's factor fails a stale hand-off, a lost clip of a ragged chunk and swapped rows
              of the two object tiles planted into the fp32 specification's result, and passes the result itself."""
import pytest
import torch

import twog_gcn_amd  # noqa: F401
from twog_gcn_amd import _lib
from tests import entity_envelope as EE
from tests import seg_persist_cases as PC
from tests.entity_envelope import reference_error, sqrt_k_bound

F32, F64 = torch.float32, torch.float64
AGREE = sqrt_k_bound(2048)   # as tests/test_gru_kernels_cpu.py: the longest sum is the 3h = 1 536 products of d_gi with W_ih at h = 512
SERVED = PC.LAUNCHED + PC.PINNED
KB = 1024


def report(c, n_cus=None, **over):
    c = dict(c, **over)
    return _lib.segrnn_persistent_plan(_lib.load(), c['bs'], c['T'], c['H'], c['O'], c['h'], n_cus or c.get('n_cus', PC.N_CUS),
                                       **PC.plan_args(c))


def test_ids_are_unique_and_every_case_names_its_branch():
    every = PC.LAUNCHED + PC.PINNED + PC.REFUSED
    assert len(PC.BY_ID) == len(every) and all(c['why'] for c in every)
    assert all(c['inst'][0] == 1 and c['inst'][1] in (1, 2) and c['x3q1'] == (c['h'] >= 256) for c in SERVED)
    assert all(c['T'] <= 4 for c in PC.LAUNCHED if c['id'] != 'h64_T33'), 'every launched case but the one long chain is short'
    from tests.test_kernels_gpu import SEG_PERSIST_SHAPES
    assert [c['shape'] for c in PC.PINNED] == SEG_PERSIST_SHAPES + EE.SEG_PERSISTENT, 'the pinned list is the older tests\' shapes'


@pytest.mark.parametrize('c', SERVED, ids=lambda c: c['id'])
def test_the_report_at_256_compute_units_equals_the_claims(c):
    p = report(c)
    assert p['served'] and p['n_cus'] == PC.N_CUS, p
    assert PC.claimed(p) == PC.claims(c), f"{c['id']} no longer reaches its branch ({c['why']}): change the shape, not the claim"


@pytest.mark.parametrize('c', SERVED, ids=lambda c: c['id'])
def test_the_plan_tiles_the_batch_and_the_launch_fits_the_device(c):
    p = report(c)
    bs, T, H, O, h = c['shape']
    cpc, n = p['cpc'], p['n_chunks']
    assert p['grid'] == 2 * n * 4 * h // 16 <= PC.N_CUS and p['grid'] % 8 == 0
    for lds in (p['lds_fwd'], p['lds_bwd']):
        assert 80 * KB < lds <= 160 * KB, 'more than half of the LDS: one workgroup per compute unit'
    err_word = _lib.load().twog_segrnn_persistent_sync_bytes() // 4 - 32
    assert p['sync_words'] == 2 * n * 4 * 32 <= err_word
    chunks = PC.chunk_of_clips(c)
    assert len(chunks) == n and chunks[0][0] == 0 and sum(k for _, k in chunks) == bs and chunks[-1][1] == p['last'] >= 1
    assert all(a[0] + a[1] == b[0] and a[1] == cpc for a, b in zip(chunks, chunks[1:])), chunks
    assert cpc * H <= 16 and cpc * O <= 32
    assert (p['mh'], p['mo']) == ((cpc * H + 15) // 16, (cpc * O + 15) // 16)
    assert p['pair_mask'] == PC.pair_mask_of(cpc, H, O) and p['pair_mask'] in (PC.M1, PC.M2, PC.M2X)
    assert p['dw_pad'] % 4 == 0 and cpc * max(H * H + H * O, H * O + O * O) <= p['dw_pad'] < cpc * max(H * H + H * O, H * O + O * O) + 4
    ns = h // 16
    assert p['scratch_bytes'] == (2 * T * ns * 2 * n * p['dw_pad'] + 2 * T * ns * bs * (H + O)) * 4 + 256


def test_the_cases_cover_every_instance_and_every_edge_of_the_plan():
    cells = {(c['h'], c['inst'][1]) for c in SERVED}
    assert cells == {(h, mo) for h in (64, 128, 256, 512) for mo in (1, 2)}, 'the eight (h, mo) cells of the forward launch'
    assert {(c['h'], c['inst'][1], c['x3q1']) for c in SERVED} == {(h, mo, h >= 256) for h, mo in cells}, 'and of the backward launch'
    assert {(c['inst'][1], c['x3q1']) for c in SERVED} == {(mo, x) for mo in (1, 2) for x in (False, True)}
    # the cells the older shapes never reached are claimed by cases this module launches
    assert {(128, 2)} <= {(c['h'], c['inst'][1]) for c in PC.LAUNCHED} and (128, 2) not in {(c['h'], c['inst'][1]) for c in PC.PINNED}
    assert {c['pair_mask'] for c in SERVED} == {PC.M1, PC.M2, PC.M2X}
    assert {c['h'] for c in PC.LAUNCHED if c['pair_mask'] == PC.M2} >= {64, 128, 512}
    assert {c['cpc'] for c in PC.LAUNCHED} >= {1, 2, 3, 8, 9, 16}
    assert {c['h'] for c in PC.LAUNCHED if c['cpc'] == 16} == {64, 512}
    assert {c['inst'][1] for c in PC.LAUNCHED if c['last'] < c['cpc']} == {1, 2}, 'a ragged last chunk with one and with two object tiles'
    assert {c['T'] for c in PC.LAUNCHED} >= {1, 2, 3, 33}
    assert {c['T'] for c in PC.LAUNCHED if c['inst'][1] == 2} >= {1, 2}, 'first / last step coincidence with two object tiles'
    assert any(c['shape'][:1] + c['shape'][2:4] == (1, 1, 1) for c in PC.LAUNCHED), 'one row of each kind'
    for key, off in (('b_hh', False), ('b_smsg', False), ('obj_mask', None), ('gates', 'closed'), ('gates', 'open'), ('obj_mask', 'all'),
                     ('obj_mask', 'one_valid')):
        assert any(key in c['inputs'] and c['inputs'][key] == off for c in PC.LAUNCHED), (key, off)
    for pattern in ('closed', 'open', 'all', 'one_valid'):
        assert {c['inst'][1] for c in PC.LAUNCHED if pattern in c['inputs'].values()} == {1, 2}, pattern


@pytest.mark.parametrize('c', PC.REFUSED, ids=lambda c: c['id'])
def test_refused_shapes_are_not_served(c):
    p = report(c)
    assert not p['served'] and p['n_cus'] == c['n_cus'], (c['why'], p)
    assert all(v == 0 for k, v in p.items() if k != 'n_cus'), p


def test_the_refusals_are_of_the_stated_kind():
    """Each refused shape is one step from a served one: the refusal is the stated reason's, not another's."""
    R = {c['id'][len('refused_'):]: c for c in PC.REFUSED}
    assert report(R['mh2'], bs=8)['served'] and report(R['mh2'], bs=8)['cpc'] == 8, '16 human rows are served'
    assert report(R['mo3_h512'], bs=2)['served'] and report(R['mo3_h128'], bs=8)['served']
    assert all(report(R['h96'], h=h)['served'] for h in (64, 128, 256, 512))
    assert report(R['H5'], H=4)['served'] and report(R['O13'], O=12)['served']
    for k in ('no_hh', 'no_ho', 'no_oh', 'no_oo', 'no_msg'):
        assert report(R[k], rels=PC.ALL_RELS, msg=True)['served'], k
    assert report(R['h512_128cus'], n_cus=256)['served'] and not report(R['h512_128cus'], n_cus=255)['served']
    assert report(R['h512_128cus'], n_cus=128, h=256)['served']


def test_the_served_range_at_256_compute_units():
    """What DESIGN.md states: chunks per direction at most 256 / (8 h / 16), capped at 16; clips per chunk at most 16 / H and 32 / O."""
    for h, most in ((64, 8), (128, 4), (256, 2), (512, 1)):
        for bs in range(1, 16 * most + 2):
            p = _lib.segrnn_persistent_plan(_lib.load(), bs, 2, 1, 2, h, PC.N_CUS)
            assert p['served'] == (bs <= 16 * most), (h, bs)
            if p['served']:
                assert p['n_chunks'] <= most and p['cpc'] == -(-bs // min(most, bs)) and p['n_chunks'] == -(-bs // p['cpc'])
    for H, O in ((1, 1), (2, 4), (3, 6), (4, 12), (1, 12), (4, 1)):
        served = [bs for bs in range(1, 40) if _lib.segrnn_persistent_plan(_lib.load(), bs, 2, H, O, 512, PC.N_CUS)['served']]
        assert served == list(range(1, min(16 // H, 32 // O) + 1)), (H, O, served)


@pytest.mark.parametrize('c', PC.LAUNCHED + [c for c in PC.REFUSED if c['step']], ids=lambda c: c['id'])
def test_every_case_builds_in_both_precisions(c):
    b32, b64, _, o32, o64 = PC.spec(c)
    judged = [(k, b32[k], b64[k]) for k in PC.fwd_keys(c)] + [(k, o32[k], o64[k]) for k in PC.bwd_keys(c, o32)]
    assert len(judged) == (17 if c['msg'] else 10)
    zero = set()
    for k, a, b in judged:
        assert a.dtype == F32 and b.dtype == F64 and a.shape == b.shape and a.numel(), (c['id'], k)
        assert torch.isfinite(a).all() and torch.isfinite(b).all(), (c['id'], k)
        if float(b.abs().max()) == 0.0:
            assert float(a.abs().max()) == 0.0, (c['id'], k)
            zero.add(k)
            continue
        e = reference_error(a, b)
        assert (e == 0 if k in c['exact'] else 0 < e <= AGREE), f"{c['id']}/{k}: e_ref = {e:.3e}"
    assert zero == set(c['zero']), f"{c['id']}: exactly zero {sorted(zero)}, expected {sorted(c['zero'])}"
    for b in (b32, b64):
        for name, v in PC.exact_zeros(c, b).items():
            assert v.numel() and float(v.abs().max()) == 0.0, f"{c['id']}: {name} is not exactly 0 in the specification"
    if c['inputs'].get('gates') == 'closed':
        assert not PC.uniform_attention_failures(c, b32['att']) and not PC.uniform_attention_failures(c, b64['att'])
    if c['inputs'].get('obj_mask') == 'one_valid':
        bs, T, H, O, h = c['shape']
        oo = b32['att'][..., H * H + 2 * H * O:].reshape(2, T, bs, O, O)
        assert float(oo.sum(-1).sum()) == 2 * T * bs * (O - 1), 'every other object receives from the valid one with weight exactly 1'


def test_the_exact_zeros_are_named_for_the_cases_that_have_them():
    named = {c['id'] for c in PC.LAUNCHED if PC.exact_zeros(c, PC.spec(c)[0]) or c['zero']}
    assert named == {c['id'] for c in PC.LAUNCHED if set(c['inputs'].values()) & {False, 'closed', 'all', 'one_valid'}}


@pytest.mark.parametrize('id,plant', PC.PLANTED, ids=[f'{i}-{f.__name__}' for i, f in PC.PLANTED])
def test_the_judgement_fails_a_planted_fault_and_passes_the_result_itself(id, plant):
    c = PC.BY_ID[id]
    b32, b64 = PC.spec(c)[:2]
    bad, touched = plant(c, b32)
    factor = EE.seg_factor(c['h'])
    for k in PC.fwd_keys(c):
        assert not EE.judge(b32[k], b32[k], b64[k], factor)[1], (id, k)
        fails = EE.judge(bad[k], b32[k], b64[k], factor)[1]
        assert bool(fails) == (k in touched), f'{id}/{k}: {fails}'
        if k in touched:
            assert any(f.startswith('row ') for f in fails) and any(f.startswith('e_hip') for f in fails), (id, k, fails)
    if plant is PC.plant_ragged_clip_lost:   # and in d_u, whose rows are the chunks (seg_persist_cases.judged_rows)
        o32, o64 = PC.spec(c)[3:]
        for k in ('d_u_h', 'd_u_o'):
            lost = o32[k].clone()
            lost[c['bs'] - 1] = 0
            good, lost, s64 = (PC.judged_rows(c, k, t) for t in (o32[k], lost, o64[k]))
            assert good.shape[0] == c['n_chunks'] and not EE.judge(good, good, s64, factor)[1]
            fails = EE.judge(lost, good, s64, factor)[1]
            assert any(f.startswith(f"row {c['n_chunks'] - 1} ") for f in fails) and any(f.startswith('e_hip') for f in fails), (id, k, fails)
