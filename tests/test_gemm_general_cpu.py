"""CPU companion of tests/test_gemm_general_gpu.py: the case list of tests/gemm_cases.py itself.

  builds   every case runs through FakeKernels.gemm in fp32 and in fp64 (s32 and s64 of the GPU test): outputs of the dtype of the
           inputs, finite, the fp32 run within a random-walk bound of the fp64 run and -- for sums of 8 terms or more -- not equal to
           it (the fp64 run really is fp64), judge(s32, s32, s64) passes, the memory around every C view is SENTINEL in both runs, and
           no row behind a ReLU is entirely clipped (judge demands exact zeros of such a row);
  reach    what each `why` claims, by plain arithmetic on the shapes: chunk sizes, the K classes of every chunk and their tile counts
           modulo 8, which operands fail the conditions of vec_ok, k-tiles of the short problems, empty split-K slices for every
           possible slice count, tile counts on either side of the 32-row / 64-row k-split threshold.
The only launch constants written down are MAXP = 8, BK = 32 and the tile sizes (tests/gemm_cases.py)."""
import pytest
import torch

import twog_gcn_amd  # noqa: F401
from tests import gemm_cases as GC
from tests.entity_envelope import judge, reference_error, sqrt_k_bound
from tests.gemm_cases import F, EXACT, JUDGE

F32, F64 = torch.float32, torch.float64


def test_ids_are_unique_and_every_case_names_its_branch():
    assert len(GC.BY_ID) == len(GC.CASES)
    assert all(c['why'] and c['tile'] in ((64, 64), (32, 64), (128, 128)) for c in GC.CASES)
    families = {c['id'].rsplit('_', 1)[0] for c in GC.CASES}
    assert families >= {'classes3_rot', 'chunks_19', 'vec_mix', 'vec_mix_ks32', 'vec_mix_ks64', 'kg64_ragged', 'kg64_whole', 'ks_single_ktile32',
                        'ks_single_ktile64', 'splitk64_mixed_vec', 'splitk64_mixed_bias_off', 'splitk64_mixed_c_odd', 'splitk128_xcd_mixed_x3',
                        'splitk128_xcd_mixed_fp32', 'batched_mixed', 'batched_mixed_bodd'}
    for fam in ('classes3_rot', 'vec_mix'):
        assert {c['id'] for c in GC.CASES if c['id'].rsplit('_', 1)[0] == fam} == {f'{fam}_{l}' for l in GC.LAYOUTS}
    assert all(p['M'] > 0 and p['N'] > 0 and p['K'] > 0 for c in GC.CASES for p in c['probs'])   # zero sizes: not defined by the ABI


@pytest.mark.parametrize('c', GC.CASES, ids=lambda c: c['id'])
def test_every_case_builds_in_both_precisions(c):
    s32, s64 = GC.gemm_run(F, c, 'cpu', F32), GC.gemm_run(F, c, 'cpu', F64)
    assert list(s32) == list(s64) and len(s32) == 2 * len(c['probs'])
    for i, p in enumerate(c['probs']):
        a, b = s32[f'C{i}'][0], s64[f'C{i}'][0]
        nb = p['batch'][0] if p['batch'] else 1
        assert s32[f'C{i}'][1] == JUDGE and a.dtype == F32 and b.dtype == F64 and a.shape == b.shape == (nb * p['M'], p['N'])
        assert torch.isfinite(a).all() and torch.isfinite(b).all()
        e = reference_error(a, b)
        assert e <= sqrt_k_bound(p['K'] + 2), f"{c['id']}/C{i}: e_ref = {e:.3e}"
        assert e > 0 or p['K'] < 8, f"{c['id']}/C{i}: the fp32 run equals the fp64 run"
        rec, fails = judge(a, a, b)
        assert not fails and rec['ratio'] <= 1.0 and rec['row_ratio'] <= 1.0, (c['id'], i, fails)
        if p['act'] == 1:
            assert float(b.amax(1).min()) > 0, f"{c['id']}/C{i}: a row is entirely clipped by the ReLU"
            assert int((b == 0).sum()) > 0   # (and the ReLU does clip)
        ar32, ar64 = s32[f'around{i}'][0], s64[f'around{i}'][0]
        assert s32[f'around{i}'][1] == EXACT and torch.equal(ar32.double(), ar64)
        assert int((ar32 == GC.SENTINEL).sum()) == ar32.numel() - a.numel() and int((ar32 == 0).sum()) == a.numel()
        assert ar32.numel() > a.numel() + 2 * p['N']   # rows above and below, columns left and right of every view


def test_the_inputs_are_the_same_values_in_both_precisions_and_on_every_call():
    c = GC.BY_ID['vec_mix_tt']
    p32, _ = GC.gemm_build(c, 'cpu', F32)
    p64, _ = GC.gemm_build(c, 'cpu', F64)
    for a, b in zip(p32, p64):
        for k in ('A', 'B', 'C', 'bias'):
            assert (a[k] is None and b[k] is None) or (a[k].shape == b[k].shape and torch.equal(a[k].double(), b[k]))
    again, _ = GC.gemm_build(c, 'cpu', F32)
    assert all(torch.equal(a['A'], b['A']) and torch.equal(a['C'], b['C']) for a, b in zip(p32, again))


# ------------------------------------------------------------------------------------------------------------------- reach
@pytest.mark.parametrize('c', GC.CASES, ids=lambda c: c['id'])
def test_chunks_and_k_classes(c):
    chunks = GC.chunks_of(c)
    assert [len(ch) for ch in chunks] == c.get('chunks', [len(c['probs'])]) and all(len(ch) <= GC.MAXP for ch in chunks)
    if 'cls_mod8' in c:
        got = [[n % 8 for _, n in GC.k_classes(ch, c['tile'])] for ch in chunks]
        assert got == c['cls_mod8'], got


def test_classes3_rot_has_four_classes_whose_remainders_all_count():
    c = GC.BY_ID['classes3_rot_nn']
    cls = GC.k_classes(c['probs'], c['tile'])
    assert cls == [(100, 10), (40, 6), (8, 1), (3, 1)]
    assert sorted(p['K'] for p in c['probs']) != [p['K'] for p in c['probs']][::-1]   # the caller's order is not the sorted one
    assert sum(1 for p in c['probs'] if p['K'] == 100) == 2
    assert all(n % 8 for _, n in cls) and sum(n for _, n in cls) == 18
    # two or more classes with a remainder: the second class's ring offset is not zero
    assert cls[0][1] % 8 == 2
    assert {(p['bias'], p['act'], p['acc']) for p in c['probs']} >= {(True, 0, False), (True, 1, False), (False, 0, True), (False, 0, False)}


def test_chunks_19_puts_the_longest_problem_into_the_last_chunk():
    c = GC.BY_ID['chunks_19_nn']
    Ks = [p['K'] for p in c['probs']]
    assert len(Ks) == 19 and Ks.index(max(Ks)) == 16 and max(Ks) == 130
    assert {31, 32, 33} <= set(Ks) and (1, 1, 1) in {(p['M'], p['N'], p['K']) for p in c['probs']}
    assert {p['M'] for p in c['probs']} >= {1, 80} and {p['N'] for p in c['probs']} >= {1, 80}
    for ch in GC.chunks_of(c):   # every chunk has its own K order, none of them sorted already
        k = [p['K'] for p in ch]
        assert k != sorted(k, reverse=True)
    assert any(sum(1 for p in ch if p['K'] == 64) == 2 for ch in GC.chunks_of(c))
    assert max(p['K'] for p in c['probs']) < 256 and not all(p['M'] >= 96 and p['N'] >= 96 for p in c['probs'][16:])


@pytest.mark.parametrize('c', [c for c in GC.CASES if 'vec' in c], ids=lambda c: c['id'])
def test_operands_fail_the_16_byte_conditions_where_the_case_says(c):
    probs, _ = GC.gemm_build(c, 'cpu', F32)
    got = []
    for d in probs:
        _, a_bs, b_bs, _ = d.get('batch', (1, 0, 0, 0))
        got.append((GC.operand_vec_ok(d['A'], a_bs), GC.operand_vec_ok(d['B'], b_bs)))
    assert got == c['vec'], got
    if c['id'].startswith('vec_mix') or 'bodd' in c['id']:
        assert {v for pair in got for v in pair} == {0, 1}   # both load forms inside one launch


def test_vec_mix_breaks_one_operand_at_a_time():
    for l in GC.LAYOUTS:
        probs, _ = GC.gemm_build(GC.BY_ID[f'vec_mix_{l}'], 'cpu', F32)
        A0, B1, A2, B2 = probs[0]['A'], probs[1]['B'], probs[2]['A'], probs[2]['B']
        for t in (A0, B1):   # pointer 4 bytes off, odd leading dimension
            assert t.data_ptr() % 16 == 4 and t.stride(0) % 2 == 1
        assert probs[0]['B'].data_ptr() % 16 == 0 and probs[1]['A'].data_ptr() % 16 == 0
        assert A2.data_ptr() % 16 == 0 and B2.data_ptr() % 16 == 0 and GC.VEC_MIX[2]['K'] % 4 == 2
    assert GC.VEC_MIX[3]['M'] == 3 and GC.VEC_MIX[4]['N'] == 2


@pytest.mark.parametrize('c', [c for c in GC.CASES if 'short' in c], ids=lambda c: c['id'])
def test_short_problems_have_fewer_k_tiles_and_empty_slices(c):
    kt = [GC.ceil_div(p['K'], GC.BK) for p in c['probs']]
    kmax = max(p['K'] for p in c['probs'])
    for short, longest in c['short'].items():
        assert kt[short] < kt[longest] and c['probs'][longest]['K'] == kmax
        if c['expect'][0] & GC.SPLITK:
            for want in range(2, 65):   # whatever count the library chooses: this problem is left with a slice of no k at all
                kps, n = GC.slices(kmax, want)
                assert n < 2 or GC.empty_slices(c['probs'][short]['K'], kps, n) >= 1, (short, want)


def test_the_split_k_cases_as_the_why_states_them():
    c = GC.BY_ID['splitk64_mixed_vec_tt']
    assert [GC.tiles(p, c['tile']) for p in c['probs']] == [2, 1, 3]
    kps, n = GC.slices(2050, 6)
    assert (kps, n) == (352, 6) and [GC.empty_slices(p['K'], kps, n) for p in c['probs']] == [0, 5, 3]
    assert [p['N'] % 4 for p in c['probs']] == [0, 1, 2]
    probs = {k: GC.gemm_build(GC.BY_ID[f'splitk64_mixed_{k}_tt'], 'cpu', F32)[0][0] for k in GC.SPLIT64_P0}
    ok = lambda d: d['C'].data_ptr() % 16 == 0 and d['C'].stride(0) % 4 == 0 and d['bias'].data_ptr() % 16 == 0
    assert ok(probs['vec'])
    assert probs['bias_off']['bias'].data_ptr() % 16 == 4 and probs['bias_off']['C'].stride(0) % 4 == 0 and probs['bias_off']['C'].data_ptr() % 16 == 0
    assert probs['c_odd']['C'].stride(0) % 2 == 1 and probs['c_odd']['bias'].data_ptr() % 16 == 0
    assert any(p['bias'] and p['acc'] and p['act'] for p in c['probs'])
    for id, short_k, last in (('splitk128_xcd_mixed_x3_tt', 2064, 16), ('splitk128_xcd_mixed_fp32_tt', 2060, 12)):
        c = GC.BY_ID[id]
        assert [GC.tiles(p, c['tile']) for p in c['probs']] == [32, 32]
        kps, n = GC.slices(8192, 8)
        assert (kps, n) == (1024, 8) and n % 8 == 0 and GC.empty_slices(short_k, kps, n) == 5 and short_k - 2 * kps == last
        assert (short_k % 16 == 0) == bool(c['expect'][0] & GC.X3)
        assert all(p['M'] >= 96 and p['N'] >= 96 for p in c['probs'])


@pytest.mark.parametrize('c', [c for c in GC.CASES if c['expect'][0] & GC.KSPLIT], ids=lambda c: c['id'])
def test_k_split_cases_sit_on_the_side_of_the_row_threshold_they_state(c):
    assert not c['ws'] and not c['akm'] and max(p['K'] for p in c['probs']) >= 256
    t32 = sum(GC.tiles(p, (32, 64)) for p in c['probs'])
    t64 = sum(GC.tiles(p, (64, 64)) for p in c['probs'])
    if c['expect'][0] & GC.ROWS32:
        assert c['tile'] == (32, 64) and t32 <= 256
    else:
        lo, hi = c['tiles64_between']
        assert c['tile'] == (64, 64) and t32 > c['tiles32_above'] and lo <= t64 <= hi
        # what keeps the group out of the bf16x3 kernels is an operand or a K, not the group's size
        probs, _ = GC.gemm_build(c, 'cpu', F32)
        assert any(p['K'] % 32 for p in c['probs']) or not all(GC.operand_vec_ok(d['A']) and GC.operand_vec_ok(d['B']) for d in probs)
    assert any(GC.ceil_div(p['K'], GC.BK) == 1 for p in c['probs']) == c['id'].startswith('ks_single_ktile')


def test_grouped_rows_cross_a_group_boundary_inside_a_k_tile():
    for c in GC.CASES:
        if not c['id'].startswith('kg64'):
            continue
        probs, _ = GC.gemm_build(c, 'cpu', F32)
        grouped = [t for d in probs for t, km in ((d['A'], c['akm']), (d['B'], c['bkm'])) if km and t.dim() == 3]
        assert grouped and all(t.shape[1] < GC.BK and t.stride(0) != t.shape[1] * t.stride(1) for t in grouped)
        assert any(t.dim() == 2 for d in probs for t in (d['A'], d['B']))
        assert all(p['N'] < 96 for p in c['probs'][:1])
        whole = all(p['K'] % GC.BK == 0 for p in c['probs']) and all(GC.operand_vec_ok(d['A']) and GC.operand_vec_ok(d['B']) for d in probs)
        assert whole == c['id'].startswith('kg64_whole')


def test_batched_cases_have_several_tiles_per_entry_and_real_strides():
    for c in GC.CASES:
        if not c['id'].startswith('batched'):
            continue
        probs, _ = GC.gemm_build(c, 'cpu', F32)
        n, a_bs, b_bs, c_bs = probs[0]['batch']
        assert n == 3 and GC.tiles(dict(c['probs'][0], batch=None), c['tile']) == 6 and 'batch' not in probs[1]
        assert a_bs > 0 and b_bs > 0 and c_bs > probs[0]['C'].shape[0] * probs[0]['C'].stride(0)
        assert (b_bs % 2 == 1) == ('bodd' in c['id']) and a_bs % 4 == 0
