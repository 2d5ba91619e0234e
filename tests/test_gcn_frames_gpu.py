"""GPU: the geometric-level GCN kernels (csrc/geo_fused.hip, geo_attn_mfma.hip, geo_gcn.hip) at batch-sized frame counts. Every
one of them is launched with a capped grid and walks the frames; the first test proves from the library's own launch plan
(HipKernels.gcn_launch_plan) that the cases of tests/gcn_frames.py make those loops turn. Every output of every case is judged
against the specification run in fp64 with the fp32 specification's own error as the yardstick, tensor-wide and per row
(tests/gcn_frames.py: R1, R2); every call runs twice and must be bit-identical; output buffers carry canary rows behind the last
frame; frames do not leak into each other, also not a non-finite one into another clip.

TWOG_GCN_FRAMES_RECORD=<file>: e_hip, e_ref, the factor needed tensor-wide, the worst row over the specification's worst row and
the R2 share of every (case, tensor) are written there as JSON (profiles/r08_gcn_frames_fp64.json is such a record)."""
import json
import os

import pytest
import torch

import twog_gcn_amd  # noqa: F401
from twog_gcn_amd import kernels as twog_kernels
from tests import gcn_frames as GF
from tests.entity_envelope import EPS

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
RECORDS = {}
CANARY = -12345.0
NODE_COUNTS = (1, 16, 19, 34, 50, 64)


@pytest.fixture(scope='module')
def K():
    twog_kernels._set_backend_for_tests(None)
    k = twog_kernels.get_kernels()
    assert k.name == 'hip'
    yield k
    dst = os.environ.get('TWOG_GCN_FRAMES_RECORD')
    if dst and RECORDS:
        fin = lambda v: (float(f'{v:.4g}') if v == v and abs(v) != float('inf') else str(v)) if isinstance(v, float) else v
        with open(dst, 'w') as f:
            json.dump({k_: {a: fin(b) for a, b in r.items()} for k_, r in sorted(RECORDS.items())}, f, indent=0)


# --------------------------------------------------------------------------------------------- the case list against the plan
def _plans(K, c):
    N, nF = c['N'], c['frames']
    names = ('fused', 'attn2_fwd', 'attn2_bwd', 'embed1_fwd', 'attn_fwd', 'attn_bwd')
    ids = (K.PLAN_FUSED_FWD, K.PLAN_ATTN2_FWD, K.PLAN_ATTN2_BWD, K.PLAN_EMBED1_FWD, K.PLAN_ATTN_FWD, K.PLAN_ATTN_BWD)
    return {n: K.gcn_launch_plan(i, nF, N) for n, i in zip(names, ids)}


def _turns(K, c):
    """Which loops of which kernel make a second trip in case c, from the launch plan and the two block-count methods."""
    N, nF, T = c['N'], c['frames'], c['T']
    pl = _plans(K, c)
    grid, FG, lds, NT = pl['fused']
    groups = -(-nF // FG)
    last_wg_ran_a_full_group = groups > grid and (groups - 1) % grid < groups - 1   # its earlier groups are never the last: full
    nblk, per = K.bn_stats_blocks(nF), -(-nF // K.bn_stats_blocks(nF))
    rows = nF * N
    return dict(
        FG=FG, NT=NT, with_m=pl['attn2_bwd'][3], lds=lds,
        fused_second_trip=groups > grid,
        fused_ragged_last_group_after_a_full_one=nF % FG != 0 and last_wg_ran_a_full_group,
        fused_trips=-(-groups // grid),
        groups_straddle_clips=T % FG != 0 and c['bs'] > 1,
        attn2_bwd_second_trip_ragged=nF > pl['attn2_bwd'][0] and nF % pl['attn2_bwd'][0] != 0,
        attn2_fwd_second_trip=nF > pl['attn2_fwd'][0],
        attn_second_trip=nF > pl['attn_fwd'][0] and nF > pl['attn_bwd'][0],
        stats_blocks_at_cap=nF // 8 > nblk,
        stats_finalize_in_flight_loop=nblk > 28 + 3,          # bn_finalize_kernel: lane p enters `b + 28 < n_blocks` from b = p <= 3
        stats_empty_trailing_block=nblk * per > nF + per,
        stats_unrolled_loop_with_remainder=per >= 8 and per % 4 != 0 and nF % 4 != 0,
        embed1_fwd_second_trip=rows > 4 * pl['embed1_fwd'][0],
        embed1_bwd_at_cap=(rows + 31) // 32 > K.embed1_bwd_blocks(rows),
        embed1_bwd_many_partials_below_cap=20 < K.embed1_bwd_blocks(rows) == (rows + 31) // 32 and rows > 16384,
    )


def test_case_list_makes_every_loop_turn(K):
    """No launch: the properties the case list was written for, from the library's launch plan. Fails when a grid cap is raised
    (or a group size changes) so that the cases silently become single-trip launches again."""
    t = {c['id']: _turns(K, c) for c in GF.CASES}
    big = {c['N']: t[c['id']] for c in GF.BIG}
    assert sorted(big) == list(NODE_COUNTS) and sorted(c['N'] for c in GF.SHARP) == list(NODE_COUNTS)
    per_n = ('fused_second_trip', 'fused_ragged_last_group_after_a_full_one', 'groups_straddle_clips', 'attn2_bwd_second_trip_ragged',
             'attn2_fwd_second_trip', 'attn_second_trip', 'stats_blocks_at_cap', 'stats_finalize_in_flight_loop',
             'stats_empty_trailing_block', 'stats_unrolled_loop_with_remainder')
    for N, r in big.items():
        for k in per_n:
            assert r[k], f'N = {N}: the batch-sized case does not reach: {k} ({r})'
        assert r['NT'] == (N + 15) // 16 and r['with_m'] == (1 if N <= 48 else 0), (N, r)
        assert r['lds'] <= 160 * 1024
    assert {r['NT'] for r in big.values()} == {1, 2, 3, 4} and {r['with_m'] for r in big.values()} == {0, 1}
    assert {N: r['FG'] for N, r in big.items()} == {1: 8, 16: 8, 19: 8, 34: 8, 50: 6, 64: 4}   # DESIGN.md section 4.4 says so
    assert any(r['embed1_fwd_second_trip'] for r in t.values())
    assert any(r['embed1_bwd_at_cap'] for r in t.values()) and any(r['embed1_bwd_many_partials_below_cap'] for r in t.values())
    bench = t[GF.BENCH[0]['id']]
    assert bench['fused_trips'] >= 3 and bench['attn2_bwd_second_trip_ragged'] is False   # 7 680 = 30 x 256: whole trips only
    # the small ones stay covered
    small = {c['id']: (c, t[c['id']]) for c in GF.SMALL}
    assert any(c['frames'] == 1 for c, _ in small.values())
    for fg in (8, 6, 4):
        assert any(r['FG'] == fg and c['frames'] == fg for c, r in small.values()), f'no case of exactly one group of {fg}'
    assert any(1 < c['frames'] < r['FG'] for c, r in small.values())
    p256 = [K.gcn_launch_plan(K.PLAN_ATTN2_BWD, n, 34)[0] for n in (256, 257)]
    assert p256 == [256, 256] and any(c['frames'] == 256 for c, _ in small.values())
    assert sum(c['frames'] == 257 for c, _ in small.values()) == 2 and {r['with_m'] for c, r in small.values() if c['frames'] == 257} == {0, 1}
    assert {c['H'] for c in GF.CASES} == {1, 2, 3}
    assert all(any(c['N'] == N and c['reduced'] for c in GF.BIG) for N in (1, 19, 34, 64))


def test_node_counts_out_of_range_are_refused_before_any_launch(K):
    lib, st = K.lib, K._stream()
    out = (twog_kernels.C.c_int * 4)()
    for n in (lib.twog_gcn_max_nodes() + 1, 0):
        assert lib.twog_gcn_fused_fwd(None, 0, 8, n, None, None, None, None, None, None, None, None, None, st) < 0
        assert lib.twog_gcn_embed1_fwd(None, 0, 8, n, None, None, None, None, st) < 0
        assert lib.twog_gcn_embed1_bwd(None, 0, 8, n, None, None, None, None, None, 1, None, None, None, None, st) < 0
        assert lib.twog_gcn_attn2_bwd(None, None, None, None, 8, n, None, None, 8, st) < 0
        assert lib.twog_gcn_attn_fwd(None, None, 8, n, None, None, st) < 0
        assert lib.twog_gcn_attn_bwd(None, None, None, None, 8, n, None, None, st) < 0
        assert lib.twog_bn_finalize(None, 1, 8, n, None, None, None, None, None, 1, None, None, None, None, None, None, st) < 0
        for kernel in range(6):
            assert lib.twog_gcn_launch_plan(kernel, 8, n, out) == -1
    assert lib.twog_gcn_launch_plan(6, 8, 34, out) < 0
    torch.cuda.synchronize()
    assert float((torch.ones(4, device=DEV) + 1).sum()) == 8.0


# ------------------------------------------------------------------------------------------------------------ the judgement
class Verdict:
    """Collects the judgement of every tensor of one case: all of them are measured (and recorded) before the case fails."""

    def __init__(self, c):
        self.c, self.fails, self.worst, self.worst_row, self.share = c, [], (0.0, ''), (0.0, ''), (0.0, '')

    def add(self, name, hip, s32, s64):
        rec, fails = GF.judge_named(self.c, name, hip, s32[name], s64[name])
        RECORDS[f"{self.c['id']}/{name}"] = rec
        self.fails += [f'{name}: {f}' for f in fails]
        self.worst, self.worst_row = max(self.worst, (rec['ratio'], name)), max(self.worst_row, (rec['r1_ratio'], name))
        if rec['rows'] >= GF.R2_MIN_ROWS:
            self.share = max(self.share, (rec['r2_share'], name))

    def same(self, name, a, b):
        if not torch.equal(a, b):
            self.fails.append(f'{name}: two runs of the same call differ')

    def canary(self, name, buf, n):
        if not bool((buf.reshape(-1)[n:] == CANARY).all()):
            self.fails.append(f'{name}: written behind the last frame')

    def check(self):
        print(f"{self.c['id']}: worst e_hip / e_ref {self.worst[0]:.2f} ({self.worst[1]}), worst row / the specification's worst row "
              f'{self.worst_row[0]:.2f} ({self.worst_row[1]}), largest R2 share {100 * self.share[0]:.4f} % ({self.share[1]})')
        assert not self.fails, f"{self.c['id']}:\n  " + '\n  '.join(self.fails)


def _buf(n, extra):
    return torch.full((n + extra,), CANARY, dtype=torch.float32, device=DEV)


def _adjacency_structure(V, name, adj, N):
    a = adj.detach().cpu().double().reshape(-1, N)
    if not torch.isfinite(a).all():
        V.fails.append(f'{name}: non-finite weights')
    elif float((a.sum(1) - 1.0).abs().max()) > 4 * EPS * N:
        V.fails.append(f'{name}: a row sums to 1 {float((a.sum(1) - 1.0).abs().max()):.2e} off (> 4 ulp x {N})')


@pytest.mark.parametrize('c', GF.CASES, ids=lambda c: c['id'])
def test_gcn_kernels_at_batch_sized_frame_counts(K, c):
    """bn_fold (both modes, with the fold), gcn_fused_fwd (with and without save_x), gcn_embed1_fwd, gcn_attn2_bwd, gcn_embed1_bwd; on
    the reduced list also gcn_attn2_fwd and the two-projection attention kernels."""
    p, s32, s64 = GF.spec(c)
    N, nF = c['N'], c['frames']
    rows = nF * N
    V = Verdict(c)
    g = lambda t: t.to(DEV)
    xh = g(p['xh'])
    for training in (True, False):
        tag = 'train_' if training else 'eval_'
        r, r2 = GF.run_bn(K, c, p, xh, training, dev=DEV), GF.run_bn(K, c, p, xh, training, dev=DEV)
        for k in r:
            if k == 'nbt':
                assert int(r[k]) == int(s32[tag + k]) == int(r2[k])
                continue
            V.add(tag + k, r[k], s32, s64)
            V.same(tag + k, r[k], r2[k])
    # every kernel is given the fp32 specification's operands, as the fp64 specification is
    ab, mi, md = (g(s32[c['fold'] + k]) for k in ('ab', 'mi', 'md'))
    w1, b1, w2, b2 = (g(p[k]) for k in ('w1', 'b1', 'w2', 'b2'))
    ptr, fstride, nf_ = K._geo(xh)
    assert nf_ == nF
    # ---- fused forward: into buffers with two frames of canary rows behind the last frame, then through HipKernels twice
    Xb, adjb, Zb = _buf(rows * 64, 2 * N * 64), _buf(rows * N, 2 * N * N), _buf(rows * 64, 2 * N * 64)
    K._check(K.lib.twog_gcn_fused_fwd(ptr, fstride, nF, N, ab.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(),
                                      md.data_ptr(), Xb.data_ptr(), adjb.data_ptr(), Zb.data_ptr(), K._stream()), 'twog_gcn_fused_fwd')
    X, adj, Z = K.gcn_fused_fwd(xh, N, ab, w1, b1, w2, b2, md)
    Xn, adjn, Zn = K.gcn_fused_fwd(xh, N, ab, w1, b1, w2, b2, md, save_x=False)
    assert Xn is None
    for name, t, buf, tn in (('X', X, Xb, X), ('adj', adj, adjb, adjn), ('Z', Z, Zb, Zn)):
        V.add(name, t, s32, s64)
        V.canary(name, buf, t.numel())
        V.same(name, t.reshape(-1), buf[:t.numel()])
        V.same(name + ' (save_x=False)', t, tn)
    _adjacency_structure(V, 'adj', adj, N)
    # ---- embed1 forward; the e1 the backward pass recomputes is what the fused kernel multiplied: X = relu(e1 W2^T + b2)
    e1b = _buf(rows * 64, 2 * N * 64)
    K._check(K.lib.twog_gcn_embed1_fwd(ptr, fstride, nF, N, ab.data_ptr(), w1.data_ptr(), b1.data_ptr(), e1b.data_ptr(), K._stream()),
             'twog_gcn_embed1_fwd')
    e1 = K.gcn_embed1_fwd(xh, N, ab, w1, b1)
    V.add('e1', e1, s32, s64)
    V.canary('e1', e1b, rows * 64)
    V.same('e1', e1.reshape(-1), e1b[:rows * 64])
    want = torch.relu(e1.double() @ w2.double().t() + b2.double())
    err, tol = float((X.double() - want).abs().max()), 1e-5 + 2e-5 * float(want.abs().max())
    if err > tol:
        V.fails.append(f'fused X vs embed1 + fp64 GEMM: {err:.3e} > {tol:.3e}')
    # ---- attention backward on the specification's saved X and adjacency
    Xs, adjs, dz = g(s32['X']), g(s32['adj']), g(p['dz'])
    nblk = K.lib.twog_gcn_attn2_bwd_blocks(nF)
    dxb, part = _buf(rows * 64, 2 * N * 64), _buf(nblk * 65 * 64, 65 * 64)
    K._check(K.lib.twog_gcn_attn2_bwd(Xs.data_ptr(), md.data_ptr(), adjs.data_ptr(), dz.data_ptr(), nF, N, dxb.data_ptr(),
                                      part.data_ptr(), nblk, K._stream()), 'twog_gcn_attn2_bwd')
    dX, dmd = K.gcn_attn2_bwd(Xs, md, adjs, dz, nF, N)
    V.add('dX', dX, s32, s64)
    V.add('dmd', dmd, s32, s64)
    V.canary('dX', dxb, rows * 64)
    V.canary('attn2 backward partials', part, nblk * 65 * 64)
    V.same('dX', dX.reshape(-1), dxb[:rows * 64])
    V.same('dmd', dmd, K.colsum(part[:nblk * 65 * 64].view(nblk, 65 * 64)).view(65, 64))
    # ---- embedding backward
    de1 = g(p['de1m'])
    r, r2 = (K.gcn_embed1_bwd(xh, N, ab, mi, w1, de1) for _ in range(2))
    for k, a, b in zip(('dw1', 'db1', 'dgamma', 'dbeta'), r, r2):
        V.add(k, a, s32, s64)
        V.same(k, a, b)
    # ---- the kernels that are in the ABI but not on the production path
    if c['reduced']:
        for name, fn in (('2', lambda: K.gcn_attn2_fwd(Xs, md, nF, N)), ('q', lambda: K.gcn_attn_fwd(g(p['qk']), Xs, nF, N))):
            (a, z), (a2, z2) = fn(), fn()
            V.add('adj' + name, a, s32, s64)
            V.add('Z' + name, z, s32, s64)
            V.same('adj' + name, a, a2)
            V.same('Z' + name, z, z2)
            _adjacency_structure(V, 'adj' + name, a, N)
        qk, sq = g(p['qk']), g(s32['adjq'])
        (dxq, dqk), (dxq2, dqk2) = (K.gcn_attn_bwd(qk, Xs, sq, dz, nF, N) for _ in range(2))
        V.add('dXq', dxq, s32, s64)
        V.add('dqk', dqk, s32, s64)
        V.same('dXq', dxq, dxq2)
        V.same('dqk', dqk, dqk2)
    torch.cuda.synchronize()
    V.check()


# ----------------------------------------------------------------------------------------------------- frame independence
def _fused(K, c, p, s32, xh, fold):
    g = lambda t: t.to(DEV)
    return K.gcn_fused_fwd(g(xh), c['N'], g(s32[fold + 'ab']), g(p['w1']), g(p['b1']), g(p['w2']), g(p['b2']), g(s32[fold + 'md']))


def _frames_that_differ(a, b, nF):
    return torch.nonzero((a.reshape(nF, -1) != b.reshape(nF, -1)).any(1) | (torch.isnan(a.reshape(nF, -1)).any(1))).flatten().tolist()


@pytest.mark.parametrize('c', GF.BIG, ids=lambda c: c['id'])
def test_a_frame_changes_only_its_own_rows(K, c):
    """With ab fixed, another geometry in one frame -- the first frame of a group, a frame in the middle of a group, both in
    groups a workgroup takes on its second trip -- leaves every row of X, adjacency and Z of every other frame bit-identical."""
    p, s32, _ = GF.spec(c)
    nF = c['frames']
    grid, FG, _, _ = K.gcn_launch_plan(K.PLAN_FUSED_FWD, nF, c['N'])
    clean = _fused(K, c, p, s32, p['xh'], c['fold'])
    for f in ((grid + 3) * FG, (grid + 4) * FG + FG // 2, FG - 1):
        assert f < nF
        xh = p['xh'].clone()
        xh.view(nF, c['H'], -1)[f, 0, 2048:] += 0.5
        got = _fused(K, c, p, s32, xh, c['fold'])
        for name, a, b in zip(('X', 'adjacency', 'Z'), got, clean):
            diff = _frames_that_differ(a, b, nF)
            ok = diff == [f] or (c['N'] == 1 and name != 'X' and diff in ([], [f]))   # one node: the weight is 1 whatever the geometry
            assert ok, f'{name}: the geometry of frame {f} changed the frames {diff[:8]}'


@pytest.mark.parametrize('c', [c for c in GF.BIG if c['N'] in (1, 19, 34, 50)], ids=lambda c: c['id'])
def test_a_non_finite_frame_stays_inside_its_clip(K, c):
    """Inference mode (running statistics), one +inf coordinate in the first frame of a clip that is not the first frame of its
    group: the frames of the OTHER clips are bit-identical to the clean run, as in the reference, which computes frame by frame.
    (The aggregation Z = S X_f runs k up to N rounded up to 16, over rows of the NEXT frame: their weights are exact zeros, and
    0 x inf must not reach the previous frame's Z.) What the non-finite frame does to its own clip is not specified."""
    p, s32, _ = GF.spec(c)
    nF, T, N = c['frames'], c['T'], c['N']
    _, FG, _, _ = K.gcn_launch_plan(K.PLAN_FUSED_FWD, nF, N)
    clip = 3
    f = clip * T
    assert f % FG != 0 and T % FG != 0     # the group of frame f starts in the previous clip
    # (with weights of both signs the +inf never reaches X: inf - inf = NaN in the 64-term sums and the kernel's relu, fmaxf(NaN, 0),
    # is 0. Here every hidden unit sees the coordinate with a positive weight and W2 >= 0, so X of that node is +inf.)
    p = dict(p, w1=torch.cat([p['w1'][:, :1], p['w1'][:, 1:2].abs() + 0.1, p['w1'][:, 2:]], 1), w2=p['w2'].abs())
    clean = _fused(K, c, p, s32, p['xh'], 'eval_')
    assert all(torch.isfinite(t).all() for t in clean)
    xh = p['xh'].clone()
    xh.view(nF, c['H'], -1)[f, 0, 2048 + 4 * min(5, N - 1) + 1] = float('inf')
    got = _fused(K, c, p, s32, xh, 'eval_')
    assert not torch.isfinite(got[0].view(nF, -1)[f]).all(), 'the +inf coordinate did not reach X: the test perturbs nothing'
    for name, a, b in zip(('X', 'adjacency', 'Z'), got, clean):
        bad = [i for i in _frames_that_differ(a, b, nF) if i // T != clip]
        assert not bad, f'{name}: a non-finite frame of clip {clip} (frame {f}) changed frames of other clips: {bad[:8]}'
