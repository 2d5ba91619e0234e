"""The general GEMM entry (twog_gemm_f32, csrc/gemm_f32.hip) at the edges that only a launch with SEVERAL problems, a split
reduction over problems of different length, or an operand off the 16-byte path reaches: case lists, seeded fp32 inputs and
gemm_run, which makes one Kx.gemm([...]) call per case. Shared by tests/test_gemm_general_cpu.py (the specification in fp32 against
fp64, and the arithmetic behind every case's `why`) and tests/test_gemm_general_gpu.py (HipKernels against both).

FakeKernels.gemm computes in the dtype it is given: its fp32 and fp64 runs on the same inputs are the s32 and s64 of
tests.entity_envelope.judge. Every C is a view inside a larger buffer pre-filled with SENTINEL (views that are not accumulated onto
hold it too: a tile that no workgroup writes stays 7.25); the buffer with the views zeroed comes back as EXACT.

A case: id, why (the branch it is there for, with the arithmetic that leads there), akm / bkm (A stored [K][M] / B stored [K][N]),
ws (split-K workspace handed over or not), probs, tile = (rows, columns) of the output tiles the launch cuts, expect = (bits, mask)
of gemm_last_class() after the call, and the claims the CPU test re-derives from the shapes: chunks, cls_mod8, vec, short, twice.

Launch structure the claims rest on (documented in csrc/gemm_f32.hip and include/twog_gcn.h): a call is worked off in chunks of
MAXP = 8 problems; a chunk's problems are sorted by K, longest first, problems of equal K form a class; k-tiles are BK = 32 deep;
tiles are 64 x 64, 32 x 64 (in-workgroup k-split at few rows, no workspace) or 128 x 128."""
import math

import torch

from tests.fake_kernels import FakeKernels
from tests.kernel_cases import rnd
from tests import stream_cases as SC

F = FakeKernels()
EXACT, JUDGE = 'exact', 'judge'
SENTINEL = 7.25
MAXP, BK = 8, 32

# bits of HipKernels.gemm_last_class() (TWOG_GEMM_CLASS_* of include/twog_gcn.h)
TILE128, WAVES8, KG, SPLITK, GATE, KSPLIT, GRUFWD, ROWS32, XSPLIT, X3, P3, P1 = (1 << i for i in range(12))
ALL = (1 << 12) - 1

LAYOUTS = {'nn': (False, False), 'nt': (False, True), 'tt': (True, True), 'tn': (True, False)}   # (akm, bkm)


def P(M, N, K, bias=False, act=0, acc=False, a='', b='', c='', bias_off=False, batch=None):
    """One problem. a / b: '' = a contiguous matrix; 'off1' = a column slice at offset 1 of a wider buffer with an odd leading
    dimension; ('kg', outer, inner, skip) = a 3-D [outer][inner][cols] view cut from [outer][inner + skip][cols + 8] at column 4
    (k-major operands only). c: '' = 16-byte aligned view with ld % 4 == 0, 'odd' = a view with an odd leading dimension.
    bias_off: the bias is the [1:] slice of a longer vector. batch = (n, 'even' | 'odd'): n entries; 'odd': B's batch stride is odd."""
    return dict(M=M, N=N, K=K, bias=bias or bias_off, act=act, acc=acc, a=a, b=b, c=c, bias_off=bias_off, batch=batch)


def _case(id, why, layout, probs, expect, ws=True, tile=(64, 64), **claims):
    akm, bkm = LAYOUTS[layout]
    return dict(id=f'{id}_{layout}', why=why, akm=akm, bkm=bkm, ws=ws, probs=probs, expect=expect, tile=tile, **claims)


# ------------------------------------------------------------------------------------------------------------ the cases
# 1. K classes and the XCD tile map
CLASSES3 = [P(70, 130, 40, bias=True), P(33, 65, 100, bias=True, act=1), P(64, 64, 8, acc=True), P(200, 96, 100), P(17, 5, 3, acc=True, bias=True)]
CLASSES3_WHY = ('five problems, caller order scrambled against K: sorted K = 100, 100, 40, 8, 3 -> four classes of 2 + 8, 6, 1, 1 tiles '
                'of 64 x 64; every remainder modulo 8 is non-zero, so the ring offsets cls_rot = 0, 2, 0, 1 all matter: 18 workgroups, '
                'XCD 0 and 1 work three tiles, the others two; no M or N reaches 96 in every problem -> 64 x 64, K < 256 -> plain kernel')
CASES = [_case('classes3_rot', CLASSES3_WHY, l, CLASSES3, (0, ALL), cls_mod8=[[2, 6, 1, 1]]) for l in LAYOUTS]

# 2. chunking past MAXP problems (the 17th is the longest: the last chunk has its own kmax, order and tile map)
CHUNKS19 = [
    P(1, 1, 1), P(80, 80, 32, bias=True, act=1), P(17, 33, 31, bias=True), P(64, 64, 33, acc=True), P(5, 70, 2), P(33, 9, 64, acc=True, bias=True),
    P(70, 3, 100), P(2, 2, 7, bias=True),
    P(40, 80, 96, acc=True), P(80, 1, 5, bias=True), P(1, 80, 64, bias=True, act=1), P(65, 65, 64), P(31, 32, 33, bias=True, act=1, acc=True),
    P(12, 77, 128), P(64, 1, 1, acc=True), P(7, 7, 32, bias=True),
    P(80, 80, 130, bias=True, act=1), P(3, 5, 31, acc=True), P(50, 20, 32)]
CASES += [_case('chunks_19', '19 problems -> chunks of 8 + 8 + 3, each sorted and mapped on its own; M, N from 1 to 80, K from 1 to 130 with '
                '31 / 32 / 33 around BK; (1, 1, 1); the second chunk has a class of two problems (K = 64: 2 + 4 tiles); the longest problem is '
                'the 17th, so the third chunk sorts it first; the class word is the last chunk\'s', l, CHUNKS19, (0, ALL),
                chunks=[8, 8, 3], cls_mod8=[[2, 1, 1, 4, 1, 1, 2, 1], [2, 2, 6, 1, 1, 2, 1], [4, 1, 1]]) for l in ('nn', 'tt')]

# 3. vec_ok per operand and per problem
VEC_MIX = [P(72, 40, 36, a='off1', bias=True), P(36, 72, 52, b='off1', act=1, bias=True), P(64, 64, 30, acc=True), P(3, 40, 20), P(40, 2, 24, bias=True)]
VEC_MIX_VEC = dict(nn=[(0, 1), (1, 0), (0, 0), (1, 1), (1, 1)], nt=[(0, 1), (1, 0), (0, 1), (1, 1), (1, 0)],
                   tt=[(0, 1), (1, 0), (1, 1), (0, 1), (1, 0)], tn=[(0, 1), (1, 0), (1, 0), (0, 1), (1, 1)])
CASES += [_case('vec_mix', 'a_vec and b_vec differ inside one launch: problem 0 has A off the 16-byte path (pointer + 4 bytes, odd ld), problem 1 '
                'has B there, problem 2 is aligned with K % 4 == 2 (scalar where K is the contiguous extent, 16-byte loads with a ragged '
                'last k-tile where it is not), problem 3 has M = 3 and problem 4 N = 2: contiguous extents below 4 in the k-major forms',
                l, VEC_MIX, (0, ALL), vec=VEC_MIX_VEC[l]) for l in LAYOUTS]
KS_MASK = KSPLIT | ROWS32 | X3 | TILE128 | SPLITK | XSPLIT | KG
VEC_KS32 = [P(72, 40, 288, a='off1', bias=True), P(36, 72, 256, b='off1', acc=True), P(64, 64, 100, bias=True, act=1)]
VEC_KS64 = [P(900, 384, 288, a='off1', bias=True), P(384, 448, 256, b='off1', acc=True), P(130, 100, 100, bias=True, act=1)]
for l in ('nn', 'nt'):
    CASES.append(_case('vec_mix_ks32', 'no workspace, row-major A, K = 288 / 256 / 100 (9 / 8 / 4 k-tiles), 9 tiles of 32 rows <= 256: the 32-row '
                       'in-workgroup k-split kernel with one operand of problems 0 and 1 on scalar loads', l, VEC_KS32, (KSPLIT | ROWS32, KS_MASK),
                       ws=False, tile=(32, 64), vec=[(0, 1), (1, 0), (1, 1)], short={2: 0, 1: 0}))
    CASES.append(_case('vec_mix_ks64', 'as vec_mix_ks32 with 268 tiles of 32 rows (> 256) = 138 tiles of 64 x 64 (<= 384, and >= 96: the bf16x3 kernels '
                       'would serve an aligned group): the unaligned operands and K = 100 switch them off for the WHOLE group -> the fp32 k-split kernel',
                       l, VEC_KS64, (KSPLIT, KS_MASK), ws=False, vec=[(0, 1), (1, 0), (1, 1)], short={2: 0, 1: 0}, tiles32_above=256,
                       tiles64_between=(96, 384)))

# 4. grouped k-major rows on the 64 x 64 tile
KG_MASK = KG | TILE128 | SPLITK | KSPLIT | X3
_kg = lambda inner: ('kg', 6, inner, 3)
CASES += [
    _case('kg64_ragged', 'k-major A and B are [6][20][cols] views of [6][23][cols + 8] buffers (rows = 120: 3 whole k-tiles + 24; inner = 20 '
          'puts a group boundary inside every k-tile) beside a problem with plain 2-D rows; N = 40 keeps the 64 x 64 class; K % 32 != 0 -> the '
          'guarded loads resolve (outer, inner) per row', 'tt', [P(72, 40, 120, a=_kg(20), b=_kg(20), bias=True, act=1), P(52, 36, 64, acc=True)],
          (KG, KG_MASK)),
    _case('kg64_whole', 'as kg64_ragged with rows = 6 x 16 = 96: whole k-tiles and aligned operands -> the branch-free kernel that carries one row '
          'pointer per pass from k-tile to k-tile (two groups per k-tile); the second problem runs through the same kernel with plain rows',
          'tt', [P(72, 40, 96, a=_kg(16), b=_kg(16), bias=True, act=1), P(52, 36, 64, acc=True)], (KG, KG_MASK)),
    _case('kg64_whole', 'only B grouped (row-major A)', 'nt', [P(72, 40, 96, b=_kg(16), acc=True, bias=True), P(52, 36, 64)], (KG, KG_MASK)),
    _case('kg64_whole', 'only A grouped (row-major B)', 'tn', [P(72, 40, 96, a=_kg(16), bias=True), P(52, 36, 64, bias=True, act=1)], (KG, KG_MASK)),
]

# 5. the in-workgroup k-split classes with a problem of a single k-tile
KS1 = [P(130, 200, 288, bias=True, act=1), P(33, 70, 256, acc=True), P(64, 64, 20, bias=True)]
KS1_BIG = [P(900, 384, 288, bias=True, act=1), P(384, 448, 256, acc=True), P(64, 64, 20, bias=True)]
for l in ('nn', 'nt'):
    CASES.append(_case('ks_single_ktile32', 'no workspace, row-major A, kmax = 288 >= 256, 26 tiles of 32 rows: the 32-row k-split kernel; problem 2 has '
                       'ONE k-tile (20 of its 32 k) where the others have 9 and 8, so most of what its second wave group multiplies is padding',
                       l, KS1, (KSPLIT | ROWS32, KS_MASK), ws=False, tile=(32, 64), short={2: 0, 1: 0}))
    CASES.append(_case('ks_single_ktile64', '260 tiles of 32 rows (> 256) = 133 of 64 x 64: the 64-row k-split class; every operand is aligned and the group is large '
                       'enough for the bf16x3 kernels, K = 20 is no multiple of 32 -> the fp32 k-split kernel for the whole group',
                       l, KS1_BIG, (KSPLIT, KS_MASK), ws=False, short={2: 0, 1: 0}, tiles32_above=256, tiles64_between=(96, 384)))

# 6. split-K over a 64 x 64 group that mixes K; the scalar branches of the reduction
SPLIT64_WHY = ('k-major A and B with workspace, 2 + 1 + 3 = 6 tiles, kmax = 2050 >= 1024: the split choice is 6 slices of 352 (the first count whose '
               '6 x s workgroups exceed 3 % of 1 024 slots); K = 300 then has FIVE slices with k_end <= k_begin and K = 1024 three, and their '
               'slabs must still be written as zeros (any split of 2 or more leaves K = 300 an empty slice); N = 37 and N = 130 take the scalar '
               'branch of the reduction; problem 2 has bias + accumulate + ReLU; problem 0 (N = 64) ')
SPLIT64_P0 = dict(vec=(P(96, 64, 2050, bias=True), 'is all aligned: the 16-byte branch of the reduction'),
                  bias_off=(P(96, 64, 2050, bias_off=True), 'has its bias 4 bytes off a 16-byte boundary: scalar branch with N % 4 == 0'),
                  c_odd=(P(96, 64, 2050, bias=True, c='odd'), 'writes a C view with an odd leading dimension: scalar branch with N % 4 == 0'))
CASES += [_case(f'splitk64_mixed_{k}', SPLIT64_WHY + w, 'tt', [p0, P(50, 37, 300, acc=True), P(64, 130, 1024, bias=True, acc=True, act=1)],
                (SPLITK, SPLITK | TILE128 | KG | KSPLIT | X3), short={1: 0, 2: 0}, twice=True) for k, (p0, w) in SPLIT64_P0.items()]

# 7. split-K dealt to XCDs (128 x 128 class) over a group that mixes K
SPLIT128_MASK = TILE128 | WAVES8 | X3 | SPLITK | KG | P3 | P1 | KSPLIT
CASES += [
    _case('splitk128_xcd_mixed_x3', 'k-major A and B with workspace, 2 x 32 = 64 tiles of 128 x 128, kmax = 8192: 8 slices of 1 024 dealt whole to the XCDs '
          '(xcd_split: (split, tile) recomputed from the linear workgroup index); K = 2064 = 2 x 1024 + 16 has two full slices, one of a single '
          '16-deep k-tile and FIVE empty ones whose slabs must be zeros; every K is a multiple of 16 -> bf16x3', 'tt',
          [P(512, 1024, 8192, bias=True), P(512, 1024, 2064, acc=True)], (TILE128 | WAVES8 | X3 | SPLITK, SPLIT128_MASK), tile=(128, 128),
          short={1: 0}, twice=True),
    _case('splitk128_xcd_mixed_fp32', 'as splitk128_xcd_mixed_x3 with K = 2060: no multiple of 16, so the whole group leaves the bf16x3 class for the native '
          'fp32 8-wave kernel; slice 2 of the short problem holds 12 k (guarded loads), five are empty', 'tt',
          [P(512, 1024, 8192, bias=True), P(512, 1024, 2060, acc=True)], (TILE128 | WAVES8 | SPLITK, SPLIT128_MASK), tile=(128, 128),
          short={1: 0}, twice=True),
]

# 8. a batched problem beside an unbatched one
BATCH_WHY = ('three batch entries of 2 x 3 = 6 tiles each (M = 70, N = 130) with non-zero strides for A, B and C, beside an unbatched problem of '
             'another K in the same launch: tile -> (entry, tile in entry)')
for l, vec, vec_odd in (('nn', [(1, 1), (1, 1)], [(1, 0), (1, 1)]), ('tn', [(0, 1), (0, 1)], [(0, 0), (0, 1)])):
    CASES.append(_case('batched_mixed', BATCH_WHY, l, [P(70, 130, 64, bias=True, act=1, batch=(3, 'even')), P(33, 40, 100, acc=True)], (0, ALL), vec=vec))
    CASES.append(_case('batched_mixed_bodd', BATCH_WHY + '; B\'s batch stride is odd: entries 1 and 2 start off the 16-byte grid -> scalar loads of B',
                       l, [P(70, 130, 64, bias=True, acc=True, batch=(3, 'odd')), P(33, 40, 100, bias=True)], (0, ALL), vec=vec_odd))

BY_ID = {c['id']: c for c in CASES}


# ------------------------------------------------------------------------------------------------- shape arithmetic
def ceil_div(a, b):
    return -(-a // b)


def tiles(p, tile):
    return (p['batch'][0] if p['batch'] else 1) * ceil_div(p['M'], tile[0]) * ceil_div(p['N'], tile[1])


def chunks_of(case):
    return [case['probs'][i:i + MAXP] for i in range(0, len(case['probs']), MAXP)]


def k_classes(chunk, tile):
    """[(K, tiles)] of a chunk, longest K first."""
    out = {}
    for p in chunk:
        out[p['K']] = out.get(p['K'], 0) + tiles(p, tile)
    return sorted(out.items(), reverse=True)


def slices(kmax, want):
    """(k per slice, slices) when a reduction of kmax is cut into `want` slices of whole k-tiles."""
    kps = ceil_div(ceil_div(kmax, want), BK) * BK
    return kps, ceil_div(kmax, kps)


def empty_slices(K, kps, n):
    return n - min(n, ceil_div(K, kps))


# ----------------------------------------------------------------------------------------------------------- inputs
def _operand(rows, cols, form, batch, seed, cv, scale):
    """-> (view of entry 0, batch stride in elements). rows x cols as stored."""
    if batch:
        n, kind = batch
        per = rows * cols + (1 if kind == 'odd' else 0)
        base = cv(rnd(n, per, seed=seed, scale=scale))
        return base[0, :rows * cols].view(rows, cols), per
    if form == 'off1':
        w = cols + (2 if cols % 2 else 3)   # odd
        return cv(rnd(rows, w, seed=seed, scale=scale))[:, 1:1 + cols], 0
    if form and form[0] == 'kg':
        _, outer, inner, skip = form
        assert outer * inner == rows
        return cv(rnd(outer, inner + skip, cols + 8, seed=seed, scale=scale))[:, skip:, 4:4 + cols], 0
    return cv(rnd(rows, cols, seed=seed, scale=scale)), 0


def _entry(t, off):
    return torch.as_strided(t, t.shape, t.stride(), t.storage_offset() + off)


def gemm_build(case, dev='cpu', dtype=torch.float32):
    """-> (the problem dicts of Kx.gemm, per problem (C buffer, [the C view of every batch entry]))."""
    cv = lambda t: t.to(dtype).to(dev)
    probs, book = [], []
    for i, p in enumerate(case['probs']):
        M, N, K, s = p['M'], p['N'], p['K'], 100 * i
        nb = p['batch'][0] if p['batch'] else 1
        A, a_bs = _operand(*((K, M) if case['akm'] else (M, K)), p['a'], p['batch'] and (nb, 'even'), s + 1, cv, 1.0)
        B, b_bs = _operand(*((K, N) if case['bkm'] else (N, K)), p['b'], p['batch'], s + 2, cv, 1.0)
        if p['c'] == 'odd':
            ld, c0 = N + (7 if N % 2 == 0 else 8), 3
        else:
            ld, c0 = ceil_div(N, 4) * 4 + 8, 4
        buf = torch.full((nb * (M + 2), ld), SENTINEL)
        if p['acc']:
            for e in range(nb):
                buf[e * (M + 2) + 1:e * (M + 2) + 1 + M, c0:c0 + N] = rnd(M, N, seed=s + 3 + e)
        buf = cv(buf)
        C, c_bs = buf[1:1 + M, c0:c0 + N], (M + 2) * ld
        bias = None
        if p['bias']:
            bias = cv(rnd(N + 1, seed=s + 9))[1:] if p['bias_off'] else cv(rnd(N, seed=s + 9))
        d = dict(A=A, B=B, C=C, bias=bias, act=p['act'], accumulate=p['acc'])
        if p['batch']:
            d['batch'] = (nb, a_bs, b_bs, c_bs)
        probs.append(d)
        book.append((buf, [_entry(C, e * c_bs) for e in range(nb)]))
    return probs, book


def gemm_outputs(book):
    """{C<i>: the written views (batch entries one below the other), JUDGE; around<i>: the buffer with the views zeroed, EXACT}"""
    out = {}
    for i, (buf, views) in enumerate(book):
        out[f'C{i}'] = (torch.cat([v.detach().clone() for v in views], 0).cpu(), JUDGE)
        around = buf.detach().clone()
        M, N = views[0].shape
        for v in views:
            off = v.storage_offset() - buf.storage_offset()
            r0, c0 = off // buf.stride(0), off % buf.stride(0)
            around[r0:r0 + M, c0:c0 + N] = 0
        out[f'around{i}'] = (around.cpu(), EXACT)
    return out


def gemm_run(Kx, case, dev='cpu', dtype=torch.float32):
    """One Kx.gemm call on the inputs of `case` cast to dtype on dev -> {name: (tensor on the CPU, JUDGE | EXACT)} per problem."""
    probs, book = gemm_build(case, dev, dtype)
    Kx.gemm(probs, a_kmajor=case['akm'], b_kmajor=case['bkm'], split_k_workspace=case['ws'])
    return gemm_outputs(book)


def operand_vec_ok(t, batch_stride=0):
    """vec_ok of csrc/gemm_f32.hip for an operand view as gemm_build passes it (its last dimension is the contiguous extent)."""
    return int(SC.vec_ok(t) and batch_stride % 4 == 0)


def longest_sum(case):
    return max(p['K'] for p in case['probs']) + 2   # products + bias + previous C
