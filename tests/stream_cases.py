"""The small streaming kernels of every training step (csrc/gate.hip, misc.hip, posfeat.hip, ssp.hip): case lists, seeded
inputs, and the executable specification (tests/fake_kernels.py) run on them. Shared by tests/test_stream_kernels_cpu.py (the
specification in fp32 against itself in fp64, and what the case list reaches) and tests/test_stream_kernels_gpu.py (the HIP
kernels against both).

Every `*_run(Kx, c, dev, dtype)` builds the inputs of case c as seeded fp32 tensors, casts them to dtype on dev, calls the
methods of Kx (FakeKernels on the CPU in fp32 / fp64, HipKernels on the GPU in fp32: all three see identical values) and returns
{name: (tensor, how)}: how = EXACT -> the HIP result must be bit-equal to the fp32 specification (copies, selections, single
fp32 additions, untouched memory around a written view); JUDGE -> tests.entity_envelope.judge, against the fp64 run with the
fp32 run's own error as the yardstick. Tensors of one value per (clip, frame, entity) are returned flat: their rows of E values
are no unit a kernel works in, so the row-wise half of the rule coincides with the tensor-wide one there.

The `why` of a case names the branch it is there for; HipKernels.stream_grid / FakeKernels.stream_grid and vec_ok() below (the
host-side conditions of the launchers) let the tests prove that it is reached; stream_grid is the library's launch-free plan on
both, no cap is written down here."""
import functools

import torch

from tests.fake_kernels import FakeKernels
from tests.kernel_cases import rnd
from twog_gcn_amd.kernels import rows_of

F = FakeKernels()
EXACT, JUDGE = 'exact', 'judge'
f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))   # a hyper-parameter as the value the C ABI (float) receives


def cv(t, dev, dtype):
    if t is None:
        return None
    return t.to(dev, dtype if t.is_floating_point() else t.dtype, copy=True)   # always a copy: the cached inputs stay as they are


def vec_ok(t):
    """The launchers' condition for the 16-byte kernels (rows_vec_ok of misc.hip, the same test in gate.hip): columns a multiple
    of 4, 16-byte aligned pointer, leading dimensions multiples of 4."""
    if t.dtype != torch.float32:   # the fp64 run of the specification: the same question in elements
        return t.shape[-1] % 4 == 0 and t.data_ptr() % (4 * t.element_size()) == 0 and all(s % 4 == 0 for s in t.stride()[:-1])
    r = rows_of(t)
    return t.shape[-1] % 4 == 0 and (r.ptr or 0) % 16 == 0 and r.ld_outer % 4 == 0 and (r.inner <= 1 or r.ld_inner % 4 == 0)


def block(base, c0, cols):
    return base[:, c0:c0 + cols]


def outside(base, c0, cols):
    """base with the column block zeroed: what a call that writes the block must leave as it was."""
    b = base.detach().clone()
    b[:, c0:c0 + cols] = 0
    return b


STREAM_SLACK = {1: 0, 4: 3, 16: 30}   # by items per thread and trip


def second_trip(Kx, plan):
    """plan = (STREAM_* name, work, items per thread and trip) -> (what one trip of the launch covers, the work that is sure to
    reach the strided main loop): a thread of that loop makes a second trip when the first is smaller (the sufficient condition
    of include/twog_gcn.h: the loops over whole groups of four leave out up to 3 items, the 16-byte body of fill_zero up to 15
    head bytes and 15 behind). The grid is the library's own answer (twog_stream_grid)."""
    name, work, per = plan
    return Kx.stream_grid(getattr(Kx, name), work) * Kx.STREAM_THREADS * per, work - STREAM_SLACK[per]


# ---------------------------------------------------------------------------------------------------------------- gates
def _g(id, bs, T, E, hidden, n_seg, bias, noise, noise_offset, force_last, thr, c0, seed, why, logit_scale=2.0):
    return dict(id=id, bs=bs, T=T, E=E, hidden=hidden, n_seg=n_seg, bias=bias, noise=noise, noise_offset=noise_offset,
                force_last=force_last, thr=thr, c0=c0, seed=seed, why=why, logit_scale=logit_scale)


GATE_CASES = [
    _g('h32_s5_rows72', 3, 6, 4, 32, 5, True, True, 2, 1, 0.5, 0, 1, 'half a wave per block of columns; rows % 4 == 0'),
    _g('h64_s1_rows105', 3, 7, 5, 64, 1, False, False, 0, 0, 0.3, 0, 2, 'rows % 4 == 1; one segment; b = None; no noise'),
    _g('h72_s5_rows70_view', 2, 7, 5, 72, 5, True, True, 0, 1, 0.3, 3, 3,
       'rows % 4 == 2; ragged second trip of the lane loop; x a column block of wider rows at an odd offset'),
    _g('h512_s8_rows75', 3, 5, 5, 512, 8, True, True, 2, 0, 0.5, 0, 4,
       'rows % 4 == 3; the product width: 8 trips of the lane loop per segment, w + s * hidden far from w + s * 64'),
    _g('h64_s8_rows3_nonoise', 1, 1, 3, 64, 8, True, False, 0, 1, 0.5, 4, 5, 'fewer rows than waves of one block; T = 1 is the last step'),
]
GATE_SATURATED = _g('saturated_h32_s5', 3, 6, 4, 32, 5, True, True, 2, 1, 0.5, 0, 6,
                    '|logit| > 20: p rounds to 0 or 1 in fp32 (judged against the fp32 specification only)', logit_scale=40.0)
HARD_MARGIN = 1e-4   # |soft64 - threshold| below which a hard decision is not compared (the margin of the omnibus test)


def _gumbel(*shape, seed):
    u = torch.rand(*shape, generator=torch.Generator().manual_seed(seed)).clamp(1e-6, 1 - 1e-6)
    return -torch.log(-torch.log(u))


@functools.lru_cache(maxsize=None)
def gate_inputs(id):
    c = next(k for k in GATE_CASES + [GATE_SATURATED] if k['id'] == id)
    bs, T, E, h, S, sd = c['bs'], c['T'], c['E'], c['hidden'], c['n_seg'], 100 * c['seed']
    rows, W = bs * T * E, (c['n_seg'] + 1) * c['hidden']      # one block of the rows belongs to no segment
    wide = rnd(rows, W + 8, seed=sd, scale=0.5)
    order = torch.randperm(S + 1, generator=torch.Generator().manual_seed(sd)).tolist()[:S]
    nE = E + c['noise_offset'] + 1
    return dict(wide=wide, seg_col=[o * h for o in order], w=rnd(1, S * h, seed=sd + 1, scale=c['logit_scale'] / (0.5 * (S * h) ** 0.5)),
                b=rnd(1, seed=sd + 2) if c['bias'] else None, noise_entities=nE,
                noise=_gumbel(T * nE, bs, 2, seed=sd + 6) if c['noise'] else None,
                d_hard=rnd(bs, T, E, seed=sd + 3), d_soft=rnd(bs, T, E, seed=sd + 4), st_mask=(rnd(bs, T, E, seed=sd + 5) > 0).float())


def gate_desc(c, dev, dtype):
    i = gate_inputs(c['id'])
    W = (c['n_seg'] + 1) * c['hidden']
    return dict(x=block(cv(i['wide'], dev, dtype), c['c0'], W), seg_col=i['seg_col'], hidden=c['hidden'], w=cv(i['w'], dev, dtype),
                b=cv(i['b'], dev, dtype), noise=cv(i['noise'], dev, dtype), bs=c['bs'], T=c['T'], E=c['E'],
                noise_entities=i['noise_entities'], noise_offset=c['noise_offset'], force_last=c['force_last'], threshold=c['thr'])


def gate_run(Kx, c, dev, dtype, saved=None):
    """Forward, then the backward pass on the saved p / soft of `saved` (the fp32 specification's: isolates the backward kernel)."""
    i, d = gate_inputs(c['id']), gate_desc(c, dev, dtype)
    Kx.gate_fwd(d)
    out = {k: (d[k].reshape(-1), JUDGE) for k in ('soft', 'p_save')}
    out['hard'] = (d['hard'].reshape(-1), None)   # compared by the tests, outside the margin
    if saved is not None:
        d['p_save'], d['soft'] = (cv(saved[k][0].reshape(c['bs'], c['T'], c['E']), dev, dtype) for k in ('p_save', 'soft'))
    dh, ds, sm = (cv(i[k], dev, dtype) for k in ('d_hard', 'd_soft', 'st_mask'))
    out['dlogit'] = (Kx.gate_bwd(d, dh, ds, sm), JUDGE)
    out['dlogit_hard_only'] = (Kx.gate_bwd(d, dh, None, None), JUDGE)
    out['dlogit_soft_only'] = (Kx.gate_bwd(d, None, ds, None), JUDGE)
    return out


def hard_comparable(c, soft64):
    return (soft64.double() - c['thr']).abs() > HARD_MARGIN


# ---------------------------------------------------------------------------------------------------------- column sums
def _cs(id, rows, cols, ld, c0, scaled, acc, vec, why):
    return dict(id=id, rows=rows, cols=cols, ld=ld, c0=c0, scaled=scaled, acc=acc, vec=vec, why=why)


COLSUM_CASES = [
    _cs('c33_r17', 17, 33, 33, 0, True, False, False, 'not vectorised: cols % 4 != 0; a ragged last pass over the 4 row lanes'),
    _cs('c36_ld37_r4', 4, 36, 37, 0, False, False, False, 'not vectorised: ld % 4 != 0; one row per row lane'),
    _cs('c64_ptr1_r3', 3, 64, 68, 1, True, True, False, 'not vectorised: pointer one float off; rows < 4: an idle row lane'),
    _cs('c8_r0', 0, 8, 8, 0, False, False, True, 'rows = 0: the sum is 0'),
    _cs('c8_r0_acc', 0, 8, 8, 0, False, True, True, 'rows = 0, accumulate: out stays'),
    _cs('c8_r1', 1, 8, 8, 0, True, False, True, 'rows = 1: three idle row lanes'),
    _cs('c12_r3', 3, 12, 16, 4, False, True, True, 'rows < 4, vectorised view'),
    _cs('c260_r197_vec', 197, 260, 264, 0, True, True, True,
        'two 256-column blocks, the second with one quad; 3 row slices of 66 rows: the 16-row loop and its remainder; accumulate over > 256 columns'),
    _cs('c260_r197_scalar', 197, 260, 264, 1, True, True, False, 'five 64-column blocks, not vectorised; 3 row slices; accumulate'),
    _cs('c516_r197_vec', 197, 516, 520, 4, False, False, True, 'three 256-column blocks; a view at a 16-byte offset'),
    _cs('c516_ld517_r17', 17, 516, 517, 0, False, True, False, 'nine 64-column blocks, not vectorised (ld % 4 != 0); accumulate'),
    _cs('c48_r64', 64, 48, 48, 0, False, False, True, 'exactly 64 rows: the 16-row loop with no remainder'),
]


@functools.lru_cache(maxsize=None)
def colsum_inputs(id):
    c = next(k for k in COLSUM_CASES if k['id'] == id)
    sd = 7 * COLSUM_CASES.index(c) + 300
    return dict(base=rnd(c['rows'], c['ld'], seed=sd), rs=rnd(c['rows'], seed=sd + 1) if c['scaled'] else None,
                out0=rnd(c['cols'], seed=sd + 2))


def colsum_problem(c, dev, dtype):
    i = colsum_inputs(c['id'])
    return block(cv(i['base'], dev, dtype), c['c0'], c['cols']), cv(i['rs'], dev, dtype), cv(i['out0'], dev, dtype), c['acc']


def colsum_run(Kx, c, dev, dtype):
    x, rs, out, acc = colsum_problem(c, dev, dtype)
    return dict(out=(Kx.colsum(x, rowscale=rs, out=out, accumulate=acc), JUDGE))


def colsum_many_run(Kx, dev, dtype, repeat=2):
    """Every problem of COLSUM_CASES `repeat` times in one colsum_many call (more than 16 problems, the two forms mixed)."""
    probs = [colsum_problem(c, dev, dtype) for _ in range(repeat) for c in COLSUM_CASES]
    Kx.colsum_many([(x, rs, out, acc) for x, rs, out, acc in probs])
    return [out for _, _, out, _ in probs]


# ------------------------------------------------------------------------------ element-wise kernels with a capped grid
def _ew(id, op, rows, cols, ld, c0, vec, why, plan=None, **kw):
    return dict(id=id, op=op, rows=rows, cols=cols, ld=ld, c0=c0, vec=vec, why=why, plan=plan, **kw)


EW_CASES = [
    _ew('relu_c33_view', 'relu_bwd', 37, 33, 80, 3, False, 'scalar kernel: ragged columns of an unaligned view'),
    _ew('relu_c36_vec', 'relu_bwd', 37, 36, 80, 4, True, '16-byte kernel on a view'),
    _ew('relu_vec_capped', 'relu_bwd', 1025, 4100, 4100, 0, True, '16-byte kernel, second trip of the stride loop, ragged',
        plan=('STREAM_RELU_BWD_VEC', 1025 * 4100, 4)),
    _ew('relu_scalar_capped', 'relu_bwd', 1049, 1001, 1001, 0, False, 'scalar kernel, second trip, ragged',
        plan=('STREAM_RELU_BWD', 1049 * 1001, 1)),
    _ew('add_c33_view', 'add_rows', 37, 33, 80, 3, False, 'ragged columns of an unaligned view'),
    _ew('add_capped', 'add_rows', 1049, 1001, 1001, 0, False, 'second trip, ragged', plan=('STREAM_ADD_ROWS', 1049 * 1001, 1)),
    _ew('rank1_c33_view', 'rank1', 37, 33, 80, 3, False, 'rank1_kernel (not vectorised): ragged columns, unaligned view'),
    _ew('rank1_c36_ld37', 'rank1', 5, 36, 37, 0, False, 'rank1_kernel: ld % 4 != 0'),
    _ew('rank1_c36_vec', 'rank1', 37, 36, 80, 4, True, 'rank1_vec_kernel on a view'),
    _ew('rank1_scalar_capped', 'rank1', 1049, 1001, 1001, 0, False, 'rank1_kernel, second trip, ragged',
        plan=('STREAM_RANK1', 1049 * 1001, 1)),
    _ew('rank1_vec_capped', 'rank1', 2049, 4100, 4100, 0, True, 'rank1_vec_kernel, second trip, ragged',
        plan=('STREAM_RANK1_VEC', 2049 * 4100, 4)),
    _ew('scale_c33_view', 'scale_rows', 37, 33, 80, 3, False, 'ragged columns of an unaligned view'),
    _ew('scale_capped', 'scale_rows', 2049, 1025, 1025, 0, False, 'second trip, ragged', plan=('STREAM_SCALE_ROWS', 2049 * 1025, 1)),
    _ew('mul_n33_acc', 'mul', 1, 33, 33, 0, False, 'accumulate, one partly filled block', accumulate=True),
    _ew('mul_capped', 'mul', 1, 8192 * 256 + 77, 0, 0, False, 'second trip, ragged', plan=('STREAM_MUL', 8192 * 256 + 77, 1),
        accumulate=False),
    _ew('mul_capped_acc', 'mul', 1, 8192 * 256 + 77, 0, 0, False, 'accumulate, second trip, ragged',
        plan=('STREAM_MUL', 8192 * 256 + 77, 1), accumulate=True),
]


def ew_run(Kx, c, dev, dtype):
    sd, rows, cols, c0 = 400 + 5 * EW_CASES.index(c), c['rows'], c['cols'], c['c0']
    t = lambda *shape, k=0: cv(rnd(*shape, seed=sd + k), dev, dtype)
    if c['op'] == 'mul':
        a, b, out = t(cols, k=1), t(cols, k=2), t(cols, k=3)
        return dict(out=(Kx.mul(a, b, out=out, accumulate=c['accumulate']), JUDGE))
    dst_b = t(rows, c['ld'], k=1)
    dst = block(dst_b, c0, cols)
    res = dict(vec=vec_ok(dst))
    if c['op'] == 'relu_bwd':
        y_b = rnd(rows, c['ld'], seed=sd + 2)
        y_b.view(-1)[::7] = 0.0
        y_b.view(-1)[3::11] = -0.0
        dy, y = block(t(rows, c['ld'], k=3), c0, cols), block(cv(y_b, dev, dtype), c0, cols)
        Kx.relu_bwd(dy, y, dx=dst)
        res.update(dx=(dst, EXACT), dx_new=(Kx.relu_bwd(dy, y), EXACT), vec=vec_ok(dst) and vec_ok(dy) and vec_ok(y))
    elif c['op'] == 'add_rows':
        Kx.add_rows(block(t(rows, c['ld'] + 4, k=2), c0 + 1, cols), dst)
        res.update(dst=(dst, EXACT))
    elif c['op'] == 'rank1':
        Kx.rank1_update(dst, t(rows, k=2), t(cols, k=3))
        res.update(dst=(dst, JUDGE))
    else:
        Kx.scale_rows(dst, t(rows, k=2))
        res.update(dst=(dst, JUDGE))
    res['outside'] = (outside(dst_b, c0, cols), EXACT)
    return res


# (rows, cols) of the 17 operations of the rowops case: the first is larger than the capped grid of its launch, the others are
# tiny (their workgroups beyond the first few find nothing to do), the 17th goes into a second launch
ROWOPS_SHAPES = [(263, 1001), (3, 33), (5, 36), (1, 1), (2, 7), (9, 4), (4, 64), (1, 300), (7, 5), (3, 3), (6, 12), (2, 2), (8, 9),
                 (1, 17), (5, 5), (11, 3), (40, 50)]
ROWOPS_PLAN = ('STREAM_ROWOPS', 263 * 1001, 1)


def rowops_run(Kx, dev, dtype):
    kinds = ['relu_bwd', 'add', 'rank1']
    ops, res = [], {}
    for n, (rows, cols) in enumerate(ROWOPS_SHAPES):
        t = lambda *shape, k=0: cv(rnd(*shape, seed=600 + 10 * n + k), dev, dtype)
        kind, c0 = kinds[n % 3], n % 4
        dst_b = t(rows, cols + 7, k=1)
        dst = block(dst_b, c0, cols)
        if kind == 'relu_bwd':
            ops.append((kind, block(t(rows, cols + 4, k=2), 1, cols), block(t(rows, cols + 3, k=3), 2, cols), dst))
        elif kind == 'add':
            ops.append((kind, block(t(rows, cols + 5, k=2), 3, cols), dst))
        else:
            ops.append((kind, dst, t(rows, k=2), t(cols, k=3)))
        res[f'op{n}_{kind}'] = (dst, JUDGE if kind == 'rank1' else EXACT)
        res[f'op{n}_outside'] = (outside(dst_b, c0, cols), EXACT)
    Kx.rowops(ops)
    return res


# ----------------------------------------------------------------------------------------------------------------- Adam
ADAM_HYPER = dict(lr=f32(1e-3), beta1=f32(0.9), beta2=f32(0.999), eps=f32(1e-8), weight_decay=f32(0.01))
ADAM_GRAD_SCALE = 0.5
ADAM_STEPS = (1, 2, 1000)
ADAM_CASES = [dict(id='n33', n=33, why='one partly filled block', plan=None),
              dict(id='n524621', n=2048 * 256 + 333, why='second trip of the stride loop, ragged', plan=('STREAM_ADAM', 2048 * 256 + 333, 1))]


def adam_run(Kx, c, dev, dtype):
    """Three updates with the step numbers ADAM_STEPS (bias corrections far apart) on non-zero moments, weight decay on."""
    n = c['n']
    p, m, v = cv(rnd(n, seed=700), dev, dtype), cv(rnd(n, seed=701, scale=0.1), dev, dtype), cv(rnd(n, seed=702) ** 2, dev, dtype)
    for k, step in enumerate(ADAM_STEPS):
        Kx.adam_step(p, cv(rnd(n, seed=703 + k), dev, dtype), m, v, step=step, grad_scale=ADAM_GRAD_SCALE, **ADAM_HYPER)
    return dict(p=(p, JUDGE), m=(m, JUDGE), v=(v, JUDGE))


# -------------------------------------------------------------------------------------------------------------- reorder
def _ro(id, bs, T, E, cols, chunks, vec, why):
    return dict(id=id, bs=bs, T=T, E=E, cols=cols, chunks=chunks, vec=vec, why=why)


REORDER_CASES = [
    _ro('c64_T7', 5, 7, 2, 64, 1, True, 'one chunk, 16-byte copies'),
    _ro('c70_T7', 5, 7, 2, 70, 1, False, 'scalar branch: cols % 4 != 0'),
    _ro('c192_T7', 5, 7, 2, 192, 3, True, 'three even chunks of 16 quads'),
    _ro('c200_T7', 5, 7, 2, 200, 3, True, 'uneven chunks: 50 quads over 3 chunks (17, 17, 16)'),
    _ro('c198_T7', 5, 7, 2, 198, 3, False, 'scalar branch over 3 chunks of 66 columns'),
    _ro('c200_T1', 5, 1, 2, 200, 3, True, 'T = 1: every frame maps to itself'),
    _ro('c1024_T7', 5, 7, 2, 1024, 16, True, 'the product width at few clips: 16 chunks'),
    _ro('c1024_pairs513', 171, 1, 3, 1024, 1, True, 'more than 512 (clip, entity) pairs: one chunk at cols = 1024'),
    _ro('c64_T300', 5, 300, 2, 64, 1, True, 'T > 256: second trip of the gate load'),
]


def reorder_gate(bs, T, E, seed):
    """Clip b: all zero / all one / only the last frame / only the first frame / random, by b % 5."""
    g = (rnd(bs, T, E, seed=seed) > 0.3).float()
    for b in range(bs):
        if b % 5 < 4:
            g[b] = (0.0, 1.0, 0.0, 0.0)[b % 5]
        if b % 5 == 2:
            g[b, T - 1] = 1
        if b % 5 == 3:
            g[b, 0] = 1
    return g


def reorder_run(Kx, c, dev, dtype):
    bs, T, E, cols = c['bs'], c['T'], c['E'], c['cols']
    hx, gate = cv(rnd(bs, T, E, cols, seed=800), dev, dtype), cv(reorder_gate(bs, T, E, 801), dev, dtype)
    return dict(fwd=(Kx.reorder_fwd(hx, gate), EXACT), bwd=(Kx.reorder_bwd(hx, gate).reshape(bs * T * E, cols), JUDGE))


# --------------------------------------------------------------------------------------------------------------- filter
FILTER_CASES = [dict(id=f'bs{bs}_T{T}_E{E}', bs=bs, T=T, E=E, why=why) for bs, T, E, why in
                [(5, 9, 7, 'more than 256 elements: a second block, partly filled'), (8, 2, 4, 'T = 2: every frame is first or last'),
                 (6, 1, 5, 'T = 1: both neighbours are the zero padding')]]
FILTER_THRESHOLDS = (0.5, 0.3125)   # both on the grid of the inputs


def filter_soft(c):
    """Values on a 1/16 grid: ties with a neighbour and soft == threshold occur, and are exact in fp32 and fp64 alike."""
    g = torch.Generator().manual_seed(900 + c['T'])
    return torch.randint(0, 17, (c['bs'], c['T'], c['E']), generator=g).float() / 16


def filter_run(Kx, c, dev, dtype):
    soft, res = cv(filter_soft(c), dev, dtype), {}
    for thr in FILTER_THRESHOLDS:
        hard, gmask = Kx.filter_fwd(soft, thr)
        res[f'hard_{thr}'], res[f'gmask_{thr}'] = (hard, EXACT), (gmask, EXACT)
    return res


# ---------------------------------------------------------------------------------------------------------------- heads
HEAD_CASES = [dict(id=f'C{C}_scale{sc}', bs=2, T=67, E=3, C=C, scale=sc, why=why, dlogits_row_factor=None) for C, sc, why in
              [(1, 3, 'one class: log-softmax is exactly 0'), (13, 3, '402 rows: a second block, partly filled'),
               (13, 80, 'logits of scale 80: the maximum must be subtracted'), (64, 3, 'C = 64'), (64, 80, 'C = 64, scale 80')]]
# Row factor 32 for dlogits of C64_scale80 (tensor-wide it stays 8 and needs 0). Measured on an MI355X: 4 of the 402 rows need
# more than 8, the worst 28.3 (profiles/stream_kernels_fp64.json); every other tensor of this suite needs at most 5.9. Why: at
# scale 80 the softmax of a row is one-hot, so the row's largest entry is dout[max] - sum_c dout[c]: the error of the whole row
# is the error of ONE 64-term fp32 sum -- one random number per implementation and summation order, not the maximum over many
# independent roundings. Among 402 such rows there are some where the specification's own sum happens to be exact to 0.07
# half-ulps of the row (e_ref 4e-9 ... 5e-8) while any other order of the same 64 additions is off by its typical 3 to 7
# half-ulps (e_hip 3.6e-7 ... 7.7e-7, against the floor of 4): test_stream_kernels_cpu.py shows that the kernel's formula
# evaluated by plain fp32 torch with a sequential sum, or with four interleaved partial sums, misses factor 8 on this case just
# so. A lost class or a wrong stride is a 1e-1 ... 1e-3 effect and fails at 32 as at 8. 32 is the ceiling entity_envelope.py
# set for a stated reason; it is not fitted to the 28.3.
HEAD_CASES[-1]['dlogits_row_factor'] = 32.0
HEAD_GUARD = 64


def head_bwd_in_plain_fp32(c, out32, partial_sums):
    """dlogits of case c as lsm_permute_bwd_kernel writes the formula, in fp32 torch on the CPU: the sum over the classes taken
    one after the other in `partial_sums` interleaved chains (1: the kernel's order)."""
    bs, T, E, C = c['bs'], c['T'], c['E'], c['C']
    o = out32.reshape(bs, C, T, E).permute(0, 2, 3, 1).reshape(-1, C)
    g = rnd(bs, C, T, E, seed=1001).permute(0, 2, 3, 1).reshape(-1, C)
    acc = [torch.zeros(o.shape[0]) for _ in range(partial_sums)]
    for k in range(C):
        acc[k % partial_sums] = acc[k % partial_sums] + g[:, k]
    while len(acc) > 1:
        acc = [acc[i] + acc[i + 1] for i in range(0, len(acc), 2)]
    return g - torch.exp(o) * acc[0][:, None]


def head_run(Kx, c, dev, dtype, saved=None):
    """out is poisoned with NaN (and followed by HEAD_GUARD more NaN the call must leave); the backward pass reads `saved`."""
    bs, T, E, C = c['bs'], c['T'], c['E'], c['C']
    n = bs * C * T * E
    buf = torch.full((n + HEAD_GUARD,), float('nan'), dtype=dtype, device=dev)
    out = Kx.logsoftmax_permute_fwd(cv(rnd(bs * T * E, C, seed=1000, scale=c['scale']), dev, dtype), bs, T, E, C,
                                    out=buf[:n].view(bs, C, T, E))
    o = out if saved is None else cv(saved['out'][0].reshape(bs, C, T, E), dev, dtype)
    dl = Kx.logsoftmax_permute_bwd(o, cv(rnd(bs, C, T, E, seed=1001), dev, dtype))
    return dict(out=(out.reshape(bs * C, T * E), JUDGE), guard=(buf[n:], None), dlogits=(dl, JUDGE))


# ---------------------------------------------------------------------------------------------------- position features
def _pe(bs, T, E, hidden, periodic, divide, c0, why, bias=True):
    return dict(id=f"{'periodic' if periodic else 'linear'}_h{hidden}_T{T}{'_div' if divide else ''}{'_blk' if c0 else ''}", bs=bs, T=T,
                E=E, hidden=hidden, periodic=periodic, divide=divide, c0=c0, why=why, bias=bias)


POS_CASES = [
    _pe(2, 7, 3, 2, True, False, 0, 'half == 1: the single frequency is 1'),
    _pe(2, 7, 3, 32, True, True, 5, '64 threads, half of them idle; output into a column block'),
    _pe(2, 7, 3, 70, True, False, 0, '64 threads, ragged second trip'),
    _pe(2, 7, 3, 256, True, True, 0, 'forward switches to 256 threads'),
    _pe(2, 7, 3, 258, True, False, 3, '256 threads, ragged second trip; output into a column block'),
    _pe(2, 7, 3, 510, True, True, 0, 'backward still 64 threads: four trips, the last ragged'),
    _pe(2, 7, 3, 512, True, False, 0, 'backward switches to 256 threads'),
    _pe(3, 1, 2, 32, True, True, 0, 'T = 1'),
    _pe(2, 120, 2, 32, True, False, 0, 'T = 120: arguments up to 120'),
    _pe(2, 7, 3, 33, False, True, 2, 'linear mode takes an odd width; output into a column block'),
    _pe(2, 7, 3, 2, False, False, 0, 'linear, two columns, no bias', bias=False),
    _pe(2, 120, 2, 256, False, True, 0, 'linear at 256 threads, T = 120'),
]


def pos_run(Kx, c, dev, dtype):
    """pos_embed_fwd with the time feature, once more with the scalars given (s_in), and for the periodic mode the backward
    pass on those scalars."""
    bs, T, E, h, c0 = c['bs'], c['T'], c['E'], c['hidden'], c['c0']
    rows, sd = bs * T * E, 1100 + h
    t = lambda *shape, k=0, sc=1.0: cv(rnd(*shape, seed=sd + k, scale=sc), dev, dtype)
    steps = cv(torch.tensor([float(T), T + 3.0, T + 1.0][:bs]), dev, dtype)
    w, b = (None, None) if c['periodic'] else (t(h, k=1), t(h, k=2) if c['bias'] else None)
    base = t(rows, h + 2 * c0, k=3)
    out = block(base, c0, h)
    s = Kx.pos_embed_fwd(out, bs, T, E, h, w=w, b=b, periodic=c['periodic'], steps=steps, divide=c['divide'])
    res = dict(out=(out, JUDGE), outside=(outside(base, c0, h), EXACT), s=(s, JUDGE))
    given = t(rows, k=4, sc=3.0)
    out2 = cv(torch.zeros(rows, h), dev, dtype)
    res['s2'] = (Kx.pos_embed_fwd(out2, bs, T, E, h, w=w, b=b, periodic=c['periodic'], s=given), JUDGE)
    res['out2'] = (out2, JUDGE)
    if c['periodic']:
        res['ds'] = (Kx.periodic_embed_bwd(block(t(rows, h + 2 * c0, k=5), c0, h), given), JUDGE)
    return res


SEGLEN_CASES = [dict(id=f'bs{bs}_T{T}_E{E}{"_div" if div else ""}', bs=bs, T=T, E=E, divide=div, why=why) for bs, T, E, div, why in
                [(99, 7, 3, True, 'bs * E = 297: a second block, partly filled'), (27, 120, 11, False, 'bs * E = 297 with T = 120'),
                 (4, 1, 3, True, 'T = 1')]]


def seglen_run(Kx, c, dev, dtype):
    bs, T, E = c['bs'], c['T'], c['E']
    u = cv((rnd(bs, T, E, seed=1200) > 0.2).float(), dev, dtype)
    steps = cv(T + torch.arange(bs).float() % 5, dev, dtype)
    du = cv(rnd(bs, T, E, seed=1201), dev, dtype)
    s = Kx.seglen_fwd(u, steps, c['divide'])
    Kx.seglen_bwd(u, steps, c['divide'], cv(rnd(bs, T, E, seed=1202), dev, dtype), du)
    return dict(s=(s.reshape(-1), JUDGE), du=(du.reshape(-1), JUDGE))


# ------------------------------------------------------------------------------------------- sender-side projection glue
def _sp(H, O, cols, ph, ps, mask, why):
    return dict(id=f"H{H}_O{O}_c{cols}{'_ph' if ph else ''}{'_ps' if ps else ''}{'' if mask else '_nomask'}", H=H, O=O, cols=cols,
                ph=ph, ps=ps, mask=mask, why=why)


SSP_CASES = [
    _sp(4, 16, 4, True, True, True, 'the limits of red[4][64] and dot[64]; one quad: 255 idle threads'),
    _sp(4, 16, 1028, True, True, True, 'the limits; a second trip of one thread: dot[] accumulates across trips'),
    _sp(4, 16, 512, True, False, True, 'ph only'),
    _sp(4, 16, 512, False, True, True, 'ps only'),
    _sp(1, 1, 512, True, True, True, 'one human, one object'),
    _sp(4, 1, 4, True, True, True, 'four humans, one object'),
    _sp(2, 3, 512, True, True, False, 'mask = None'),
]
SSP_N_INST, SSP_IPC = 12, 4


def ssp_inputs(c):
    """att_off > 0 inside the wider natt of the attention layout; clip 0 fully masked."""
    H, O, cols, n = c['H'], c['O'], c['cols'], SSP_N_INST
    natt = H * H + 2 * H * O + O * O
    mask = (rnd(n // SSP_IPC, O, seed=1302) > -0.5).float()
    mask[0] = 0
    return dict(att=torch.softmax(rnd(n, natt, seed=1301), -1), mask=mask if c['mask'] else None, gi=rnd(n * O, cols, seed=1303),
                ph=rnd(n * H, cols, seed=1304) if c['ph'] else None, ps=rnd(n, cols, seed=1305) if c['ps'] else None,
                dgi=rnd(n * O, cols, seed=1306), natt=natt, off=H * H + H * O, n_inst=n, ipc=SSP_IPC)


def ssp_run(Kx, c, dev, dtype):
    from tests.entity_envelope import ssp_run as run
    return {k: (v, JUDGE) for k, v in run(Kx, ssp_inputs(c), c['H'], c['O'], c['ps'], dev=dev, dtype=dtype).items()}


SSP_GATHER = dict(bs=3, T=5, H=4, O=16, cols=48)


def ssp_gather_run(Kx, dev, dtype):
    """Both leading dimensions of the weights larger than dense, the gradient rows a column block of wider rows."""
    g = SSP_GATHER
    bs, T, H, O, cols = g['bs'], g['T'], g['H'], g['O'], g['cols']
    natt = H * H + 2 * H * O + O * O
    ld_frame, ld_clip = natt + 5, T * (natt + 5) + 7
    att = cv(torch.softmax(rnd(bs * ld_clip, seed=1401), -1) * natt, dev, dtype)
    dgi = block(cv(rnd(bs * T * O, cols + 8, seed=1402), dev, dtype), 4, cols)
    return dict(qh=(Kx.ssp_gather(dgi, att, ld_clip, ld_frame, H * H + H * O, bs * T, T, H, O), JUDGE))


# ------------------------------------------------------------------------------------------------------------ fill_zero
FILL_BYTE, FILL_ROW = 0xA5, 128
FILL_PAIRS = [(off, n) for off in range(18) for n in range(49)]
# (offset, bytes): 13 head bytes, then 256 16-byte stores more than one trip of the capped grid covers, then 10 tail bytes
FILL_BIG = (3, 16 * 1024 * 1024 + 4096 + 7)
FILL_BIG_PLAN = ('STREAM_FILL_ZERO', FILL_BIG[1], 16)


def fill_run(Kx, dev, pairs=FILL_PAIRS, row=FILL_ROW):
    """One row of `row` bytes per (offset, length): rows start 16-byte aligned, the slice [16 + offset, 16 + offset + length) is
    cleared through Kx.fill_zero. -> the whole buffer (uint8)."""
    buf = torch.full((len(pairs), row), FILL_BYTE, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 16 == 0
    for k, (off, n) in enumerate(pairs):
        Kx.fill_zero(buf[k, 16 + off:16 + off + n])
    return buf


def fill_expected(pairs=FILL_PAIRS, row=FILL_ROW):
    want = torch.full((len(pairs), row), FILL_BYTE, dtype=torch.uint8)
    for k, (off, n) in enumerate(pairs):
        want[k, 16 + off:16 + off + n] = 0
    return want


# ---------------------------------------------------------------------------------------------------------- copy_blocks
COPY_SENTINEL, COPY_GUARD = 7.25, 8
COPY_SIZES = (1, 3, 4, 5, 255, 1027)
COPY_BIG = 512 * 256 * 4 + 1029               # floats: 257 quads beyond one trip of the capped grid, and a one-float tail
COPY_BIG_PLAN = ('STREAM_COPY_BLOCKS', COPY_BIG, 4)
# (n, src offset, dst offset) in floats from a 16-byte boundary; offsets (0, 0) take the 16-byte path with its n % 4 tail
COPY_PAIRS = [(n, so, do) for n in COPY_SIZES for so in range(4) for do in range(4)] + [(COPY_BIG, 0, 0), (COPY_BIG, 1, 0), (COPY_BIG, 2, 2)]


def copy_run(Kx, dev, pairs=COPY_PAIRS):
    """All pairs in one copy_blocks call (the wrapper splits it into launches of 16, so aligned and unaligned pairs share
    launches). Each destination lies in one buffer of sentinels with at least COPY_GUARD of them on either side. -> that buffer."""
    slot = lambda n: (n + 2 * COPY_GUARD + 3 + 3) // 4 * 4
    total = sum(slot(n) for n, _, _ in pairs)
    src_all = cv(rnd(total, seed=1500), dev, torch.float32)
    dst_all = torch.full((total,), COPY_SENTINEL, dtype=torch.float32, device=dev)
    assert src_all.data_ptr() % 16 == 0 and dst_all.data_ptr() % 16 == 0
    calls, o = [], 0
    for n, so, do in pairs:
        calls.append((src_all[o + COPY_GUARD + so:o + COPY_GUARD + so + n], dst_all[o + COPY_GUARD + do:o + COPY_GUARD + do + n]))
        o += slot(n)
    Kx.copy_blocks(calls)
    return dst_all


def copy_expected(pairs=COPY_PAIRS):
    slot = lambda n: (n + 2 * COPY_GUARD + 3 + 3) // 4 * 4
    total = sum(slot(n) for n, _, _ in pairs)
    src_all, want, o = rnd(total, seed=1500), torch.full((total,), COPY_SENTINEL), 0
    for n, so, do in pairs:
        want[o + COPY_GUARD + do:o + COPY_GUARD + do + n] = src_all[o + COPY_GUARD + so:o + COPY_GUARD + so + n]
        o += slot(n)
    return want
