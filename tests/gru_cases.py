"""The GRU family (csrc/gru.hip and the gate epilogues of csrc/gemm_f32.hip): case lists, seeded inputs, and the executable
specification (tests/fake_kernels.py, tests/baseline_helpers.py) run on them. Shared by tests/test_gru_kernels_cpu.py (the
specification against torch.nn.GRU / GRUCell and autograd, and what the case list reaches) and tests/test_gru_kernels_gpu.py
(the HIP kernels against the specification in fp32 and fp64).

Every `*_run(Kx, c, dev, dtype)` builds the inputs of case c as seeded fp32 tensors, casts them to dtype on dev, calls the
methods of Kx (the specification on the CPU in fp32 / fp64, HipKernels on the GPU in fp32: all three see identical values) and
returns {name: (tensor, how)}: how = EXACT -> the HIP result must be bit-equal to the fp32 specification (untouched memory
around a written view, rows a gate of exactly 0 passes through, gradients that are exact zeros); JUDGE ->
tests.entity_envelope.judge against the fp64 run with the fp32 run's own error as the yardstick; None -> for the test itself.

The step kernels (twog_gru_step_fwd / twog_gru_step_bwd) are called directly, with caller-owned buffers: every operand is a
view inside a larger buffer -- a block of columns of wider rows with guard rows above and below (`plain`: twog_rows_t with
inner = 1), or the (clip, entity) rows of a [bs][T][E][w] tensor at t = 1 (`be`: inner = E) -- and the buffers of the written
operands are returned whole with the view zeroed (`*_outside`, EXACT). The `why` of a case names the branch it is there for;
`vec` / `launches` / `threads` (forward step) and `cls` (gate-fused backward) are what the GPU test reads back from the
library (twog_gru_step_last_path, twog_gemm_last_class) after the call."""
import functools

import torch

from tests.baseline_helpers import BaselineFakeKernels
from tests.kernel_cases import rnd
from twog_gcn_amd.kernels import rows_of

F = BaselineFakeKernels()
EXACT, JUDGE = 'exact', 'judge'
SENTINEL = 7.25
TOP, BOTTOM = 4, 1     # guard rows of a plain buffer (TOP a multiple of 4: the view's alignment is its column offset's)
T_BE, AT = 2, 1        # frames of a `be` buffer, and the frame the view is taken at
ALIGNED = (4, 4)       # (column offset, columns behind the view) of an operand that keeps 16-byte alignment


def cv(t, dev, dtype):
    if t is None:
        return None
    return t.to(dev, dtype if t.is_floating_point() else t.dtype, copy=True)


def _seed(*parts):
    s = 0
    for p in parts:
        for ch in str(p):
            s = (s * 131 + ord(ch)) % 1000003
    return s


def _place(kind, bs, E, W, c0, pad, values, dev, dtype, fill=None, seed=0):
    """One operand -> (buffer, view). kind: 'p' (rows, W) / 'p3' (rows, 1, W) views of a plain buffer, 'be' the (bs, E, W)
    view of a [bs][T_BE][E][c0 + W + pad] buffer at frame AT. The buffer holds `fill` (or seeded noise), the view `values`."""
    shape = (bs, T_BE, E, c0 + W + pad) if kind == 'be' else (TOP + bs * E + BOTTOM, c0 + W + pad)
    base = torch.full(shape, fill) if fill is not None else rnd(*shape, seed=seed + 1)
    base = cv(base, dev, dtype)
    if kind == 'be':
        view = base[:, AT, :, c0:c0 + W]
    else:
        view = base[TOP:TOP + bs * E, c0:c0 + W]
        if kind == 'p3':
            assert E == 1
            view = view.unsqueeze(1)
    if values is not None:
        view.copy_(cv(values, dev, dtype).reshape(view.shape))
    return base, view


def _outside(base, view_of):
    """The buffer with the view zeroed: what a call that writes the view must leave as it was."""
    b = base.detach().clone()
    view_of(b).zero_()
    return b


def _gate_values(bs, E, seed):
    """u in (0, 1) with every fifth row exactly 0 and the rows after those exactly 1."""
    u = torch.sigmoid(rnd(bs * E, seed=seed))
    u[0::5] = 0.0
    u[1::5] = 1.0
    return u


def _u_place(form, bs, E, values, dev, dtype, seed):
    """form 'row': one value per row with a row stride of 3 ((rows, 1) view: u_inner = 1); 'be': the (bs, E) view of a
    (bs, T_BE, E) tensor at frame AT (u_inner = E, ld_outer = T_BE * E). -> (buffer, view)."""
    if form == 'row':
        assert E == 1
        base = cv(rnd(bs + 2, 3, seed=seed + 1), dev, dtype)
        view = base[1:bs + 1, 1:2]
    else:
        base = cv(rnd(bs, T_BE, E, seed=seed + 1), dev, dtype)
        view = base[:, AT]
    view.copy_(cv(values, dev, dtype).reshape(view.shape))
    return base, view


def _u_view(form, base, bs):
    return base[1:bs + 1, 1:2] if form == 'row' else base[:, AT]


def _view_of(kind, bs, E, W, c0):
    if kind == 'be':
        return lambda b: b[:, AT, :, c0:c0 + W]
    return lambda b: b[TOP:TOP + bs * E, c0:c0 + W]


# ------------------------------------------------------------------------------------------------- the forward gate step
def _fd(rows=3, h=64, lay='plain', E=1, gi2=False, h_prev=True, save=True, u=None, at=None):
    """One forward descriptor. lay 'plain': bs = rows, E = 1, every operand a block of columns of a plain buffer; 'be': rows
    = bs * E, gi / gi2 / h_out / save the (b, e) rows of [bs][T][E][w] tensors, gh and h_prev plain rows (as the frame
    recurrence mixes them). at: {operand: (column offset, columns behind)} where it differs from ALIGNED."""
    return dict(rows=rows, h=h, lay=lay, E=E, gi2=gi2, h_prev=h_prev, save=save, u=u, at=at or {})


def _fc(id, why, descs, vec, launches=1, threads=None, seed=None, same_as=None, saturate=False):
    if threads is None:
        hmax = max(d['h'] for d in descs)
        threads = 256 if vec or hmax >= 256 else (hmax + 63) // 64 * 64
    return dict(id=id, why=why, descs=descs, vec=vec, launches=launches, threads=threads, seed=seed if seed is not None else id,
                same_as=same_as, saturate=saturate)


VEC_HIDDEN = (64, 128, 256, 512, 1024)
SCALAR_HIDDEN_4 = {32: 'hidden < 64', 100: '256 % (h / 4) != 0', 192: '256 % (h / 4) != 0',
                   768: '256 % (h / 4) != 0; three trips of the stride loop', 1028: 'h / 4 > 256; five trips, the last ragged',
                   300: '256 % (h / 4) != 0; two trips, the second ragged'}
SCALAR_HIDDEN_ODD = (1, 3, 63, 65, 255, 257)
HIDDEN = VEC_HIDDEN + tuple(SCALAR_HIDDEN_4) + SCALAR_HIDDEN_ODD

STEP_FWD_CASES = []
for _h, _rows in [(64, 1), (64, 16), (64, 17), (64, 33), (128, 9), (256, 5), (512, 3), (1024, 1), (1024, 3)]:
    STEP_FWD_CASES.append(_fc(f'h{_h}_r{_rows}', f'16-byte kernel, {1024 // _h} rows per block: rows around that', [_fd(_rows, _h)], True))
for _h, _w in SCALAR_HIDDEN_4.items():
    STEP_FWD_CASES.append(_fc(f'h{_h}_r3', f'scalar kernel although h % 4 == 0: {_w}', [_fd(3, _h)], False))
for _h in SCALAR_HIDDEN_ODD:
    STEP_FWD_CASES.append(_fc(f'h{_h}_r3', 'scalar kernel: h % 4 != 0' + ('; a ragged second trip' if _h > 256 else ''), [_fd(3, _h)], False))

# alignment: one operand at a time loses what the 16-byte kernel needs; same values as the aligned case -> same bits
ALIGN_BREAKS = []
for _h in (64, 512):
    _r = 5 if _h == 64 else 3
    STEP_FWD_CASES.append(_fc(f'align_h{_h}_plain', 'the aligned run the plain alignment variants are compared with',
                              [_fd(_r, _h, gi2=True)], True, seed=f'align{_h}p'))
    STEP_FWD_CASES.append(_fc(f'align_h{_h}_be', 'the aligned run the (b, e)-row alignment variants are compared with; inner > 1 in the 16-byte kernel',
                              [_fd(2 * _r, _h, lay='be', E=_r, gi2=True)], True, seed=f'align{_h}b'))
    for _op in ('gi', 'gi2', 'gh', 'h_prev', 'h_out', 'save'):
        for _how, _at in (('ptr', (5, 3)), ('ldo', (4, 5))):
            _id = f'align_h{_h}_{_op}_{_how}'
            _why = (f'{_op} a column block at an odd float offset' if _how == 'ptr' else f'{_op} with ld_outer % 4 != 0') + ' -> scalar kernel'
            STEP_FWD_CASES.append(_fc(_id, _why, [_fd(_r, _h, gi2=True, at={_op: _at})], False, seed=f'align{_h}p', same_as=f'align_h{_h}_plain'))
            ALIGN_BREAKS.append(_id)
    for _op in ('gi', 'gi2', 'h_out', 'save'):
        _id = f'align_h{_h}_{_op}_ldi'
        STEP_FWD_CASES.append(_fc(_id, f'{_op} with ld_inner % 4 != 0 and inner > 1 (E = 4: pointer and ld_outer stay aligned) -> scalar kernel',
                                  [_fd(8, _h, lay='be', E=4, gi2=True, at={_op: (4, 5)})], False, seed=f'align{_h}i', same_as=f'align_h{_h}_be4'))
        ALIGN_BREAKS.append(_id)
    STEP_FWD_CASES.append(_fc(f'align_h{_h}_be4', 'the aligned run of the ld_inner variants (E = 4)',
                              [_fd(8, _h, lay='be', E=4, gi2=True)], True, seed=f'align{_h}i'))

# descriptor groups
STEP_FWD_CASES += [
    _fc('mixed_hidden_64_128', 'descriptors of different hidden in one chunk: scalar kernel, block size from the larger hidden',
        [_fd(5, 64), _fd(3, 128), _fd(7, 64, lay='be', E=7)], False, threads=128),
    _fc('rows_1_17_0_40', 'equal hidden, different rows, a descriptor with rows = 0 between live ones: grid from the largest',
        [_fd(1, 64), _fd(17, 64), _fd(0, 64), _fd(40, 64)], True),
    _fc('descs_9', '9 descriptors: two chunks (8 + 1)', [_fd(1 + k % 5, 64) for k in range(9)], True, launches=2),
    _fc('descs_17', '17 descriptors: three chunks (8 + 8 + 1)', [_fd(1 + k % 5, 64) for k in range(17)], True, launches=3),
    _fc('descs_9_scalar_tail', '9 descriptors, the ninth of another hidden: a 16-byte chunk, then a scalar chunk of one',
        [_fd(2, 64) for _ in range(8)] + [_fd(3, 100)], False, launches=2, threads=128),
    _fc('rows_all_0', 'a second chunk of nothing but rows = 0 descriptors launches nothing',
        [_fd(2, 64) for _ in range(8)] + [_fd(0, 64)], True, launches=1),
    _fc('mixed_rows_forms', 'plain rows and (b, e) rows with inner > 1 mixed in one call, rows 70',
        [_fd(70, 128), _fd(70, 128, lay='be', E=7), _fd(3, 128, lay='be', E=3, u='be')], True),
]
# operands present or absent, in both kernels (h = 128: 16-byte, h = 100: scalar)
for _h, _vec in ((128, True), (100, False)):
    _k = '16-byte' if _vec else 'scalar'
    STEP_FWD_CASES += [
        _fc(f'h{_h}_gi2', f'{_k} kernel: gi2 present', [_fd(9, _h, gi2=True)], _vec),
        _fc(f'h{_h}_no_hprev', f'{_k} kernel: h_prev absent (zeros)', [_fd(9, _h, h_prev=False)], _vec),
        _fc(f'h{_h}_no_save', f'{_k} kernel: save absent', [_fd(9, _h, save=False)], _vec),
        _fc(f'h{_h}_u_row', f'{_k} kernel: u with inner <= 1, one value per row with a row stride; u == 0 / u == 1 rows', [_fd(12, _h, u='row')], _vec),
        _fc(f'h{_h}_u_be', f'{_k} kernel: u a (bs, E) view of a (bs, T, E) tensor at t = 1 (u_inner = E, ld_outer = T * E)',
            [_fd(15, _h, lay='be', E=5, u='be')], _vec),
        _fc(f'h{_h}_u_no_hprev', f'{_k} kernel: u with h_prev absent: (1 - u) * 0', [_fd(7, _h, lay='be', E=7, u='be', h_prev=False, gi2=True)], _vec),
        _fc(f'h{_h}_saturated', f'{_k} kernel: pre-activations of +-30 and +-100: expf overflows to inf, gates exactly 0 or 1, all finite',
            [_fd(6, _h)], _vec, saturate=True),
    ]
STEP_FWD_BY_ID = {c['id']: c for c in STEP_FWD_CASES}
SATURATED_BEYOND = 90.0   # |pre-activation| from which fp32 sigmoid / tanh must be exactly 0, 1 or +-1


def _fwd_layout(d, name):
    """(kind, column offset, columns behind) of operand `name` of descriptor d."""
    if d['lay'] == 'plain':
        kind = 'p3' if name in ('gi', 'h_out') else 'p'
    else:
        kind = 'p' if name in ('gh', 'h_prev') else 'be'
    return (kind,) + tuple(d['at'].get(name, ALIGNED))


def _saturating_offsets(rows, h, seed):
    """Added to gi: +-30 / +-100 by (row, unit, gate) in a fixed pattern, a quarter of the entries left alone."""
    levels = torch.tensor([0.0, 30.0, -30.0, 100.0, -100.0, 0.0, 100.0, -100.0])
    idx = (torch.arange(rows)[:, None] * 3 + torch.arange(3 * h)[None, :] * 5 + torch.arange(3 * h)[None, :] // h) % 8
    return levels[idx]


def step_fwd_build(c, dev, dtype):
    """-> (descriptor dicts for Kx.gru_step_fwd, per-descriptor bookkeeping)."""
    steps, book = [], []
    for k, d in enumerate(c['descs']):
        E, h = d['E'], d['h']
        bs = d['rows'] // E
        assert bs * E == d['rows']
        sd = lambda name: _seed(c['seed'], k, name)
        val = lambda name, W, scale=1.0: rnd(d['rows'], W, seed=sd(name), scale=scale)
        vals = dict(gi=val('gi', 3 * h), gi2=val('gi2', 3 * h, 0.5) if d['gi2'] else None, gh=val('gh', 3 * h),
                    h_prev=val('h_prev', h) if d['h_prev'] else None)
        if c['saturate']:
            vals['gi'] = vals['gi'] * 0.25 + _saturating_offsets(d['rows'], h, sd('sat'))
            vals['gh'] = vals['gh'] * 0.25
        st, bk = dict(rows=d['rows'], hidden=h), dict(vals=vals, bs=bs)
        for name, W in (('gi', 3 * h), ('gi2', 3 * h), ('gh', 3 * h), ('h_prev', h)):
            if vals[name] is None:
                st[name] = None
                continue
            kind, c0, pad = _fwd_layout(d, name)
            _, st[name] = _place(kind, bs, E, W, c0, pad, vals[name], dev, dtype, seed=sd(name))
        for name, W in (('h_out', h), ('save', 4 * h)):
            if name == 'save' and not d['save']:
                st[name] = None
                continue
            kind, c0, pad = _fwd_layout(d, name)
            bk[name + '_base'], st[name] = _place(kind, bs, E, W, c0, pad, None, dev, dtype, fill=SENTINEL)
            bk[name + '_view'] = _view_of(kind, bs, E, W, c0)
        st['u'] = None
        if d['u']:
            bk['u_vals'] = _gate_values(bs, E, sd('u'))
            _, st['u'] = _u_place(d['u'], bs, E, bk['u_vals'], dev, dtype, sd('u'))
        steps.append(st)
        book.append(bk)
    return steps, book


def step_fwd_run(Kx, c, dev, dtype):
    steps, book = step_fwd_build(c, dev, dtype)
    Kx.gru_step_fwd(steps)
    out = {}
    ungated = []
    for k, (d, st, bk) in enumerate(zip(c['descs'], steps, book)):
        h = d['h']
        out[f'h_out{k}'] = (st['h_out'].reshape(-1, h), JUDGE)
        out[f'h_out{k}_outside'] = (_outside(bk['h_out_base'], bk['h_out_view']), EXACT)
        if d['save']:
            out[f'save{k}'] = (st['save'].reshape(-1, h), JUDGE)
            out[f'save{k}_outside'] = (_outside(bk['save_base'], bk['save_view']), EXACT)
        if d['u']:
            u0, u1 = bk['u_vals'] == 0, bk['u_vals'] == 1
            assert bool(u0.any()) and bool(u1.any())
            # u == 0: the previous state (zeros where it is absent) bit for bit; u == 1: the ungated state of the same kernel
            out[f'h_out{k}_where_u0'] = (st['h_out'].reshape(-1, h)[u0.to(dev)], EXACT)
            s2 = dict(st, u=None, save=None, h_out=torch.empty_like(st['h_out']))
            ungated.append((k, s2, u1))
        if c['saturate']:
            pre = (bk['vals']['gi'].double() + bk['vals']['gh'].double())[:, :2 * h]   # of r and z
            out[f'saturated{k}_mask'] = (pre.abs() > SATURATED_BEYOND, None)
            out[f'saturated{k}_rz'] = (st['save'].reshape(-1, 4 * h)[:, :2 * h], None)
    if ungated:
        Kx.gru_step_fwd([s2 for _, s2, _ in ungated])
        for k, s2, u1 in ungated:
            h = c['descs'][k]['h']
            diff = steps[k]['h_out'].reshape(-1, h)[u1.to(dev)] - s2['h_out'].reshape(-1, h)[u1.to(dev)]
            out[f'h_out{k}_where_u1_minus_ungated'] = (diff, EXACT)
    return out


def step_fwd_vec_expected(c):
    """gru_step_vec_ok of csrc/gru.hip on the fp32 descriptors of the case as HipKernels packs them (rows_of) -> the kernel of
    the LAST chunk that launches, the launches of the call, the block size of that chunk."""
    steps, _ = step_fwd_build(c, 'cpu', torch.float32)

    def rows_ok(t):
        if t is None or t.numel() == 0:
            return True
        r = rows_of(t)
        return r.ptr % 16 == 0 and r.ld_outer % 4 == 0 and (r.inner <= 1 or r.ld_inner % 4 == 0)

    last, launches = None, 0
    for i in range(0, len(steps), 8):
        chunk = steps[i:i + 8]
        if max(s['rows'] for s in chunk) <= 0:
            continue
        hmax = max(s['hidden'] for s in chunk)
        vec = all(s['hidden'] % 4 == 0 and 64 <= s['hidden'] <= 1024 and 256 % (s['hidden'] // 4) == 0 and s['hidden'] == hmax and
                  all(rows_ok(s[k]) for k in ('gi', 'gi2', 'gh', 'h_prev', 'h_out', 'save')) for s in chunk)
        last, launches = (vec, 256 if vec or hmax >= 256 else (hmax + 63) // 64 * 64), launches + 1
    return last[0], last[1], launches


# ------------------------------------------------------------------------------------------------ the backward gate step
def _bd(rows=3, h=64, lay='plain', E=1, dh2=True, h_prev=True, acc=False, alias=False, u=None, du=False, share_u=None):
    """One backward descriptor; dh / save / dgi / dgh follow `lay`, dh2 / h_prev / dh_prev are plain rows (the carried gradient
    of the recurrences). alias: dh_prev IS dh2. share_u: u and du are those of descriptor `share_u` of the same call."""
    return dict(rows=rows, h=h, lay=lay, E=E, dh2=dh2, h_prev=h_prev, acc=acc, alias=alias, u=u, du=du, share_u=share_u)


def _bc(id, why, descs):
    return dict(id=id, why=why, descs=descs, seed=id)


STEP_BWD_CASES = []
for _h in HIDDEN:
    _bt = min(256, (_h + 63) // 64 * 64)
    STEP_BWD_CASES.append(_bc(f'h{_h}', f'block of {_bt} threads, {(_h + _bt - 1) // _bt} trip(s); block reduction of du over {_bt // 64} wave(s), u with inner <= 1',
                              [_bd(5 if _h <= 128 else 3, _h, u='row', du=True)]))
for _h in (64, 300):
    STEP_BWD_CASES += [
        _bc(f'h{_h}_no_dh2', 'dh2 absent', [_bd(5, _h, dh2=False)]),
        _bc(f'h{_h}_no_hprev', 'h_prev absent (zeros)', [_bd(5, _h, h_prev=False, u='row', du=True)]),
        _bc(f'h{_h}_accumulate', 'dh_prev_accumulate = 1 onto a pre-filled buffer', [_bd(5, _h, acc=True)]),
        _bc(f'h{_h}_accumulate_u', 'dh_prev_accumulate = 1 with the (1 - u) * dh path', [_bd(5, _h, acc=True, u='row', du=True)]),
        _bc(f'h{_h}_alias', 'dh_prev aliasing dh2, as the frame recurrence calls it', [_bd(5, _h, alias=True)]),
        _bc(f'h{_h}_u_no_du', 'u present, du absent', [_bd(5, _h, u='row')]),
        _bc(f'h{_h}_u_be', 'u / du (bs, E) views of (bs, T, E) tensors at t = 1 (u_inner = E > 1), du pre-filled with non-zero values',
            [_bd(15, _h, lay='be', E=5, u='be', du=True)]),
        _bc(f'h{_h}_two_into_one_du', 'two descriptors of one call add into the same du tensor (atomicAdd), as both directions of the segment loop do',
            [_bd(12, _h, lay='be', E=4, u='be', du=True), _bd(12, _h, lay='be', E=4, u='be', du=True, share_u=0)]),
    ]
STEP_BWD_CASES += [
    _bc('rows_70_17_0_1', 'equal hidden, rows 70 / 17 / 0 / 1 in one launch: grid from the largest', [_bd(70, 64), _bd(17, 64), _bd(0, 64), _bd(1, 64)]),
    _bc('mixed_hidden_64_300', 'descriptors of different hidden: block size from the larger, the smaller idles most threads',
        [_bd(3, 64, u='row', du=True), _bd(3, 300, u='row', du=True)]),
    _bc('descs_9', '9 descriptors: two launches (8 + 1)', [_bd(1 + k % 4, 64) for k in range(9)]),
]
STEP_BWD_BY_ID = {c['id']: c for c in STEP_BWD_CASES}
PLANTS = ('r0', 'r1', 'z0', 'z1', 'n+', 'n-')   # planted in units 0 .. 5 (as far as hidden goes) of every row


def _saved_gates(rows, h, seed):
    """save = [r | z | n | hn] as a forward step leaves it (an INPUT of the backward step), with gates planted at exactly 0
    and 1 and n at exactly +-1 in the first units; -> (save, mask of the entries of dgi and of dgh that must be exact zeros)."""
    r, z = torch.sigmoid(rnd(rows, h, seed=seed)), torch.sigmoid(rnd(rows, h, seed=seed + 1))
    n, hn = torch.tanh(rnd(rows, h, seed=seed + 2)), rnd(rows, h, seed=seed + 3)
    zero = torch.zeros(rows, 3 * h, dtype=torch.bool)
    for j, p in enumerate(PLANTS[:h]):
        if p[0] == 'r':
            r[:, j] = float(p[1])
            zero[:, j] = True                      # dr_pre = dn_pre * hn * r * (1 - r)
        elif p[0] == 'z':
            z[:, j] = float(p[1])
            zero[:, h + j] = True                  # dz_pre = dz * z * (1 - z)
        else:
            n[:, j] = 1.0 if p[1] == '+' else -1.0
            zero[:, j] = zero[:, 2 * h + j] = True  # dn_pre = dn * (1 - n * n), and dr_pre has it as a factor
    return torch.cat([r, z, n, hn], -1), zero


def step_bwd_build(c, dev, dtype):
    steps, book = [], []
    for k, d in enumerate(c['descs']):
        E, h, rows = d['E'], d['h'], d['rows']
        bs = rows // E
        assert bs * E == rows
        sd = lambda name: _seed(c['seed'], k, name)
        main = 'be' if d['lay'] == 'be' else 'p3'
        save, zero = _saved_gates(rows, h, sd('save'))
        st, bk = dict(rows=rows, hidden=h, dh_prev_accumulate=int(d['acc'])), dict(bs=bs, zero=zero)
        _, st['dh'] = _place(main, bs, E, h, *ALIGNED, rnd(rows, h, seed=sd('dh')), dev, dtype, seed=sd('dh'))
        _, st['save'] = _place('be' if d['lay'] == 'be' else 'p', bs, E, 4 * h, *ALIGNED, save, dev, dtype, seed=sd('save'))
        st['h_prev'] = _place('p', bs, E, h, *ALIGNED, rnd(rows, h, seed=sd('h_prev')), dev, dtype, seed=sd('h_prev'))[1] if d['h_prev'] else None
        st['dh2'] = None
        if d['dh2'] or d['alias']:
            bk['dh2_base'], st['dh2'] = _place('p', bs, E, h, *ALIGNED, rnd(rows, h, seed=sd('dh2')), dev, dtype, fill=SENTINEL)
        for name, W in (('dgi', 3 * h), ('dgh', 3 * h)):
            bk[name + '_base'], st[name] = _place(main, bs, E, W, *ALIGNED, None, dev, dtype, fill=SENTINEL)
            bk[name + '_view'] = _view_of(main, bs, E, W, ALIGNED[0])
        if d['alias']:
            bk['dh_prev_base'], st['dh_prev'] = bk['dh2_base'], st['dh2']
        else:   # pre-filled with values of the gradient's size: accumulate = 1 adds to them, accumulate = 0 replaces them
            bk['dh_prev_base'], st['dh_prev'] = _place('p', bs, E, h, *ALIGNED, rnd(rows, h, seed=sd('dh_prev')), dev, dtype, fill=SENTINEL)
        bk['dh_prev_view'] = _view_of('p', bs, E, h, ALIGNED[0])
        st['u'] = st['du'] = None
        if d['share_u'] is not None:
            st['u'], st['du'] = steps[d['share_u']]['u'], steps[d['share_u']]['du']
        elif d['u']:
            _, st['u'] = _u_place(d['u'], bs, E, _gate_values(bs, E, sd('u')), dev, dtype, sd('u'))
            if d['du']:   # pre-filled with non-zero values: the kernel adds
                bk['du_base'], st['du'] = _u_place(d['u'], bs, E, rnd(rows, seed=sd('du')), dev, dtype, sd('du'))
        steps.append(st)
        book.append(bk)
    return steps, book


def step_bwd_run(Kx, c, dev, dtype):
    steps, book = step_bwd_build(c, dev, dtype)
    Kx.gru_step_bwd(steps)
    out = {}
    for k, (d, st, bk) in enumerate(zip(c['descs'], steps, book)):
        h = d['h']
        for name, W in (('dgi', 3 * h), ('dgh', 3 * h), ('dh_prev', h)):
            out[f'{name}{k}'] = (st[name].reshape(-1, W), JUDGE)
            out[f'{name}{k}_outside'] = (_outside(bk[name + '_base'], bk[name + '_view']), EXACT)
        zero = bk['zero'].to(dev)
        out[f'planted_zeros{k}'] = (torch.cat([st['dgi'].reshape(-1, 3 * h)[zero], st['dgh'].reshape(-1, 3 * h)[zero]]), EXACT)
        if 'du_base' in bk:
            out[f'du{k}'] = (st['du'].reshape(-1), JUDGE)
            out[f'du{k}_outside'] = (_outside(bk['du_base'], lambda b, f=d['u'], n=bk['bs']: _u_view(f, b, n)), EXACT)
    return out


# -------------------------------------------------------------------------------------------------- the frame recurrences
# bits of HipKernels.gemm_last_class() (TWOG_GEMM_CLASS_* of include/twog_gcn.h)
GATE, KSPLIT, GRUFWD, ROWS32, XSPLIT, X3 = 16, 32, 64, 128, 256, 512


def _rc(id, why, h, bs, T, Es, bias=True, nd=2, cls=None):
    return dict(id=id, why=why, h=h, bs=bs, T=T, Es=tuple(Es), bias=bias, nd=nd, cls=cls)


H_WHY = {16: 'below the fused forward (h < 32)', 32: 'one partly filled unit tile; 3h = 96 < 256: the plain gate-fused backward',
         50: 'h % 32 != 0 and h % 4 != 0: nothing 16-byte, forward unfused', 72: 'h % 32 != 0: forward unfused; a partial second unit tile in the backward',
         88: 'K = 3h = 264 >= 256 but no multiple of 16 or 32', 96: 'a partial second unit tile in the fused forward; K = 288',
         100: 'h % 32 != 0 with h % 4 == 0', 256: 'four whole unit tiles; the fused forward on the bf16 matrix cores from here',
         512: 'the product width: eight unit tiles, the limit of the gate-fused backward',
         544: 'nine unit tiles in the fused forward, the last partial; backward fusion refused ((h + 63) / 64 > 8)',
         576: 'nine whole unit tiles in the fused forward; backward fusion refused'}
T_WHY = {1: 'T = 1: first and last step coincide, the backward makes no GEMM', 2: 'T = 2: the only carry GEMM is the first and the last',
         3: 'T = 3: one middle step', 9: 'T = 9'}
REC_CASES = [_rc(f'h{h}_T{T}', f'{T_WHY[T]}; {H_WHY[h]}', h, 3, T, (2, 3, 1)) for h in H_WHY for T in T_WHY]
REC_CASES.append(_rc('h64_T33', 'T = 33: a chain long enough for a wrong step index to compound', 64, 3, 33, (2, 3, 1)))
# rows per (type, direction): around one and two 64-row (32-row) tiles, with inner > 1 wherever the number factors
ROW_SHAPES = {1: (1, 1), 31: (31, 1), 32: (4, 8), 33: (3, 11), 63: (7, 9), 64: (8, 8), 65: (5, 13), 130: (10, 13)}
for _h in (32, 96):
    for _rows, (_bs, _E) in ROW_SHAPES.items():
        REC_CASES.append(_rc(f'h{_h}_rows{_rows}', f'{_rows} rows per direction (bs = {_bs}, E = {_E}), one type', _h, _bs, 3, (_E,)))
    for _bs in (7, 32, 65):
        REC_CASES.append(_rc(f'h{_h}_bs{_bs}_E2_9_1', f'three types of different E in one call: rows {2 * _bs} / {9 * _bs} / {_bs}', _h, _bs, 3, (2, 9, 1)))
REC_CASES.append(_rc('h64_four_types', 'four types: the 8 descriptors of one chunk, 8 problems of one grouped launch', 64, 3, 3, (2, 3, 1, 4)))
for _h in (32, 72, 96):
    REC_CASES.append(_rc(f'h{_h}_no_bias', 'b_hh_f = b_hh_r = None: hn of the first step is exactly 0', _h, 3, 3, (2, 3, 1), bias=False))
REC_CASES += [_rc(f'seq_h{h}_T{T}', f'single direction (ND = 1), rows h / 3h wide; {T_WHY.get(T, "T = 5")}', h, 3, T, (2, 3, 1), nd=1,
                  bias=(T != 2)) for h in (16, 96, 512) for T in (1, 2, 5)]
# The gate-fused backward classes the default environment reaches (twog_internal_gemm_gate_bwd; DESIGN.md section 2 derives
# the shapes): per class the smallest (h, E, bs); t64 / t32 = 64-row / 32-row tiles of the launch.
REC_CLASS_CASES = [
    _rc('cls_plain', 'gemm_gate_bwd_kernel<2>: K = 96 < 256', 32, 3, 2, (2, 3, 1), cls=GATE),
    _rc('cls_xs32', 'gemm_gate_bwd_xs32_kernel: K = 288 >= 256 and t32 = 12 <= 256: 32-row tiles, reduction split over workgroups',
        96, 3, 2, (2, 3, 1), cls=GATE | KSPLIT | ROWS32 | XSPLIT),
    _rc('cls_xl', 'gemm_gate_bwd_x3su_kernel<1, 2> (XL): h = 512, t32 = 272 > 256, t64 = 144 in 129 .. 170: three slices promise 15 %',
        512, 27, 2, (19,), cls=GATE | X3 | XSPLIT),
    _rc('cls_xs64', 'gemm_gate_bwd_xs_kernel: K = 900 (no multiple of 32: not X3), t64 = 270 in 257 .. 384: two slices pay',
        300, 45, 2, (37,), cls=GATE | KSPLIT | XSPLIT),
    _rc('cls_x3su_workload', 'gemm_gate_bwd_x3su_kernel<2, 2>: the 176-tile launch of the workload (K % 64 == 0, t64 <= 256, neither split pays)',
        512, 64, 3, (2, 8, 1), cls=GATE | KSPLIT | X3),
    _rc('cls_x3s2', 'gemm_gate_bwd_x3s_kernel<2>: K = 288 a multiple of 32 but not of 64, t32 = 260 > 256, t64 = 132',
        96, 41, 2, (50,), cls=GATE | KSPLIT | X3),
    _rc('cls_ks', 'gemm_gate_bwd_ks_kernel<2>: K = 264 no multiple of 32, t32 = 260 > 256, t64 = 132 <= 384',
        88, 41, 2, (50,), cls=GATE | KSPLIT),
    _rc('cls_x3s1', 'gemm_gate_bwd_x3s_kernel<1>: h = 512, t64 = 400 > 384 and no XL split promises 15 %',
        512, 29, 2, (53,), cls=GATE | X3),
]
REC_ALL = REC_CASES + REC_CLASS_CASES
# E = 0 for one type among live ones. What the launchers do with it (read in csrc/gru.hip, csrc/gemm_f32.hip): the GEMM problem
# with M = 0 has no tile (prepare_group: tiles_m = 0; the tile -> problem search of the kernels takes the LAST problem whose
# tile_start is not beyond the tile, so a problem without tiles is never chosen), the gate descriptor with rows = 0 has no live
# block, the gate-fused launch skips a gate with rows <= 0: no buffer of that type is read or written. The fused forward step
# refuses such a call as a whole (rows <= 0 -> the GEMM + gate pair), so the case runs with TWOG_GRU_FWD_FUSION=0 on both sides.
REC_EMPTY_TYPE = _rc('h96_E2_0_3', 'E = 0 for one type among live ones: equal, bit for bit, to the call without that type', 96, 3, 3, (2, 0, 3))
REC_BY_ID = {c['id']: c for c in REC_ALL + [REC_EMPTY_TYPE]}
REC_TOO_MANY_TYPES = 5


@functools.lru_cache(maxsize=4)
def rec_inputs(id):
    """fp32 inputs of a recurrence case (cached: callers cast copies, never write)."""
    c = REC_BY_ID[id]
    h, bs, T, nd = c['h'], c['bs'], c['T'], c['nd']
    ws = min(0.2, 1.6 / h ** 0.5)   # hidden pre-activations stay O(1) at every width
    types = []
    for i, E in enumerate(c['Es']):
        sd = _seed(id, i)
        y = dict(gi=rnd(bs, T, E, nd * 3 * h, seed=sd), d_out=rnd(bs, T, E, nd * h, seed=sd + 5))
        for j, sfx in enumerate(('_f', '_r')[:nd]):
            y['w_hh' + sfx] = rnd(3 * h, h, seed=sd + 10 + j, scale=ws)
            y['b_hh' + sfx] = rnd(3 * h, seed=sd + 20 + j) if c['bias'] else None
        types.append(y)
    return types


def rec_run(Kx, c, dev, dtype, saved=None, part='both', live_only=False):
    """Forward, then the backward pass on the `out` / `save` of `saved` (the fp32 specification's, cast: isolates the backward
    launches). part: 'fwd' / 'bwd' / 'both'. The GEMM class after each pass goes along where Kx reports one. live_only: the
    types with E = 0 are left out of both calls (the results keep the numbers of the case's types)."""
    h, bs, T, nd = c['h'], c['bs'], c['T'], c['nd']
    number = [k for k, E in enumerate(c['Es']) if E > 0 or not live_only]
    ins = [rec_inputs(c['id'])[k] for k in number]
    cls_of = getattr(Kx, 'gemm_last_class', lambda: None)
    res = {}
    wkeys = ('w_hh_f', 'w_hh_r') if nd == 2 else ('w_hh_f',)
    if part != 'bwd':
        if nd == 2:
            types = [{k: cv(y[k], dev, dtype) for k in ('gi', 'w_hh_f', 'b_hh_f', 'w_hh_r', 'b_hh_r')} for y in ins]
            fw = Kx.bigru_fwd(types, bs, T, h)
        else:
            types = [dict(gi=cv(y['gi'], dev, dtype), w_hh=cv(y['w_hh_f'], dev, dtype), b_hh=cv(y['b_hh_f'], dev, dtype)) for y in ins]
            fw = Kx.gru_seq_fwd(types, bs, T, h)
        res['cls_fwd'] = (cls_of(), None)
        for k, (o, s) in zip(number, fw):
            res[f'out{k}'], res[f'save{k}'] = (o.reshape(-1, h), JUDGE), (s.reshape(-1, h), JUDGE)
    if part != 'fwd':
        src = saved if saved is not None else res
        E_of = lambda k: c['Es'][k]
        types = []
        for k, y in zip(number, ins):
            o = cv(src[f'out{k}'][0].reshape(bs, T, E_of(k), nd * h), dev, dtype)
            s = cv(src[f'save{k}'][0].reshape(*((2,) if nd == 2 else ()), bs, T, E_of(k), 4 * h), dev, dtype)
            t = dict(d_out=cv(y['d_out'], dev, dtype), save=s, out=o)
            if nd == 2:
                t.update(w_hh_f=cv(y['w_hh_f'], dev, dtype), w_hh_r=cv(y['w_hh_r'], dev, dtype))
            else:
                t['w_hh'] = cv(y['w_hh_f'], dev, dtype)
            types.append(t)
        bw = Kx.bigru_bwd(types, bs, T, h) if nd == 2 else Kx.gru_seq_bwd(types, bs, T, h)
        res['cls_bwd'] = (cls_of(), None)
        for k, (dgi, dgh) in zip(number, bw):
            res[f'd_gi{k}'], res[f'd_gh{k}'] = (dgi.reshape(-1, 3 * h), JUDGE), (dgh.reshape(-1, 3 * h), JUDGE)
    return res


def rec_fwd_fused(c, fusion):
    """Whether the forward chain of case c takes the fused step (gemm_gru_fwd_kernel) under TWOG_GRU_FWD_FUSION = fusion: the
    rule tests/test_kernels_gpu.py::test_bigru asserts."""
    return fusion == '7' and c['h'] % 32 == 0


def rec_bwd_fused(c, no_gate_fusion):
    """Whether the backward chain runs the gate backward in the epilogue of the carry GEMM (bigru_bwd_impl of csrc/gru.hip)."""
    return c['T'] > 1 and (c['h'] + 63) // 64 <= 8 and not no_gate_fusion
