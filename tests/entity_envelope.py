"""The entity range of the tuned attention family (up to 4 humans and 12 objects): case lists, the executable specification
run in fp32 and in fp64, and the rule by which a kernel result is judged. Shared by tests/test_entity_envelope_cpu.py
(specification fp32 vs fp64) and tests/test_entity_envelope_gpu.py (HIP kernels vs both).

How a result is judged. For an output tensor X: hip (fp32, GPU), s32 (the specification in fp32 on the CPU), s64 (the
specification in fp64 on fp64 copies of the same inputs);
    e_hip = max|hip - s64| / max|s64|,  e_ref = max|s32 - s64| / max|s64|,  required: e_hip <= factor * e_ref + 4 * 2^-24.
The yardstick is the fp32 specification's own error, measured per tensor: never a number taken from the kernel. factor = 8
covers a different summation tree of the same length, expf and the kernels' fused multiply-adds; the floor covers tensors
the specification reproduces exactly (copies: e_ref = 0). The same rule holds for the worst ROW (each row scaled by its own
largest |s64|, e_ref taken from that row): the tensor-wide maximum hides an error confined to one small receiver, which is
what a wrong index for human 3 or object 11 produces. Rows that are zero in the specification (masked or virtual entities)
must be exactly zero."""
import functools
import math

import torch

from tests.fake_kernels import FakeKernels
from tests.kernel_cases import rnd, _attn_case, _seg_params, attn_bwd_case

F = FakeKernels()
EPS = 2.0 ** -24
FACTOR = 8.0            # see the module docstring
FACTOR_X3 = 8.0 * 1.25  # tensors behind the X3 GEMMs (bf16 matrix cores, fp32 split in three): 1.25 is the measured ratio of
                        # the X3 error to the native fp32-MFMA error (test_gemm_x3_error_equals_the_native_fp32_mfma_kernels)

# bits of HipKernels.attn_last_path() (TWOG_ATTN_PATH_* of include/twog_gcn.h)
STAGED, GRAM_COLS, DW_COLS, DW_WG, BWD = 1, 2, 4, 8, 16


def path(bits, threads):
    return bits | threads << 16


FWD_STAGED, FWD_ROWS, FWD_COLS = path(STAGED, 1024), path(0, 512), path(GRAM_COLS, 256)
BWD_STAGED, BWD_STAGED_WG = path(BWD | STAGED, 1024), path(BWD | STAGED | DW_WG, 1024)
BWD_ROWS, BWD_COLS = path(BWD, 256), path(BWD | DW_COLS, 256)


def _c(H, O, D, h, n_inst, ipc, fwd, bwd, sh=True, dwx=False, why='', fwd_row_factor=None):
    return dict(H=H, O=O, D=D, h=h, n_inst=n_inst, ipc=ipc, fwd=fwd, bwd=bwd, sh=sh, dwx=dwx, why=why,
                fwd_row_factor=fwd_row_factor,
                id=f'H{H}_O{O}_D{D}_h{h}_n{n_inst}')


# latency regime (at most 1024 instances: rows staged in LDS while they fit 160 KB)
ATTN_LATENCY = [
    _c(3, 3, 64, 32, 6, 3, FWD_STAGED, BWD_STAGED, dwx=True, why='E = 6 with three humans'),
    _c(2, 4, 64, 32, 6, 2, FWD_STAGED, BWD_STAGED_WG, why='E = 6'),
    _c(3, 4, 96, 48, 9, 3, FWD_STAGED, BWD_STAGED, sh=False, why='E = 7'),
    _c(4, 12, 128, 64, 8, 2, FWD_STAGED, BWD_STAGED, dwx=True, why='the corner: staged pair loop with natt = 256, Q = 4'),
    _c(4, 12, 1024, 512, 6, 2, FWD_STAGED, BWD_ROWS, dwx=True,
       why='the corner at full width: the backward rows (82 x 516 floats) overflow the LDS -> unstaged'),
    _c(4, 1, 64, 32, 12, 3, FWD_STAGED, BWD_STAGED, why='one object: object -> object off'),
    _c(1, 12, 64, 32, 6, 2, FWD_STAGED, BWD_STAGED, sh=False, why='one human: human -> human off; O > 8 keeps the pair loop'),
    _c(3, 10, 128, 64, 10, 2, FWD_STAGED, BWD_STAGED, why='E = 13'),
    _c(4, 11, 40, 20, 9, 3, FWD_STAGED, BWD_STAGED, dwx=True, why='widths that are multiples of 4 but not of 8 / 64'),
    _c(2, 9, 2048, 1024, 6, 3, FWD_ROWS, BWD_ROWS, why='forward and backward overflow the LDS: unstaged at few instances'),
    _c(2, 8, 1024, 512, 6, 2, FWD_STAGED, BWD_STAGED_WG, dwx=True, why='wave-group dL/dw on (H <= 2, O <= 8)'),
    _c(3, 8, 1024, 512, 6, 2, FWD_STAGED, BWD_STAGED, dwx=True, why='wave-group dL/dw off across the H <= 2 boundary'),
]
# throughput regime (more than 1024 instances: streaming from global memory)
ATTN_THROUGHPUT = [
    _c(3, 3, 64, 32, 1100, 10, FWD_COLS, BWD_ROWS, why='column Gram <6,16>; row-form backward (H > 2)'),
    _c(4, 2, 200, 48, 1100, 10, FWD_COLS, BWD_ROWS, dwx=True, sh=False, why='column Gram <6,16>; row-form backward'),
    _c(3, 7, 1024, 512, 1100, 10, FWD_COLS, BWD_ROWS, dwx=True, why='column Gram <10,64> at full width'),
    _c(4, 6, 64, 32, 1100, 10, FWD_COLS, BWD_ROWS, why='column Gram <10,64>'),
    _c(1, 9, 200, 48, 1100, 10, FWD_COLS, BWD_ROWS, dwx=True, why='column Gram <10,64>; O > 8 with H <= 2: row-form backward'),
    _c(2, 8, 64, 32, 1100, 10, FWD_COLS, BWD_COLS, dwx=True, why='both column forms (the baseline layout, as an anchor)'),
    _c(3, 8, 200, 48, 1100, 10, FWD_ROWS, BWD_ROWS, sh=False, why='E = 11: row-parallel Gram'),
    # Row factor 32 (forward only; tensor-wide it stays 8 and needs 1.03). Measured on an MI355X: 1 to 15 of the 4 400 /
    # 13 200 receiver rows per tensor need 9.1 ... 24.1 (att_oo; profiles/r07_entity_envelope_fp64.json), every other case at
    # most 3.5. Why: at D = 1024 a receiver's weights and its message sum inherit the rounding error of a few 1024-term
    # scores, so the error of a row is essentially ONE random number per implementation -- not the maximum over many
    # independent roundings as in the wide rows. Among 17 600 such rows of 4 to 12 weights there are rows where the
    # specification's error happens to be 20 to 30 times below its typical size (e_ref of those rows: 1.3e-8 ... 9e-8, under
    # one ulp of the row's largest weight) while the kernel's independent error is of typical size (4e-7 ... 1.2e-6 of the
    # row maximum: 1 to 2.5 times the TENSOR-wide e_ref of 4e-7). A ratio of two independent errors over that many short
    # rows has this tail whatever the kernel does; a lost sender or a wrong index is a 1e-2 ... 1e-4 effect and fails at 32
    # as at 8. 32 is the ceiling up to which the rule accepts a stated reason; it is not fitted to the 24.1.
    _c(4, 12, 1024, 512, 1100, 10, FWD_ROWS, BWD_ROWS, dwx=True, why='the corner at full width, streaming', fwd_row_factor=32.0),
    _c(2, 12, 64, 32, 1100, 10, FWD_ROWS, BWD_ROWS, why='E = 14'),
]
ATTN_CASES = ATTN_LATENCY + ATTN_THROUGHPUT
# one grouped launch, throughput regime: the host decides per launch over all descriptors, so the (2, 8) descriptor runs
# the non-column forms; it has fewer instances than the launch's grid is wide
GROUPED = [_c(2, 8, 64, 32, 1040, 10, FWD_ROWS, BWD_ROWS, dwx=True), _c(4, 12, 64, 32, 1100, 10, FWD_ROWS, BWD_ROWS, dwx=True)]
GROUPED_ALLOC = 1100

# (H, O, ph, ps, cols): sender-side projection glue (ssp.hip accepts H <= 4, O <= 16); 1536 = 3h at h = 512
SSP_CASES = [(4, 12, True, True, 1536), (4, 16, True, False, 96), (1, 16, False, True, 96), (3, 13, True, True, 96),
             (4, 16, True, True, 200)]
SSP_GATHER = (3, 5, 4, 12, 48)   # (bs, T, H, O, cols) at the segment-level placement

# (bs, T, H, O, h) of the launch-per-step segment recurrence; the third has 72 object rows: more than one 64-row tile
SEG_STEPWISE = [(3, 5, 4, 12, 64), (2, 4, 3, 10, 128), (6, 3, 4, 12, 512), (5, 4, 3, 11, 96)]
# persistent launch: one chunk of 16 / 32 rows exactly, two object tiles ((2,7,..), (4,5,..), (3,6,..)), a ragged last chunk
# ((3,6,..): chunks of 2 and 1 clips)
SEG_PERSISTENT = [(8, 6, 4, 12, 64), (2, 7, 4, 12, 512), (4, 5, 4, 8, 512), (3, 6, 3, 10, 256)]
SEG_FWD_KEYS = ['hs_h', 'hs_o', 'save_h', 'save_o', 'msrc_h', 'msrc_o', 'mg_h', 'mg_o', 'att']


def to64(x):
    if isinstance(x, torch.Tensor):
        return x.double() if x.dtype == torch.float32 else x.clone()
    if isinstance(x, dict):
        return {k: to64(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(to64(v) for v in x)
    return x


# ------------------------------------------------------------------------------------------------------------ attention
def attn_desc(c, dev, seed=11, n_alloc=None):
    """Forward descriptor of case c: partly masked clips and an all-virtual one, receiver mask on, geometry senders on.
    n_alloc: the buffers hold that many instances, the descriptor covers the first n_inst of them."""
    H, O = c['H'], c['O']
    d = _attn_case(dev, H, O, c['D'], c['h'], n_alloc or c['n_inst'], c['ipc'], True, 1, seed=seed)
    d['n_inst'] = c['n_inst']
    if H == 1:
        d['msg_hh'] = None
        d.pop('out_hh')
    if O == 1:
        d['msg_oo'] = None
        d.pop('out_oo')
    if not c['sh']:
        d.pop('msg_sh')
        d.pop('out_sh')
    return d


def first_instances(d, n, n_alloc):
    """The row tensors of a descriptor built for n_alloc instances cut to the first n (the specification reshapes by n_inst)."""
    out = {}
    for k, v in d.items():
        if isinstance(v, torch.Tensor) and k != 'obj_mask' and v.shape[0] % n_alloc == 0:
            v = v[:n * (v.shape[0] // n_alloc)]
        out[k] = first_instances(v, n, n_alloc) if isinstance(v, dict) else v
    return out


def attn_outputs(d):
    return {k: v for k, v in d.items() if k.startswith('out_') or k == 'att'}


def attn_bwd_outputs(b):
    return {k: v for k, v in b.items() if k.startswith('dmsg_') or k in ('dfeat_h', 'dfeat_o')}


def attn_spec(c, seed=11, n_alloc=None):
    """The specification of case c in fp32 and fp64: (d32, d64, b32, b64). The backward pass of both reads the fp32 run's saved
    weights, as the kernel under test does."""
    d32 = attn_desc(c, 'cpu', seed, n_alloc)
    b32 = attn_bwd_case('cpu', dict(d32, n_inst=n_alloc or c['n_inst']), seed=seed + 100, dw_extra=c['dwx'])
    if n_alloc:
        d32 = first_instances(d32, c['n_inst'], n_alloc)
        b32 = first_instances(b32, c['n_inst'], n_alloc)
    b32['f'] = d32
    d64 = to64(d32)
    F.attn_fwd([d32])
    F.attn_fwd([d64])
    b64 = to64({k: v for k, v in b32.items() if k != 'f'})
    b64['f'] = dict(d64, att=d32['att'].double())
    F.attn_bwd([b32])
    F.attn_bwd([b64])
    return d32, d64, b32, b64


def split_att(att, n, H, O):
    """The saved weights [n][natt] as one (receivers, senders) matrix per relation."""
    att = att.reshape(n, -1)
    out, o = {}, 0
    for r, (R, S) in (('hh', (H, H)), ('oh', (H, O)), ('ho', (O, H)), ('oo', (O, O))):
        out['att_' + r] = att[:, o:o + R * S].reshape(n * R, S)
        o += R * S
    return out


def att_structure_failures(att, d):
    """Structural checks of the saved weights of a forward call: rows of active receivers sum to 1, excluded and masked
    senders have weight exactly 0, nothing is NaN (the all-virtual clip yields zeros)."""
    n, H, O = d['n_inst'], d['H'], d['O']
    fails = []
    att = att.detach().cpu().double().reshape(-1, H * H + 2 * H * O + O * O)[:n]
    if not torch.isfinite(att).all():
        fails.append('non-finite attention weights')
    m = d['obj_mask'].detach().cpu().repeat_interleave(d['inst_per_clip'], 0)[:n] != 0    # (n, O)
    w = {k: v.reshape(n, -1, v.shape[-1]) for k, v in split_att(att, n, H, O).items()}
    eyeH, eyeO = torch.eye(H, dtype=torch.bool), torch.eye(O, dtype=torch.bool)
    valid = {'att_hh': (~eyeH).expand(n, H, H), 'att_oh': m.unsqueeze(1).expand(n, H, O),
             'att_ho': torch.ones(n, O, H, dtype=torch.bool), 'att_oo': (~eyeO).unsqueeze(0) & m.unsqueeze(1)}
    for k, ok in valid.items():
        x = w[k]
        if d.get('msg_' + k[4:]) is None:   # relation off: all weights zero
            ok = torch.zeros(x.shape, dtype=torch.bool)
        if (~ok).any() and float(x[~ok].abs().max()) != 0.0:
            fails.append(f'{k}: an excluded or masked sender has a non-zero weight')
        active = ok.any(-1)
        S = x.shape[-1]
        off = (x.sum(-1) - 1.0).abs()[active]
        if off.numel() and float(off.max()) > 4 * EPS * S:
            fails.append(f'{k}: a row of weights sums to 1 {float(off.max()):.2e} off (> 4 ulp x {S})')
    return fails


# ------------------------------------------------------------------------------------------------------- the judgement
def _rows(t):
    return t.reshape(-1, t.shape[-1]) if t.dim() > 1 else t.reshape(1, -1)


def reference_error(s32, s64):
    s32, s64 = s32.detach().cpu().double(), s64.detach().cpu().double()
    scale = float(s64.abs().max()) if s64.numel() else 0.0
    return (float((s32 - s64).abs().max()) / scale) if scale > 0 else 0.0


_EMPTY = dict(e_hip=0.0, e_ref=0.0, ratio=0.0, row_e_hip=0.0, row_e_ref=0.0, row_ratio=0.0, row=-1)


def judge(hip, s32, s64, factor=FACTOR, row_factor=None):
    """-> (record, failures). record: e_hip, e_ref, ratio = (e_hip - floor) / e_ref (the factor this tensor needs), and the
    same for the row that needs the largest factor. row_factor: the factor of the row-wise rule where it differs."""
    row_factor = factor if row_factor is None else row_factor
    hip, s32, s64 = (t.detach().cpu().double() for t in (hip, s32, s64))
    assert hip.shape == s32.shape == s64.shape, (hip.shape, s32.shape, s64.shape)
    fails = []
    if not hip.numel():
        return dict(_EMPTY), fails
    if not torch.isfinite(hip).all():
        fails.append('non-finite values')
        hip = torch.nan_to_num(hip, nan=1e30, posinf=1e30, neginf=-1e30)
    floor = 4 * EPS
    need = lambda e, ref: 0.0 if e <= floor else ((e - floor) / ref if ref > 0 else float('inf'))
    scale = float(s64.abs().max())
    if scale == 0.0:
        if float(hip.abs().max()) != 0.0:
            fails.append('the specification is all zeros, the kernel result is not')
        return dict(_EMPTY), fails
    e_hip, e_ref = float((hip - s64).abs().max()) / scale, float((s32 - s64).abs().max()) / scale
    if e_hip > factor * e_ref + floor:
        fails.append(f'e_hip {e_hip:.3e} > {factor:g} x e_ref {e_ref:.3e} + 4 x 2^-24 (needs {need(e_hip, e_ref):.1f})')
    rh, r32, r64 = _rows(hip), _rows(s32), _rows(s64)
    rs = r64.abs().amax(1)
    live = rs > 0
    if (~live).any() and float(rh[~live].abs().max()) != 0.0:
        bad = int(torch.nonzero((~live) & (rh.abs().amax(1) != 0))[0])
        fails.append(f'row {bad} is zero in the specification (masked / virtual entity) and not exactly zero in the kernel result')
    rsafe = rs.clamp_min(1e-300)
    er_hip = torch.where(live, (rh - r64).abs().amax(1) / rsafe, torch.zeros_like(rs))
    er_ref = torch.where(live, (r32 - r64).abs().amax(1) / rsafe, torch.zeros_like(rs))
    excess = er_hip - (row_factor * er_ref + floor)
    ratio_rows = torch.where(er_hip > floor, (er_hip - floor) / er_ref.clamp_min(1e-300), torch.zeros_like(rs))
    wr = int(torch.argmax(ratio_rows))
    if float(excess.max()) > 0:
        br = int(torch.argmax(excess))
        fails.append(f'row {br} of {rh.shape[0]}: e_hip {float(er_hip[br]):.3e} > {row_factor:g} x e_ref {float(er_ref[br]):.3e} '
                     f'+ 4 x 2^-24 (needs {need(float(er_hip[br]), float(er_ref[br])):.1f}; {int((excess > 0).sum())} rows beyond)')
    rec = dict(e_hip=e_hip, e_ref=e_ref, ratio=need(e_hip, e_ref), row_e_hip=float(er_hip[wr]), row_e_ref=float(er_ref[wr]),
               row_ratio=need(float(er_hip[wr]), float(er_ref[wr])), row=wr)
    return rec, fails


# ------------------------------------------------------------------------------------------------ segment recurrence
def seg_factor(h):
    return FACTOR_X3 if h >= 256 else FACTOR   # wide reductions multiply on the bf16 matrix cores (X3)


@functools.lru_cache(maxsize=2)
def seg_spec(bs, T, H, O, h):
    """(forward buffers fp32 / fp64, incoming gradients, backward outputs fp32 / fp64); both backward runs read the fp32
    forward buffers, as the kernel under test does. (Cached: callers must not write into the result.)"""
    p32 = _seg_params('cpu', bs, T, H, O, h, (True, True, True, True), True)
    p64 = to64(p32)
    wih_h, wih_o = p64['_keep']   # the message blocks of W_ih are views of the whole matrices: rebuilt from the fp64 copies
    p64['w_ihm_h'], p64['w_ihm_o'] = [w[:, 3 * h:] for w in wih_h], [w[:, 4 * h:] for w in wih_o]
    b32, b64 = F.segrnn_fwd(p32), F.segrnn_fwd(p64)
    dh_h, dh_o = rnd(bs, T, H, 2 * h, seed=31), rnd(bs, T, O, 2 * h, seed=32)
    o32 = F.segrnn_bwd(p32, b32, dh_h, dh_o)
    o64 = F.segrnn_bwd(p64, to64(b32), dh_h.double(), dh_o.double())
    return b32, b64, (dh_h, dh_o), o32, o64


# ------------------------------------------------------------------------------------------- sender-side projection
def ssp_inputs(H, O, ph_on, ps_on, cols, n_inst=12, ipc=4):
    natt = H * H + 2 * H * O + O * O
    att = torch.softmax(rnd(n_inst, natt, seed=1), -1)
    mask = (rnd(n_inst // ipc, O, seed=2) > -0.5).float()
    mask[0] = 0
    return dict(att=att, mask=mask, gi=rnd(n_inst * O, cols, seed=3), ph=rnd(n_inst * H, cols, seed=4) if ph_on else None,
                ps=rnd(n_inst, cols, seed=5) if ps_on else None, dgi=rnd(n_inst * O, cols, seed=6), natt=natt,
                off=H * H + H * O, n_inst=n_inst, ipc=ipc)


def ssp_run(Kx, i, H, O, ps_on, dev='cpu', dtype=torch.float32, gi_zero=False):
    """ssp_fwd and ssp_bwd of Kx on the inputs i -> dict of result tensors (gi, qh, qs, dw where defined)."""
    cv = lambda t: None if t is None else t.to(dtype).to(dev)
    gi, ph, ps, att, mask, dgi = (cv(i[k]) for k in ('gi', 'ph', 'ps', 'att', 'mask', 'dgi'))
    gi = torch.zeros_like(gi) if gi_zero else gi.clone()
    Kx.ssp_fwd(gi, ph, ps, att, mask, i['n_inst'], i['ipc'], H, O, i['off'])
    dw = torch.zeros(i['n_inst'], i['natt'], dtype=dtype, device=dev)
    qh, qs = Kx.ssp_bwd(dgi, ph, att, mask, i['n_inst'], i['ipc'], H, O, i['off'], ps_on, dw=dw)
    out = dict(gi=gi)
    if ph is not None:
        out.update(qh=qh, dw=dw)
    if ps_on:
        out['qs'] = qs
    return out


def ssp_gather_inputs():
    bs, T, H, O, cols = SSP_GATHER
    natt = H * H + 2 * H * O + O * O
    return dict(att=torch.softmax(rnd(T, bs, natt, seed=1), -1), dgi_full=rnd(bs * T * O, 2 * cols, seed=2), natt=natt,
                off=H * H + H * O)


def ssp_gather_run(Kx, i, dev='cpu', dtype=torch.float32):
    bs, T, H, O, cols = SSP_GATHER
    att, dgi = i['att'].to(dtype).to(dev), i['dgi_full'].to(dtype).to(dev)
    return Kx.ssp_gather(dgi[:, cols:], att, i['natt'], bs * i['natt'], i['off'], bs * T, T, H, O)


def sqrt_k_bound(K):
    """Random-walk bound of an fp32 sum of K terms, relative to the largest value: 16 x 2^-24 x sqrt(K)."""
    return 16 * EPS * math.sqrt(K)
