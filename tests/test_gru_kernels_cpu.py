"""CPU companion of tests/test_gru_kernels_gpu.py: the specification of the GRU family and the case lists of tests/gru_cases.py
themselves.

  operation  the specification IS the operation, in fp64: bigru_fwd / gru_seq_fwd against torch.nn.GRU, the gated step against
             u * GRUCell(x, h) + (1 - u) * h, bigru_bwd (chained with the input-projection identity) and gru_step_bwd against
             autograd;
  builds     ids are unique and every case names its branch; every case runs through the specification in fp32 and in fp64: finite,
             outputs of the dtype of the inputs, what the GPU test demands bit for bit is the same value in both runs, every judged
             tensor has e_ref > 0 (a case whose fp32 specification is exact measures nothing), planted gates give exact zeros;
  reach      the forward-step cases reach the kernel, block size and launch count they state, by gru_step_vec_ok of csrc/gru.hip
             evaluated on the descriptors HipKernels would pack (rows_of);
  packing    rows_of / _u_fields address exactly the elements of the views the cases pass."""
import types

import pytest
import torch

import twog_gcn_amd  # noqa: F401
from twog_gcn_amd.kernels import HipKernels, rows_of
from tests import gru_cases as GC
from tests.entity_envelope import reference_error, sqrt_k_bound
from tests.gru_cases import F, EXACT

F32, F64 = torch.float32, torch.float64
# the fp32 specification against the fp64 one, relative to the tensor's largest value: a random walk over the longest sum of any
# case (the 1 536 products of the carried gradient at h = 512) with the head room of entity_envelope.sqrt_k_bound
AGREE = sqrt_k_bound(2048)


def rnd64(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64)


# ------------------------------------------------------------------------------------------ the specification is the operation
def _gru_and_projections(bs, T, E, I, h, nd, seed):
    """torch.nn.GRU in fp64, inputs x [bs][T][E][I], and the recurrence's operand gi = W_ih x + b_ih [bs][T][E][nd * 3h]."""
    torch.manual_seed(seed)
    gru = torch.nn.GRU(I, h, batch_first=True, bidirectional=nd == 2).double()
    x = rnd64(bs, T, E, I, seed=seed + 1).requires_grad_()
    sfx = ['', '_reverse'][:nd]
    gi = torch.cat([x @ getattr(gru, 'weight_ih_l0' + s).t() + getattr(gru, 'bias_ih_l0' + s) for s in sfx], -1)
    return gru, x, gi, sfx


def _torch_gru_out(gru, x):
    bs, T, E, I = x.shape
    out, _ = gru(x.permute(0, 2, 1, 3).reshape(bs * E, T, I))
    return out.reshape(bs, E, T, -1).permute(0, 2, 1, 3)


@pytest.mark.parametrize('nd', [2, 1])
@pytest.mark.parametrize('T', [1, 2, 5])
def test_recurrence_specification_equals_torch_gru_forward_and_backward(nd, T):
    bs, E, I, h = 2, 3, 5, 7
    gru, x, gi, sfx = _gru_and_projections(bs, T, E, I, h, nd, seed=10 * T + nd)
    want = _torch_gru_out(gru, x)
    w = [getattr(gru, 'weight_hh_l0' + s).detach() for s in sfx]
    b = [getattr(gru, 'bias_hh_l0' + s).detach() for s in sfx]
    if nd == 2:
        ty = dict(gi=gi.detach().contiguous(), w_hh_f=w[0], b_hh_f=b[0], w_hh_r=w[1], b_hh_r=b[1])
        (out, save), = F.bigru_fwd([ty], bs, T, h)
    else:
        (out, save), = F.gru_seq_fwd([dict(gi=gi.detach().contiguous(), w_hh=w[0], b_hh=b[0])], bs, T, h)
    assert out.dtype == save.dtype == F64
    assert float((out - want.detach()).abs().max()) <= 1e-12
    # backward: loss = sum(out * d_out); the specification's d_gi / d_gh chained with the projection identities
    d_out = rnd64(*want.shape, seed=99)
    (want * d_out).sum().backward()
    if nd == 2:
        (d_gi, d_gh), = F.bigru_bwd([dict(d_out=d_out, save=save, out=out, w_hh_f=w[0], w_hh_r=w[1])], bs, T, h)
    else:
        (d_gi, d_gh), = F.gru_seq_bwd([dict(d_out=d_out, save=save, out=out, w_hh=w[0])], bs, T, h)
    assert d_gi.dtype == d_gh.dtype == F64
    xd = x.detach()
    dx = 0
    for d, s in enumerate(sfx):
        gi_d, gh_d = d_gi[..., d * 3 * h:(d + 1) * 3 * h], d_gh[..., d * 3 * h:(d + 1) * 3 * h]
        w_ih = getattr(gru, 'weight_ih_l0' + s)
        dx = dx + gi_d @ w_ih.detach()
        hprev = torch.zeros(bs, T, E, h, dtype=F64)
        if d == 0:
            hprev[:, 1:] = out[:, :-1, :, :h]
        else:
            hprev[:, :-1] = out[:, 1:, :, h:]
        for got, par in ((gi_d.reshape(-1, 3 * h).t() @ xd.reshape(-1, I), w_ih), (gi_d.sum((0, 1, 2)), getattr(gru, 'bias_ih_l0' + s)),
                         (gh_d.reshape(-1, 3 * h).t() @ hprev.reshape(-1, h), getattr(gru, 'weight_hh_l0' + s)),
                         (gh_d.sum((0, 1, 2)), getattr(gru, 'bias_hh_l0' + s))):
            assert float((got - par.grad).abs().max()) <= 1e-10
    assert float((dx - x.grad).abs().max()) <= 1e-10


def _gated_cell_case(seed, with_u):
    bs, E, I, h = 3, 4, 5, 6
    torch.manual_seed(seed)
    cell = torch.nn.GRUCell(I, h).double()
    x, hp = rnd64(bs * E, I, seed=seed + 1), rnd64(bs * E, h, seed=seed + 2)
    u = torch.sigmoid(rnd64(bs, E, seed=seed + 3)) if with_u else None
    if with_u:
        u[0, 0], u[1, 1] = 0.0, 1.0
    return bs, E, h, cell, x, hp, u


@pytest.mark.parametrize('with_u', [True, False])
def test_step_specification_equals_the_gated_grucell_forward_and_backward(with_u):
    bs, E, h, cell, x, hp, u = _gated_cell_case(5, with_u)
    gi = (x @ cell.weight_ih.t() + cell.bias_ih).detach().reshape(bs, E, 3 * h).requires_grad_()
    gh = (hp @ cell.weight_hh.t() + cell.bias_hh).detach().reshape(bs, E, 3 * h).requires_grad_()
    want = cell(x, hp).reshape(bs, E, h)
    if with_u:
        want = u.unsqueeze(-1) * want + (1 - u.unsqueeze(-1)) * hp.reshape(bs, E, h)
    h_out, save = torch.zeros(bs, E, h, dtype=F64), torch.zeros(bs, E, 4 * h, dtype=F64)
    F.gru_step_fwd([dict(gi=gi.detach(), gi2=None, gh=gh.detach(), h_prev=hp.reshape(bs, E, h), h_out=h_out, save=save, u=u, rows=bs * E, hidden=h)])
    assert float((h_out - want.detach()).abs().max()) <= 1e-12
    # autograd of the same step written on gi / gh / h_prev / u as leaves
    hpl = hp.reshape(bs, E, h).clone().requires_grad_()
    ul = u.clone().requires_grad_() if with_u else None
    r, z, n, _, g = F._gates(gi, gh, hpl, h)
    new = g if ul is None else ul.unsqueeze(-1) * g + (1 - ul.unsqueeze(-1)) * hpl
    assert float((new.detach() - h_out).abs().max()) <= 1e-12
    dh, dh2 = rnd64(bs, E, h, seed=7), rnd64(bs, E, h, seed=8)
    (new * (dh + dh2)).sum().backward()
    dgi, dgh, dhp = (torch.zeros(bs, E, w, dtype=F64) for w in (3 * h, 3 * h, h))
    du = torch.full((bs, E), 0.5, dtype=F64) if with_u else None
    F.gru_step_bwd([dict(dh=dh, dh2=dh2, save=save, h_prev=hp.reshape(bs, E, h), dgi=dgi, dgh=dgh, dh_prev=dhp, u=u, du=du, rows=bs * E, hidden=h)])
    for got, leaf in ((dgi, gi), (dgh, gh), (dhp, hpl)):
        assert float((got - leaf.grad).abs().max()) <= 1e-10
    if with_u:
        assert float((du - 0.5 - ul.grad).abs().max()) <= 1e-10


# ----------------------------------------------------------------------------------------------------------- the case lists
LISTS = [('step_fwd', GC.STEP_FWD_CASES, GC.step_fwd_run), ('step_bwd', GC.STEP_BWD_CASES, GC.step_bwd_run)]


def test_ids_are_unique_and_every_case_names_its_branch():
    for cases in (GC.STEP_FWD_CASES, GC.STEP_BWD_CASES, GC.REC_ALL):
        assert len({c['id'] for c in cases}) == len(cases)
        assert all(c['why'] for c in cases)
    assert {c['same_as'] for c in GC.STEP_FWD_CASES if c['same_as']} <= set(GC.STEP_FWD_BY_ID)
    assert set(GC.HIDDEN) == {64, 128, 256, 512, 1024, 32, 100, 192, 768, 1028, 1, 3, 63, 65, 255, 257, 300}
    assert {c['T'] for c in GC.REC_CASES if c['nd'] == 2} >= {1, 2, 3, 9, 33}
    assert {c['h'] for c in GC.REC_CASES if c['nd'] == 2} >= {16, 32, 50, 72, 88, 96, 100, 256, 512, 544, 576}
    assert len({c['cls'] for c in GC.REC_CLASS_CASES}) == 7   # two kernels share GATE | KSPLIT | X3


def _check_runs(name, s32, s64):
    for k, (a, how) in s32.items():
        b = s64[k][0]
        if how is None:
            continue
        assert a.dtype == F32 and b.dtype == F64 and a.shape == b.shape, (name, k, a.dtype, b.dtype)
        assert torch.isfinite(a).all() and torch.isfinite(b).all(), (name, k)
        if how == EXACT:
            assert torch.equal(a.double(), b), f'{name}/{k}: demanded bit for bit of the kernel, but the fp32 and fp64 specification differ'
        elif a.numel():
            e = reference_error(a, b)
            assert 0 < e <= AGREE, f'{name}/{k}: e_ref = {e:.3e}'


@pytest.mark.parametrize('name,cases,run', LISTS, ids=[l[0] for l in LISTS])
def test_every_step_case_builds_in_both_precisions(name, cases, run):
    for c in cases:
        s32, s64 = run(F, c, 'cpu', F32), run(F, c, 'cpu', F64)
        _check_runs(f"{name}/{c['id']}", s32, s64)
        for k, (a, how) in s32.items():
            if k.startswith('planted_zeros'):
                assert a.numel() or c['descs'][int(k[13:])]['rows'] == 0
                assert float(a.abs().max() if a.numel() else 0) == 0.0 and float(s64[k][0].abs().max() if a.numel() else 0) == 0.0, (c['id'], k)
            if k.endswith('_mask'):
                rz = s32[k[:-4] + 'rz'][0]
                assert int(a.sum()) >= a.numel() // 4 and bool(((rz[a] == 0) | (rz[a] == 1) | (rz[a] < 1e-38)).all()), c['id']


def test_gate_of_zero_passes_the_previous_state_and_gate_of_one_the_ungated_state():
    for c in GC.STEP_FWD_CASES:
        for k, d in enumerate(c['descs']):
            if not d['u']:
                continue
            steps, book = GC.step_fwd_build(c, 'cpu', F32)
            s32 = GC.step_fwd_run(F, c, 'cpu', F32)
            u0 = book[k]['u_vals'] == 0
            hp = steps[k]['h_prev'].reshape(-1, d['h'])[u0] if d['h_prev'] else torch.zeros(int(u0.sum()), d['h'])
            assert torch.equal(s32[f'h_out{k}_where_u0'][0], hp), c['id']
            assert float(s32[f'h_out{k}_where_u1_minus_ungated'][0].abs().max()) == 0.0


@pytest.mark.parametrize('c', GC.REC_ALL + [GC.REC_EMPTY_TYPE], ids=lambda c: c['id'])
def test_every_recurrence_case_builds_in_both_precisions(c):
    s32 = GC.rec_run(F, c, 'cpu', F32)
    s64 = GC.rec_run(F, c, 'cpu', F64, saved=s32)
    _check_runs(c['id'], s32, s64)
    assert len(c['Es']) <= 4 < GC.REC_TOO_MANY_TYPES
    if c is GC.REC_EMPTY_TYPE:
        live = GC.rec_run(F, c, 'cpu', F32, live_only=True)
        assert all(torch.equal(v, live[k][0]) for k, (v, how) in s32.items() if how and v.numel()) and len(live) == len(s32) - 4
    if not c['bias']:   # hn of the first step of either direction: rows that are exactly zero, which the judge demands of the kernel
        assert int((s32['save0'][0].abs().amax(1) == 0).sum()) == c['nd'] * c['bs'] * c['Es'][0]


# ------------------------------------------------------------------------------------------------------------------- reach
@pytest.mark.parametrize('c', GC.STEP_FWD_CASES, ids=lambda c: c['id'])
def test_forward_step_cases_reach_the_kernel_they_state(c):
    assert GC.step_fwd_vec_expected(c) == (c['vec'], c['threads'], c['launches'])


def test_the_alignment_variants_differ_from_their_aligned_case_in_one_operand_only():
    assert len(GC.ALIGN_BREAKS) == 2 * (6 * 2 + 4)
    for id in GC.ALIGN_BREAKS:
        c = GC.STEP_FWD_BY_ID[id]
        a = GC.STEP_FWD_BY_ID[c['same_as']]
        assert a['vec'] and not c['vec'] and len(c['descs'][0]['at']) == 1
        assert {k: v for k, v in c['descs'][0].items() if k != 'at'} == {k: v for k, v in a['descs'][0].items() if k != 'at'}
        s_c, s_a = GC.step_fwd_run(F, c, 'cpu', F32), GC.step_fwd_run(F, a, 'cpu', F32)
        assert torch.equal(s_c['h_out0'][0], s_a['h_out0'][0]) and torch.equal(s_c['save0'][0], s_a['save0'][0]), id


# ----------------------------------------------------------------------------------------------------------------- packing
def _row_address(t, i):
    return t[i].data_ptr() if t.dim() == 2 else t[i // t.shape[1], i % t.shape[1]].data_ptr()


def _check_rows(t, rows, width, what):
    if t is None or rows == 0:
        return
    r = rows_of(t)
    assert t.shape[-1] == width and t.numel() == rows * width, what
    inner = max(r.inner, 1)
    for i in range(rows):
        assert r.ptr + 4 * ((i // inner) * r.ld_outer + (i % inner) * r.ld_inner) == _row_address(t, i), (what, i)


def _check_u(u, rows, what):
    g = types.SimpleNamespace()
    HipKernels._u_fields(g, u)
    if u is None:
        assert (g.u, g.u_inner) == (0, 1)
        return
    for i in range(rows):   # gate_u of csrc/gru.hip
        off = i * g.u_ld_outer if g.u_inner <= 1 else (i // g.u_inner) * g.u_ld_outer + (i % g.u_inner) * g.u_ld_inner
        assert g.u + 4 * off == u[i // u.shape[1], i % u.shape[1]].data_ptr(), (what, i)


def test_descriptor_packing_addresses_the_rows_of_the_views_the_cases_pass():
    for c in GC.STEP_FWD_CASES:
        steps, _ = GC.step_fwd_build(c, 'cpu', F32)
        for st in steps:
            h = st['hidden']
            for k, w in (('gi', 3 * h), ('gi2', 3 * h), ('gh', 3 * h), ('h_prev', h), ('h_out', h), ('save', 4 * h)):
                _check_rows(st[k], st['rows'], w, (c['id'], k))
            _check_u(st['u'], st['rows'], c['id'])
    for c in GC.STEP_BWD_CASES:
        steps, _ = GC.step_bwd_build(c, 'cpu', F32)
        for st in steps:
            h = st['hidden']
            for k, w in (('dh', h), ('dh2', h), ('save', 4 * h), ('h_prev', h), ('dgi', 3 * h), ('dgh', 3 * h), ('dh_prev', h)):
                _check_rows(st[k], st['rows'], w, (c['id'], k))
            _check_u(st['u'], st['rows'], c['id'])
            if st['du'] is not None:
                assert st['du'].shape == st['u'].shape and st['du'].stride() == st['u'].stride(), c['id']   # "addressed like u"
