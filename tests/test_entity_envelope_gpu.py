"""GPU: the tuned attention family over its whole entity range -- up to 4 humans and 12 objects (16 objects for the
sender-side projection glue): csrc/attn.hip, ssp.hip, segrnn.hip, seg_persist.hip. Every case asserts the code path it was
written for (HipKernels.attn_last_path / last_segrnn_persistent), runs twice (bit-identical: fixed summation order) and
is judged against the executable specification run in fp64, with the fp32 specification's own error as the yardstick,
tensor-wide and per row (tests/entity_envelope.py). tests/test_entity_envelope_cpu.py checks the fp64 specification itself.

TWOG_ENVELOPE_RECORD=<file>: e_hip, e_ref and their ratio of every (case, tensor) are written there as JSON
(profiles/r07_entity_envelope_fp64.json is such a record)."""
import json
import os

import pytest
import torch

import twog_gcn_amd  # noqa: F401
from twog_gcn_amd import kernels as twog_kernels
from tests import entity_envelope as EE
from tests.entity_envelope import F, FACTOR
from tests.kernel_cases import _seg_params, attn_bwd_case

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
RECORDS = {}


@pytest.fixture(scope='module')
def K():
    twog_kernels._set_backend_for_tests(None)
    k = twog_kernels.get_kernels()
    assert k.name == 'hip'
    yield k
    dst = os.environ.get('TWOG_ENVELOPE_RECORD')
    if dst and RECORDS:
        fin = lambda v: v if not isinstance(v, float) or v == v and abs(v) != float('inf') else str(v)
        with open(dst, 'w') as f:
            json.dump({k_: {a: fin(b) for a, b in r.items()} for k_, r in sorted(RECORDS.items())}, f, indent=1)


class Verdict:
    """Collects the judgement of every tensor of one case: all of them are measured (and recorded) before the case fails."""

    def __init__(self, case):
        self.case, self.fails, self.worst, self.worst_row = case, [], (0.0, ''), (0.0, '')

    def add(self, name, hip, s32, s64, factor=FACTOR, row_factor=None):
        rec, fails = EE.judge(hip, s32, s64, factor, row_factor)
        RECORDS[f'{self.case}/{name}'] = dict(rec, factor=factor, row_factor=row_factor or factor)
        self.fails += [f'{name}: {f}' for f in fails]
        self.worst, self.worst_row = max(self.worst, (rec['ratio'], name)), max(self.worst_row, (rec['row_ratio'], name))

    def same(self, name, a, b):
        if not torch.equal(a, b):
            self.fails.append(f'{name}: two runs of the same call differ')

    def check(self):
        print(f'{self.case}: worst e_hip / e_ref {self.worst[0]:.2f} ({self.worst[1]}), worst row {self.worst_row[0]:.2f} '
              f'({self.worst_row[1]})')
        assert not self.fails, f'{self.case}:\n  ' + '\n  '.join(self.fails)


def close(a, b, rtol, atol, what):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    err = (a - b).abs().max().item() if a.numel() else 0.0
    tol = atol + rtol * b.abs().max().item() if b.numel() else atol
    assert err <= tol, f'{what}: max err {err:.3e} > tol {tol:.3e}'


# ------------------------------------------------------------------------------------------------------------ attention
def _judge_forward(V, c, dg, dg2, d32, d64, tag=''):
    n, H, O = c['n_inst'], c['H'], c['O']
    for k in EE.attn_outputs(d32):
        got = dg[k][:d32[k].shape[0]]
        V.add(tag + k, got, d32[k], d64[k], row_factor=c['fwd_row_factor'])
        V.same(tag + k, dg[k], dg2[k])
    # the saved weights once more, one row per receiver and relation
    g, s32, s64 = (EE.split_att(t, n, H, O) for t in (dg['att'][:n].cpu(), d32['att'], d64['att']))
    for k in g:
        V.add(tag + k, g[k], s32[k], s64[k], row_factor=c['fwd_row_factor'])
    V.fails += [tag + f for f in EE.att_structure_failures(dg['att'], dg)]


def _judge_backward(V, bg, bg2, b32, b64, tag=''):
    for k in EE.attn_bwd_outputs(b32):
        V.add(tag + k, bg[k][:b32[k].shape[0]], b32[k], b64[k])
        V.same(tag + k, bg[k], bg2[k])


@pytest.mark.parametrize('c', EE.ATTN_CASES, ids=lambda c: c['id'])
def test_entity_attention_over_the_entity_range(K, c):
    """attn_fwd / attn_bwd per case of tests/entity_envelope.py (why each is there is said in the list)."""
    d32, d64, b32, b64 = EE.attn_spec(c)
    dg, dg2 = EE.attn_desc(c, DEV), EE.attn_desc(c, DEV)
    K.attn_fwd([dg])
    ran = K.attn_last_path()
    K.attn_fwd([dg2])
    assert ran == c['fwd'], f"forward took path {ran:#x}, the case was written for {c['fwd']:#x} ({c['why']})"
    V = Verdict(c['id'])
    _judge_forward(V, c, dg, dg2, d32, d64)
    # backward on the specification's saved weights, so that the comparison isolates the backward kernel
    for d in (dg, dg2):
        d['att'] = d32['att'].to(DEV)
    bg, bg2 = (attn_bwd_case(DEV, d, seed=111, dw_extra=c['dwx']) for d in (dg, dg2))
    K.attn_bwd([bg])
    ran = K.attn_last_path()
    K.attn_bwd([bg2])
    assert ran == c['bwd'], f"backward took path {ran:#x}, the case was written for {c['bwd']:#x} ({c['why']})"
    _judge_backward(V, bg, bg2, b32, b64)
    torch.cuda.synchronize()
    V.check()


def _base(t):
    return t._base if t._base is not None else t


def test_grouped_attention_call_mixing_a_small_and_the_largest_layout(K):
    """One launch for a (2, 8) and a (4, 12) descriptor with different instance counts: the host decides per launch over all
    descriptors, so the (2, 8) one runs the non-column forms; the workgroups beyond its 1040 instances write nothing."""
    CANARY = 7.25
    specs = [EE.attn_spec(c, n_alloc=EE.GROUPED_ALLOC) for c in EE.GROUPED]

    def descs():
        ds = [EE.attn_desc(c, DEV, n_alloc=EE.GROUPED_ALLOC) for c in EE.GROUPED]
        for d in ds:
            for k in EE.attn_outputs(d):
                _base(d[k]).fill_(CANARY)
        return ds

    def untouched_elsewhere(V, tag, outs, before, n, n_alloc):
        """Nothing but the first n instances' rows of each output view changed in its underlying buffer."""
        for k, t in outs.items():
            now = _base(t).clone()
            rows = n * (t.shape[0] // n_alloc)
            view = now.as_strided(t.size(), t.stride(), t.storage_offset())
            view[:rows] = before[k].as_strided(t.size(), t.stride(), t.storage_offset())[:rows]
            if not torch.equal(now, before[k]):
                V.fails.append(f'{tag}{k}: the call wrote outside the rows of its {n} instances')

    V = Verdict('grouped_H2_O8_n1040+H4_O12_n1100')
    dg, dg2 = descs(), descs()
    before = [{k: _base(t).clone() for k, t in EE.attn_outputs(d).items()} for d in dg]
    K.attn_fwd(dg)
    ran = K.attn_last_path()
    K.attn_fwd(dg2)
    assert ran == EE.FWD_ROWS, f'{ran:#x}'
    for i, c in enumerate(EE.GROUPED):
        _judge_forward(V, c, dg[i], dg2[i], specs[i][0], specs[i][1], tag=f'd{i} ')
        untouched_elsewhere(V, f'd{i} ', EE.attn_outputs(dg[i]), before[i], c['n_inst'], EE.GROUPED_ALLOC)
    bgs = []
    for ds in (dg, dg2):
        bb = []
        for i, (c, d) in enumerate(zip(EE.GROUPED, ds)):
            d['att'] = torch.cat([specs[i][0]['att'].to(DEV), d['att'][c['n_inst']:]])
            b = attn_bwd_case(DEV, dict(d, n_inst=EE.GROUPED_ALLOC), seed=111, dw_extra=c['dwx'])
            b['f'] = d
            for k in b:
                if k.startswith('dmsg_'):
                    b[k].fill_(CANARY)
            bb.append(b)
        bgs.append(bb)
    before = [{k: _base(t).clone() for k, t in EE.attn_bwd_outputs(b).items()} for b in bgs[0]]
    K.attn_bwd(bgs[0])
    ran = K.attn_last_path()
    K.attn_bwd(bgs[1])
    assert ran == EE.BWD_ROWS, f'{ran:#x}'
    for i, c in enumerate(EE.GROUPED):
        _judge_backward(V, bgs[0][i], bgs[1][i], specs[i][2], specs[i][3], tag=f'd{i} ')
        untouched_elsewhere(V, f'd{i} ', EE.attn_bwd_outputs(bgs[0][i]), before[i], c['n_inst'], EE.GROUPED_ALLOC)
    V.check()


# ------------------------------------------------------------------------------------------- sender-side projection
@pytest.mark.parametrize('H,O,ph_on,ps_on,cols', EE.SSP_CASES)
def test_sender_side_projection_over_the_entity_range(K, H, O, ph_on, ps_on, cols):
    i = EE.ssp_inputs(H, O, ph_on, ps_on, cols)
    s32, s64 = EE.ssp_run(F, i, H, O, ps_on), EE.ssp_run(F, i, H, O, ps_on, dtype=torch.float64)
    g1, g2 = EE.ssp_run(K, i, H, O, ps_on, dev=DEV), EE.ssp_run(K, i, H, O, ps_on, dev=DEV)
    V = Verdict(f'ssp_H{H}_O{O}_ph{int(ph_on)}_ps{int(ps_on)}_cols{cols}')
    for k in s32:
        V.add(k, g1[k], s32[k], s64[k])
        V.same(k, g1[k], g2[k])
    # adjointness: <ssp_fwd(0; ph, ps), dgi> == <ph, qh> + <ps, qs>, on the kernels' own results
    z = EE.ssp_run(K, i, H, O, ps_on, dev=DEV, gi_zero=True)['gi'].cpu().double()
    lhs = (z * i['dgi'].double()).sum()
    rhs = ((i['ph'].double() * g1['qh'].cpu().double()).sum() if ph_on else 0.0) + \
          ((i['ps'].double() * g1['qs'].cpu().double()).sum() if ps_on else 0.0)
    assert abs(float(lhs - rhs)) < 1e-3 * max(1.0, abs(float(lhs))), (float(lhs), float(rhs))
    V.check()


def test_sender_side_gather_at_the_segment_level_placement_with_4_humans_and_12_objects(K):
    i = EE.ssp_gather_inputs()
    s32, s64 = EE.ssp_gather_run(F, i), EE.ssp_gather_run(F, i, dtype=torch.float64)
    g1, g2 = EE.ssp_gather_run(K, i, dev=DEV), EE.ssp_gather_run(K, i, dev=DEV)
    V = Verdict('ssp_gather_H4_O12')
    V.add('qh', g1, s32, s64)
    V.same('qh', g1, g2)
    V.check()


# ------------------------------------------------------------------------------------------------ segment recurrence
def _seg_backward_inputs(b32, own):
    bg = {k: v.to(DEV) for k, v in b32.items()}   # the specification's forward buffers: isolates the backward kernels
    for k in own:
        if k not in bg:
            bg[k] = own[k]
    return bg


@pytest.mark.parametrize('fusion', ['0', '7'])
@pytest.mark.parametrize('bs,T,H,O,h', EE.SEG_STEPWISE)
def test_segment_recurrence_launch_per_step_over_the_entity_range(K, bs, T, H, O, h, fusion, monkeypatch):
    monkeypatch.setenv('TWOG_GRU_FWD_FUSION', fusion)
    monkeypatch.setenv('TWOG_SEG_PERSIST', '0')
    b32, b64, (dh_h, dh_o), o32, o64 = EE.seg_spec(bs, T, H, O, h)
    pg = _seg_params(DEV, bs, T, H, O, h, (True, True, True, True), True)
    g1 = K.segrnn_fwd(pg)
    assert not K.last_segrnn_persistent
    g2 = K.segrnn_fwd(pg)
    V = Verdict(f'segrnn_stepwise_f{fusion}_bs{bs}_T{T}_H{H}_O{O}_h{h}')
    for k in EE.SEG_FWD_KEYS:
        V.add('fwd ' + k, g1[k], b32[k], b64[k], EE.seg_factor(h))
        V.same('fwd ' + k, g1[k], g2[k])
    bg = _seg_backward_inputs(b32, g1)
    o1 = K.segrnn_bwd(pg, bg, dh_h.to(DEV), dh_o.to(DEV))
    assert not K.last_segrnn_bwd_persistent
    o2 = K.segrnn_bwd(pg, bg, dh_h.to(DEV), dh_o.to(DEV))
    for k in o32:
        V.add('bwd ' + k, o1[k], o32[k], o64[k], EE.seg_factor(h))
        V.same('bwd ' + k, o1[k], o2[k])
    V.check()


@pytest.mark.parametrize('bs,T,H,O,h', EE.SEG_PERSISTENT)
def test_segment_recurrence_persistent_launch_over_the_entity_range(K, bs, T, H, O, h, monkeypatch):
    """The persistent launch must serve these shapes (asserted: a shape the library refuses is a failure, not a skip); its
    results against the launch-per-step path at the bar of the existing persistent test, and against fp64."""
    from twog_gcn_amd.kernels import PERSIST
    PERSIST.backoff.clear()
    monkeypatch.setenv('TWOG_PERSIST_CHECK', 'sync')
    b32, b64, (dh_h, dh_o), o32, o64 = EE.seg_spec(bs, T, H, O, h)
    pg = _seg_params(DEV, bs, T, H, O, h, (True, True, True, True), True)
    dh_h, dh_o = dh_h.to(DEV), dh_o.to(DEV)
    monkeypatch.setenv('TWOG_SEG_PERSIST', '0')
    gs = K.segrnn_fwd(pg)
    assert not K.last_segrnn_persistent
    monkeypatch.delenv('TWOG_SEG_PERSIST')
    g1 = K.segrnn_fwd(pg)
    assert K.last_segrnn_persistent, 'the persistent launch did not serve this shape'
    g2 = K.segrnn_fwd(pg)
    torch.cuda.synchronize()
    V = Verdict(f'segrnn_persistent_bs{bs}_T{T}_H{H}_O{O}_h{h}')
    for k in EE.SEG_FWD_KEYS:
        close(g1[k], gs[k], rtol=5e-5, atol=5e-6, what='persistent vs stepwise: ' + k)
        V.add('fwd ' + k, g1[k], b32[k], b64[k], EE.seg_factor(h))
        V.same('fwd ' + k, g1[k], g2[k])
    bg = _seg_backward_inputs(b32, g1)
    monkeypatch.setenv('TWOG_SEG_PERSIST', '0')
    o0 = K.segrnn_bwd(pg, bg, dh_h, dh_o)
    assert not K.last_segrnn_bwd_persistent
    monkeypatch.delenv('TWOG_SEG_PERSIST')
    o1 = K.segrnn_bwd(pg, bg, dh_h, dh_o)
    assert K.last_segrnn_bwd_persistent, 'the persistent backward launch did not serve this shape'
    o2 = K.segrnn_bwd(pg, bg, dh_h, dh_o)
    torch.cuda.synchronize()
    for k in o32:
        close(o1[k], o0[k], rtol=1e-4, atol=1e-5, what='persistent vs stepwise bwd: ' + k)
        V.add('bwd ' + k, o1[k], o32[k], o64[k], EE.seg_factor(h))
        V.same('bwd ' + k, o1[k], o2[k])
    V.check()
