"""GPU: the GRU family over the cases of tests/gru_cases.py -- the gate step kernels of csrc/gru.hip called directly
(twog_gru_step_fwd: 16-byte and scalar kernel, chunks of 8 descriptors; twog_gru_step_bwd: du addressing, atomicAdd, block
reduction) and the frame recurrences (twog_bigru_fwd / bwd, twog_gru_seq_fwd / bwd on the launch-per-step path: the GEMM + gate
pair and the fused forward step, the gate backward in its own launch and in the epilogue of every gate-fused GEMM class the default
environment reaches).

Every floating-point result is judged by tests.entity_envelope.judge against the specification run in fp64, with the fp32
specification's own error as the yardstick (e_hip <= 8 x e_ref + 4 x 2^-24, tensor-wide and per row; 8 x 1.25 behind a launch
whose reported class has the X3 bit); the memory around every written view, rows behind a gate of exactly 0 and gradients of
planted gates must be bit-equal to the fp32 specification. Every case proves the branch its `why` names: the forward step by
HipKernels.gru_step_last_path (kernel, block size, launches of the call), the recurrences by HipKernels.gemm_last_class.
tests/test_gru_kernels_cpu.py checks the case list and the specification themselves.

TWOG_GRU_RECORD=<file>: e_hip, e_ref, their ratio and the worst row of every (case, tensor) are written there as JSON, a line per case
(profiles/gru_kernels_fp64.json is such a record)."""
import json
import os

import pytest
import torch

import twog_gcn_amd  # noqa: F401
from twog_gcn_amd import kernels as twog_kernels
from tests import entity_envelope as EE
from tests import gru_cases as GC
from tests.gru_cases import F, EXACT, JUDGE

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32, F64 = torch.float32, torch.float64
RECORDS = {}


@pytest.fixture(scope='module')
def K():
    twog_kernels._set_backend_for_tests(None)
    k = twog_kernels.get_kernels()
    assert k.name == 'hip'
    yield k
    dst = os.environ.get('TWOG_GRU_RECORD')
    if dst and RECORDS:
        write_record(dst)


RECORD_FIELDS = ('e_hip', 'e_ref', 'ratio', 'row_ratio', 'row', 'factor')


def write_record(dst):
    """One line per case: {tensor: [RECORD_FIELDS]} (row: the row that needs the largest factor, row_ratio: that factor)."""
    fin = lambda v: (float(f'{v:.3g}') if v == v and abs(v) != float('inf') else str(v)) if isinstance(v, float) else v
    cases = {}
    for name, r in sorted(RECORDS.items()):
        case, tensor = name.split('/', 1)
        cases.setdefault(case, {})[tensor] = [fin(r[f]) for f in RECORD_FIELDS]
    with open(dst, 'w') as f:
        f.write('{"_fields": ' + json.dumps(list(RECORD_FIELDS)))
        for case, tensors in cases.items():
            f.write(',\n' + json.dumps(case) + ': ' + json.dumps(tensors, separators=(',', ':')))
        f.write('\n}\n')


class Verdict:
    """Collects the judgement of every tensor of one case: all of them are measured (and recorded) before the case fails."""

    def __init__(self, case):
        self.case, self.fails, self.worst = case, [], (0.0, '')

    def add(self, name, hip, s32, s64, factor):
        rec, fails = EE.judge(hip, s32, s64, factor)
        RECORDS[f'{self.case}/{name}'] = dict(rec, factor=factor)
        self.fails += [f'{name}: {f}' for f in fails]
        self.worst = max(self.worst, (max(rec['ratio'], rec['row_ratio']), name))

    def exact(self, name, hip, s32):
        hip = hip.detach().cpu()
        if hip.shape != s32.shape or hip.dtype != s32.dtype:
            self.fails.append(f'{name}: shape / dtype {tuple(hip.shape)} {hip.dtype}, specification {tuple(s32.shape)} {s32.dtype}')
        elif not torch.equal(hip, s32):
            bad = hip != s32
            self.fails.append(f'{name}: not bit-equal to the fp32 specification in {int(bad.sum())} of {bad.numel()} places, the first at '
                              f'{torch.nonzero(bad)[0].tolist()}')

    def all(self, hip, s32, s64, tag='', factor=EE.FACTOR):
        for k, (v, how) in hip.items():
            if how == EXACT:
                self.exact(tag + k, v, s32[k][0])
            elif how == JUDGE:
                self.add(tag + k, v, s32[k][0], s64[k][0], factor)

    def check(self):
        print(f'{self.case}: worst e_hip / e_ref {self.worst[0]:.2f} ({self.worst[1]})')
        assert not self.fails, f'{self.case}:\n  ' + '\n  '.join(self.fails)


def three(K, run, c):
    s32, s64 = run(F, c, 'cpu', F32), run(F, c, 'cpu', F64)
    hip = run(K, c, DEV, F32)
    torch.cuda.synchronize()
    return hip, s32, s64


# ------------------------------------------------------------------------------------------------- the forward gate step
@pytest.mark.parametrize('c', GC.STEP_FWD_CASES, ids=lambda c: c['id'])
def test_forward_step(K, c):
    steps, _ = GC.step_fwd_build(c, DEV, F32)
    K.gru_step_fwd(steps)
    ran = K.gru_step_last_path()   # of the case's own call (step_fwd_run may follow it with the ungated call of the u == 1 check)
    assert ran == (c['vec'], c['threads'], c['launches']), f'(16-byte kernel, block size, launches) = {ran}: the case does not reach its branch'
    hip, s32, s64 = three(K, GC.step_fwd_run, c)
    V = Verdict('step_fwd_' + c['id'])
    V.all(hip, s32, s64)
    for k in [k for k in hip if k.endswith('_mask')]:
        mask, rz = hip[k][0], hip[k[:-4] + 'rz'][0].cpu()
        if not bool(((rz[mask] == 0) | (rz[mask] == 1)).all()):
            V.fails.append(f'{k}: a gate behind a pre-activation beyond +-{GC.SATURATED_BEYOND:g} is not exactly 0 or 1')
        if not bool(((rz >= 0) & (rz <= 1)).all()):
            V.fails.append(f'{k}: a gate outside [0, 1]')
    V.check()


def test_forward_step_alignment_variants_equal_the_aligned_run_bit_for_bit(K):
    """"Same arithmetic per element" (csrc/gru.hip): the scalar kernel, taken because ONE operand lost its alignment, returns the
    bits of the 16-byte kernel on the same values."""
    aligned = {}
    for id in GC.ALIGN_BREAKS:
        c = GC.STEP_FWD_BY_ID[id]
        if c['same_as'] not in aligned:
            aligned[c['same_as']] = GC.step_fwd_run(K, GC.STEP_FWD_BY_ID[c['same_as']], DEV, F32)
            assert K.gru_step_last_path()[0], c['same_as']
        got, want = GC.step_fwd_run(K, c, DEV, F32), aligned[c['same_as']]
        assert not K.gru_step_last_path()[0], id
        torch.cuda.synchronize()
        for k in ('h_out0', 'save0'):
            assert torch.equal(got[k][0], want[k][0]), f'{id}: {k} differs from the aligned run'


# ------------------------------------------------------------------------------------------------ the backward gate step
@pytest.mark.parametrize('c', GC.STEP_BWD_CASES, ids=lambda c: c['id'])
def test_backward_step(K, c):
    V = Verdict('step_bwd_' + c['id'])
    V.all(*three(K, GC.step_bwd_run, c))
    V.check()


# -------------------------------------------------------------------------------------------------- the frame recurrences
@pytest.mark.parametrize('c', GC.REC_ALL, ids=lambda c: c['id'])
def test_frame_recurrence(K, c, monkeypatch):
    """Forward with TWOG_GRU_FWD_FUSION 0 and 7, backward with and without TWOG_NO_GATE_FUSION (both read per call), the backward
    runs on the fp32 specification's forward buffers. The class of the last launch after each pass: the fused forward step where
    forced and served (the rule of test_bigru); the gate-fused GEMM of step 1 -- of the class the case states, where it states
    one -- where the backward fuses."""
    monkeypatch.setenv('TWOG_BIGRU_PERSIST', '0')
    s32 = GC.rec_run(F, c, 'cpu', F32)
    s64 = GC.rec_run(F, c, 'cpu', F64, saved=s32)
    V = Verdict('rec_' + c['id'])
    for fusion in ('0', '7'):
        monkeypatch.setenv('TWOG_GRU_FWD_FUSION', fusion)
        hip = GC.rec_run(K, c, DEV, F32, part='fwd')
        torch.cuda.synchronize()
        cls, fused = hip['cls_fwd'][0], GC.rec_fwd_fused(c, fusion)
        if ((cls & ~GC.X3) == GC.GRUFWD) != fused or (fused and bool(cls & GC.X3) != (c['h'] >= 256)):
            V.fails.append(f'forward, fusion {fusion}: class {cls:#x}')
        V.all(hip, s32, s64, tag=f'fusion{fusion}/', factor=EE.FACTOR_X3 if cls & GC.X3 else EE.FACTOR)
    for no_fusion in (False, True):
        if no_fusion:
            monkeypatch.setenv('TWOG_NO_GATE_FUSION', '1')
        else:
            monkeypatch.delenv('TWOG_NO_GATE_FUSION', raising=False)
        hip = GC.rec_run(K, c, DEV, F32, saved=s32, part='bwd')
        torch.cuda.synchronize()
        cls, fused = hip['cls_bwd'][0], GC.rec_bwd_fused(c, no_fusion)
        if c['T'] > 1:   # (T = 1: no GEMM, the word is an earlier launch's)
            if bool(cls & GC.GATE) != fused or (fused and c['cls'] is not None and cls != c['cls']):
                V.fails.append(f"backward, {'unfused' if no_fusion else 'fused'}: class {cls:#x}" + (f", the case is for {c['cls']:#x}" if c['cls'] else ''))
        x3 = c['T'] > 1 and cls & GC.X3
        V.all(hip, s32, s64, tag='unfused/' if no_fusion else 'fused/', factor=EE.FACTOR_X3 if x3 else EE.FACTOR)
    V.check()


def test_a_type_without_entities_among_live_ones_changes_nothing(K, monkeypatch):
    """E = 0 (gru_cases.REC_EMPTY_TYPE states what the launchers do with M = 0 and rows = 0): the live types are judged as in
    every case and equal the call without the empty type bit for bit, forward and backward, fused and unfused gate backward."""
    c = GC.REC_EMPTY_TYPE
    monkeypatch.setenv('TWOG_BIGRU_PERSIST', '0')
    monkeypatch.setenv('TWOG_GRU_FWD_FUSION', '0')
    s32 = GC.rec_run(F, c, 'cpu', F32)
    s64 = GC.rec_run(F, c, 'cpu', F64, saved=s32)
    V = Verdict('rec_' + c['id'])
    for no_fusion in (False, True):
        if no_fusion:
            monkeypatch.setenv('TWOG_NO_GATE_FUSION', '1')
        else:
            monkeypatch.delenv('TWOG_NO_GATE_FUSION', raising=False)
        hip = GC.rec_run(K, c, DEV, F32, saved=s32)
        assert bool(hip['cls_bwd'][0] & GC.GATE) != no_fusion, hex(hip['cls_bwd'][0])
        live = GC.rec_run(K, c, DEV, F32, saved=s32, live_only=True)
        torch.cuda.synchronize()
        V.all(hip, s32, s64, tag='unfused/' if no_fusion else 'fused/')
        empty = [k for k, E in enumerate(c['Es']) if E == 0]
        for k, (v, how) in hip.items():
            if how is None:
                continue
            if int(k[-1]) in empty:
                assert v.numel() == 0 and k not in live
            elif not torch.equal(v, live[k][0]):
                V.fails.append(f'{k}: differs from the call without the empty type')
    V.check()


def test_five_types_are_refused_without_a_launch(K, monkeypatch):
    monkeypatch.setenv('TWOG_BIGRU_PERSIST', '0')
    h, bs, T = 32, 2, 2
    fwd = [dict(gi=torch.zeros(bs, T, 1, 6 * h, device=DEV), w_hh_f=torch.zeros(3 * h, h, device=DEV), b_hh_f=None,
                w_hh_r=torch.zeros(3 * h, h, device=DEV), b_hh_r=None) for _ in range(GC.REC_TOO_MANY_TYPES)]
    bwd = [dict(d_out=torch.zeros(bs, T, 1, 2 * h, device=DEV), save=torch.zeros(2, bs, T, 1, 4 * h, device=DEV),
                out=torch.zeros(bs, T, 1, 2 * h, device=DEV), w_hh_f=y['w_hh_f'], w_hh_r=y['w_hh_r']) for y in fwd]
    K.bigru_fwd(fwd[:1], bs, T, h)   # a known state of both words: neither a GEMM nor a gate launch may follow
    before = K.gemm_last_class(), K.gru_step_last_path()
    with pytest.raises(RuntimeError, match='twog_bigru_fwd failed with code -1'):
        K.bigru_fwd(fwd, bs, T, h)
    with pytest.raises(RuntimeError, match='twog_bigru_bwd failed with code -1'):
        K.bigru_bwd(bwd, bs, T, h)
    seq = [dict(gi=y['gi'][..., :3 * h].contiguous(), w_hh=y['w_hh_f'], b_hh=None) for y in fwd]
    with pytest.raises(RuntimeError, match='twog_gru_seq_fwd failed with code -1'):
        K.gru_seq_fwd(seq, bs, T, h)
    torch.cuda.synchronize()
    assert (K.gemm_last_class(), K.gru_step_last_path()) == before
