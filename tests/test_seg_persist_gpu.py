"""GPU: the segment-level recurrence as one persistent launch, forward and backward (csrc/seg_persist.hip), over the cases of
tests/seg_persist_cases.py -- all eight (h, mo) cells of both launches, every chunk size and pair mask make_plan() produces, short
sequences, the optional inputs absent, degenerate gates and masks.

For every launched case: the library's report for THIS device equals the case's claims (so the case provably reaches its branch);
with the switch unset the forward and the backward run persistently -- a launch that does not run, or that gave up, is a failure;
every forward tensor and every backward output (the backward on the fp32 specification's forward buffers) is judged by
tests.entity_envelope.judge against the specification run in fp64 with the fp32 specification's own error as the yardstick,
tensor-wide and per row, factor entity_envelope.seg_factor(h); two calls are bit-identical; the bars of the older persistent tests
hold against the launch-per-step path (forward rtol 5e-5 / atol 5e-6, backward 1e-4 / 1e-5); everything is finite; the zeros the
case's inputs make exact are exact. None of these numbers is tuned to a run. The rows of d_u_* are the plan's chunks
(seg_persist_cases.judged_rows says why). A refused shape sets neither persistent flag and the launch-per-step path passes the same
judgement. tests/test_seg_persist_cpu.py checks the case lists and the specification themselves.

TWOG_SEG_PERSIST_RECORD=<file>: e_hip, e_ref, their ratio and the worst row of every (case, tensor) are written there as JSON, a
line per case (profiles/seg_persist_fp64.json is such a record)."""
import json
import os

import pytest
import torch

import twog_gcn_amd  # noqa: F401
from twog_gcn_amd import kernels as twog_kernels
from twog_gcn_amd.kernels import PERSIST
from tests import entity_envelope as EE
from tests import seg_persist_cases as PC

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
RECORDS = {}
RECORD_FIELDS = ('e_hip', 'e_ref', 'ratio', 'row_ratio', 'row', 'factor')


@pytest.fixture(scope='module')
def K():
    twog_kernels._set_backend_for_tests(None)
    k = twog_kernels.get_kernels()
    assert k.name == 'hip'
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus == PC.N_CUS, (f'this device has {cus} compute units: the claims of tests/seg_persist_cases.py (instance, chunks and pair '
                             f'mask per case) are stated for {PC.N_CUS}')
    yield k
    dst = os.environ.get('TWOG_SEG_PERSIST_RECORD')
    if dst and RECORDS:
        write_record(dst)


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


def bar(fails, what, a, b, rtol, atol):
    """The bar of the older persistent tests (tests/test_kernels_gpu.py: close): max |a - b| <= atol + rtol x max |b|."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    err, tol = float((a - b).abs().max()), atol + rtol * float(b.abs().max())
    if not err <= tol:
        fails.append(f'{what}: max err {err:.3e} > tol {tol:.3e}')


def backward_inputs(b32, own):
    bg = {k: v.to(DEV) for k, v in b32.items()}   # the specification's forward buffers: isolates the backward kernel
    bg.update({k: v for k, v in own.items() if k not in bg})
    return bg


class Verdict:
    def __init__(self, c):
        self.c, self.fails, self.worst, self.factor = c, [], (0.0, ''), EE.seg_factor(c['h'])

    def judge(self, k, v, s32, s64, again):
        c = self.c
        rec, f = EE.judge(*(PC.judged_rows(c, k, t) for t in (v, s32, s64)), self.factor)
        RECORDS[f"{c['id']}/{k}"] = dict(rec, factor=self.factor)
        self.fails += [f'{k}: {x}' for x in f]
        self.worst = max(self.worst, (max(rec['ratio'], rec['row_ratio']), k))
        if not bool(torch.isfinite(v).all()):
            self.fails.append(f'{k}: non-finite values')
        if not torch.equal(v, again):
            self.fails.append(f'{k}: two runs differ')
        if k in c['zero'] and float(v.abs().max()) != 0.0:
            self.fails.append(f'{k}: not exactly 0')

    def check(self, what):
        c = self.c
        print(f"{c['id']} {what}: worst e_hip / e_ref {self.worst[0]:.2f} ({self.worst[1]})")
        assert not self.fails, f"{c['id']} ({c['why']}):\n  " + '\n  '.join(self.fails)


def fresh_policy(monkeypatch):
    for name, fresh in (('backoff', {}), ('refused', set()), ('clean', {})):
        monkeypatch.setattr(PERSIST, name, fresh)
    monkeypatch.setenv('TWOG_PERSIST_CHECK', 'sync')


@pytest.mark.parametrize('c', PC.LAUNCHED, ids=lambda c: c['id'])
def test_persistent_launches(K, c, monkeypatch):
    plan = K.segrnn_persistent_plan(*c['shape'])
    assert plan['served'] and PC.claimed(plan) == PC.claims(c), f"{c['id']} does not reach its branch on this device: {plan}"
    fresh_policy(monkeypatch)
    b32, b64, (dh_h, dh_o), o32, o64 = PC.spec(c)
    pg = PC.params(c, DEV)
    dh_h, dh_o = dh_h.to(DEV), dh_o.to(DEV)

    monkeypatch.setenv('TWOG_SEG_PERSIST', '0')
    step = K.segrnn_fwd(pg)
    assert not K.last_segrnn_persistent
    monkeypatch.delenv('TWOG_SEG_PERSIST')
    g1 = K.segrnn_fwd(pg)
    assert K.last_segrnn_persistent, 'the persistent forward launch did not run, or gave up'
    g2 = K.segrnn_fwd(pg)
    assert K.last_segrnn_persistent
    bg = backward_inputs(b32, g1)
    monkeypatch.setenv('TWOG_SEG_PERSIST', '0')
    ostep = K.segrnn_bwd(pg, bg, dh_h, dh_o)
    assert not K.last_segrnn_bwd_persistent
    monkeypatch.delenv('TWOG_SEG_PERSIST')
    o1 = K.segrnn_bwd(pg, bg, dh_h, dh_o)
    assert K.last_segrnn_bwd_persistent, 'the persistent backward launch did not run, or gave up'
    o2 = K.segrnn_bwd(pg, bg, dh_h, dh_o)
    assert K.last_segrnn_bwd_persistent
    torch.cuda.synchronize()

    V = Verdict(c)
    for k in PC.fwd_keys(c):
        V.judge(k, g1[k], b32[k], b64[k], g2[k])
        bar(V.fails, f'{k} against the launch-per-step path', g1[k], step[k], 5e-5, 5e-6)
    assert sorted(o1) == sorted(o32) == PC.bwd_keys(c, o32)
    for k in PC.bwd_keys(c, o32):
        V.judge(k, o1[k], o32[k], o64[k], o2[k])
        bar(V.fails, f'{k} against the launch-per-step path', o1[k], ostep[k], 1e-4, 1e-5)
    for name, v in PC.exact_zeros(c, {k: g1[k].cpu() for k in PC.fwd_keys(c)}).items():
        if float(v.abs().max()) != 0.0:
            V.fails.append(f'{name}: not exactly 0')
    if c['inputs'].get('gates') == 'closed':
        V.fails += PC.uniform_attention_failures(c, g1['att'])
    V.check(f"<{plan['mh']}, {plan['mo']}{', x3q1' if plan['x3q1'] else ''}> cpc {plan['cpc']} x {plan['n_chunks']}")


@pytest.mark.parametrize('c', PC.REFUSED, ids=lambda c: c['id'])
def test_refused_shapes_run_per_step(K, c, monkeypatch):
    """The report with the device's own compute-unit count (the case with fewer is a statement about another device: as given) says
    "not served"; through the wrapper with the switch unset neither persistent flag is set, and the launch-per-step results pass
    the judgement. Not run through the wrapper: H = 5 and O = 13, which the launch-per-step path's attention kernels reject too
    (up to 4 humans and 12 objects), and the 128-compute-unit case."""
    p = K.segrnn_persistent_plan(*c['shape'], 0 if c['n_cus'] == PC.N_CUS else c['n_cus'], **PC.plan_args(c))
    assert not p['served'] and p['n_cus'] == c['n_cus'], (c['why'], p)
    if not c['step']:
        return
    fresh_policy(monkeypatch)
    monkeypatch.delenv('TWOG_SEG_PERSIST', raising=False)
    b32, b64, (dh_h, dh_o), o32, o64 = PC.spec(c)
    pg = PC.params(c, DEV)
    dh_h, dh_o = dh_h.to(DEV), dh_o.to(DEV)
    g1 = K.segrnn_fwd(pg)
    assert not K.last_segrnn_persistent, 'a refused shape was launched persistently'
    g2 = K.segrnn_fwd(pg)
    bg = backward_inputs(b32, g1)
    o1 = K.segrnn_bwd(pg, bg, dh_h, dh_o)
    assert not K.last_segrnn_bwd_persistent, 'a refused shape was launched persistently'
    o2 = K.segrnn_bwd(pg, bg, dh_h, dh_o)
    torch.cuda.synchronize()
    V = Verdict(c)
    for k in PC.fwd_keys(c):
        V.judge(k, g1[k], b32[k], b64[k], g2[k])
    for k in PC.bwd_keys(c, o32):
        V.judge(k, o1[k], o32[k], o64[k], o2[k])
    V.check('per step')
