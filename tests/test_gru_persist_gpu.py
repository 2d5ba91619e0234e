"""GPU: the frame-level BiGRU as one persistent launch (csrc/gru_persist.hip) over the cases of tests/gru_persist_cases.py -- all
twelve forward instances bigru_persist_fwd_kernel<NKB, TWC>, the four backward widths, and the partition edges of plan().

For every case: the library's report for THIS device equals the case's claims (so the case provably reaches its branch); the launch
is taken where the case says (default policy: forward and backward persistent with the switch unset; TWC > 1: not under the default
policy, forward under TWOG_BIGRU_PERSIST=1 with the backward staying per step) -- a launch that does not run is a failure; every
output (out, save; d_gi, d_gh of the backward on the fp32 specification's out / save) is judged by tests.entity_envelope.judge
against the specification run in fp64 with the fp32 specification's own error as the yardstick, tensor-wide and per row, factor
FACTOR_X3 (these kernels multiply with the 3 x bf16 split at every width); two calls are bit-identical; the bars of the older
persistent tests of tests/test_kernels_gpu.py hold against the launch-per-step path and the fp32 specification; everything is
finite, and without a bias hn of the first step of either direction is exactly 0. None of these numbers is tuned to a run.
tests/test_gru_persist_cpu.py checks the case lists and the specification themselves.

TWOG_GRU_PERSIST_RECORD=<file>: e_hip, e_ref, their ratio and the worst row of every (case, tensor) are written there as JSON, a
line per case (profiles/gru_persist_fp64.json is such a record)."""
import json
import os

import pytest
import torch

import twog_gcn_amd  # noqa: F401
from twog_gcn_amd import kernels as twog_kernels
from twog_gcn_amd.kernels import PERSIST
from tests import entity_envelope as EE
from tests import gru_cases as GC
from tests import gru_persist_cases as PC
from tests.gru_cases import F, JUDGE

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32, F64 = torch.float32, torch.float64
RECORDS = {}
RECORD_FIELDS = ('e_hip', 'e_ref', 'ratio', 'row_ratio', 'row', 'factor')


@pytest.fixture(scope='module')
def K():
    twog_kernels._set_backend_for_tests(None)
    k = twog_kernels.get_kernels()
    assert k.name == 'hip'
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus == PC.N_CUS, (f'this device has {cus} compute units: the claims of tests/gru_persist_cases.py (instance and partition '
                             f'per case) are stated for {PC.N_CUS}')
    yield k
    dst = os.environ.get('TWOG_GRU_PERSIST_RECORD')
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


def check_case(K, c, monkeypatch, forced):
    plan = K.bigru_persistent_plan(c['Es'], c['bs'], c['h'])
    assert plan['served'] and PC.claimed(plan) == PC.claims(c), f"{c['id']} does not reach its branch on this device: {plan}"
    for name, fresh in (('backoff', {}), ('refused', set()), ('clean', {})):
        monkeypatch.setattr(PERSIST, name, fresh)
    monkeypatch.setenv('TWOG_PERSIST_CHECK', 'sync')
    s32 = GC.rec_run(F, c, 'cpu', F32)
    s64 = GC.rec_run(F, c, 'cpu', F64, saved=s32)
    ran = lambda: (bool(K.last_bigru_persistent), bool(K.last_bigru_bwd_persistent))

    monkeypatch.setenv('TWOG_BIGRU_PERSIST', '0')
    step = GC.rec_run(K, c, DEV, F32, saved=s32)
    assert ran() == (False, False)
    monkeypatch.delenv('TWOG_BIGRU_PERSIST')
    if forced:
        GC.rec_run(K, c, DEV, F32, saved=s32)
        assert ran() == (False, False), 'more than one tile per wave: not the default path, forward or backward'
        monkeypatch.setenv('TWOG_BIGRU_PERSIST', '1')
    hip = GC.rec_run(K, c, DEV, F32, saved=s32)
    assert ran() == (True, not forced), f'(forward, backward) persistent = {ran()}: a launch the case is for did not run'
    again = GC.rec_run(K, c, DEV, F32, saved=s32)
    assert ran() == (True, not forced)
    torch.cuda.synchronize()

    fails, worst = [], (0.0, '')
    names = [k for k, (_, how) in hip.items() if how == JUDGE and (not forced or k.startswith(('out', 'save')))]
    assert len(names) == (2 if forced else 4) * len(c['Es'])
    for k in names:
        v = hip[k][0]
        rec, f = EE.judge(v, s32[k][0], s64[k][0], EE.FACTOR_X3)
        RECORDS[f"{c['id']}/{k}"] = dict(rec, factor=EE.FACTOR_X3)
        fails += [f'{k}: {x}' for x in f]
        worst = max(worst, (max(rec['ratio'], rec['row_ratio']), k))
        if not bool(torch.isfinite(v).all()):
            fails.append(f'{k}: non-finite values')
        if not torch.equal(v, again[k][0]):
            fails.append(f'{k}: two runs of the persistent launch differ')
        bar(fails, f'{k} against the fp32 specification', v, s32[k][0], 1e-4, 1e-5)
        if k.startswith('out'):
            bar(fails, f'{k} against the launch-per-step path', v, step[k][0], 2e-5, 2e-6)
        if k.startswith('d_gi'):
            bar(fails, f'{k} against the launch-per-step path', v, step[k][0], 5e-5, 5e-6)
    if not c['bias']:
        for k in range(len(c['Es'])):
            hn = hip[f'save{k}'][0][PC.first_step_hn_rows(c, k)]
            if float(hn.abs().max()) != 0.0:
                fails.append(f'save{k}: hn of the first step of a direction is not exactly 0 without a bias')
    print(f"{c['id']} <{plan['nkb']}, {plan['twc']}>: worst e_hip / e_ref {worst[0]:.2f} ({worst[1]})")
    assert not fails, f"{c['id']} ({c['why']}):\n  " + '\n  '.join(fails)


@pytest.mark.parametrize('c', PC.DEFAULT, ids=lambda c: c['id'])
def test_default_policy_launches(K, c, monkeypatch):
    """At most one tile per wave: forward and backward persistent with TWOG_BIGRU_PERSIST unset."""
    check_case(K, c, monkeypatch, forced=False)


@pytest.mark.parametrize('c', PC.FORCED, ids=lambda c: c['id'])
def test_forced_forward_instances(K, c, monkeypatch):
    """TWC = 2 and 4: shipped, and taken under TWOG_BIGRU_PERSIST=1; the backward reports "not served" and runs per step."""
    check_case(K, c, monkeypatch, forced=True)


@pytest.mark.parametrize('id,why,Es,bs,h,n_cus', PC.REFUSED, ids=[r[0] for r in PC.REFUSED])
def test_refused_shapes_are_refused_for_this_device_too(K, id, why, Es, bs, h, n_cus):
    """The report with the device's own compute-unit count (the case with fewer is a statement about another device: as given)."""
    p = K.bigru_persistent_plan(Es, bs, h, 0 if n_cus == PC.N_CUS else n_cus)
    assert not p['served'] and p['n_cus'] == n_cus, (why, p)
