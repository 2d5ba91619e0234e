"""GPU: the general GEMM entry (twog_gemm_f32, csrc/gemm_f32.hip) over the cases of tests/gemm_cases.py -- launches of several
problems (K classes and the XCD tile map, chunks of 8), split-K over problems of different length (empty slices, the scalar and the
16-byte branch of the reduction, whole splits dealt to XCDs), operands that are 16-byte loadable per operand and per problem,
grouped k-major rows on the 64 x 64 tile, the in-workgroup k-split classes beside a problem of a single k-tile, batched beside
unbatched problems.

Every C is judged by tests.entity_envelope.judge against the specification run in fp64, with the fp32 specification's own error as
the yardstick (e_hip <= 8 x e_ref + 4 x 2^-24, tensor-wide and per row; 8 x 1.25 where gemm_last_class() reports the X3 bit); the
memory around every C view must be bit-equal to the fp32 specification (untouched); every case asserts the class word it states.
Split-K cases run on a workspace whose slabs were filled with NaN (a slice that leaves its slab unwritten shows) and twice, bit for
bit. tests/test_gemm_general_cpu.py checks the case list and the arithmetic behind each case.

TWOG_GEMM_RECORD=<file>: e_hip, e_ref, their ratio and the worst row of every (case, problem) are written there as JSON, a line per
case (profiles/gemm_general_fp64.json is such a record)."""
import json
import os

import pytest
import torch

import twog_gcn_amd  # noqa: F401
from twog_gcn_amd import kernels as twog_kernels
from tests import entity_envelope as EE
from tests import gemm_cases as GC
from tests.gemm_cases import F, EXACT, JUDGE

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
    yield k
    dst = os.environ.get('TWOG_GEMM_RECORD')
    if dst and RECORDS:
        write_record(dst)


def write_record(dst):
    """One line per case: {problem: [RECORD_FIELDS]} (row: the row that needs the largest factor, row_ratio: that factor)."""
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


def poison_slabs(K):
    """NaN into the first 64 MB of slabs of the split-K workspace (the reserved 16 KB in front stay zero): more than any case uses."""
    ws = K.workspace(320 << 20, DEV, 'splitk')
    ws[4096:4096 + (16 << 20)].fill_(float('nan'))


@pytest.mark.parametrize('c', GC.CASES, ids=lambda c: c['id'])
def test_general_gemm(K, c):
    s32, s64 = GC.gemm_run(F, c, 'cpu', F32), GC.gemm_run(F, c, 'cpu', F64)
    if c['expect'][0] & GC.SPLITK:
        poison_slabs(K)
    hip = GC.gemm_run(K, c, DEV, F32)
    cls = K.gemm_last_class()
    fails = []
    want, mask = c['expect']
    if cls & mask != want:
        fails.append(f'class {cls:#x}, the case is for {want:#x} under mask {mask:#x}: it does not reach its branch')
    factor = EE.FACTOR_X3 if cls & GC.X3 else EE.FACTOR
    worst = (0.0, '')
    for k, (v, how) in hip.items():
        if how == EXACT:
            if not torch.equal(v, s32[k][0]):
                bad = v != s32[k][0]
                fails.append(f'{k}: the memory around the C view changed in {int(bad.sum())} places, the first at {torch.nonzero(bad)[0].tolist()}')
        else:
            assert how == JUDGE
            rec, f = EE.judge(v, s32[k][0], s64[k][0], factor)
            RECORDS[f"{c['id']}/{k}"] = dict(rec, factor=factor)
            fails += [f'{k}: {x}' for x in f]
            worst = max(worst, (max(rec['ratio'], rec['row_ratio']), k))
    if c.get('twice'):
        poison_slabs(K)
        again = GC.gemm_run(K, c, DEV, F32)
        assert K.gemm_last_class() == cls
        fails += [f'{k}: the second call differs from the first' for k, (v, _) in again.items() if not torch.equal(v, hip[k][0])]
    print(f"{c['id']}: class {cls:#x}, worst e_hip / e_ref {worst[0]:.2f} ({worst[1]})")
    assert not fails, f"{c['id']}:\n  " + '\n  '.join(fails)
