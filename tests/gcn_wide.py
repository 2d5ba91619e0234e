"""The wide family of the geometric-level GCN kernels (csrc/geo_wide.hip, 65 ... 256 nodes and, forced, fewer): the case list and
the judgement, shared by tests/test_gcn_wide_cpu.py (the specification itself) and tests/test_gcn_wide_gpu.py (the kernels).

Inputs, the executable specification in fp32 / fp64, its second fp32 evaluation and the row rules are those of
tests/gcn_frames.py, unchanged (inputs, _spec, permuted, judge_rows, rows_of). What differs is R2: the fixed 0.2 % cap of that
module presumes rows of at most 64 weights; here the cap of a case is 1 / (2 x FG x N), half the share of rows that a defect
bound to one (frame slot of a group, node) position moves, with FG the frames per trip of the wide plan (1). It applies in the
spread regime to tensors of at least R2_MIN_ROWS rows, as before. tests/test_gcn_wide_cpu.py shows that two fp32 evaluations of
the specification stay under the cap of every case of this list.

The gradient of the geometry input (gcn_input_bwd, tests/input_grad_fake.py) joins the specification as 'dxg_eval' and, where
the case takes the train-mode fold, 'dxg_train'; like the other backward kernels it reads the fp32 run's saved tensors."""
import functools

import torch

from tests import gcn_frames as GF
from tests.input_grad_fake import InputGradFakeKernels

WIDE_MAX = 256          # twog_gcn_wide_max_nodes(); tests/test_gcn_wide_cpu.py compares it with the library
TUNED_MAX = 64          # twog_gcn_max_nodes()
MAX_GRID = 256          # frames the wide attention kernels take per trip of the grid; the GPU test reads it from the plan
FG = 1                  # frames per workgroup trip of the wide plan; the GPU test reads it from the plan
NODE_COUNTS = (65, 72, 80, 176, 255, 256)
IF = InputGradFakeKernels()


def _w(N, bs, T, H, regime='spread', why='', forced=False):
    c = GF._c(N, bs, T, H, regime, why)
    c['forced'] = forced
    if forced:
        c['id'] += '_forced'
    return c


ONE = [_w(N, 1, 1, 1, why='one frame') for N in NODE_COUNTS]
THREE = ([_w(N, 1, 3, 2, why='three frames, the geometry of human 0 of 2') for N in NODE_COUNTS] +
         [_w(N, 3, 1, 3, why='three frames, the geometry of human 0 of 3') for N in NODE_COUNTS])
SECOND_TRIP = [_w(N, 1, MAX_GRID + 1, 2, why='grid + 1 frames: one workgroup makes a second trip, the others do not')
               for N in (72, 256)]
SHARP = [_w(N, 2, 4, 2, 'sharp', why='scores up to +-500: the row max over all column tiles') for N in (72, 256)]
FORCED = [_w(N, 2, 5, 2, why='the wide family below its threshold', forced=True) for N in (34, 64)]
CASES = ONE + THREE + SECOND_TRIP + SHARP + FORCED


def r2_cap(c, fg=FG):
    return 1.0 / (2 * fg * c['N'])


@functools.lru_cache(maxsize=2)
def _spec_cached(cid):
    c = next(c for c in CASES if c['id'] == cid)
    p, s32, s64 = GF._spec(c)
    N = c['N']
    ab, mi = (s32[c['fold'] + k] for k in ('ab', 'mi'))
    modes = [('dxg_eval', False)] + ([('dxg_train', True)] if c['fold'] == 'train_' else [])
    for s, cv in ((s32, lambda t: t), (s64, lambda t: t.double())):
        for name, training in modes:
            out = torch.zeros(p['xh'].shape, dtype=cv(ab).dtype)
            IF.gcn_input_bwd(cv(p['xh']), N, cv(ab), cv(mi), cv(p['w1']), cv(p['de1m']),
                             cv(s32['dgamma']) if training else None, cv(s32['dbeta']) if training else None, training, out)
            s[name] = out[:, :, 0, 2048:].reshape(-1, 4).clone()
    return p, s32, s64


def spec(c):
    """(p, s32, s64) of tests/gcn_frames._spec plus the input gradient. (Cached: callers must not write into the result.)"""
    return _spec_cached(c['id'])


def permuted(c, p, s32):
    """gcn_frames.permuted plus the input gradient with the 64 hidden features in another order."""
    out = GF.permuted(c, p, s32)
    g = torch.Generator().manual_seed(11)
    ph = torch.randperm(64, generator=g)
    ab, mi = (s32[c['fold'] + k] for k in ('ab', 'mi'))
    for name in ('dxg_eval', 'dxg_train'):
        if name in s32:
            training = name == 'dxg_train'
            t = torch.zeros(p['xh'].shape)
            IF.gcn_input_bwd(p['xh'], c['N'], ab, mi, p['w1'][ph], p['de1m'][:, ph].contiguous(),
                             s32['dgamma'] if training else None, s32['dbeta'] if training else None, training, t)
            out[name] = t[:, :, 0, 2048:].reshape(-1, 4).clone()
    return out


def judge_named(c, name, hip, s32, s64, fg=FG):
    """gcn_frames.judge_named with this module's R2 cap: the tensor-wide rule, R1 and the exact zeros come from
    gcn_frames.judge_rows unchanged (its own fixed-cap R2 message is replaced by the cap of the case)."""
    N = c['N']
    r1 = c['regime'] == 'spread' or name in GF.SHARP_R1 or name.split('_')[0] in ('train', 'eval')
    rec, fails = GF.judge_rows(GF.rows_of(name, hip, N), GF.rows_of(name, s32, N), GF.rows_of(name, s64, N), c['regime'], r1)
    fails = [f for f in fails if not f.startswith('R2')]
    cap = r2_cap(c, fg)
    if c['regime'] == 'spread' and rec['rows'] >= GF.R2_MIN_ROWS and rec['r2_share'] > cap:
        fails.append(f'R2: {100 * rec["r2_share"]:.3f} % of {rec["rows"]} rows miss their own-row rule, cap 1 / (2 x {fg} x {N}) = '
                     f'{100 * cap:.3f} %')
    return rec, fails
