"""GPU: the 16-byte fused epilogues of the recurrence chains (csrc/gemm_f32.hip: the GATE branch of gemm_tile and
gemm_gru_fwd_kernel put the wave's tiles through LDS, so that a lane owns four consecutive columns of a row).

Reference inside the same build: the unfused path (TWOG_NO_GATE_FUSION=1 for the backward chains, TWOG_GRU_FWD_FUSION=0 for the
forward step; both read per call). The frame-level BiGRU and the segment-level recurrence run with T = 3 (first step: no previous
state; a middle step; the last step) and every output tensor is compared. The fused and the unfused path differ by the summation
order of the carry; PARENT is that difference, max |fused - unfused| / max |unfused| over the tensors of a pass, measured at
these shapes on the commit before the 16-byte epilogues (profiles/chain_epilogue_vec_ab.txt). The bound is twice that figure:
the gate arithmetic and every summation order are unchanged.

Second check: the 16-byte epilogue against the dword epilogue of the same build (TWOG_GATE_EPI_VEC=0 / TWOG_GRU_FWD_EPI_VEC=0,
the path unaligned operands take): every tensor bit-equal, d_u included (its row partials keep the dword epilogue's association).

Cases (the smallest shapes at which each branch can go wrong; the class of the last launch is asserted):
  a  h = 96,  bs = 5,  E = (2, 5, 1): the fp32 fused kernels; ragged rows and a ragged last column tile; grouped rows (inner = E)
  b  h = 256, bs = 24, E = (2, 8, 1): the fused forward step on the bf16 matrix cores; rows no multiple of 64 (the backward still takes
     the fp32 32-row class: the bf16x3 64x64 gate classes are the REC_CLASS_CASES of tests/gru_cases.py)
  c  h = 512, bs = 64, E = (2, 8, 1): the launches of the benchmark (gemm_gate_bwd_x3su_kernel<2, 2>, <1, 2> with the last
     arriver at the segment level, gemm_gru_fwd_kernel<2, 2, true>)
  the segment level (a, c) has the learned gate u (d_u from the row partials) and, in its first step, no previous state."""
import pytest
import torch

import twog_gcn_amd  # noqa: F401
from twog_gcn_amd import kernels as twog_kernels
from tests import gru_cases as GC
from tests.kernel_cases import rnd, _seg_params

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = torch.float32

CASES = {'a': (96, 5, (2, 5, 1)), 'b': (256, 24, (2, 8, 1)), 'c': (512, 64, (2, 8, 1))}
T = 3
# max |fused - unfused| / max |unfused| over the tensors of the pass on the parent commit (see the module docstring)
PARENT = {
    'bigru_a_fwd': 4.05e-7, 'bigru_a_bwd': 1.79e-7, 'bigru_b_fwd': 5.52e-7, 'bigru_b_bwd': 1.16e-7, 'bigru_c_fwd': 8.92e-7, 'bigru_c_bwd': 1.67e-7,
    'seg_a_fwd': 2.34e-6, 'seg_a_bwd': 2.07e-7, 'seg_c_fwd': 5.25e-6, 'seg_c_bwd': 2.05e-7,
}


@pytest.fixture(scope='module')
def K():
    twog_kernels._set_backend_for_tests(None)
    k = twog_kernels.get_kernels()
    assert k.name == 'hip'
    return k


def rel_diff(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


def bigru_case(name):
    h, bs, Es = CASES[name]
    c = GC._rc('epilogue_vec_' + name, 'tests/test_chain_epilogue_vec_gpu.py', h, bs, T, Es)
    GC.REC_BY_ID.setdefault(c['id'], c)   # (rec_inputs looks the case up by id)
    return c


def tensors(res):
    return {k: v[0] for k, v in res.items() if not k.startswith('cls')}


def bigru_runs(K, name, env):
    """{pass: {variant: tensors}} and the launch classes. Variants: fused (the 16-byte epilogue), dword (the same launches with
    the dword epilogue), unfused. The backward runs on the unfused forward's buffers."""
    c = bigru_case(name)
    env.setenv('TWOG_BIGRU_PERSIST', '0')
    out, cls = {'fwd': {}, 'bwd': {}}, {}
    for variant, fusion, vec in (('unfused', '0', '1'), ('fused', '7', '1'), ('dword', '7', '0')):
        env.setenv('TWOG_GRU_FWD_FUSION', fusion)
        env.setenv('TWOG_GRU_FWD_EPI_VEC', vec)
        res = GC.rec_run(K, c, DEV, F32, part='fwd')
        out['fwd'][variant], cls['fwd_' + variant] = tensors(res), res['cls_fwd'][0]
    saved = {k: (v, None) for k, v in out['fwd']['unfused'].items()}
    env.setenv('TWOG_GRU_FWD_FUSION', '0')
    for variant, unfused, vec in (('unfused', True, '1'), ('fused', False, '1'), ('dword', False, '0')):
        if unfused:
            env.setenv('TWOG_NO_GATE_FUSION', '1')
        else:
            env.delenv('TWOG_NO_GATE_FUSION', raising=False)
        env.setenv('TWOG_GATE_EPI_VEC', vec)
        res = GC.rec_run(K, c, DEV, F32, saved=saved, part='bwd')
        out['bwd'][variant], cls['bwd_' + variant] = tensors(res), res['cls_bwd'][0]
    torch.cuda.synchronize()
    return out, cls


def seg_runs(K, name, env):
    h, bs, Es = CASES[name]
    H, O = Es[0], Es[1]
    env.setenv('TWOG_SEG_PERSIST', '0')
    p = _seg_params(DEV, bs, T, H, O, h, (True, True, True, True), True)
    dh_h, dh_o = rnd(bs, T, H, 2 * h, seed=31).to(DEV), rnd(bs, T, O, 2 * h, seed=32).to(DEV)
    fkeys = ('hs_h', 'hs_o', 'save_h', 'save_o', 'msrc_h', 'msrc_o', 'mg_h', 'mg_o', 'att')
    out, cls, bufs = {'fwd': {}, 'bwd': {}}, {}, {}
    for variant, fusion, vec in (('unfused', '0', '1'), ('fused', '7', '1'), ('dword', '7', '0')):
        env.setenv('TWOG_GRU_FWD_FUSION', fusion)
        env.setenv('TWOG_GRU_FWD_EPI_VEC', vec)
        bufs[variant] = K.segrnn_fwd(p)
        cls['fwd_' + variant] = K.gemm_last_class()
        out['fwd'][variant] = {k: bufs[variant][k] for k in fkeys}
    env.setenv('TWOG_GRU_FWD_FUSION', '0')
    for variant, unfused, vec in (('unfused', True, '1'), ('fused', False, '1'), ('dword', False, '0')):
        if unfused:
            env.setenv('TWOG_NO_GATE_FUSION', '1')
        else:
            env.delenv('TWOG_NO_GATE_FUSION', raising=False)
        env.setenv('TWOG_GATE_EPI_VEC', vec)
        out['bwd'][variant] = K.segrnn_bwd(p, bufs['unfused'], dh_h, dh_o)
        cls['bwd_' + variant] = K.gemm_last_class()
    torch.cuda.synchronize()
    return out, cls


def figures(out):
    """{pass: (worst figure, its tensor)}: fused against unfused."""
    fig = {}
    for part in ('fwd', 'bwd'):
        fig[part] = max((rel_diff(v, out[part]['unfused'][k]), k) for k, v in out[part]['fused'].items() if v.numel())
    return fig


def judge(level, name, out):
    fails = []
    for part, (fig, worst) in figures(out).items():
        key = f'{level}_{name}_{part}'
        print(f'{key}: fused against unfused {fig:.3e} ({worst}), parent {PARENT[key]:.3e}')
        if not fig <= 2 * PARENT[key]:
            fails.append(f'{key}: {fig:.3e} ({worst}) is more than twice the parent commit\'s {PARENT[key]:.3e}')
        for k, v in out[part]['fused'].items():
            w = out[part]['dword'][k]
            if not torch.isfinite(v).all():
                fails.append(f'{key}: {k} is not finite')
            if not torch.equal(v, w):
                fails.append(f'{key}: {k} of the 16-byte epilogue is not bit-equal to the dword epilogue\'s ({rel_diff(v, w):.3e})')
    assert not fails, '\n  '.join(fails)


@pytest.mark.parametrize('name', ['a', 'b', 'c'])
def test_bigru_fused_epilogues_against_the_unfused_path(K, name, monkeypatch):
    out, cls = bigru_runs(K, name, monkeypatch)
    h = CASES[name][0]
    x3 = GC.X3 if h >= 256 else 0
    assert cls['fwd_fused'] == cls['fwd_dword'] == GC.GRUFWD | x3, hex(cls['fwd_fused'])
    assert cls['bwd_fused'] == cls['bwd_dword'] and cls['bwd_fused'] & GC.GATE and not cls['bwd_unfused'] & GC.GATE, hex(cls['bwd_fused'])
    # a and b (24 + 96 + 12 32-row tiles per direction at most): gemm_gate_bwd_xs32_kernel, fp32, slices over workgroups and the
    # last arriver's epilogue (the X3 64x64 gate classes: REC_CLASS_CASES of tests/gru_cases.py); c: gemm_gate_bwd_x3su_kernel<2, 2>,
    # the 176-tile launch of the benchmark
    want = GC.GATE | GC.KSPLIT | GC.X3 if name == 'c' else GC.GATE | GC.KSPLIT | GC.ROWS32 | GC.XSPLIT
    assert cls['bwd_fused'] == want, hex(cls['bwd_fused'])
    judge('bigru', name, out)


@pytest.mark.parametrize('name', ['a', 'c'])
def test_segment_fused_epilogues_against_the_unfused_path(K, name, monkeypatch):
    out, cls = seg_runs(K, name, monkeypatch)
    h = CASES[name][0]
    x3 = GC.X3 if h >= 256 else 0
    assert cls['fwd_fused'] == cls['fwd_dword'] == GC.GRUFWD | x3, hex(cls['fwd_fused'])
    # (the last launch of the segment backward is not a gate-fused one, so its class says nothing here. That the gate-fused
    # launches ran shows in d_u: the epilogue's row partials are summed in another order than the gate kernel's)
    du = [out['bwd']['fused'][k] for k in ('d_u_h', 'd_u_o')]
    assert all(float(v.abs().max()) > 0 for v in du)
    assert any(not torch.equal(out['bwd']['fused'][k], out['bwd']['unfused'][k]) for k in ('d_u_h', 'd_u_o')), 'the gate-fused launches did not run'
    judge('seg', name, out)
