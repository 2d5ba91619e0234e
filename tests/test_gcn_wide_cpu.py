"""CPU companion of tests/test_gcn_wide_gpu.py, the wide family of the geometric-level GCN kernels (65 ... 256 nodes).

  G18   the oracle (oracle/cpu_ref.geo_gcn) against the real reference's Geo_gcn at N = 65, 72, 176 and 256
        (tools/make_golden_gcn_wide.py), by the assertions of tests/test_oracle_golden.py::test_g1_geo_gcn;
  plan  twog_gcn_wide_launch_plan over every node count, from the library, without a GPU call;
  cases for every case of tests/gcn_wide.py a second fp32 evaluation of the specification passes the judgement the kernels get,
        the R2 cap 1 / (2 FG N) included."""
import ctypes

import numpy as np
import pytest
import torch

import twog_gcn_amd  # noqa: F401
from twog_gcn_amd import _lib, models
from oracle import cpu_ref, detgen
from tests import gcn_frames as GF
from tests import gcn_wide as GW
from tests.helpers import GOLDEN, det_state_dict, rel_err

TOL = 2e-5   # tests/test_oracle_golden.py


# ----------------------------------------------------------------------------------------------------------------- G18
@pytest.mark.parametrize('N', [65, 72, 176, 256])
@pytest.mark.parametrize('mode', ['train', 'eval'])
def test_g18_geo_gcn_beyond_64_nodes(N, mode):
    z = np.load(f'{GOLDEN}/g18_geo_gcn_wide.npz')
    y_stride, g_stride, g_whole = int(z['y_stride']), int(z['grad_stride']), int(z['grad_whole'])
    key = f'N{N}_{mode}'
    names = [k[len(key) + 6:] for k in z.files if k.startswith(key + '_grad_')]
    assert len(names) >= 10
    m_shapes = {k: tuple(v.shape) for k, v in models.GeoGcnParams(N, 4, 128).state_dict().items()}
    assert set(names) <= set(m_shapes)
    shapes = {n: m_shapes[n] for n in names}
    shapes.update({'joint_embed.cnn.0.bn.running_mean': (4 * N,), 'joint_embed.cnn.0.bn.running_var': (4 * N,),
                   'joint_embed.cnn.0.bn.num_batches_tracked': ()})
    sd = {'g.' + k: v for k, v in det_state_dict(shapes, seed=100 + N, requires_grad=True).items()}
    bs, T = 2, 2
    x = torch.from_numpy(detgen.normal(f'g18.x.{N}', (bs, 4, N, T), std=1.0, seed=1))
    r = torch.from_numpy(detgen.normal(f'g18.r.{N}', (bs, 128, N, T), std=1.0, seed=2))
    bn_state = {}
    y = cpu_ref.geo_gcn(sd, x, training=(mode == 'train'), prefix='g', bn_state=bn_state)
    yn, want = y.detach().numpy(), z[key + '_y']
    if want.ndim == 1:   # y of the two largest node counts is stored sampled
        assert want.size == -(-yn.size // y_stride)
        yn = yn.reshape(-1)[::y_stride]
    else:
        assert want.shape == (bs, 128, N, T)
    assert rel_err(yn, want) < TOL
    (y * r).sum().backward()
    for n in names:
        g, want, gmax = sd['g.' + n].grad.numpy(), z[f'{key}_grad_{n}'], float(z[f'{key}_gradmax_{n}'])
        if g.size > g_whole:
            g = g.reshape(-1)[::g_stride]
        assert g.shape == want.shape, n
        assert np.abs(g - want).max() < 5e-5 * gmax + 2e-6, n   # (the scale is the whole tensor's largest value, as in G1)
    if mode == 'train':
        assert rel_err(bn_state['running_mean'].numpy(), z[key + '_running_mean']) < TOL
        assert rel_err(bn_state['running_var'].numpy(), z[key + '_running_var']) < TOL
        assert int(bn_state['num_batches_tracked']) == int(z[key + '_nbt'])


# ---------------------------------------------------------------------------------------------------------------- plan
def test_wide_launch_plan_from_the_library():
    """Host arithmetic only: no device is opened."""
    lib = _lib.load()
    out = (ctypes.c_int * 4)()
    nmax = lib.twog_gcn_wide_max_nodes()
    assert nmax == GW.WIDE_MAX == models.GCN_MAX_NODES and nmax >= 176 and nmax % 16 == 0
    assert lib.twog_gcn_max_nodes() == GW.TUNED_MAX == 64
    for N in range(1, nmax + 1):
        for frames in (1, 7, 300):
            for kernel in range(3):
                assert lib.twog_gcn_wide_launch_plan(kernel, frames, N, out) == 0, (kernel, frames, N)
                grid, fg, lds, variant = out
                assert grid >= 1 and fg >= 1 and 0 <= lds <= 160 * 1024, (kernel, frames, N, tuple(out))
                if kernel == 0:
                    assert variant * 16 >= N and variant in (4, 8, 12, 16)
                if kernel < 2:
                    assert grid == min(frames, GW.MAX_GRID) and fg == GW.FG
    for kernel in range(3):
        assert lib.twog_gcn_wide_launch_plan(kernel, 7, 0, out) == -1
        assert lib.twog_gcn_wide_launch_plan(kernel, 7, nmax + 1, out) == -1
    assert lib.twog_gcn_wide_launch_plan(99, 7, 72, out) == -2
    assert lib.twog_gcn_launch_plan(0, 7, 65, out) == -1    # the tuned kernels keep their limit


def test_a_model_beyond_the_wide_limit_is_listed_as_unsupported():
    from tests.test_parity_gpu import STAGE1
    N = models.GCN_MAX_NODES
    ok = models.TGGCN(input_size=(2048 + 4 * N, 2048), num_classes=(13, None), hidden_size=8, gcn_node=N, **dict(STAGE1))
    assert ok._unsupported == []
    bad = models.TGGCN(input_size=(2048 + 4 * (N + 1), 2048), num_classes=(13, None), hidden_size=8, gcn_node=N + 1, **dict(STAGE1))
    assert len(bad._unsupported) == 1 and f'gcn_node = {N + 1} > {N}' in bad._unsupported[0]


# --------------------------------------------------------------------------------------------------------------- cases
def test_the_case_list_covers_what_the_issue_of_the_wide_family_names():
    ids = [c['id'] for c in GW.CASES]
    assert len(set(ids)) == len(ids)
    assert [c['N'] for c in GW.ONE] == [65, 72, 80, 176, 255, 256] and all(c['frames'] == 1 for c in GW.ONE)
    assert sorted((c['N'], c['H']) for c in GW.THREE) == sorted((N, H) for N in GW.NODE_COUNTS for H in (2, 3))
    assert [(c['N'], c['frames']) for c in GW.SECOND_TRIP] == [(72, GW.MAX_GRID + 1), (256, GW.MAX_GRID + 1)]
    assert [(c['N'], c['regime']) for c in GW.SHARP] == [(72, 'sharp'), (256, 'sharp')]
    assert [(c['N'], c['forced']) for c in GW.FORCED] == [(34, True), (64, True)]
    assert all(c['N'] > GW.TUNED_MAX or c['forced'] for c in GW.CASES)


@pytest.mark.parametrize('c', GW.CASES, ids=lambda c: c['id'])
def test_a_second_fp32_evaluation_of_the_specification_passes_the_rule(c):
    """The judgement of tests/test_gcn_wide_gpu.py applied to the feature-permuted fp32 evaluation of the specification in the
    kernel's place: tensor-wide, R1, exact zeros and R2 under the cap of the case."""
    p, s32, s64 = GW.spec(c)
    assert all(s64[k].dtype == torch.float64 for k in s64 if not k.endswith('nbt'))
    alt = GW.permuted(c, p, s32)
    assert set(alt) == set(s32)
    fails, worst, share = [], (0.0, ''), (0.0, '')
    for k, v in alt.items():
        if k.endswith('nbt'):
            continue
        rec, f = GW.judge_named(c, k, v, s32[k], s64[k])
        fails += [f'{k}: {x}' for x in f]
        worst = max(worst, (rec['r1_ratio'], k))
        if rec['rows'] >= GF.R2_MIN_ROWS:
            share = max(share, (rec['r2_share'], k))
    print(f"{c['id']}: worst row / the specification's worst row {worst[0]:.2f} ({worst[1]}), largest R2 share "
          f'{100 * share[0]:.4f} % ({share[1]}) of the cap {100 * GW.r2_cap(c):.3f} %')
    assert not fails, '\n  '.join(fails)
    if c['regime'] == 'sharp':
        assert GF.adjacency_stats(s64['adj'])[1] > 0.9, 'sharp inputs: the median largest weight is not near one'


def test_the_rule_sees_a_defect_bound_to_one_node_position():
    """A small error at one node of every frame moves 1 / N of the rows, twice the cap, each by less than R1 allows."""
    c = GW.SECOND_TRIP[0]
    p, s32, s64 = GW.spec(c)
    z = s32['Z'].clone().view(c['frames'], c['N'], 64)
    assert not GW.judge_named(c, 'Z', z, s32['Z'], s64['Z'])[1]
    z[:, 7] += 32 * GF.EPS * z[:, 7].abs().amax(-1, keepdim=True)
    rec, fails = GW.judge_named(c, 'Z', z, s32['Z'], s64['Z'])
    assert any(f.startswith('R2') for f in fails), (rec, fails)
