"""CPU companion of tests/test_gcn_frames_gpu.py: the executable specification of the geometric-level GCN kernels run in fp64
is the reference of every comparison there. For every case of tests/gcn_frames.py: the fp64 run really is an fp64 run and the
fp32 run sits within the random-walk bound of a 64-term fp32 sum from it (so the yardstick is neither zero nor inflated); the
inputs have the property their regime is named for (conditions on the inputs, not tolerances); a second fp32 evaluation of the
specification put in the kernel's place passes the tensor-wide rule, R1 and R2; and the specification is frame-local."""
import pytest
import torch

from tests import gcn_frames as GF
from tests.entity_envelope import F, reference_error, sqrt_k_bound

ARITH = ['train_ab', 'train_mi', 'train_md', 'train_rm', 'train_rv', 'X', 'adj', 'Z', 'e1', 'dX', 'dmd', 'dw1', 'db1', 'dgamma',
         'dbeta']   # (the eval-mode fold copies the running statistics: no arithmetic beyond a handful of roundings)
SPREAD = [c for c in GF.CASES if c['regime'] == 'spread']


@pytest.mark.parametrize('c', GF.CASES, ids=lambda c: c['id'])
def test_specification_in_fp64_and_the_inputs_of_each_regime(c):
    p, s32, s64 = GF.spec(c)
    N = c['N']
    assert s32.keys() == s64.keys()
    worst = (0.0, '')
    for k in s32:
        if k.endswith('nbt'):
            assert int(s32[k]) == int(s64[k]) == (6 if k.startswith('train') else 5)
            continue
        assert s32[k].dtype == torch.float32 and s64[k].dtype == torch.float64, (k, s32[k].dtype, s64[k].dtype)
        assert torch.isfinite(s64[k]).all(), k
        if c['regime'] != 'spread' or k not in ARITH:
            continue
        e = reference_error(s32[k], s64[k])
        worst = max(worst, (e, k))
        # one node: the only weight is exactly 1, Z = X, no gradient through it; one frame of one node: db1 = de1, nothing is summed
        trivial = N == 1 and (k in ('adj', 'Z', 'dX', 'dmd') or c['frames'] == 1)
        assert trivial or e > 0, f'{k}: the fp64 run equals the fp32 run -- it did not run in fp64'
        assert e <= sqrt_k_bound(64), f'{k}: fp32 specification {e:.3e} from fp64 > 16 x 2^-24 x sqrt(64) = {sqrt_k_bound(64):.3e}'
    n_eff, w_max = GF.adjacency_stats(s64['adj'])
    print(f"{c['id']}: fp32 specification at most {worst[0]:.2e} from fp64 ({worst[1]}); median effective senders {n_eff:.1f}, "
          f'median largest weight {w_max:.3f}')
    if c['regime'] == 'spread' and N >= 16:
        assert n_eff >= N / 4, f'spread inputs: median effective number of senders {n_eff:.1f} < N / 4'
    if c['regime'] == 'sharp' and N > 1:
        assert w_max > 0.9, f'sharp inputs: median largest weight {w_max:.3f} <= 0.9'


@pytest.mark.parametrize('c', GF.CASES, ids=lambda c: c['id'])
def test_a_second_fp32_evaluation_of_the_specification_passes_the_rule(c):
    """The rule by which the kernels are judged, applied to the feature-permuted fp32 evaluation of the specification in the
    kernel's place: tensor-wide, R1 and R2 for every tensor of every case."""
    p, s32, s64 = GF.spec(c)
    alt = GF.permuted(c, p, s32)
    fails, worst, share = [], (0.0, ''), (0.0, '')
    for k, v in alt.items():
        if k.endswith('nbt'):
            continue
        rec, f = GF.judge_named(c, k, v, s32[k], s64[k])
        fails += [f'{k}: {x}' for x in f]
        worst, share = max(worst, (rec['r1_ratio'], k)), max(share, (rec['r2_share'], k))
    print(f"{c['id']}: worst row / the specification's worst row {worst[0]:.2f} ({worst[1]}), largest R2 share "
          f'{100 * share[0]:.4f} % ({share[1]})')
    assert not fails, '\n  '.join(fails)


def test_the_rule_sees_a_defect_bound_to_one_frame_slot_and_node():
    """R2 is what holds a small error at one (frame slot of a group, node) position: it moves 1 / (FG x N) of the rows, each by
    less than R1's eight worst-row errors, and is caught by the 0.2 % cap; the unmodified fp32 specification passes."""
    c = GF.BIG[4]   # N = 50, FG = 6: the smallest share of the list, 0.33 %
    p, s32, s64 = GF.spec(c)
    N, FG = c['N'], 6
    z = s32['Z'].clone().view(c['frames'], N, 64)
    assert not GF.judge_named(c, 'Z', z, s32['Z'], s64['Z'])[1]
    z[3::FG, 7] += 32 * GF.EPS * z[3::FG, 7].abs().amax(-1, keepdim=True)   # 32 ulps of the row's largest value (2e-6)
    rec, fails = GF.judge_named(c, 'Z', z, s32['Z'], s64['Z'])
    assert any(f.startswith('R2') for f in fails), (rec, fails)
    # and a lost sender in one row is an R1 failure
    z = s32['Z'].clone().view(c['frames'], N, 64)
    z[1000, 11] -= s32['adj'][1000, 11, N - 1] * s32['X'].view(c['frames'], N, 64)[1000, N - 1]
    assert any(f.startswith('R1') for f in GF.judge_named(c, 'Z', z, s32['Z'], s64['Z'])[1])


def test_the_specification_is_frame_local():
    """With ab fixed, another geometry in one frame changes that frame's rows of X, adjacency and Z and no others."""
    c = GF.SMALL[2]
    p, s32, _ = GF.spec(c)
    N, f = c['N'], 3
    xh = p['xh'].clone()
    xh[0, f, 0, 2048:] += 1.0
    X, adj, Z = F.gcn_fused_fwd(xh, N, s32[c['fold'] + 'ab'], p['w1'], p['b1'], p['w2'], p['b2'], s32[c['fold'] + 'md'])
    for got, ref in ((X, s32['X']), (adj, s32['adj']), (Z, s32['Z'])):
        got, ref = got.reshape(c['frames'], -1), ref.reshape(c['frames'], -1)
        changed = (got != ref).any(1)
        assert changed.tolist() == [i == f for i in range(c['frames'])]
