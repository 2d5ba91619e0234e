"""CPU companion of tests/test_entity_envelope_gpu.py: the executable specification (tests/fake_kernels.py) run in fp64 is the
reference of every comparison there, so for every case of those lists the fp64 run must really be an fp64 run, and the
fp32 run must sit within the ordinary random-walk bound of an fp32 sum from it: 16 x 2^-24 x sqrt(K) of each tensor's
largest value, K the longest reduction in the tensor's definition (D for the attention, the column count for the
sender-side projection, T x h for the recurrence). Guards against a specification that silently stays in fp32 (then the
two runs agree exactly, and the GPU test's yardstick collapses) or that degrades."""
import pytest
import torch

from tests import entity_envelope as EE
from tests.entity_envelope import F, reference_error, sqrt_k_bound


def _check(pairs, K, what):
    """pairs: {name: (s32, s64)}"""
    worst, differs = (0.0, ''), False
    for name, (s32, s64) in pairs.items():
        assert s32.dtype == torch.float32 and s64.dtype == torch.float64, (what, name, s32.dtype, s64.dtype)
        assert torch.isfinite(s64).all(), (what, name)
        e = reference_error(s32, s64)
        differs = differs or e > 0
        worst = max(worst, (e, name))
        assert e <= sqrt_k_bound(K), f'{what} {name}: fp32 specification {e:.3e} from fp64 > 16 x 2^-24 x sqrt({K}) = {sqrt_k_bound(K):.3e}'
    assert differs, f'{what}: the fp64 run equals the fp32 run in every tensor -- it did not run in fp64'
    print(f'{what}: fp32 specification at most {worst[0]:.2e} from fp64 ({worst[1]}), bound {sqrt_k_bound(K):.2e}')


@pytest.mark.parametrize('c', EE.ATTN_CASES + EE.GROUPED, ids=lambda c: c['id'])
def test_attention_specification_in_fp64(c):
    n_alloc = EE.GROUPED_ALLOC if c in EE.GROUPED else None
    d32, d64, b32, b64 = EE.attn_spec(c, n_alloc=n_alloc)
    pairs = {k: (d32[k], d64[k]) for k in EE.attn_outputs(d32)}
    pairs.update({k: (b32[k], b64[k]) for k in EE.attn_bwd_outputs(b32)})
    _check(pairs, c['D'], 'attention ' + c['id'])
    assert not EE.att_structure_failures(d64['att'], d64)


@pytest.mark.parametrize('bs,T,H,O,h', EE.SEG_STEPWISE + EE.SEG_PERSISTENT)
def test_segment_recurrence_specification_in_fp64(bs, T, H, O, h):
    b32, b64, _, o32, o64 = EE.seg_spec(bs, T, H, O, h)
    pairs = {'fwd ' + k: (b32[k], b64[k]) for k in EE.SEG_FWD_KEYS}
    pairs.update({'bwd ' + k: (o32[k], o64[k]) for k in o32})
    _check(pairs, T * h, f'segment recurrence {(bs, T, H, O, h)}')


@pytest.mark.parametrize('H,O,ph_on,ps_on,cols', EE.SSP_CASES)
def test_sender_side_projection_specification_in_fp64(H, O, ph_on, ps_on, cols):
    i = EE.ssp_inputs(H, O, ph_on, ps_on, cols)
    s32, s64 = EE.ssp_run(F, i, H, O, ps_on), EE.ssp_run(F, i, H, O, ps_on, dtype=torch.float64)
    _check({k: (s32[k], s64[k]) for k in s32}, cols, f'ssp {(H, O, ph_on, ps_on, cols)}')


def test_sender_side_gather_specification_in_fp64():
    i = EE.ssp_gather_inputs()
    _check({'qh': (EE.ssp_gather_run(F, i), EE.ssp_gather_run(F, i, dtype=torch.float64))}, EE.SSP_GATHER[3], 'ssp_gather')


def test_judgement_sees_a_lost_sender_and_a_nonzero_virtual_row():
    """The rule itself: a result that loses one small sender's contribution in one row fails row-wise even where the
    tensor-wide maximum hides it; a masked row that is not exactly zero fails; the specification's own fp32 run passes."""
    g = torch.Generator().manual_seed(0)
    w = torch.softmax(torch.randn(6, 12, generator=g, dtype=torch.float64), -1)
    m = torch.randn(12, 64, generator=g, dtype=torch.float64)
    m[:, :] *= torch.logspace(0, -4.5, 12, dtype=torch.float64).unsqueeze(1)   # the twelfth sender is a small one
    s64 = w @ m
    s64[2] = 0.0                                                             # a virtual receiver
    s32 = (w.float() @ m.float())
    s32[2] = 0.0
    assert not EE.judge(s32, s32, s64)[1]
    lost = ((w[:, :11] @ m[:11]).float())
    lost[2] = 0.0
    rec, fails = EE.judge(lost, s32, s64)
    assert fails and rec['row_ratio'] > EE.FACTOR, (rec, fails)
    assert float((lost.double() - s64).abs().max() / s64.abs().max()) < 1e-4   # the bar of the older tests does not see it
    dirty = s32.clone()
    dirty[2, 5] = 1e-30
    assert any('not exactly zero' in f for f in EE.judge(dirty, s32, s64)[1])
