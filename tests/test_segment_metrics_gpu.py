"""GPU: twog_segment_f1 / twog_segment_f1_accumulate through the C ABI -- golden G17 (the reference's per-example F1@k,
bit for bit), seeded random sequences against the numpy specification (tests/segment_metrics_ref.py) in both label
layouts up to the longest sequence the kernel takes, the refusals, a size-independent property at 1 536 sequences,
run-to-run identity, and EvaluationAccumulator(f1_route='workgroup'): no synchronisation in `update`, the fp64 reference
mean, the default route, the rank merge on an RCCL group. Counts are integers and compared exactly; the per-example F1 is
compared with ==."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import twog_gcn_amd  # noqa: F401
from twog_gcn_amd import kernels as twog_kernels
from twog_gcn_amd import postprocess as pp
from tests import evaluation_ref as E
from tests import segment_metrics_ref as S
from tests.helpers import ROOT
from tests.test_evaluation_cpu import OVERLAPS, cases
from tests.test_evaluation_gpu import random_case
from tests.test_segment_metrics_cpu import (FP32_EPS, MATRICES, check_workgroup_accumulator, dump_case, g17, matrix,
                                            run_accumulator, same_bits)
from oracle import postprocess_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
OVERLAP_SETS = ((1.0,), (0.1, 0.5, 1.0), (0.1, 0.25, 1.0 / 3.0, 0.5, 0.75, 0.9, 1.0, 1e-9))


def K():
    k = twog_kernels.get_kernels()
    assert k.name == 'hip'
    return k


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(res):
    """(f1, tp, fp, fn, valid) of K().segment_f1 as numpy arrays."""
    return [t.cpu().numpy() for t in res[:5]]


def entity_minor(y, E_):
    """(n_seq, n_steps) -> (n_seq / E, n_steps, E) holding the same sequences (sequence b * E + e)."""
    return np.ascontiguousarray(y.reshape(-1, E_, y.shape[1]).transpose(0, 2, 1))


def check_against(got, want, what):
    f1, tp, fp, fn, valid = got
    assert np.array_equal(valid, want[4]), what
    assert np.array_equal(tp, want[1]) and np.array_equal(fp, want[2]) and np.array_equal(fn, want[3]), what
    assert f1.dtype == np.float64 and same_bits(f1, want[0]), (what, np.abs(f1 - want[0]).max())


@pytest.mark.parametrize('name', MATRICES)
def test_golden_g17_through_the_abi(name):
    z = g17()
    yt, yp, ncls = matrix(z, name)
    got = host(K().segment_f1(dev(yt), dev(yp), ncls, OVERLAPS, -1))
    want = S.segment_f1(yt, yp, ncls, OVERLAPS, ignore_value=-1)
    check_against(got, want, name)
    assert same_bits(got[0], z[f'{name}_f1']) and np.array_equal(got[4], z[f'{name}_valid'])   # the reference's own values
    # the host layer on the device
    res = pp.f1_at_k_per_example(dev(yt), dev(yp), ncls, OVERLAPS, ignore_value=-1.0, need_counts=True)
    assert res.route == 'workgroup' and res.f1.device.type == 'cuda' and same_bits(res.f1.cpu().numpy(), z[f'{name}_f1'])
    multi = pp.evaluate_f1_at_k_multi({'sub-activity_recognition': dev(yt)}, {'sub-activity_recognition': dev(yp)}, ncls, None)
    assert [multi[ov]['sub-activity_recognition'] for ov in OVERLAPS] == z[f'{name}_mean'].tolist()


def test_golden_g17_text():
    z = g17()
    types, targets, outputs, n_names, ids = dump_case(z)
    outputs = {t: dev(outputs[t]) for t in types}
    targets = {t: dev(targets[t]) for t in types}
    for k, ov in enumerate(OVERLAPS):
        text = pp.f1_scores_per_example(outputs, targets, ids, n_names['sub-activity_recognition'],
                                        n_names['affordance_recognition'], ov)
        assert text.encode() == str(z[f'dump_text_{k}']).encode()


def random_sequences(n_seq, n_steps, ncls, seed):
    """The sequences of test_postprocess_gpu.test_random_sequences_vs_oracle."""
    rng = np.random.RandomState(seed)
    runs = lambda: np.repeat(rng.randint(0, ncls + 1, size=n_steps), rng.randint(1, 6, size=n_steps))[:n_steps]
    yt = np.stack([runs() for _ in range(n_seq)]).astype(np.int64)
    yp = np.stack([runs() for _ in range(n_seq)]).astype(np.int64)
    yp[: n_seq // 2] = yt[: n_seq // 2]
    yp[: n_seq // 2, ::7] = (yp[: n_seq // 2, ::7] + 1) % (ncls + 1)
    yt[rng.rand(n_seq, n_steps) < 0.1] = -1
    if n_seq > 4:
        yt[1] = -1
    return yt, yp


def shapes():
    max_steps, _ = K().segment_f1_limits()
    return [(37, 120, 13, 0), (5, 1, 3, 1), (64, 333, 10, 2), (3, 17, 1, 3), (6, 1061, 13, 4), (6, max_steps, 13, 5)]


@pytest.mark.parametrize('shape', range(6))
def test_random_sequences_vs_specification(shape):
    n_seq, n_steps, ncls, seed = shapes()[shape]
    yt, yp = random_sequences(n_seq, n_steps, ncls, seed)
    E_ = 2 if n_seq % 2 == 0 else (3 if n_seq % 3 == 0 else n_seq)
    for overlaps in OVERLAP_SETS:
        want = S.segment_f1(yt, yp, ncls, overlaps, ignore_value=-1)
        assert want[4].sum() >= n_seq - 1 and want[1].sum() > 0
        check_against(host(K().segment_f1(dev(yt), dev(yp), ncls, overlaps, -1)), want, (shape, overlaps, 'sequence-major'))
        got = K().segment_f1(dev(entity_minor(yt, E_)), dev(entity_minor(yp, E_)), ncls, overlaps, -1, entity_minor=True)
        check_against(host(got), want, (shape, overlaps, 'entity-minor', E_))
    # no ignore value: -1 is a label like any other. And labels are compared as int64: these agree in their low 32 bits
    wide = lambda y: y * (np.int64(1) << 32) + 7 - (np.int64(1) << 50)
    for t, p in ((yt, yp), (wide(yt), wide(yp))):
        want = S.segment_f1(t, p, ncls, (0.25,), ignore_value=None)
        assert want[4].all() and want[1].sum() > 0
        check_against(host(K().segment_f1(dev(t), dev(p), ncls, (0.25,), None)), want, (shape, 'no ignore value'))


def test_one_step_more_than_the_limit_is_refused_and_falls_back():
    max_steps, max_overlaps = K().segment_f1_limits()
    assert max_steps >= 4096 and max_overlaps == 8
    yt, yp = random_sequences(4, max_steps + 1, 13, 6)
    with pytest.raises(RuntimeError, match='twog_segment_f1 failed with code -2'):
        K().segment_f1(dev(yt), dev(yp), 13, OVERLAPS, -1)
    res = pp.f1_at_k_per_example(dev(yt), dev(yp), 13, OVERLAPS, ignore_value=-1.0)
    assert res.route == 'thread' and res.tp is None
    want = S.segment_f1(yt, yp, 13, OVERLAPS, ignore_value=-1)
    assert np.array_equal(res.valid.cpu().numpy(), want[4])
    assert np.abs(res.f1.cpu().numpy() - want[0]).max() <= FP32_EPS      # that route stores fp32
    with pytest.raises(ValueError, match='workgroup route'):
        pp.f1_at_k_per_example(dev(yt), dev(yp), 13, OVERLAPS, ignore_value=-1.0, need_counts=True)
    at_limit = pp.f1_at_k_per_example(dev(yt[:, :max_steps]), dev(yp[:, :max_steps]), 13, OVERLAPS, ignore_value=-1.0)
    assert at_limit.route == 'workgroup'


def test_overlaps_the_kernel_does_not_take_are_refused_and_fall_back():
    yt, yp = random_sequences(8, 50, 5, 7)
    for overlaps in ((0.0,), (0.25, -0.1), (float('nan'),), tuple(0.1 * (j + 1) for j in range(9)), ()):
        with pytest.raises(RuntimeError, match='twog_segment_f1 failed with code -1'):
            K().segment_f1(dev(yt), dev(yp), 5, overlaps, -1)
    res = pp.f1_at_k_per_example(dev(yt), dev(yp), 5, (0.0, 0.25), ignore_value=-1.0)
    assert res.route == 'thread' and res.tp is None
    for k, ov in enumerate((0.0, 0.25)):
        for s in range(8):
            keep = yt[s] != -1
            if keep.any():
                assert abs(res.f1[s, k].item() - R.f1_at_k_single_example(yt[s][keep], yp[s][keep], 5, ov)) <= FP32_EPS
    nine = pp.f1_at_k_per_example(dev(yt), dev(yp), 5, [0.1 * (j + 1) for j in range(9)], ignore_value=-1.0, need_counts=True)
    assert nine.route == 'workgroup'
    want = S.segment_f1(yt, yp, 5, [0.1 * (j + 1) for j in range(9)], ignore_value=-1)
    check_against([t.cpu().numpy() for t in nine[:5]], want, 'nine overlaps')


def test_predictions_equal_to_targets_give_one_at_1536_sequences():
    bs, C, T, E_, ds = 768, 13, 120, 2, 3
    g = torch.Generator().manual_seed(0)
    logp = torch.log_softmax(torch.randn(bs, C, T, E_, generator=g), 1).to(DEV)
    lab = pp.predict_labels(logp, torch.zeros(bs, T * ds + 2, E_, dtype=torch.int64, device=DEV), ds)
    assert lab.shape == (bs, T * ds + 2, E_) and bs * E_ == 1536
    f1, tp, fp, fn, valid, _ = K().segment_f1(lab, lab, C, (0.1, 0.5, 1.0), -1, entity_minor=True)
    assert f1.shape == (1536, 3) and bool((f1 == 1.0).all()) and bool((valid == 1).all())
    assert not fp.any().item() and not fn.any().item()
    segments = 1 + (lab[:, 1:] != lab[:, :-1]).sum(1).reshape(-1)          # (bs, E) -> sequence b * E + e
    assert torch.equal(tp, segments.to(torch.int32).unsqueeze(1).expand(-1, 3))
    seq = lab.transpose(1, 2).reshape(-1, lab.shape[1]).contiguous()
    again = K().segment_f1(seq, seq, C, (0.1, 0.5, 1.0), -1)
    assert all(torch.equal(a, b) for a, b in zip(again[:5], (f1, tp, fp, fn, valid)))


def test_repeated_runs_are_bit_identical():
    yt, yp = random_sequences(256, 360, 13, 8)
    t, p = dev(entity_minor(yt, 2)), dev(entity_minor(yp, 2))
    sums = K().zeros(2 * 8, dtype=torch.float64, device=DEV)
    first = None
    for _ in range(5):
        res = K().segment_f1(t, p, 13, OVERLAP_SETS[2], -1, entity_minor=True)
        sums.zero_()
        K().segment_f1_accumulate(res[0], res[4], sums[:8], sums[8:])
        got = [x.cpu() for x in res[:5]] + [sums.cpu()]
        first = got if first is None else first
        assert all(a.dtype == b.dtype and a.numpy().tobytes() == b.numpy().tobytes() for a, b in zip(got, first))
    f1, valid, want_sums = first[0].numpy(), first[4].numpy(), first[5].numpy()
    assert valid.sum() == 255 and (want_sums[8:] == 255.0).all()
    # only the order of the fp64 sum differs from numpy's: n values in [0, 1]
    assert np.abs(want_sums[:8] - f1.sum(0)).max() <= 2 * 256 * 2.0 ** -53 * 256
    # it ADDS to what the slots hold
    K().segment_f1_accumulate(res[0], res[4], sums[:8], sums[8:])
    assert np.array_equal(sums.cpu().numpy(), 2 * want_sums)


def accumulator_case():
    logp, tgt, index = random_case(16, 13, 20, 2, 3, 61, seed=2, with_index=True)
    return logp, tgt, index, [dev(logp)] * 2, [dev(tgt)] * 2, dev(index)


def test_workgroup_update_does_not_synchronise_and_matches_the_reference_mean():
    logp, tgt, index, outs, tgts, si = accumulator_case()
    acc = pp.EvaluationAccumulator(['a', 'b'], 13, downsampling=3, overlaps=OVERLAPS, f1_route='workgroup')
    default = pp.EvaluationAccumulator(['a', 'b'], 13, downsampling=3, overlaps=OVERLAPS)
    acc.update(outs, tgts, si)                                # allocation and library load happen here
    probe = torch.ones(1, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(RuntimeError):                     # the mode is live in this build
            probe.item()
        acc.update(outs, tgts, si)
        acc.update(outs, tgts)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert acc.last_f1_route == 'workgroup'
    for step_index in (si, si, None):
        default.update(outs, tgts, step_index)
    assert default.last_f1_route == 'thread'
    res, res_default = acc.result(), default.result()
    seq_t, seq_p = [], []
    for idx in (index, index, None):
        _, _, labels, kept = E.eval_update(logp, 3, tgt, idx)
        # sequences of different length cannot be stacked: pad the shorter with ignored steps
        width = tgt.shape[1]
        pad = lambda a, v: np.concatenate([a, np.full((a.shape[0], width - a.shape[1], a.shape[2]), v, dtype=a.dtype)], 1)
        seq_t.append(pad(kept, -1).transpose(0, 2, 1).reshape(-1, width))
        seq_p.append(pad(labels, 0).transpose(0, 2, 1).reshape(-1, width))
    seq_t, seq_p = np.concatenate(seq_t), np.concatenate(seq_p)
    for name in ('a', 'b'):
        assert np.array_equal(res[name]['confusion'], res_default[name]['confusion'])
        for ov in OVERLAPS:
            want = R.f1_at_k(seq_t, seq_p, 13, ov, ignore_value=-1.0)
            assert abs(res[name]['f1@k'][ov] - want) <= 1e-12, (name, ov, res[name]['f1@k'][ov], want)   # the summation order
            assert abs(res[name]['f1@k'][ov] - res_default[name]['f1@k'][ov]) <= 1e-6, (name, ov)        # fp32 values there


def test_workgroup_accumulator_on_golden_g15_and_its_fallback():
    for case in cases():
        acc = run_accumulator(case, DEV, overlaps=OVERLAPS, f1_route='workgroup')
        assert acc.last_f1_route == 'workgroup'
        check_workgroup_accumulator(case, acc.result())
    case = next(c for c in cases() if c.name == 'cad120')
    acc = run_accumulator(case, DEV, overlaps=(0.0, 0.25), f1_route='workgroup')
    assert acc.last_f1_route == 'thread'
    thread = run_accumulator(case, DEV, overlaps=(0.0, 0.25))
    assert torch.equal(acc._state, thread._state)             # the fallback IS the default route


def _rccl_worker(rank, world, port, ret):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY='0')
    torch.cuda.set_device(0)
    dist.init_process_group('nccl', rank=rank, world_size=world, device_id=torch.device('cuda', 0))
    ret['backend'] = dist.get_backend()
    case = next(c for c in cases() if c.name == 'cad120')
    acc = run_accumulator(case, DEV, overlaps=OVERLAPS, f1_route='workgroup')
    before = acc._state.clone()
    acc.all_reduce()
    acc.all_reduce(group=dist.group.WORLD)
    torch.cuda.synchronize()
    ret['identity'] = torch.equal(acc._state, before)     # one rank: the sum is the state itself, bit for bit
    ret['route'] = acc.last_f1_route
    check_workgroup_accumulator(case, acc.result())
    ret['checked'] = True
    dist.destroy_process_group()


def test_all_reduce_on_a_single_rank_rccl_group():
    port = 36500 + os.getpid() % 2000
    ret = mp.Manager().dict()
    mp.spawn(_rccl_worker, args=(1, port, ret), nprocs=1, join=True)
    assert ret['backend'] == 'nccl' and ret['identity'] and ret['checked'] and ret['route'] == 'workgroup'
