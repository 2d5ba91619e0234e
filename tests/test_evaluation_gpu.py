"""GPU: twog_eval_update / twog_confusion_counts through the C ABI -- golden G15 (the reference's evaluation and
scikit-learn), seeded random cases against the numpy specification (tests/evaluation_ref.py), the evaluation batch of
predict.py and a shape the capped grid needs two trips for (there also by a size-independent property), the class limit,
run-to-run identity, accumulation, the rank merge on an RCCL group and the absence of synchronisation in `update`.
Labels, counts and flags are integers and compared exactly."""
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
from tests.helpers import ROOT
from tests.test_evaluation_cpu import (OVERLAPS, cases, check_host_layer_against_golden, check_label_level_mirrors,
                                       check_result_against_golden, run_accumulator)
from oracle import postprocess_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def K():
    k = twog_kernels.get_kernels()
    assert k.name == 'hip'
    return k


def state(C):
    s = K().zeros(C * C + 2, dtype=torch.int64, device=DEV)
    return s[:C * C].view(C, C), s[C * C:]


def random_case(bs, C, T, E, ds, T_tgt, seed, with_index):
    rng = np.random.RandomState(seed)
    logp = torch.log_softmax(torch.from_numpy(rng.randn(bs, C, T, E).astype(np.float32)), 1).numpy()
    steps = np.minimum(np.arange(T_tgt) // ds, T - 1)
    tgt = np.where(rng.rand(bs, T_tgt, E) < 0.5, logp.argmax(1)[:, steps], rng.randint(0, C, size=(bs, T_tgt, E))).astype(np.int64)
    tgt[rng.rand(bs, T_tgt, E) < 0.1] = -1                     # about 10 % ignored
    tgt[bs // 2] = -1                                          # one fully ignored clip
    index = None
    if with_index:
        S = max(1, T_tgt // 2 + 1)
        index = np.full((bs, S), -1, dtype=np.int32)
        for b in range(bs):
            n = rng.randint(0, S + 1)
            index[b, :n] = np.sort(rng.choice(T_tgt, size=n, replace=n > T_tgt))
    return logp, tgt, index


def run_kernel(logp, ds, tgt, index, want_labels=True):
    C = logp.shape[1]
    counts, flags = state(C)
    si = None if index is None else torch.from_numpy(index).to(DEV)
    out = K().eval_update(torch.from_numpy(logp).to(DEV), ds, torch.from_numpy(tgt).to(DEV), si, counts, flags, want_labels)
    return counts, flags, out


def test_golden_g15():
    check_host_layer_against_golden(DEV)
    check_label_level_mirrors(DEV)


@pytest.mark.parametrize('splits', [2, 5])
def test_golden_g15_over_batch_partitions(splits):
    for case in cases():
        check_result_against_golden(case, run_accumulator(case, DEV, splits=splits).result())


@pytest.mark.parametrize('with_index', [False, True])
@pytest.mark.parametrize('ds', [1, 3, 4])
@pytest.mark.parametrize('E_', [1, 2, 16])
@pytest.mark.parametrize('C', [1, 13, 64])
def test_random_cases_vs_specification(C, E_, ds, with_index):
    bs, T = 5, 7
    for T_tgt in (T * ds - 2 if ds > 1 else T, T * ds + 3):
        logp, tgt, index = random_case(bs, C, T, E_, ds, T_tgt, seed=C * 1000 + E_ * 10 + ds, with_index=with_index)
        counts, flags, (labels, kept) = run_kernel(logp, ds, tgt, index)
        want_counts, want_flags, want_labels, want_kept = E.eval_update(logp, ds, tgt, index)
        assert np.array_equal(labels.cpu().numpy(), want_labels)
        assert np.array_equal(kept.cpu().numpy(), want_kept)
        assert np.array_equal(counts.cpu().numpy(), want_counts) and want_counts.sum() > 0
        assert np.array_equal(flags.cpu().numpy(), want_flags) and not want_flags.any()
        # the label-array entry point on the emitted labels gives the same matrix
        c2, f2 = state(C)
        K().confusion_counts(kept, labels, C, c2, f2)
        assert torch.equal(c2, counts) and not f2.any().item()
        # and no optional outputs: the same counts
        c3, _, out = run_kernel(logp, ds, tgt, index, want_labels=False)
        assert out is None and torch.equal(c3, counts)


def test_flags_vs_specification():
    logp, tgt, index = random_case(4, 6, 5, 2, 2, 11, seed=7, with_index=True)
    tgt[0, 0, 0], tgt[1, 2, 1], tgt[3, 4, 0] = 6, -2, 99
    index[0, 0], index[1, :3], index[3, -1] = 0, (2, 11, 12), 4     # two entries beyond the 11 target steps
    counts, flags, (labels, kept) = run_kernel(logp, 2, tgt, index)
    want_counts, want_flags, want_labels, want_kept = E.eval_update(logp, 2, tgt, index)
    assert want_flags[0] >= 2 and want_flags[1] == 4
    assert np.array_equal(flags.cpu().numpy(), want_flags) and np.array_equal(counts.cpu().numpy(), want_counts)
    assert np.array_equal(labels.cpu().numpy(), want_labels) and np.array_equal(kept.cpu().numpy(), want_kept)
    yt = np.array([0, 5, -1, 6, 2, -7, 3], dtype=np.int64)
    yp = np.array([0, 6, 9, 1, -1, 2, 3], dtype=np.int64)
    c2, f2 = state(6)
    K().confusion_counts(torch.from_numpy(yt).to(DEV), torch.from_numpy(yp).to(DEV), 6, c2, f2)
    want_c, want_f = E.confusion_counts(yt, yp, 6)
    assert want_f[0] == 4 and np.array_equal(c2.cpu().numpy(), want_c) and np.array_equal(f2.cpu().numpy(), want_f)


def long_shape():
    """More positions than one trip of the capped grid covers, derived from the cap the library reports."""
    _, per_trip = K().eval_limits()
    bs, E_ = 128, 2
    T_tgt = per_trip // (bs * E_) + 37
    assert bs * T_tgt * E_ > per_trip
    return bs, 13, (T_tgt + 2) // 3, E_, 3, T_tgt


@pytest.mark.parametrize('shape', ['predict_batch', 'long'])
def test_evaluation_batch_sizes(shape):
    bs, C, T, E_, ds, T_tgt = (128, 13, 120, 2, 3, 360) if shape == 'predict_batch' else long_shape()
    logp, tgt, _ = random_case(bs, C, T, E_, ds, T_tgt, seed=11, with_index=False)
    counts, flags, (labels, kept) = run_kernel(logp, ds, tgt, None)
    # vectorised restatement (the loop specification is slow at this size): labels of predict_labels, pairs by bincount
    want_labels = R.predict_labels(logp, ds, T_tgt)
    assert np.array_equal(labels.cpu().numpy(), want_labels) and np.array_equal(kept.cpu().numpy(), tgt)
    keep = tgt != -1
    want = np.bincount(tgt[keep] * C + want_labels[keep], minlength=C * C).reshape(C, C)
    assert np.array_equal(counts.cpu().numpy(), want) and not flags.any().item()
    # size-independent property: targets set to the kernel's own labels (ignored ones kept) give a diagonal matrix whose
    # trace is the number of non-ignored positions
    own = torch.where(kept == -1, kept, labels)
    c2, f2 = state(C)
    K().eval_update(torch.from_numpy(logp).to(DEV), ds, own, None, c2, f2)
    c2 = c2.cpu().numpy()
    assert np.array_equal(c2, np.diag(np.diag(c2))) and np.trace(c2) == int(keep.sum()) and not f2.any().item()
    # the Bimanual index at this size: half of the clips at half rate
    is15 = np.arange(bs) % 2 == 1
    si = pp.half_rate_step_index(T_tgt, is15)
    c3, f3, (lab3, kept3) = run_kernel(logp, ds, tgt, si.numpy())
    idx = si.numpy().astype(np.int64)
    sel_l = np.where(idx[..., None] >= 0, np.take_along_axis(want_labels, np.maximum(idx, 0)[..., None].repeat(E_, 2), 1), 0)
    sel_t = np.where(idx[..., None] >= 0, np.take_along_axis(tgt, np.maximum(idx, 0)[..., None].repeat(E_, 2), 1), -1)
    assert np.array_equal(lab3.cpu().numpy(), sel_l) and np.array_equal(kept3.cpu().numpy(), sel_t)
    keep3 = sel_t != -1
    assert np.array_equal(c3.cpu().numpy(), np.bincount(sel_t[keep3] * C + sel_l[keep3], minlength=C * C).reshape(C, C))


def test_more_than_the_class_limit_raises():
    max_classes, _ = K().eval_limits()
    assert max_classes == 64
    C = max_classes + 1
    counts, flags = state(C)
    with pytest.raises(RuntimeError, match='-2'):
        K().eval_update(torch.zeros(1, C, 2, 1, device=DEV), 1, torch.zeros(1, 2, 1, dtype=torch.int64, device=DEV), None,
                        counts, flags)
    with pytest.raises(RuntimeError, match='-2'):
        K().confusion_counts(torch.zeros(4, dtype=torch.int64, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV),
                             C, counts, flags)
    acc = pp.EvaluationAccumulator(['x'], C)
    with pytest.raises(RuntimeError):
        acc.update([torch.zeros(1, C, 2, 1, device=DEV)], [torch.zeros(1, 2, 1, dtype=torch.int64, device=DEV)])
    torch.cuda.synchronize()
    assert not counts.any().item()


def test_repeated_runs_give_identical_counts():
    logp, tgt, index = random_case(128, 13, 120, 2, 3, 360, seed=5, with_index=True)
    first = None
    for _ in range(5):
        counts, flags, _ = run_kernel(logp, 3, tgt, index, want_labels=False)
        got = torch.cat([counts.reshape(-1), flags]).cpu()
        first = got if first is None else first
        assert torch.equal(got, first)
    assert first.sum() > 0


def test_accumulation_over_batches_equals_one_call_on_the_concatenation():
    logp, tgt, index = random_case(24, 13, 20, 2, 3, 61, seed=9, with_index=True)
    whole, _, _ = run_kernel(logp, 3, tgt, index, want_labels=False)
    counts, flags = state(13)
    for sl in (slice(0, 1), slice(1, 12), slice(12, 24)):
        K().eval_update(torch.from_numpy(logp[sl]).to(DEV), 3, torch.from_numpy(tgt[sl]).to(DEV),
                        torch.from_numpy(index[sl]).to(DEV), counts, flags)
    assert torch.equal(counts, whole) and whole.sum().item() > 0
    # the accumulator, F1@k included, against the oracle on the concatenated sequences
    acc = pp.EvaluationAccumulator(['a'], 13, downsampling=3, overlaps=OVERLAPS)
    for sl in (slice(0, 1), slice(1, 12), slice(12, 24)):
        acc.update([torch.from_numpy(logp[sl]).to(DEV)], [torch.from_numpy(tgt[sl]).to(DEV)], torch.from_numpy(index[sl]).to(DEV))
    res = acc.result()['a']
    want_counts, _, want_labels, want_kept = E.eval_update(logp, 3, tgt, index)
    assert np.array_equal(res['confusion'], want_counts)
    steps = want_labels.shape[1]
    seq_t, seq_p = want_kept.transpose(0, 2, 1).reshape(-1, steps), want_labels.transpose(0, 2, 1).reshape(-1, steps)
    for ov in OVERLAPS:
        assert abs(res['f1@k'][ov] - R.f1_at_k(seq_t, seq_p, 13, ov, ignore_value=-1.0)) < 1e-6
    want = E.precision_recall_f1(want_counts, 'macro')
    assert all(abs(res['macro'][k] - want[k]) <= 1e-12 for k in want)


def _rccl_worker(rank, world, port, ret):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY='0')
    torch.cuda.set_device(0)
    dist.init_process_group('nccl', rank=rank, world_size=world, device_id=torch.device('cuda', 0))
    ret['backend'] = dist.get_backend()
    case = next(c for c in cases() if c.name == 'cad120')
    acc = run_accumulator(case, DEV)
    before = acc._state.clone()
    acc.all_reduce()
    acc.all_reduce(group=dist.group.WORLD)
    torch.cuda.synchronize()
    ret['identity'] = torch.equal(acc._state, before)     # one rank: the sum is the state itself, bit for bit
    check_result_against_golden(case, acc.result())
    ret['checked'] = True
    dist.destroy_process_group()


def test_all_reduce_on_a_single_rank_rccl_group():
    port = 34500 + os.getpid() % 2000
    ret = mp.Manager().dict()
    mp.spawn(_rccl_worker, args=(1, port, ret), nprocs=1, join=True)
    assert ret['backend'] == 'nccl' and ret['identity'] and ret['checked']


def test_update_does_not_synchronise():
    logp, tgt, index = random_case(16, 13, 20, 2, 3, 61, seed=2, with_index=True)
    outs = [torch.from_numpy(logp).to(DEV)] * 2
    tgts = [torch.from_numpy(tgt).to(DEV)] * 2
    si = torch.from_numpy(index).to(DEV)
    acc = pp.EvaluationAccumulator(['a', 'b'], 13, downsampling=3, overlaps=OVERLAPS)
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
    res = acc.result()
    want, _, _, _ = E.eval_update(logp, 3, tgt, index)
    want_plain, _, _, _ = E.eval_update(logp, 3, tgt, None)
    assert np.array_equal(res['a']['confusion'], 2 * want + want_plain) and np.array_equal(res['b']['confusion'], res['a']['confusion'])
