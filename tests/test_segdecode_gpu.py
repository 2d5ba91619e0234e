"""GPU: twog_segdecode and twog_duration_counts against the numpy specification (tests/segdecode_ref.py). Labels and counts
are compared as integers and scores bit for bit: the operation order is fixed, so equality is exact. The shapes are the
smallest at which the kernel can go wrong -- one class count either side of every template edge, one step either side of
the staging chunk, durations below, at and beyond the sequence, one step either side of the LDS / workspace boundary, more
entities than one workgroup takes, the longest sequence once per route -- not evaluation shapes."""
import numpy as np
import pytest
import torch

import twog_gcn_amd  # noqa: F401
from twog_gcn_amd import kernels as twog_kernels
from twog_gcn_amd import postprocess as pp
from tests import segdecode_cases as SC
from tests import segdecode_ref as S
from tests import viterbi_cases as VC

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
OVERLAPS = (0.1, 0.25, 0.5)
TEMPLATE = {1: 8, 8: 8, 9: 16, 16: 16, 17: 32, 32: 32, 33: 64, 64: 64}


def K():
    k = twog_kernels.get_kernels()
    assert k.name == 'hip'
    return k


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and a.tobytes() == b.tobytes()


def ragged(bs, T):
    """Lengths that include T, 1 and 0 (and one beyond T and one below 0, which the kernel clamps)."""
    return np.asarray([T, 1, 0, T + 5, -3, max(1, T - 1), max(1, T // 2)][:bs], dtype=np.int64)


def check(logp, A, pi, dur, lengths, ds, T_out, what, route=None):
    bs, C, T, E = logp.shape
    plan = K().segdecode_plan(bs, C, T, E, dur.shape[1])
    assert route is None or plan['route'] == route, (what, plan)
    inputs = [dev(logp), dev(A), dev(dur), dev(pi), dev(lengths)]
    labels, score = K().segment_decode(*inputs, ds, T_out)
    want, want_score = S.segment_labels(logp, A, dur, pi, lengths, ds, T_out, fast=True)
    labels, score = labels.cpu().numpy(), score.cpu().numpy()
    assert labels.dtype == np.int64 and labels.shape == want.shape, what
    bad = np.argwhere(labels != want)
    assert bad.size == 0, (what, plan, bad[:5], labels[tuple(bad[0])], want[tuple(bad[0])])
    assert same_bits(score, want_score), (what, plan, score, want_score)
    for t, before in zip(inputs, (logp, A, dur, pi, lengths)):       # the inputs are read only
        assert t is None or np.array_equal(t.cpu().numpy(), before, equal_nan=True), what
    return labels, score


def durations_for(T):
    return (1, 2, 16, 17, T, T + 3, 128)


@pytest.mark.parametrize('C', sorted(TEMPLATE))
def test_decode_equals_the_specification(C):
    """One class count either side of every template edge; for each, T either side of the staging chunk and over two
    chunks, every D of the list (below, at and beyond T, the largest), E in {1, 3, 9}, downsampling 1 and 3 with a T_out
    that is shorter or longer than T * ds, ragged lengths in every second launch."""
    n = 0
    for T in (1, 15, 16, 17, 33):
        Ds = durations_for(T)
        for D in [Ds[(n + k) % len(Ds)] for k in range(3)]:       # 15 launches: every entry of the list comes twice
            E, ds, bs = (1, 3, 9)[n % 3], (1, 3)[n % 2], (4, 3, 2)[n % 3]
            T_out = T * ds + (-2, 0, 4)[n % 3] if T * ds > 2 else T * ds + 1
            logp, A, pi, dur = SC.random_batch(1000 * C + 10 * T + n, bs, C, T, E, D)
            plan = K().segdecode_plan(bs, C, T, E, D)
            assert plan['class_template'] == TEMPLATE[C] and plan['groups'] == -(-E // plan['waves']) and (E < 9 or plan['groups'] >= 2)
            check(logp, A, pi if n % 4 else None, dur, ragged(bs, T) if n % 2 else None, ds, T_out, (C, T, D, E, ds), 'lds')
            n += 1


@pytest.mark.parametrize('T', (1, 15, 16, 17, 33))
def test_every_duration_at_every_length(T):
    """Every D of the list at every T, at a class count in the middle of a template and at the largest."""
    for n, D in enumerate(durations_for(T)):
        for C, E in ((10, 3), (64, 9 if n % 2 else 1)):
            logp, A, pi, dur = SC.random_batch(77 * T + n + C, 2, C, T, E, D)
            check(logp, A, pi, dur, np.asarray([T, T - 1], dtype=np.int64) if n % 2 else None, 3 if n % 3 == 0 else 1,
                  3 * T + 1 if n % 3 == 0 else T, (C, T, D, E))


def lds_boundary(bs, C, E, D):
    """The largest T whose back-pointers stay in LDS, asked of twog_segdecode_plan (0: none does)."""
    lo, hi = 0, S.MAX_STEPS
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if K().segdecode_plan(bs, C, mid, E, D)['route'] == 'lds':
            lo = mid
        else:
            hi = mid - 1
    return lo


@pytest.mark.parametrize('C, E, D, waves_beyond', ((32, 3, 3, 3), (33, 9, 40, 8), (64, 1, 16, 1), (64, 3, 128, 1)))
def test_either_side_of_the_lds_boundary(C, E, D, waves_beyond):
    """The longest sequence whose back-pointers fit in LDS, and one step more, which goes to the workspace. The waves per
    workgroup differ between the two (the LDS route gives up waves to keep the back-pointers inside); both equal the
    specification, so neither the route nor the waves show in the result."""
    bs = 1
    T_lds = lds_boundary(bs, C, E, D)
    inside, beyond = K().segdecode_plan(bs, C, T_lds, E, D), K().segdecode_plan(bs, C, T_lds + 1, E, D)
    assert 16 < T_lds < S.MAX_STEPS and inside['route'] == 'lds' and beyond['route'] == 'workspace'
    assert inside['class_template'] == beyond['class_template'] == (32 if C == 32 else 64)
    assert inside['workspace_bytes'] == 0 and beyond['workspace_bytes'] == bs * E * (-(-((T_lds + 2) // 2 * C) // 64) * 64) * 4
    assert inside['waves'] == 1 and beyond['waves'] == waves_beyond        # as many as the budget holds rings for
    logp, A, pi, dur = SC.random_batch(30 + C + E, bs, C, T_lds + 1, E, D)
    check(np.ascontiguousarray(logp[:, :, :T_lds]), A, pi, dur, None, 1, T_lds, ('at', C, T_lds, E), 'lds')
    check(logp, A, pi, dur, None, 1, T_lds + 1, ('beyond', C, T_lds + 1, E), 'workspace')


@pytest.mark.parametrize('C, T, E, D, waves', ((12, 700, 9, 40, 7), (8, 1500, 9, 128, 4), (16, 4096, 3, 5, 1)))
def test_waves_given_up_for_the_back_pointers(C, T, E, D, waves):
    """The two small class templates never leave LDS: one wave's back-pointers fit at any length, and the workgroup takes
    as many waves as the budget holds. Wave counts that are no power of two, and more workgroups per clip for them."""
    plan = K().segdecode_plan(1, C, T, E, D)
    assert K().segdecode_plan(1, C, S.MAX_STEPS, 9, S.MAX_DURATION)['route'] == 'lds'
    assert plan['route'] == 'lds' and plan['waves'] == waves < min(E, 8) and plan['groups'] == -(-E // waves), plan
    logp, A, pi, dur = SC.random_batch(60 + C, 1, C, T, E, D)
    check(logp, A, pi, dur, None, 1, T, (C, T, E, D), 'lds')


@pytest.mark.parametrize('C, E, route', ((64, 2, 'workspace'), (10, 2, 'lds')))
def test_the_longest_sequence_with_the_longest_duration(C, E, route):
    logp, A, pi, dur = SC.random_batch(40 + C, 1, C, S.MAX_STEPS, E, S.MAX_DURATION)
    check(logp, A, pi, dur, None, 1, S.MAX_STEPS, (C, E), route)


def test_limits_and_refusals():
    assert K().segdecode_limits() == (S.MAX_CLASSES, S.MAX_STEPS, S.MAX_DURATION) == twog_kernels.segdecode_limits()
    for shape, D in (((1, 65, 3, 1), 2), ((1, 2, S.MAX_STEPS + 1, 1), 2), ((1, 2, 5, 1), S.MAX_DURATION + 1)):
        with pytest.raises(ValueError, match='up to 64 classes, 4096 model steps and durations up to 128'):
            K().segment_decode(torch.zeros(*shape, device=DEV), torch.zeros(shape[1], shape[1], device=DEV),
                               torch.zeros(shape[1], D, device=DEV))
    T = S.MAX_STEPS
    plan = K().segdecode_plan(1, 64, T, 1, 128)
    assert plan['route'] == 'workspace' and plan['workspace_bytes'] == 2 * 64 * T
    logp = torch.zeros(1, 64, T, 1, device=DEV)
    A, dur = torch.zeros(64, 64, device=DEV), torch.zeros(64, 128, device=DEV)
    labels, score = torch.full((1, 8, 1), 7, dtype=torch.int64, device=DEV), torch.full((1, 1), 7.0, device=DEV)
    small = torch.zeros(16, device=DEV)

    def call(ws=0, n=0, bs=1, C=64, T=T, E=1, D=128, ds=1, T_out=8):
        return K().lib.twog_segdecode(logp.data_ptr(), bs, C, T, E, A.data_ptr(), 0, dur.data_ptr(), D, 0, ds, T_out,
                                      labels.data_ptr(), score.data_ptr(), ws, n, 0)
    assert call() == -3 and call(small.data_ptr(), 64) == -3                   # the workspace route without its workspace
    assert call(D=0) == -1 and call(C=0) == -1 and call(T=0) == -1 and call(E=0) == -1 and call(bs=-1) == -1
    assert call(ds=0) == -1 and call(T_out=-1) == -1
    assert call(D=129) == -2 and call(C=65) == -2 and call(T=T + 1) == -2 and call(bs=65536, T=4, D=4) == -2
    counts = torch.zeros(64, 128, dtype=torch.int64, device=DEV)
    tgt = torch.zeros(1, 4, 1, dtype=torch.int64, device=DEV)
    dc = lambda C=64, D=128, stride=1, E=1: K().lib.twog_duration_counts(tgt.data_ptr(), 1, 4, E, C, D, stride, -1, counts.data_ptr(), 0)
    assert dc(D=0) == -1 and dc(stride=0) == -1 and dc(C=0) == -1 and dc(E=0) == -1 and dc(C=65) == -2 and dc(D=129) == -2
    torch.cuda.synchronize()
    assert int(labels.min()) == 7 and float(score[0, 0]) == 7.0 and int(counts.sum()) == 0     # a refusal writes nothing


@pytest.mark.parametrize('case', SC.hand_cases(), ids=lambda c: c.name)
def test_hand_cases(case):
    logp, lengths = SC.hand_batch(case, E=3)
    labels, score = K().segment_decode(dev(logp), dev(case.A), dev(case.dur), dev(case.pi), dev(lengths))
    for e in range(3):
        assert labels[0, :, e].tolist() == case.path and float(score[0, e]) == case.score


@pytest.mark.parametrize('forbid', (0.0, 0.3))
def test_dyadic_ties(forbid):
    """The tie cases of the CPU file (there checked against brute force), many sequences to a launch: equal scores are the
    rule on this grid, so the strict comparison and the order of the candidates decide every label and every length."""
    for C in (1, 2, 3):
        for L in range(1, 7):
            for D in (1, 2, 3):
                for no_self in (False, True):
                    logp, A, pi, dur = SC.dyadic_batch(1000 * C + 10 * L + D, 4, C, L, 3, D, forbid, no_self, lowest=1)
                    check(logp, A, pi, dur, None, 1, L, ('dyadic', C, L, D, no_self), 'lds')
    for D in (5, 40):                                 # and on the eighths up to -4 over several chunks
        logp, A, pi, dur = SC.dyadic_batch(77 + D, 3, 7, 53, 3, D, forbid)
        check(logp, A, pi, dur, ragged(3, 53), 2, 110, ('dyadic long', D), 'lds')
    zero = np.zeros((7, 7), dtype=np.float32)         # nothing but the emissions: the per-step argmax
    labels, _ = check(logp, zero, None, np.zeros((7, 4), dtype=np.float32), None, 2, 110, 'zero model', 'lds')
    assert torch.equal(dev(labels), K().predict_labels(dev(logp), 2, 110))


def test_duration_one_without_scores_is_the_viterbi_decode_on_the_device():
    for seed, (C, T, E) in enumerate(((1, 5, 1), (10, 35, 3), (33, 17, 9), (64, 64, 2))):
        for logp, A, pi in (VC.random_batch(seed, 3, C, T, E), VC.dyadic_batch(seed, 3, C, T, E, 0.3)):
            lengths = dev(ragged(3, T))
            inputs = dev(logp), dev(A)
            want, want_score = K().viterbi_decode(*inputs, dev(pi), lengths, 2, 2 * T + 3)
            got, score = K().segment_decode(*inputs, torch.zeros(C, 1, device=DEV), dev(pi), lengths, 2, 2 * T + 3)
            assert torch.equal(got, want) and same_bits(score.cpu().numpy(), want_score.cpu().numpy()), (C, T, E)


def test_a_sequence_alone_equals_the_same_sequence_in_a_batch():
    logp, A, pi, dur = SC.random_batch(9, 4, 12, 35, 9, 20)
    lengths = np.asarray([35, 20, 7, 1], dtype=np.int64)
    labels, score = check(logp, A, pi, dur, lengths, 2, 80, 'batch', 'lds')
    again, again_score = K().segment_decode(dev(logp), dev(A), dev(dur), dev(pi), dev(lengths), 2, 80)
    assert np.array_equal(again.cpu().numpy(), labels) and same_bits(again_score.cpu().numpy(), score)     # a rerun
    for b, e in ((0, 0), (1, 8), (2, 4), (3, 7)):
        alone = np.ascontiguousarray(logp[b:b + 1, :, :, e:e + 1])
        one, one_score = K().segment_decode(dev(alone), dev(A), dev(dur), dev(pi), dev(lengths[b:b + 1]), 2, 80)
        assert np.array_equal(one.cpu().numpy()[0, :, 0], labels[b, :, e]) and same_bits(one_score.cpu().numpy()[0], score[b, e:e + 1])


@pytest.mark.parametrize('C, T, E, D', ((10, 33, 3, 17), (64, 0, 2, 16)))
def test_guard_words_and_run_to_run_identity(C, T, E, D):
    """labels, score and the workspace sit inside one buffer of 0x5a bytes with 256 guard bytes around each: nothing but
    the three is written. T = 0 stands for one step beyond the LDS boundary (the workspace route)."""
    bs, ds = 3, 2
    T = T or lds_boundary(bs, C, E, D) + 1
    T_out = T * ds + 3
    plan = K().segdecode_plan(bs, C, T, E, D)
    ws_bytes = plan['workspace_bytes']
    assert plan['route'] == ('workspace' if C == 64 else 'lds') and (ws_bytes > 0) == (plan['route'] == 'workspace')
    logp, A, pi, dur = SC.random_batch(50 + C, bs, C, T, E, D)
    lengths = np.asarray([T, T - 3, 0], dtype=np.int64)
    sizes = [8 * bs * T_out * E, 4 * bs * E, ws_bytes]
    span = [(s + 255) // 256 * 256 for s in sizes]
    buf = torch.full((256 * 4 + sum(span),), 0x5a, dtype=torch.uint8, device=DEV)
    guards = torch.ones(buf.numel(), dtype=torch.bool)     # every byte outside labels, score and the workspace
    at, offsets = 256, []
    for s, sp in zip(sizes, span):
        offsets.append(at)
        guards[at:at + s] = False
        at += sp + 256
    guards = guards.to(DEV)
    labels = buf[offsets[0]:offsets[0] + sizes[0]].view(torch.int64).view(bs, T_out, E)
    score = buf[offsets[1]:offsets[1] + sizes[1]].view(torch.float32).view(bs, E)
    inputs = [dev(logp), dev(A), dev(pi), dev(dur), dev(lengths)]
    before = buf.clone()
    results = []
    for _ in range(2):
        buf.copy_(before)
        rc = K().lib.twog_segdecode(inputs[0].data_ptr(), bs, C, T, E, inputs[1].data_ptr(), inputs[2].data_ptr(),
                                    inputs[3].data_ptr(), D, inputs[4].data_ptr(), ds, T_out, labels.data_ptr(),
                                    score.data_ptr(), buf.data_ptr() + offsets[2], ws_bytes,
                                    torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
        assert torch.equal(buf[guards], before[guards])
        results.append((labels.cpu().numpy().copy(), score.cpu().numpy().copy()))
    want, want_score = S.segment_labels(logp, A, dur, pi, lengths, ds, T_out, fast=True)
    for got, got_score in results:
        assert np.array_equal(got, want) and same_bits(got_score, want_score)
    for t, was in zip(inputs, (logp, A, pi, dur, lengths)):
        assert np.array_equal(t.cpu().numpy(), was)


def test_nan_and_the_all_inf_model_stay_inside():
    """NaN is out of contract, and so is +inf: whatever the labels are, they are labels. A model that forbids everything
    gives label 0 and score -inf, as the specification does."""
    logp, A, pi, dur = SC.random_batch(3, 2, 10, 40, 3, 12)
    logp[0, 3, 5:9, 1] = np.nan
    A[2, 4] = np.nan
    A[1, :] = np.inf
    dur[3, 2] = np.nan
    dur[5, :] = np.inf
    pi[7] = np.nan
    logp[1, :, 7, 0] = -np.inf
    labels, score = K().segment_decode(dev(logp), dev(A), dev(dur), dev(pi), None, 2, 85)
    assert labels.shape == (2, 85, 3) and int(labels.min()) >= 0 and int(labels.max()) < 10
    every = np.full_like(logp, np.nan)
    labels, _ = K().segment_decode(dev(every), dev(np.full_like(A, np.nan)), dev(np.full_like(dur, np.nan)), dev(np.full_like(pi, np.nan)))
    assert int(labels.min()) >= 0 and int(labels.max()) < 10
    for C, T, E, D in ((10, 40, 3, 12), (64, 33, 2, 128)):
        logp = SC.random_batch(4, 2, C, T, E, D)[0]
        none = lambda *shape: np.full(shape, -np.inf, dtype=np.float32)
        labels, score = check(logp, none(C, C), none(C), none(C, D), np.asarray([T, 3], dtype=np.int64), 1, T, 'all -inf')
        assert not labels.any() and np.isneginf(score).all()


# ---------------------------------------------------------------------------------------------------- duration counts
@pytest.mark.parametrize('stride', (1, 2, 3))
def test_duration_counts(stride):
    for name, targets, C, D, ignore in SC.count_cases():
        want = S.duration_counts(targets, C, D, stride, ignore)
        assert np.array_equal(want, SC.double_loop_counts(targets, C, D, stride, ignore)), name
        t = dev(targets)
        got = pp.duration_counts(t, C, D, stride=stride, ignore_index=ignore)
        assert got.dtype == torch.int64 and got.device == t.device and np.array_equal(got.cpu().numpy(), want), name
        assert pp.duration_counts(t, C, D, stride=stride, ignore_index=ignore, out=got) is got
        assert np.array_equal(got.cpu().numpy(), 2 * want), name                  # a second call accumulates
        assert np.array_equal(t.cpu().numpy(), targets)
    rng = np.random.default_rng(stride)                                           # several workgroups, 64 classes, D = 128
    big = np.repeat(rng.integers(-1, 66, size=(6, 40, 3)), rng.integers(1, 50, size=40), axis=1)[:, :901].astype(np.int64)
    got = pp.duration_counts(dev(big), 64, 128, stride=stride)
    assert np.array_equal(got.cpu().numpy(), S.duration_counts(big, 64, 128, stride, -1)) and int(got.sum()) > 100
    probs = pp.duration_log_probs(got, smoothing=0.5)
    assert probs.device == got.device and np.array_equal(probs.cpu().numpy(), S.duration_log_probs(got.cpu().numpy(), 0.5))


# ---------------------------------------------------------------------------------------------------- the accumulator
def run(acc, batches, step_index=None):
    for logp, tgt, lengths in batches:
        acc.update([dev(logp)] * len(acc.names), [dev(tgt)] * len(acc.names), step_index=step_index, lengths=dev(lengths))
    return acc


def test_accumulator_with_a_decoder_is_its_kernels_on_the_specification_labels():
    batches = VC.accumulator_batches(bs=4, C=13, T=20, E=3, ds=3, T_tgt=61)
    _, A, pi, dur = SC.random_batch(1, 1, 13, 1, 1, 9)
    kwargs = dict(downsampling=3, overlaps=OVERLAPS, f1_route='workgroup', edit=True)
    index = dev(pp.segment_step_index([[0, 3, 4, 9, 60], [1, 2], [], [5, 6, 7, 8, 16, 17, 40]]).numpy())
    for step_index in (None, index):
        acc = run(pp.EvaluationAccumulator(['a', 'b'], 13, decoder=pp.SegmentalDecoder(A, dur, pi), **kwargs), batches, step_index)
        spec = run(pp.EvaluationAccumulator(['a', 'b'], 13, decoder=SC.SpecDecoder(A, dur, pi), **kwargs), batches, step_index)
        assert torch.equal(acc._state, spec._state)                               # integers exactly, sums bit for bit
        res = acc.result()
        assert res['a']['confusion'].sum() > 0 and res['a']['edit'] == spec.result()['a']['edit']
        plain = run(pp.EvaluationAccumulator(['a', 'b'], 13, **kwargs), batches, step_index)
        assert not torch.equal(plain._state, acc._state)                          # the decoder is not the argmax here
