"""GPU: twog_gumbel_noise_fill against its numpy specification (tests/gumbel_noise_ref.py) and inside the model.

  1. the raw generator output, bit for bit: every shape, a non-zero clip offset, a call number beyond 2^32; the Random123
     known answers through the entry point;
  2. the noise against the fp64 specification of the same u;
  3. the call number advances on the device; 4. a captured fill draws the next call's noise at every replay;
  5. shard invariance; 6. the model with device noise equals the model fed the same buffer through the override.

Shapes: the smallest at which the kernel can go wrong -- one thread; (3, 3, 5); (2, 16, 67) = 2 144 threads, which crosses a
wave and a workgroup and ends in a ragged one. The grid is not capped (one thread per pair, at most 2^31 - 1 pairs), so
there is no second trip to test; the known-answer fill below runs 15.5 M threads over 60 755 workgroups.

The second Random123 vector (every counter and key word 0xffffffff) cannot be reached through the entry point: its last
counter word is t * 256 + slot with t = 2^24 - 1, and the entry point takes T < 2^24, so t <= 2^24 - 2 (and T * E * bs would
be 2^32 pairs). It is checked on the specification (tests/test_device_noise_cpu.py); here the other five words are all-ones
at the small shapes, against the specification.
"""
import numpy as np
import pytest
import torch

import twog_gcn_amd  # noqa: F401
from twog_gcn_amd import kernels as twog_kernels
from tests import gumbel_noise_ref as R
from tests.helpers import g4_inputs, load_g4
from tests.input_grad_cases import build_model, g4_loss

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SHAPES = [(1, 1, 1), (3, 3, 5), (2, 16, 67)]
SEED, CALLS, CLIP = 0x0123456789abcdef, 2 ** 32 + 5, 1000
ALL_ONES = (2 ** 64 - 1, 2 ** 64 - 1, 2 ** 32 - 1)      # seed, calls, clip offset (clip offset + b wraps modulo 2^32)


@pytest.fixture(autouse=True)
def hip_backend():
    twog_kernels._set_backend_for_tests(None)
    assert twog_kernels.get_kernels().name == 'hip'
    yield


def _fill(K, state, T, E, bs, clip=0, want_words=False):
    noise = torch.full((T * E, bs, 2), float('nan'), device=DEV)
    words = torch.zeros(T * E * bs * 4, dtype=torch.int32, device=DEV) if want_words else None
    K.gumbel_noise_fill(noise, T, E, bs, clip, state, words)
    if want_words:
        return noise, words.cpu().numpy().view(np.uint32).reshape(T, E, bs, 4)
    return noise


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize('seed,calls,clip', [(SEED, CALLS, CLIP), ALL_ONES], ids=['offset', 'all_ones'])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_words_are_the_specification_bit_for_bit(shape, seed, calls, clip):
    K = twog_kernels.get_kernels()
    T, E, bs = shape
    state = K.new_noise_state(seed, calls, device=DEV)
    _, words = _fill(K, state, T, E, bs, clip, want_words=True)
    assert np.array_equal(words, R.noise_words(seed, calls, T, E, bs, clip))


def test_known_answers_through_the_entry_point():
    """Random123's Philox4x32-10 vectors 1 and 3 (tests/test_device_noise_cpu.py: KAT). Vector 3's last counter word
    0x03707344 is t = 0x037073, slot = 0x44: the last pair of a (0x037074, 0x45, 1) fill."""
    K = twog_kernels.get_kernels()
    _, w = _fill(K, K.new_noise_state(0, 0, device=DEV), 1, 1, 1, 0, want_words=True)
    assert [int(x) for x in w.reshape(4)] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    seed, calls, clip = 0x299f31d0a4093822, 0x85a308d3243f6a88, 0x13198a2e
    T, E = 0x037073 + 1, 0x44 + 1
    state = K.new_noise_state(seed, calls, device=DEV)
    noise = torch.empty(T * E, 1, 2, device=DEV)
    words = torch.empty(T * E * 4, dtype=torch.int32, device=DEV)
    K.gumbel_noise_fill(noise, T, E, 1, clip, state, words)
    last_t = words.view(T, E, 4)[T - 1].cpu().numpy().view(np.uint32)                  # slots 0 .. 0x44 of t = 0x037073
    assert [int(x) for x in last_t[E - 1]] == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    assert np.array_equal(last_t.reshape(1, E, 1, 4), R.noise_words(seed, calls, 1, E, 1, clip, t0=T - 1))
    got = noise.view(T, E, 2)[T - 1].cpu().numpy().astype(np.float64)
    want = R.gumbel_of_words(last_t[:, :2])
    assert (np.abs(got - want) <= 2.0 ** -22 * np.maximum(1.0, np.abs(want))).all()
    assert bool(torch.isfinite(noise).all())
    assert [v % 2 ** 64 for v in state.tolist()] == [seed, calls + 1]


def test_rejected_arguments():
    K = twog_kernels.get_kernels()
    state = K.new_noise_state(1, 0, device=DEV)
    buf = torch.empty(2 * 257 * 2, device=DEV)
    with pytest.raises(RuntimeError, match='twog_gumbel_noise_fill failed with code -1'):
        K.gumbel_noise_fill(buf, 1, 257, 2, 0, state)                                  # more slots than a counter word holds
    lib = K.lib
    assert lib.twog_gumbel_noise_fill(buf.data_ptr(), 1, 1, 1, 0, None, None, K._stream()) == -1          # no state
    assert lib.twog_gumbel_noise_fill(buf.data_ptr(), 1 << 24, 1, 1, 0, state.data_ptr(), None, K._stream()) == -1
    assert lib.twog_gumbel_noise_fill(buf.data_ptr(), (1 << 24) - 1, 256, 1, 0, state.data_ptr(), None, K._stream()) == -2
    assert state.tolist() == [1, 0]                                                    # a rejected call draws nothing


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize('shape', SHAPES + [(128, 4, 64)], ids=str)
def test_noise_against_the_fp64_specification(shape):
    """|got - g| <= 2^-22 * max(1, |g|) with g the fp64 value of the same fp32-exact u: two logf of at most 2 ulp each; the
    inner one's relative error 2^-22 becomes an absolute error of the result, the outer one's is relative to |g|. Not a
    measured number: a value beyond it says something about the build (a fast-math flag). The measured maximum is written
    by tools/device_noise_cost.py."""
    K = twog_kernels.get_kernels()
    T, E, bs = shape
    state = K.new_noise_state(SEED, CALLS, device=DEV)
    noise, words = _fill(K, state, T, E, bs, CLIP, want_words=True)
    got = noise.cpu().numpy().astype(np.float64).reshape(T, E, bs, 2)
    assert np.isfinite(got).all()
    want = R.gumbel_of_words(words[..., :2])
    ratio = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print(f'shape {shape}: max |delta| / max(1, |g|) = {ratio.max() * 2 ** 22:.4f} x 2^-22')
    assert (ratio <= 2.0 ** -22).all(), ratio.max()
    assert np.array_equal(want, R.gumbel_noise(SEED, CALLS, T, E, bs, CLIP))


# ---------------------------------------------------------------------------------------------------------------- 3
def test_call_number_advances_on_the_device():
    K = twog_kernels.get_kernels()
    T, E, bs = 3, 3, 5
    state = K.new_noise_state(SEED, 5, device=DEV)
    got = [_fill(K, state, T, E, bs, CLIP, want_words=True)[1] for _ in range(3)]
    for k, w in enumerate(got):
        assert np.array_equal(w, R.noise_words(SEED, 5 + k, T, E, bs, CLIP)), k
    assert state.tolist() == [SEED, 8]
    # across the 32-bit boundary of the call number: both counter words move
    state = K.new_noise_state(SEED, 2 ** 32 - 1, device=DEV)
    got = [_fill(K, state, T, E, bs, want_words=True)[1] for _ in range(2)]
    assert np.array_equal(got[0], R.noise_words(SEED, 2 ** 32 - 1, T, E, bs))
    assert np.array_equal(got[1], R.noise_words(SEED, 2 ** 32, T, E, bs))
    assert state.tolist() == [SEED, 2 ** 32 + 1]


# ---------------------------------------------------------------------------------------------------------------- 4
def test_captured_fill_draws_new_noise_at_every_replay():
    """The call number is read from device memory by the captured launches themselves, so a graph captured once advances
    like direct calls do. The capture is of one stream and the entry point forks none: the graph is the fill and the
    one-thread advance behind it, a chain without parallel branches (the structure itself is not read back here)."""
    K = twog_kernels.get_kernels()
    T, E, bs = 2, 16, 67
    direct_state = K.new_noise_state(SEED, 40, device=DEV)
    direct = [_fill(K, direct_state, T, E, bs, CLIP).clone() for _ in range(3)]      # (also loads the code object)
    state = K.new_noise_state(SEED, 40, device=DEV)
    noise = torch.zeros(T * E, bs, 2, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        K.gumbel_noise_fill(noise, T, E, bs, CLIP, state)
    assert state.tolist() == [SEED, 40] and not bool(noise.any())                      # capturing ran nothing
    for k in range(3):
        graph.replay()
        assert torch.equal(noise, direct[k]), k
    assert state.tolist() == [SEED, 43] == direct_state.tolist()


# ---------------------------------------------------------------------------------------------------------------- 5
def test_shard_invariance_on_the_device():
    K = twog_kernels.get_kernels()
    T, E = 5, 4
    full = _fill(K, K.new_noise_state(9, 3, device=DEV), T, E, 4).view(T, E, 4, 2)
    shard = _fill(K, K.new_noise_state(9, 3, device=DEV), T, E, 2, clip=2).view(T, E, 2, 2)
    assert torch.equal(full[:, :, 2:4], shard)
    small = _fill(K, K.new_noise_state(9, 3, device=DEV), 3, 2, 4).view(3, 2, 4, 2)
    assert torch.equal(full[:3, :2], small)
    wide = _fill(K, K.new_noise_state(9, 3, device=DEV), T, E, 300).view(T, E, 300, 2)     # another grid altogether
    assert torch.equal(wide[:, :, :4], full)


# ---------------------------------------------------------------------------------------------------------------- 6
def test_model_with_device_noise_equals_the_override_of_the_same_buffer():
    K = twog_kernels.get_kernels()
    name = 'c2_stage1'
    z, meta = load_g4(name)
    kw = {k: v.to(DEV) for k, v in g4_inputs(z).items()}
    bs, T = kw['x_human'].shape[:2]
    n_gated = z['gumbel_noise'].size // (T * bs * 2)
    assert n_gated > 0

    def run(model):
        out = model(**kw)
        g4_loss(name, meta, out).backward()
        return [o.detach() for o in out], {n: p.grad for n, p in model.named_parameters()}

    a = build_model(meta, DEV).train().use_device_noise(11)
    torch.manual_seed(3)
    rng = torch.get_rng_state()
    out_a, grads_a = run(a)
    assert torch.equal(torch.get_rng_state(), rng), 'the device route drew from the CPU default generator'
    assert a.device_noise_state() == (11, 1)

    b = build_model(meta, DEV).train()
    b._gumbel_noise_override = _fill(K, K.new_noise_state(11, 0, device=DEV), T, n_gated, bs)
    out_b, grads_b = run(b)
    assert len(out_a) == len(out_b)
    for i, (x, y) in enumerate(zip(out_a, out_b)):
        assert torch.equal(x, y), i
    assert grads_a.keys() == grads_b.keys() and any(g is not None for g in grads_a.values())
    for n, g in grads_a.items():
        assert (g is None) == (grads_b[n] is None), n
        if g is not None:
            assert torch.equal(g, grads_b[n]), n
    # the noise decides gates: another call's noise gives another result
    out_c, _ = run(a)
    assert not all(torch.equal(x, y) for x, y in zip(out_a, out_c))
