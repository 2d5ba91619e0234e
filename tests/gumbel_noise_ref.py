"""The numpy specification of twog_gumbel_noise_fill (include/twog_gcn.h): Philox4x32-10 keyed by the seed and counted by
(call, clip, time step, slot), the 23-bit uniform of its first two output words, and the Gumbel transform of that uniform in
fp64. Written from the published algorithm (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11),
not from the kernel; the GPU tests judge the kernel against it and the test double (tests/gumbel_noise_fake.py) is built on it."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57      # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85      # Weyl increments of the key
MASK32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit words, key: two; broadcast against each other -> four uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & MASK32 for x in counter]
    k = [np.asarray(x, dtype=np.uint64) & MASK32 for x in key]
    c = list(np.broadcast_arrays(*c))
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]       # < 2^64: exact in uint64
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK32]
        k = [(k[0] + np.uint64(W0)) & MASK32, (k[1] + np.uint64(W1)) & MASK32]
    return [x.astype(np.uint32) for x in c]


def noise_words(seed, calls, T, E, bs, clip_offset=0, t0=0, slot0=0):
    """uint32 [T][E][bs][4]: the generator output at time steps t0 .. t0 + T - 1, slots slot0 .. slot0 + E - 1 and clips
    clip_offset .. clip_offset + bs - 1. seed and calls are taken modulo 2^64."""
    seed, calls = int(seed) % 2 ** 64, int(calls) % 2 ** 64
    t = np.arange(t0, t0 + T, dtype=np.uint64)[:, None, None]
    slot = np.arange(slot0, slot0 + E, dtype=np.uint64)[None, :, None]
    clip = (np.arange(bs, dtype=np.uint64)[None, None, :] + np.uint64(clip_offset)) & MASK32
    assert t0 + T <= 1 << 24 and slot0 + E <= 256
    w = philox4x32_10((calls & MASK32, calls >> 32, clip, t * np.uint64(256) + slot), (seed & MASK32, seed >> 32))
    return np.stack(w, axis=-1)


def uniform_of_words(w):
    """u = ((w >> 9) + 0.5) * 2^-23 computed in fp32, where every step is exact: u in [2^-24, 1 - 2^-24]."""
    u = (np.asarray(w, dtype=np.uint32) >> np.uint32(9)).astype(np.float32)
    u = (u + np.float32(0.5)) * np.float32(2.0 ** -23)
    assert u.dtype == np.float32
    return u


def gumbel_of_words(w):
    """fp64 -log(-log(u)) of the fp32-exact u."""
    return -np.log(-np.log(uniform_of_words(w).astype(np.float64)))


def gumbel_noise(seed, calls, T, E, bs, clip_offset=0, t0=0, slot0=0):
    """fp64 [T][E][bs][2]: the noise pairs (output words 0 and 1; words 2 and 3 are unused)."""
    return gumbel_of_words(noise_words(seed, calls, T, E, bs, clip_offset, t0, slot0)[..., :2])
