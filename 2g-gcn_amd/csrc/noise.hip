// Gumbel noise of the segment-boundary gates, drawn on the device by a counter-based generator (Philox4x32-10).
//
// Reference: gumbel_sigmoid / sample_gumbel (pyrutils/torch/distributions.py:4-36) draw g = -log(-log(u)) per gate call on the
// host's default generator; gate.hip reads the pre-drawn values as [T][noise_entities][bs][2]. Here every pair is a pure function
// of (seed, call number, clip, time step, noise slot) -- see twog_gumbel_noise_fill in include/twog_gcn.h -- so that a clip's
// noise does not depend on the batch it sits in, the rank that holds it or the launch geometry, and the call number lives in
// device memory: the same two launches, captured once, draw new noise at every replay.
// One thread per (t, slot, b), b fastest: a wave writes 64 consecutive float2 (512 B) and, for the test hook, 64 uint4 (1 KiB).
// Integer work only in front of two logf per value; no LDS.
#include "twog_common.h"

namespace {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(PHILOX_M0, c.x), lo0 = PHILOX_M0 * c.x;
        const uint32_t hi1 = __umulhi(PHILOX_M1, c.z), lo1 = PHILOX_M1 * c.z;
        c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
        k0 += PHILOX_W0;
        k1 += PHILOX_W1;
    }
    return c;
}

// 23 bits of a word -> u in [2^-24, 1 - 2^-24] (every step exact in fp32) -> standard Gumbel, finite by construction
__device__ __forceinline__ float gumbel_of_word(uint32_t w) {
    const float u = ((float)(w >> 9) + 0.5f) * 0x1p-23f;
    return -logf(-logf(u));
}

__global__ __launch_bounds__(256) void gumbel_noise_kernel(float2* __restrict__ noise, uint4* __restrict__ words,
                                                           const int64_t* __restrict__ state, uint32_t E, uint32_t bs,
                                                           uint32_t clip_offset, uint32_t total) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    const uint64_t seed = (uint64_t)state[0], calls = (uint64_t)state[1];
    const uint32_t r = i / bs, b = i - r * bs;
    const uint32_t t = r / E, slot = r - t * E;
    const uint4 w = philox4x32_10(make_uint4((uint32_t)calls, (uint32_t)(calls >> 32), clip_offset + b, t * 256u + slot),
                                  (uint32_t)seed, (uint32_t)(seed >> 32));
    noise[i] = make_float2(gumbel_of_word(w.x), gumbel_of_word(w.y));
    if (words) words[i] = w;
}

// the call number moves on behind the fill, in stream order: a launch of its own, so no workgroup of the fill can see the new
// value, and nothing the host knows about the call number enters either launch
__global__ void gumbel_noise_advance_kernel(int64_t* state) {
    if (blockIdx.x == 0 && threadIdx.x == 0) state[1] = (int64_t)((uint64_t)state[1] + 1u);
}

}  // namespace

extern "C" int twog_gumbel_noise_fill(float* noise, int T, int noise_entities, int bs, uint32_t clip_offset, int64_t* state,
                                      uint32_t* words_or_null, void* stream) {
    if (!state || noise_entities > 256 || T >= (1 << 24)) return -1;
    if (T < 0 || noise_entities < 0 || bs < 0) return -1;
    const int64_t total = (int64_t)T * noise_entities * bs;
    if (total >= (int64_t(1) << 31)) return -2;
    if (total > 0 && !noise) return -1;
    if ((reinterpret_cast<uintptr_t>(noise) & 7) || (reinterpret_cast<uintptr_t>(words_or_null) & 15)) return -1;   // 8 / 16-byte stores
    hipStream_t st = (hipStream_t)stream;
    if (total > 0) {
        hipLaunchKernelGGL(gumbel_noise_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                           reinterpret_cast<float2*>(noise), reinterpret_cast<uint4*>(words_or_null), state,
                           (uint32_t)noise_entities, (uint32_t)bs, clip_offset, (uint32_t)total);
        TWOG_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(gumbel_noise_advance_kernel, dim3(1), dim3(64), 0, st, state);
    TWOG_CHECK_LAUNCH();
    return 0;
}
