// Input augmentation on the device: one random similarity transform of the skeleton block per clip, uniform jitter and dropout
// of the feature channels. Contract, key layout and arithmetic: twog_augment_inputs in include/twog_gcn.h.
//
// No reference counterpart in the 2G-GCN trainer (its loaders hand the stored features over unchanged); SGN, the model Geo_gcn
// is taken from, rotates its skeletons at random in its loader. Here the draw is a pure function of (seed, epoch, clip id,
// element) through Philox4x32-10 (the generator of noise.hip under other keys), so a clip's augmentation does not depend on the
// batch it sits in, the rank that holds it or the launch geometry, and (seed, epoch) live in device memory: a captured launch
// draws anew once the epoch has moved on.
// Every floating-point operation is rounded once (contraction off, correctly rounded division, no transcendentals): the numpy
// specification tests/augment_ref.py is met bit for bit.
// Launches: parameters (only for the test hook), geometry (one thread per node, recomputing its clip's four parameters: one
// generator call), features (one workgroup per (clip, frame, entity) row and trip on a capped grid, humans and objects in the
// same launch; a lane takes 16 bytes = two generator calls per trip, or one element in the scalar form). No LDS, no atomics.
#include "twog_common.h"

#pragma clang fp contract(off)

namespace {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;
constexpr int AUGMENT_THREADS = 256;
constexpr int AUGMENT_GRID_CAP = 2048;   // 8 workgroups per CU

__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)PHILOX_M0 * c.x, p1 = (uint64_t)PHILOX_M1 * c.z;   // hi and lo of one 32 x 32 -> 64 product
        c = make_uint4((uint32_t)(p1 >> 32) ^ c.y ^ k0, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ c.w ^ k1, (uint32_t)p0);
        k0 += PHILOX_W0;
        k1 += PHILOX_W1;
    }
    return c;
}

// r = 2u - 1 with u = ((w >> 9) + 0.5) * 2^-23 as in noise.hip: every step exact in fp32 (an odd numerator below 2^23)
__device__ __forceinline__ float signed_unit(uint32_t w) {
    const float u = ((float)(w >> 9) + 0.5f) * 0x1p-23f;
    return (u + u) - 1.0f;
}

// (a, b, tx, ty) of one clip: generator call 0 under the geometry key
__device__ __forceinline__ float4 clip_transform(const twog_augment_t& g, uint64_t seed, uint64_t epoch, uint32_t clip) {
    const uint4 w = philox4x32_10(make_uint4((uint32_t)epoch, (uint32_t)(epoch >> 32), clip, 0u), (uint32_t)seed,
                                  (uint32_t)(seed >> 32) ^ TWOG_AUGMENT_TAG_GEOMETRY);
    const float t = g.tan_half_max * signed_unit(w.x);
    const float q = t * t;
    const float d = 1.0f + q;
    const float c = __fdiv_rn(1.0f - q, d);
    const float s = __fdiv_rn(t + t, d);
    const float gain = 1.0f + g.scale_max * signed_unit(w.y);
    return make_float4(gain * c, gain * s, g.shift_max * signed_unit(w.z), g.shift_max * signed_unit(w.w));
}

__global__ __launch_bounds__(AUGMENT_THREADS) void augment_params_kernel(twog_augment_t g) {
    const int b = blockIdx.x * AUGMENT_THREADS + threadIdx.x;
    if (b >= g.bs) return;
    const float4 p = clip_transform(g, (uint64_t)g.state[0], (uint64_t)g.state[1], (uint32_t)g.clip_ids[b]);
    float* out = g.params_out + 4 * (int64_t)b;
    out[0] = p.x; out[1] = p.y; out[2] = p.z; out[3] = p.w;
}

// one thread per (clip, frame, human row, node)
__global__ __launch_bounds__(AUGMENT_THREADS) void augment_geometry_kernel(twog_augment_t g, int64_t total) {
    const uint64_t seed = (uint64_t)g.state[0], epoch = (uint64_t)g.state[1];
    for (int64_t i = (int64_t)blockIdx.x * AUGMENT_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * AUGMENT_THREADS) {
        const int64_t row = i / g.N;             // (b * T + t) * H + h
        const int n = (int)(i - row * g.N);
        const int64_t bt = row / g.H;
        const int64_t b = bt / g.T;
        const int t = (int)(bt - b * g.T);
        if (g.steps && !((float)t < g.steps[b])) continue;
        float* p = g.x_human + row * g.F_h + g.geo_offset + 4 * n;
        const float x = p[0], y = p[1], vx = p[2], vy = p[3];
        if (!(x != 0.0f || y != 0.0f)) continue;   // a missing object or a padded frame stays zero
        const float4 m = clip_transform(g, seed, epoch, (uint32_t)g.clip_ids[b]);
        const float dx = x - g.cx, dy = y - g.cy;
        p[0] = ((m.x * dx - m.y * dy) + g.cx) + m.z;
        p[1] = ((m.y * dx + m.x * dy) + g.cy) + m.w;
        p[2] = m.x * vx - m.y * vy;
        p[3] = m.y * vx + m.x * vy;
    }
}

// first word: dropout, second word: jitter
__device__ __forceinline__ float augment_value(float x, uint32_t w_drop, uint32_t w_jitter, const twog_augment_t& g) {
    const float v = (x + g.amp * signed_unit(w_jitter)) * g.keep_scale;
    return (w_drop >> 8) >= g.drop_threshold ? v : 0.0f;
}

// one workgroup per row and trip; rows of clip b: T * H human rows (frame-major), then T * O object rows
__global__ __launch_bounds__(AUGMENT_THREADS) void augment_features_kernel(twog_augment_t g, int64_t rows_total, int vec_h,
                                                                           int vec_o) {
    const uint64_t seed = (uint64_t)g.state[0], epoch = (uint64_t)g.state[1];
    const uint32_t c0 = (uint32_t)epoch, c1 = (uint32_t)(epoch >> 32), k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const int64_t human_rows = (int64_t)g.T * g.H, clip_rows = (int64_t)g.T * (g.H + g.O);
    for (int64_t r = blockIdx.x; r < rows_total; r += gridDim.x) {
        const int64_t b = r / clip_rows, rr = r - b * clip_rows;
        const bool human = rr < human_rows;
        const int64_t row_in = human ? rr : rr - human_rows;   // t * entities + entity: the row inside the clip's block
        const int entities = human ? g.H : g.O;
        const int64_t t = row_in / entities;
        const int entity = (int)(row_in - t * entities);
        if (g.steps && !((float)t < g.steps[b])) continue;
        if (!human && g.objects_mask && !(g.objects_mask[b * g.O + entity] > 0.0f)) continue;
        const int F = human ? g.F_h : g.F_o, width = human ? g.geo_offset : g.F_o;
        const uint64_t e_row = (uint64_t)row_in * (uint64_t)F;   // < 2^33: element number of the row's first channel
        float* row = (human ? g.x_human + b * human_rows * g.F_h : g.x_objects + b * (clip_rows - human_rows) * g.F_o) + e_row;
        const uint32_t clip = (uint32_t)g.clip_ids[b];
        const uint32_t key1 = k1 ^ (human ? TWOG_AUGMENT_TAG_HUMAN : TWOG_AUGMENT_TAG_OBJECT);
        if (human ? vec_h : vec_o) {
            float4* row4 = reinterpret_cast<float4*>(row);
            for (int c4 = threadIdx.x; c4 < (width >> 2); c4 += AUGMENT_THREADS) {
                const uint32_t index = (uint32_t)((e_row + 4u * (uint32_t)c4) >> 1);   // e_row % 4 == 0: elements 2 index .. 2 index + 3
                float4 v = row4[c4];
                const uint4 wa = philox4x32_10(make_uint4(c0, c1, clip, index), k0, key1);
                const uint4 wb = philox4x32_10(make_uint4(c0, c1, clip, index + 1u), k0, key1);
                v.x = augment_value(v.x, wa.x, wa.y, g);
                v.y = augment_value(v.y, wa.z, wa.w, g);
                v.z = augment_value(v.z, wb.x, wb.y, g);
                v.w = augment_value(v.w, wb.z, wb.w, g);
                row4[c4] = v;
            }
        } else {
            for (int c = threadIdx.x; c < width; c += AUGMENT_THREADS) {
                const uint64_t e = e_row + (uint32_t)c;
                const uint4 w = philox4x32_10(make_uint4(c0, c1, clip, (uint32_t)(e >> 1)), k0, key1);
                row[c] = (e & 1u) ? augment_value(row[c], w.z, w.w, g) : augment_value(row[c], w.x, w.y, g);
            }
        }
    }
}

inline bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

}  // namespace

extern "C" int twog_augment_grid(int64_t work) {
    if (work < 0) return -2;
    return (int)(work < 1 ? 1 : work > AUGMENT_GRID_CAP ? AUGMENT_GRID_CAP : work);
}

extern "C" int twog_augment_inputs(const twog_augment_t* a, void* stream) {
    if (!a) return -1;
    twog_augment_t g = *a;
    if (g.bs < 0 || g.T < 0 || g.H < 0 || g.O < 0 || g.F_h < 0 || g.F_o < 0 || g.N < 0 || g.geo_offset < 0) return -1;
    if ((int64_t)g.geo_offset + 4 * (int64_t)g.N != (int64_t)g.F_h) return -1;
    if (g.drop_threshold >= (1u << 24)) return -1;
    if (misaligned(g.x_human, 4) || misaligned(g.x_objects, 4) || misaligned(g.steps, 4) || misaligned(g.objects_mask, 4) ||
        misaligned(g.params_out, 4) || misaligned(g.clip_ids, 8) || misaligned(g.state, 8))
        return -1;
    if (!g.x_objects) g.O = 0;
    typedef unsigned __int128 u128;
    const u128 human_block = (u128)g.T * g.H * g.F_h, object_block = (u128)g.T * g.O * g.F_o;
    if (human_block > ((u128)1 << 33) || object_block > ((u128)1 << 33)) return -2;   // the element pair number is a counter word
    if ((human_block + object_block) * (u128)g.bs >= ((u128)1 << 62)) return -1;
    if (g.bs == 0) return 0;
    if (!g.clip_ids || !g.state || (human_block > 0 && !g.x_human)) return -1;
    hipStream_t st = (hipStream_t)stream;
    if (g.params_out) {
        hipLaunchKernelGGL(augment_params_kernel, dim3((unsigned)((g.bs + AUGMENT_THREADS - 1) / AUGMENT_THREADS)),
                           dim3(AUGMENT_THREADS), 0, st, g);
        TWOG_CHECK_LAUNCH();
    }
    const int64_t nodes = (int64_t)g.bs * g.T * g.H * g.N;
    if ((g.tan_half_max != 0.0f || g.scale_max != 0.0f || g.shift_max != 0.0f) && nodes > 0) {
        const int grid = twog_augment_grid((nodes + AUGMENT_THREADS - 1) / AUGMENT_THREADS);
        hipLaunchKernelGGL(augment_geometry_kernel, dim3((unsigned)grid), dim3(AUGMENT_THREADS), 0, st, g, nodes);
        TWOG_CHECK_LAUNCH();
    }
    const int64_t rows = (int64_t)g.bs * g.T * (g.H + g.O);
    if ((g.amp != 0.0f || g.drop_threshold != 0u) && rows > 0 && (g.geo_offset > 0 || (int64_t)g.O * g.F_o > 0)) {
        const int vec_h = !misaligned(g.x_human, 16) && g.F_h % 4 == 0 && g.geo_offset % 4 == 0;
        const int vec_o = !misaligned(g.x_objects, 16) && g.F_o % 4 == 0;
        hipLaunchKernelGGL(augment_features_kernel, dim3((unsigned)twog_augment_grid(rows)), dim3(AUGMENT_THREADS), 0, st, g,
                           rows, vec_h, vec_o);
        TWOG_CHECK_LAUNCH();
    }
    return 0;
}
