// What the label-chain kernels share: viterbi.hip (decode), crf.hip (CRF loss, forward and backward), segdecode.hip
// (segmental decode) and semicrf.hip (semi-Markov CRF loss, forward and backward). DESIGN sections 4.14 to 4.17.
//
// Shape of a recursion kernel. The recurrence is serial in t and parallel in the class: one wave per sequence (clip b,
// entity e), lane c owns class c, values of other classes come by v_readlane. A workgroup is one clip and up to LC_MAX_WAVES
// neighbouring entities: together its EW waves stage time chunks of the clip's (C, LC_CHUNK, EW) slab into one of two LDS
// buffers, so that the floats of a step that sit side by side in memory are fetched once, and the loads of the next chunk are
// in flight (in registers) while this one is consumed. A buffer is C rows of LC_CHUNK * EW + 1 floats (odd stride: lanes c hit
// different banks); wave w reads step tt of class c at [c * row + tt * EW + w].
//
// Everything here is plain C++ apart from the qualifier LC_HD, so the index arithmetic also compiles for the host
// (tests/test_label_chain_cpu.py runs it there).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <type_traits>
#include "../../include/twog_gcn.h"

#ifdef __HIPCC__
#include "twog_common.h"
#define LC_HD __host__ __device__ __forceinline__
#else
#define LC_HD inline
#endif

constexpr int LC_MAX_CLASSES = 64;      // one wave: lane c owns class c (EVAL_MAX_CLASSES of postprocess.hip)
constexpr int LC_MAX_STEPS = 4096;      // SEGF1_MAX_STEPS of postprocess.hip: what the segment metrics take
constexpr int LC_CHUNK = 16;            // steps per staged chunk
constexpr int LC_MAX_WAVES = 8;         // entities of one clip per workgroup
constexpr size_t LC_LDS_LIMIT = 160 * 1024;
static_assert(TWOG_VITERBI_CHUNK == LC_CHUNK && TWOG_CRF_CHUNK == LC_CHUNK, "the public chunk sizes are the one internal chunk");

inline bool lc_shape_ok(int bs, int C, int T, int E) { return bs >= 0 && C >= 1 && T >= 1 && E >= 1; }
inline bool lc_within_limits(int C, int T) { return C <= LC_MAX_CLASSES && T <= LC_MAX_STEPS; }
// ... and a launch: offsets within a clip fit an int, the clips fit gridDim.y
inline bool lc_launchable(int bs, int C, int T, int E) {
    return lc_within_limits(C, T) && (int64_t)C * T * E <= INT32_MAX && bs <= 65535;
}

LC_HD constexpr int lc_row(int waves) { return LC_CHUNK * waves + 1; }

struct LcGeometry {
    int waves;             // entities per workgroup
    int groups;            // workgroups per clip
    int row;               // row stride of a staging buffer
    size_t buf_floats;     // one staging buffer
};
inline LcGeometry lc_geometry(int C, int E, int max_waves) {
    LcGeometry g;
    g.waves = E < max_waves ? E : max_waves;
    g.groups = (E + g.waves - 1) / g.waves;
    g.row = lc_row(g.waves);
    g.buf_floats = (size_t)C * g.row;
    return g;
}

// f(std::integral_constant<int, CMAX>) for the class ceiling CMAX of n_classes: the kernels are instantiated at 8, 16, 32, 64.
template <class F>
inline int lc_dispatch_classes(int n_classes, F&& f) {
    if (n_classes <= 8) return f(std::integral_constant<int, 8>{});
    if (n_classes <= 16) return f(std::integral_constant<int, 16>{});
    if (n_classes <= 32) return f(std::integral_constant<int, 32>{});
    return f(std::integral_constant<int, 64>{});
}

#ifdef __HIPCC__
// The launch of one kernel instance: grid (groups, bs), a wave per entity; its dynamic-LDS limit is raised once per device.
template <auto Kernel, class... Args>
inline int lc_launch(const LcGeometry& g, int bs, size_t lds_bytes, void* stream, Args... args) {
    static std::atomic<uint32_t> lds_attr_done{0};
    twog_allow_dynamic_lds(Kernel, (int)LC_LDS_LIMIT, lds_attr_done);
    hipLaunchKernelGGL(Kernel, dim3(g.groups, bs), dim3(64 * g.waves), lds_bytes, (hipStream_t)stream, args...);
    TWOG_CHECK_LAUNCH();
    return 0;
}

// The max-plus step over the classes (viterbi.hip, segdecode.hip): m = max over c' of (d[c'] + a[c']), arg = the smallest c'
// that attains it: a candidate replaces the running best only when it is strictly greater. d[c'] comes from lane c' by
// v_readlane. Four independent runs over ascending ranges, merged in ascending order under the same rule, give what one run
// over 0 .. CMAX - 1 gives. Rows c' >= C hold -inf in `a` and in d: they never win.
template <int CMAX>
__device__ __forceinline__ void lc_best_predecessor(float d, const float (&a)[CMAX], float& m, int& arg) {
    constexpr int Q = CMAX / 4;
    float bq[4];
    int aq[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        bq[j] = lane_value(d, j * Q) + a[j * Q];
        aq[j] = j * Q;
#pragma unroll
        for (int i = 1; i < Q; ++i) {
            const float cand = lane_value(d, j * Q + i) + a[j * Q + i];
            if (cand > bq[j]) { bq[j] = cand; aq[j] = j * Q + i; }
        }
    }
    m = bq[0];
    arg = aq[0];
#pragma unroll
    for (int j = 1; j < 4; ++j)
        if (bq[j] > m) { m = bq[j]; arg = aq[j]; }
}

// top = max over the lanes of d, y = the smallest lane that attains it: a scalar run over the lanes, strict comparison.
template <int CMAX>
__device__ __forceinline__ void lc_best_class(float d, float& top, int& y) {
    top = lane_value(d, 0);
    y = 0;
#pragma unroll
    for (int cp = 1; cp < CMAX; ++cp) {
        const float v = lane_value(d, cp);
        if (v > top) { top = v; y = cp; }
    }
}

// The loss kernels (crf.hip, semicrf.hip). A sequence's forward result is LC_SEQ_WORDS floats: logZ, gold, nll, K (int bits).
constexpr int LC_SEQ_WORDS = 4;
constexpr int LC_FINAL_THREADS = 256;
static_assert(TWOG_CRF_SEQ_WORDS == LC_SEQ_WORDS && TWOG_SEMICRF_SEQ_WORDS == LC_SEQ_WORDS, "one layout of the per-sequence words");

// the label of a step as the chain sees it: the class of a kept step, -1 for a removed one (the NLL terms' rule)
__device__ __forceinline__ int lc_chain_label(long long y, long long ignore, int C) {
    return twog_label_kept(y, ignore, C) ? (int)y : -1;
}

namespace {
// One workgroup: sum of nll_seq and of K over the sequences in fp64, thread i taking sequences i, i + 256, ... and the
// threads' sums added in a fixed tree; {sum, count} into stats, weight * sum / count (0 when nothing is kept) into loss.
__global__ __launch_bounds__(LC_FINAL_THREADS) void lc_nll_final_kernel(const float* __restrict__ seq, int64_t n_seq,
                                                                         float weight, double* stats, float* loss) {
    __shared__ double red[2][LC_FINAL_THREADS];
    double sum = 0.0, cnt = 0.0;
    for (int64_t s = threadIdx.x; s < n_seq; s += LC_FINAL_THREADS) {
        sum += (double)seq[s * LC_SEQ_WORDS + 2];
        cnt += (double)__float_as_int(seq[s * LC_SEQ_WORDS + 3]);
    }
    red[0][threadIdx.x] = sum;
    red[1][threadIdx.x] = cnt;
    __syncthreads();
    for (int o = LC_FINAL_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            red[0][threadIdx.x] += red[0][threadIdx.x + o];
            red[1][threadIdx.x] += red[1][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        stats[0] = red[0][0];
        stats[1] = red[1][0];
        loss[0] = weight * (float)(red[1][0] > 0.0 ? red[0][0] / red[1][0] : 0.0);
    }
}
}  // namespace
#endif

// What thread tid of 64 * EW stages of every chunk: elements k * 64 * EW + tid of the (C, chunk, EW) slab, k = 0 .. R - 1 with
// R = CMAX / 4. A class row of the slab is LC_CHUNK * EW = a quarter of the threads, so element k is class 4 k + c0 at the same
// (step tt, entity e0 + ew) for every k: the offsets are one base and one stride each. goff counts from input[b][0][t0][e0],
// soff within a staging buffer. Everything but c0, tt, soff0, goff0 and column is uniform over the workgroup.
struct LcStager {
    int C, E, c0, tt, soff0, sstep;
    int64_t goff0, gstep;
    bool column;              // the thread's entity exists
    LC_HD void init(int tid, int C_, int T, int E_, int EW, int e0) {
        const int per_class = LC_CHUNK * EW, row = lc_row(EW);
        C = C_;
        E = E_;
        c0 = tid / per_class;
        const int rem = tid - c0 * per_class;
        tt = rem / EW;
        const int ew = rem - tt * EW;
        column = e0 + ew < E;
        goff0 = ((int64_t)c0 * T + tt) * E + ew;
        gstep = (int64_t)4 * T * E;
        soff0 = c0 * row + rem;
        sstep = 4 * row;
    }
    LC_HD bool has(int k) const { return column && 4 * k + c0 < C; }
    LC_HD int64_t goff(int k) const { return goff0 + k * gstep; }
    LC_HD int soff(int k) const { return soff0 + k * sstep; }

    // the thread's elements of the chunk at t0 into registers; steps from `limit` on (the clip's length, or T) read as 0
    template <int R>
    LC_HD void fetch(const float* base, int t0, int limit, float (&pre)[R]) const {
#pragma unroll
        for (int k = 0; k < R; ++k) pre[k] = (has(k) && t0 + tt < limit) ? base[(int64_t)t0 * E + goff(k)] : 0.0f;
    }
    template <int R>
    LC_HD void commit(float* stage_buf, const float (&pre)[R]) const {
#pragma unroll
        for (int k = 0; k < R; ++k)
            if (has(k)) stage_buf[soff(k)] = pre[k];
    }
};
