// Segmental (semi-Markov) decoding of frame labels: Viterbi over whole segments with a per-class duration score, and the
// duration statistics of a label tensor. The reference project has no such decode; the definition is
// the numpy specification tests/segdecode_ref.py, restated at twog_segdecode in include/twog_gcn.h.
//
// The kernel has the shape of label_chain.h (one wave per sequence, lane c owns class c, the slab staged in chunks). A step
// t first takes e[t][c] = max over c' of (d[t-1][c'] + A[c'][c]) exactly as the Viterbi step does (lc_best_predecessor: the
// column A[:, c] in registers, d by v_readlane), then runs over the segment lengths l = 1 .. min(D, t + 1). What that run
// needs of the past, e[t-l+1][c] and logp[t-l+1][c], sits in a ring of the last Dr = min(D, T) steps in LDS, one float2 per
// (step, class): lane c reads and writes only its own column, so the ring needs no barrier and a ds_read_b64 of the wave
// is conflict-free. dur is staged once per workgroup, transposed to [l][c]. Back-pointers are two bytes per (t, c),
// len - 1 and prev, two steps packed into the 32-bit word of lane c; the words sit in LDS when they fit beside the rest and
// in the caller's workspace otherwise. The backtrace hops from segment to segment: a word is read with the lane that wrote
// it and picked by v_readlane, and the labels of a segment are written by the whole wave.
//
// All arithmetic is one fp32 add per operation in the order of the specification, comparisons are strict, and nothing
// depends on the launch geometry: the same sequence gives the same bits in any batch.
#include "twog_common.h"
#include "label_chain.h"

namespace {

constexpr int SEG_BLOCK = 8;          // segment lengths whose ring and dur reads are in flight together

static_assert(TWOG_SEGDEC_MAX_DURATION <= 256 && LC_MAX_CLASSES <= 256, "len - 1 and prev are one byte each");

struct SegPlan {
    LcGeometry g;
    int cmax;             // the class template
    int Dr;               // ring depth: min(D, T)
    int route;            // TWOG_SEGDEC_ROUTE_*
    size_t lds_bytes;     // dynamic LDS of the launch
    int64_t seq_words;    // back-pointer words of one sequence
    size_t ws_bytes;      // caller's workspace (0 on the LDS route)
};

// LDS of a workgroup of `waves` waves without back-pointers: the rings, dur, the two staging buffers
inline size_t seg_lds_bytes(int C, int Dr, int waves) {
    return (size_t)waves * Dr * C * sizeof(float2) + (size_t)Dr * C * sizeof(float) + 2 * (size_t)C * lc_row(waves) * sizeof(float);
}

// The one statement of the geometry and the route: twog_segdecode_plan reports it, the launcher uses it. The waves of a
// workgroup follow from the LDS budget: as many entities (up to LC_MAX_WAVES) as it holds rings AND back-pointers for; when
// not even one wave's back-pointers fit, they go to the workspace and the waves are as many as it holds rings for (one
// always fits: static_assert below). Waves are independent, so fewer of them per workgroup only means more workgroups.
inline SegPlan seg_plan(int bs, int C, int T, int E, int D) {
    SegPlan p;
    p.cmax = lc_dispatch_classes(C, [](auto cmax) { return (int)decltype(cmax)::value; });
    p.Dr = D < T ? D : T;
    const int64_t words = (int64_t)((T + 1) / 2) * C;
    const int most = E < LC_MAX_WAVES ? E : LC_MAX_WAVES;
    const bool bp_fits = seg_lds_bytes(C, p.Dr, 1) + (size_t)words * 4 <= LC_LDS_LIMIT;
    int waves = most;
    while (waves > 1 && seg_lds_bytes(C, p.Dr, waves) + (bp_fits ? (size_t)waves * words * 4 : 0) > LC_LDS_LIMIT) --waves;
    p.g = lc_geometry(C, E, waves);
    const size_t base = seg_lds_bytes(C, p.Dr, p.g.waves);
    if (bp_fits) {
        p.route = TWOG_SEGDEC_ROUTE_LDS;
        p.lds_bytes = base + (size_t)p.g.waves * words * 4;
        p.seq_words = words;
        p.ws_bytes = 0;
    } else {
        p.route = TWOG_SEGDEC_ROUTE_WORKSPACE;
        p.lds_bytes = base;
        p.seq_words = (words + 63) / 64 * 64;                      // whole 256-byte pieces: no line is shared by two waves
        p.ws_bytes = (size_t)bs * E * p.seq_words * 4;
    }
    return p;
}
static_assert((size_t)TWOG_SEGDEC_MAX_DURATION * LC_MAX_CLASSES * (sizeof(float2) + sizeof(float)) +
                      2 * (size_t)LC_MAX_CLASSES * (LC_CHUNK + 1) * sizeof(float) <= LC_LDS_LIMIT,
              "one wave at the largest C and D fits the LDS budget");

// grid (groups, bs), 64 * EW threads: wave w decodes entity blockIdx.x * EW + w of clip blockIdx.y.
// LDS: ring[EW][Dr][C] float2 (e, logp), dur_s[Dr][C], stage[2][C][lc_row(EW)] floats, then on the LDS route EW * seq_words
// back-pointer words. Every offset is a multiple of 8 bytes where a float2 is read.
template <int CMAX>
__global__ __launch_bounds__(64 * LC_MAX_WAVES) void segdecode_kernel(
    const float* __restrict__ logp, int C, int T, int E, const float* __restrict__ A, const float* __restrict__ pi,
    const float* __restrict__ dur, int D, int Dr, const long long* __restrict__ lengths, int ds, int T_out,
    long long* __restrict__ labels, float* __restrict__ score, unsigned* __restrict__ ws, long long seq_words, int EW,
    int bp_in_lds) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int R = CMAX / 4;                       // staged elements per thread and chunk
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nthreads = 64 * EW;
    const int b = blockIdx.y, e0 = blockIdx.x * EW, e = e0 + w;
    const bool decodes = e < E;                       // wave-uniform; a wave without an entity still stages
    const int row = lc_row(EW);
    float2* ring = reinterpret_cast<float2*>(smem) + (size_t)w * Dr * C;
    float* dur_s = smem + (size_t)2 * EW * Dr * C;
    float* stage = dur_s + (size_t)Dr * C;
    unsigned* bpw = bp_in_lds ? reinterpret_cast<unsigned*>(stage + 2 * C * row) + (int64_t)w * seq_words
                              : ws + ((int64_t)b * E + (decodes ? e : 0)) * seq_words;

    int L = T;
    if (lengths) {
        const long long given = lengths[b];
        L = given < 0 ? 0 : (given > T ? T : (int)given);
    }
    if (L == 0) {                                     // label 0 everywhere, score 0.0 (the whole workgroup leaves: L is the clip's)
        if (decodes) {
            for (int tp = lane; tp < T_out; tp += 64) labels[((int64_t)b * T_out + tp) * E + e] = 0;
            if (lane == 0) score[(int64_t)b * E + e] = 0.0f;
        }
        return;
    }

    for (int idx = tid; idx < C * Dr; idx += nthreads) {          // dur[c][l-1] -> dur_s[l-1][c]; visible after the first barrier
        const int c = idx / Dr, l = idx - c * Dr;
        dur_s[l * C + c] = dur[(int64_t)c * D + l];
    }

    LcStager S;
    S.init(tid, C, T, E, EW, e0);
    const float* base = logp + (int64_t)b * C * T * E + e0;
    float pre[R];

    const float NEG_INF = -__builtin_inff();
    const bool owns = lane < C;
    const int col = owns ? lane : 0;                  // a lane without a class reads column 0 and writes nothing
    float a[CMAX];
#pragma unroll
    for (int cp = 0; cp < CMAX; ++cp) a[cp] = (owns && cp < C) ? A[cp * C + lane] : NEG_INF;
    const float pi_c = (owns && pi) ? pi[lane] : 0.0f;
    const int my_row = col * row + w;

    float d = NEG_INF;
    unsigned pack = 0u;
    int slot = 0;                                     // t mod Dr: where step t sits in the ring
    const int n_chunks = (L + LC_CHUNK - 1) / LC_CHUNK;
    S.fetch<R>(base, 0, L, pre);
    for (int ch = 0; ch < n_chunks; ++ch) {
        const int buf = ch & 1, t0 = ch * LC_CHUNK;
        S.commit<R>(stage + buf * C * row, pre);   // buffer `buf` was last read in chunk ch - 2, which every wave left before the barrier of ch - 1
        __syncthreads();
        if (ch + 1 < n_chunks) S.fetch<R>(base, t0 + LC_CHUNK, L, pre);   // in flight while this chunk is consumed
        if (!decodes) continue;
        const float* mine = stage + buf * C * row + my_row;
        const int n_here = L - t0 < LC_CHUNK ? L - t0 : LC_CHUNK;
        for (int tt = 0; tt < n_here; ++tt) {
            const int t = t0 + tt;
            const float x = mine[tt * EW];
            float ev = pi_c;
            int pv = 0;
            if (t > 0) lc_best_predecessor<CMAX>(d, a, ev, pv);
            if (owns) ring[slot * C + lane] = make_float2(ev, x);
            // l = 1 from registers, l = 2 .. min(Dr, t + 1) from the ring, walking back from `slot`
            float acc = 0.0f + x;
            float best = (ev + dur_s[col]) + acc;
            int len = 1;
            // The walk is cut where the ring wraps, and each piece into blocks of SEG_BLOCK lengths whose reads are all
            // issued before the first is used: a single wave per SIMD hides no LDS latency by itself. The adds and the
            // comparisons stay in ascending l.
            const int n = t + 1 < Dr ? t + 1 : Dr;
            int s = __builtin_amdgcn_readfirstlane(slot);          // ring index of the step consumed last
            int l = 2;
            while (l <= n) {
                if (s == 0) s = Dr;
                const int run = n - l + 1 < s ? n - l + 1 : s;     // lengths l .. l + run - 1 sit at s - 1, s - 2, .. s - run
                const float2* rp = ring + (s - 1) * C + col;
                const float* dp = dur_s + (l - 1) * C + col;
                // lengths l + k .. l + k + cnt - 1; `whole` blocks (cnt = SEG_BLOCK) are one straight piece of code, the short
                // last block re-reads its first entry in place of the ones it does not have and skips their updates
                auto block = [&](int k, int cnt, auto whole) {
                    float2 v[SEG_BLOCK];
                    float du[SEG_BLOCK];
#pragma unroll
                    for (int j = 0; j < SEG_BLOCK; ++j) {
                        const int kj = k + ((decltype(whole)::value || j < cnt) ? j : 0);
                        v[j] = rp[-kj * C];
                        du[j] = dp[kj * C];
                    }
#pragma unroll
                    for (int j = 0; j < SEG_BLOCK; ++j) {
                        if (decltype(whole)::value || j < cnt) {
                            acc = acc + v[j].y;
                            const float cand = (v[j].x + du[j]) + acc;
                            if (cand > best) { best = cand; len = l + k + j; }
                        }
                    }
                };
                int k = 0;
                for (; k + SEG_BLOCK <= run; k += SEG_BLOCK) block(k, SEG_BLOCK, std::true_type{});
                if (k < run) block(k, run - k, std::false_type{});
                s -= run;
                l += run;
            }
            d = owns ? best : NEG_INF;
            pack |= ((unsigned)(len - 1) | ((unsigned)pv << 8)) << (16 * (t & 1));
            if ((t & 1) == 1 || t == L - 1) {
                if (owns) bpw[(int64_t)(t >> 1) * C + lane] = pack;
                pack = 0u;
            }
            slot = slot + 1 == Dr ? 0 : slot + 1;
        }
    }
    if (!decodes) return;

    // the last segment's class = the smallest c attaining max d[L-1][.]
    float top;
    int y;
    lc_best_class<CMAX>(d, top, y);
    if (lane == 0) score[(int64_t)b * E + e] = top;

    // Backtrace, one segment per trip: len of (t, c) and prev of (t - len + 1, c), each from the word its lane c wrote.
    // Segment [s0, t] of class c writes out[t'] for s0 <= t' / ds <= t, the last one also everything behind it. Whatever the
    // bytes hold, 1 <= len <= t + 1 and prev < C are enforced here, so t falls on every trip and no index leaves its buffer.
    long long* out = labels + (int64_t)b * T_out * E + e;
    int c = y < C ? y : C - 1, t = L - 1;
    while (true) {
        c = __builtin_amdgcn_readfirstlane(c);
        const unsigned word_t = owns ? bpw[(int64_t)(t >> 1) * C + lane] : 0u;
        int len = (int)((((unsigned)__builtin_amdgcn_readlane((int)word_t, c)) >> (16 * (t & 1))) & 0xffu) + 1;
        len = len > t + 1 ? t + 1 : len;
        const int s0 = t - len + 1;
        const int64_t lo = (int64_t)s0 * ds;
        const int64_t hi_steps = t == L - 1 ? (int64_t)T_out : (int64_t)(t + 1) * ds;
        const int64_t hi = hi_steps < T_out ? hi_steps : T_out;
        for (int64_t tp = lo + lane; tp < hi; tp += 64) out[tp * E] = c;
        if (s0 == 0) break;
        const unsigned word_s = owns ? bpw[(int64_t)(s0 >> 1) * C + lane] : 0u;
        const int prev = (int)((((unsigned)__builtin_amdgcn_readlane((int)word_s, c)) >> (16 * (s0 & 1) + 8)) & 0xffu);
        c = prev < C ? prev : C - 1;
        t = s0 - 1;
    }
}

// Duration counts of a label tensor at the model's rate: position (b, k, e) reads targets[b][k * stride][e]. The thread of
// a position that starts a run (a kept label whose predecessor differs, is dropped or does not exist) walks the run, at
// most D steps, and adds one to (label, min(n, D) - 1). A private 32-bit histogram per workgroup in LDS, flushed with one
// integer atomic per non-empty cell: the totals do not depend on the order.
constexpr int DUR_GRID_CAP = 1024;

__global__ __launch_bounds__(256) void duration_counts_kernel(const long long* __restrict__ targets, int n_steps, int64_t n,
                                                              int T_tgt, int E, int C, int D, int stride, long long ignore,
                                                              long long* counts) {
    extern __shared__ unsigned hist[];
    for (int k = threadIdx.x; k < C * D; k += 256) hist[k] = 0u;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int e = (int)(i % E);
        const int64_t bk = i / E;
        const int k = (int)(bk % n_steps);
        const int64_t b = bk / n_steps;
        const long long* seq = targets + b * T_tgt * E + e;           // seq[(int64_t)k * stride * E]: step k
        const long long y = seq[(int64_t)k * stride * E];
        if (!twog_label_kept(y, ignore, C)) continue;
        if (k > 0 && seq[(int64_t)(k - 1) * stride * E] == y) continue;   // inside a run
        int run = 1;
        while (run < D && k + run < n_steps && seq[(int64_t)(k + run) * stride * E] == y) ++run;
        atomicAdd(&hist[(int)y * D + run - 1], 1u);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < C * D; k += 256) {
        const unsigned v = hist[k];
        if (v != 0u) atomicAdd(reinterpret_cast<unsigned long long*>(counts + k), (unsigned long long)v);
    }
}

inline bool seg_duration_ok(int D) { return D <= TWOG_SEGDEC_MAX_DURATION; }

}  // namespace

extern "C" int twog_segdecode_limits(int* max_classes, int* max_steps, int* max_duration) {
    if (max_classes) *max_classes = LC_MAX_CLASSES;
    if (max_steps) *max_steps = LC_MAX_STEPS;
    if (max_duration) *max_duration = TWOG_SEGDEC_MAX_DURATION;
    return 0;
}

extern "C" int twog_segdecode_plan(int bs, int n_classes, int T, int E, int D, int32_t* out, size_t* workspace_bytes) {
    if (!lc_shape_ok(bs, n_classes, T, E) || D < 1) return -1;
    if (!lc_within_limits(n_classes, T) || !seg_duration_ok(D)) return -2;
    const SegPlan p = seg_plan(bs, n_classes, T, E, D);
    if (out) {
        out[0] = p.cmax;
        out[1] = p.g.waves;
        out[2] = p.g.groups;
        out[3] = p.route;
    }
    if (workspace_bytes) *workspace_bytes = p.ws_bytes;
    return 0;
}

extern "C" int twog_segdecode(const float* logp, int bs, int n_classes, int T, int E, const float* A, const float* pi,
                              const float* dur, int D, const int64_t* lengths, int downsampling, int T_out, int64_t* labels,
                              float* score, void* workspace, size_t workspace_bytes, void* stream) {
    if (!lc_shape_ok(bs, n_classes, T, E) || D < 1 || downsampling < 1 || T_out < 0) return -1;
    if (!lc_launchable(bs, n_classes, T, E) || !seg_duration_ok(D)) return -2;
    if (bs == 0) return 0;
    const SegPlan p = seg_plan(bs, n_classes, T, E, D);
    if (p.route == TWOG_SEGDEC_ROUTE_WORKSPACE && (workspace == nullptr || workspace_bytes < p.ws_bytes)) return -3;
    return lc_dispatch_classes(n_classes, [&](auto cmax) {
        return lc_launch<segdecode_kernel<decltype(cmax)::value>>(
            p.g, bs, p.lds_bytes, stream, logp, n_classes, T, E, A, pi, dur, D, p.Dr, reinterpret_cast<const long long*>(lengths),
            downsampling, T_out, reinterpret_cast<long long*>(labels), score, reinterpret_cast<unsigned*>(workspace),
            (long long)p.seq_words, p.g.waves, p.route == TWOG_SEGDEC_ROUTE_LDS ? 1 : 0);
    });
}

extern "C" int twog_duration_counts(const int64_t* targets, int bs, int T_tgt, int E, int n_classes, int D, int stride,
                                    int64_t ignore_index, int64_t* counts, void* stream) {
    if (bs < 0 || T_tgt < 0 || E < 1 || n_classes < 1 || D < 1 || stride < 1) return -1;
    if (n_classes > LC_MAX_CLASSES || !seg_duration_ok(D)) return -2;
    const int n_steps = T_tgt > 0 ? (T_tgt - 1) / stride + 1 : 0;
    const int64_t n = (int64_t)bs * n_steps * E;
    if (n == 0) return 0;
    const int grid = (int)((n + 255) / 256 < DUR_GRID_CAP ? (n + 255) / 256 : DUR_GRID_CAP);
    hipLaunchKernelGGL(duration_counts_kernel, dim3(grid), dim3(256), (size_t)n_classes * D * sizeof(unsigned),
                       (hipStream_t)stream, reinterpret_cast<const long long*>(targets), n_steps, n, T_tgt, E, n_classes, D,
                       stride, (long long)ignore_index, reinterpret_cast<long long*>(counts));
    TWOG_CHECK_LAUNCH();
    return 0;
}
