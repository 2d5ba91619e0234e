// Viterbi decoding of frame labels under a label-transition model, and the transition statistics of a label tensor
// (DESIGN section 4.14). The reference project decodes with a per-step argmax only; the definition is the numpy
// specification tests/viterbi_ref.py, restated at twog_viterbi_decode in include/twog_gcn.h.
//
// The decode kernel has the shape of label_chain.h (one wave per sequence, lane c owns class c, the slab staged in chunks).
// The column A[:, c] lives in registers; d[t-1][c'] is taken from lane c' by v_readlane (a constant lane per unrolled
// iteration), so a step needs no LDS exchange and no barrier. Back-pointers are one byte per (t, c), four steps packed into
// the 32-bit word of lane c; the words sit in LDS when the whole sequence fits beside the staging buffers and in the caller's
// workspace otherwise. The backtrace reads a word with the lane that wrote it and follows the path with v_readlane, so the
// only dependent chain is scalar.
//
// All arithmetic is one fp32 add per operation in the order of the specification, comparisons are strict, and nothing
// depends on the launch geometry: the same sequence gives the same bits in any batch.
#include "twog_common.h"
#include "label_chain.h"

namespace {

struct VitPlan {
    LcGeometry g;
    int route;            // TWOG_VITERBI_ROUTE_*
    size_t lds_bytes;     // dynamic LDS of the launch
    int64_t seq_words;    // back-pointer words of one sequence
    size_t ws_bytes;      // caller's workspace (0 on the LDS route)
};

// The one statement of the route: twog_viterbi_workspace reports it, the launcher uses it.
inline VitPlan vit_plan(int bs, int C, int T, int E) {
    VitPlan p;
    p.g = lc_geometry(C, E, LC_MAX_WAVES);
    const size_t stage_bytes = 2 * p.g.buf_floats * sizeof(float);
    const int64_t words = (int64_t)((T + 3) / 4) * C;
    const size_t with_bp = stage_bytes + (size_t)p.g.waves * words * 4;
    if (with_bp <= LC_LDS_LIMIT) {
        p.route = TWOG_VITERBI_ROUTE_LDS;
        p.lds_bytes = with_bp;
        p.seq_words = words;
        p.ws_bytes = 0;
    } else {
        p.route = TWOG_VITERBI_ROUTE_WORKSPACE;
        p.lds_bytes = stage_bytes;
        p.seq_words = (words + 63) / 64 * 64;                      // whole 256-byte pieces: no line is shared by two waves
        p.ws_bytes = (size_t)bs * E * p.seq_words * 4;
    }
    return p;
}

// grid (groups, bs), 64 * EW threads: wave w decodes entity blockIdx.x * EW + w of clip blockIdx.y.
// LDS: stage[2][C][lc_row(EW)] floats, then on the LDS route EW * seq_words back-pointer words.
template <int CMAX>
__global__ __launch_bounds__(64 * LC_MAX_WAVES) void viterbi_kernel(
    const float* __restrict__ logp, int C, int T, int E, const float* __restrict__ A, const float* __restrict__ pi,
    const long long* __restrict__ lengths, int ds, int T_out, long long* __restrict__ labels, float* __restrict__ score,
    unsigned* __restrict__ ws, long long seq_words, int EW, int bp_in_lds) {
    extern __shared__ float smem[];
    constexpr int R = CMAX / 4;                       // staged elements per thread and chunk: C * LC_CHUNK * EW / (64 * EW)
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nthreads = 64 * EW;
    const int b = blockIdx.y, e0 = blockIdx.x * EW, e = e0 + w;
    const bool decodes = e < E;                       // wave-uniform; a wave without an entity still stages
    const int row = lc_row(EW), per_class = LC_CHUNK * EW;
    float* stage = smem;
    unsigned* bpw = bp_in_lds ? reinterpret_cast<unsigned*>(smem + 2 * C * row) + (int64_t)w * seq_words
                              : ws + ((int64_t)b * E + (decodes ? e : 0)) * seq_words;

    int L = T;
    if (lengths) {
        const long long given = lengths[b];
        L = given < 0 ? 0 : (given > T ? T : (int)given);
    }
    if (L == 0) {                                     // label 0 everywhere, score 0.0
        if (decodes) {
            for (int tp = lane; tp < T_out; tp += 64) labels[((int64_t)b * T_out + tp) * E + e] = 0;
            if (lane == 0) score[(int64_t)b * E + e] = 0.0f;
        }
        return;
    }

    // What this thread stages of every chunk: element k * nthreads + tid of the (C, chunk, EW) slab. goff: its offset from
    // logp[b][0][t0][e0] (-1: nothing), soff: its place in a staging buffer, tt: its step within the chunk. The mapping is
    // LcStager's (label_chain.h); the decode keeps it as arrays and its own loops because its 64-class instance measured 1 %
    // slower on the stager's members.
    int goff[R], soff[R], tt_of[R];
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const int idx = k * nthreads + tid;
        const int c = idx / per_class, rem = idx - c * per_class;
        const int tt = rem / EW, ew = rem - tt * EW;
        const bool any = c < C && e0 + ew < E;
        goff[k] = any ? (c * T + tt) * E + ew : -1;   // < C * T * E, checked by the launcher to fit an int
        soff[k] = c * row + rem;
        tt_of[k] = tt;
    }
    const float* base = logp + (int64_t)b * C * T * E + e0;
    float pre[R];
    auto fetch = [&](int t0) {
#pragma unroll
        for (int k = 0; k < R; ++k)
            pre[k] = (goff[k] >= 0 && t0 + tt_of[k] < L) ? base[(int64_t)t0 * E + goff[k]] : 0.0f;
    };
    auto commit = [&](int buf) {
#pragma unroll
        for (int k = 0; k < R; ++k)
            if (goff[k] >= 0) stage[buf * C * row + soff[k]] = pre[k];
    };

    const float NEG_INF = -__builtin_inff();
    const bool owns = lane < C;
    float a[CMAX];
#pragma unroll
    for (int cp = 0; cp < CMAX; ++cp) a[cp] = (owns && cp < C) ? A[cp * C + lane] : NEG_INF;
    const float pi_c = (owns && pi) ? pi[lane] : 0.0f;
    const int my_row = (owns ? lane : 0) * row + w;

    float d = NEG_INF;
    unsigned pack = 0u;
    const int n_chunks = (L + LC_CHUNK - 1) / LC_CHUNK;
    fetch(0);
    for (int ch = 0; ch < n_chunks; ++ch) {
        const int buf = ch & 1, t0 = ch * LC_CHUNK;
        commit(buf);          // buffer `buf` was last read in chunk ch - 2, which every wave left before the barrier of ch - 1
        __syncthreads();
        if (ch + 1 < n_chunks) fetch(t0 + LC_CHUNK);   // in flight while this chunk is consumed
        if (!decodes) continue;
        const float* mine = stage + buf * C * row + my_row;
        const int n_here = L - t0 < LC_CHUNK ? L - t0 : LC_CHUNK;
        float x = mine[0];
        for (int tt = 0; tt < n_here; ++tt) {
            const int t = t0 + tt;
            const float x_next = tt + 1 < n_here ? mine[(tt + 1) * EW] : 0.0f;   // read ahead of the step that needs it
            if (t == 0) {
                d = x + pi_c;
            } else {
                float m;
                int arg;
                lc_best_predecessor<CMAX>(d, a, m, arg);      // label_chain.h
                d = m + x;
                pack |= (unsigned)arg << (8 * (t & 3));
            }
            if (!owns) d = NEG_INF;
            if ((t & 3) == 3 || t == L - 1) {
                if (owns) bpw[(int64_t)(t >> 2) * C + lane] = pack;
                pack = 0u;
            }
            x = x_next;
        }
    }
    if (!decodes) return;

    // y[L-1] = the smallest c attaining max d[L-1][.]: a scalar run over the lanes, strict comparison (lc_best_class of
    // label_chain.h is this run; called here it reorders the kernel's code, so the measured form stays written out)
    float top = lane_value(d, 0);
    int y = 0;
#pragma unroll
    for (int cp = 1; cp < CMAX; ++cp) {
        const float v = lane_value(d, cp);
        if (v > top) { top = v; y = cp; }
    }
    if (lane == 0) score[(int64_t)b * E + e] = top;

    // backtrace, four blocks of four steps per trip: the words of a trip are loaded together (their addresses do not depend
    // on the path), lane c reading the word it wrote; the path then moves by v_readlane. Labels are written as the steps are
    // resolved: out[t'] = y[min(t' / ds, L - 1)], the block that holds step L - 1 also writes everything behind it.
    long long* out = labels + (int64_t)b * T_out * E + e;
    for (int q_hi = (L - 1) >> 2; q_hi >= 0; q_hi -= 4) {
        unsigned W[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) W[j] = (owns && q_hi - j >= 0) ? bpw[(int64_t)(q_hi - j) * C + lane] : 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int q = q_hi - j;
            if (q < 0) break;
            int ys[4];
#pragma unroll
            for (int k = 3; k >= 0; --k) {
                const int t = 4 * q + k;
                ys[k] = y;
                if (t <= L - 1 && t >= 1) {
                    const unsigned word = (unsigned)__builtin_amdgcn_readlane((int)W[j], __builtin_amdgcn_readfirstlane(y));
                    y = (int)((word >> (8 * k)) & 0xffu);
                    y = y < C ? y : C - 1;            // cannot happen: every byte written is below C
                }
            }
            const int64_t lo = (int64_t)4 * q * ds;
            const int64_t hi_steps = 4 * q + 3 >= L - 1 ? (int64_t)T_out : (int64_t)(4 * q + 4) * ds;
            const int64_t hi = hi_steps < T_out ? hi_steps : T_out;
            for (int64_t tp = lo + lane; tp < hi; tp += 64) {
                int t = (int)(tp / ds);
                t = t < L - 1 ? t : L - 1;
                const int k = t - 4 * q;
                out[tp * E] = k == 0 ? ys[0] : (k == 1 ? ys[1] : (k == 2 ? ys[2] : ys[3]));
            }
        }
    }
}

// Transition counts of a label tensor at the model's rate: pair (b, k, e) is targets[b][k * stride][e] ->
// targets[b][(k + 1) * stride][e]. A private 32-bit histogram per workgroup in LDS (a workgroup sees far fewer than 2^32
// pairs), flushed with one integer atomic per non-empty cell: the totals do not depend on the order.
constexpr int TRANS_GRID_CAP = 1024;

__global__ __launch_bounds__(256) void transition_counts_kernel(const long long* __restrict__ targets, int n_pairs,
                                                                int64_t n, int T_tgt, int E, int C, int stride,
                                                                long long ignore, long long* counts) {
    extern __shared__ unsigned hist[];
    for (int k = threadIdx.x; k < C * C; k += 256) hist[k] = 0u;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int e = (int)(i % E);
        const int64_t bk = i / E;
        const int k = (int)(bk % n_pairs);
        const int64_t b = bk / n_pairs;
        const long long from = targets[(b * T_tgt + (int64_t)k * stride) * E + e];
        const long long to = targets[(b * T_tgt + (int64_t)(k + 1) * stride) * E + e];
        if (twog_label_kept(from, ignore, C) && twog_label_kept(to, ignore, C))
            atomicAdd(&hist[(int)from * C + (int)to], 1u);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < C * C; k += 256) {
        const unsigned v = hist[k];
        if (v != 0u) atomicAdd(reinterpret_cast<unsigned long long*>(counts + k), (unsigned long long)v);
    }
}

}  // namespace

extern "C" int twog_viterbi_limits(int* max_classes, int* max_steps) {
    if (max_classes) *max_classes = LC_MAX_CLASSES;
    if (max_steps) *max_steps = LC_MAX_STEPS;
    return 0;
}

extern "C" int twog_viterbi_workspace(int bs, int n_classes, int T, int E, size_t* bytes) {
    if (!lc_shape_ok(bs, n_classes, T, E)) return -1;
    if (!lc_within_limits(n_classes, T)) return -2;
    const VitPlan p = vit_plan(bs, n_classes, T, E);
    if (bytes) *bytes = p.ws_bytes;
    return p.route;
}

extern "C" int twog_viterbi_decode(const float* logp, int bs, int n_classes, int T, int E, const float* A, const float* pi,
                                   const int64_t* lengths, int downsampling, int T_out, int64_t* labels, float* score,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    if (!lc_shape_ok(bs, n_classes, T, E) || downsampling < 1 || T_out < 0) return -1;
    if (!lc_launchable(bs, n_classes, T, E)) return -2;
    if (bs == 0) return 0;
    const VitPlan p = vit_plan(bs, n_classes, T, E);
    if (p.route == TWOG_VITERBI_ROUTE_WORKSPACE && (workspace == nullptr || workspace_bytes < p.ws_bytes)) return -3;
    return lc_dispatch_classes(n_classes, [&](auto cmax) {
        return lc_launch<viterbi_kernel<decltype(cmax)::value>>(
            p.g, bs, p.lds_bytes, stream, logp, n_classes, T, E, A, pi, reinterpret_cast<const long long*>(lengths), downsampling,
            T_out, reinterpret_cast<long long*>(labels), score, reinterpret_cast<unsigned*>(workspace), (long long)p.seq_words,
            p.g.waves, p.route == TWOG_VITERBI_ROUTE_LDS ? 1 : 0);
    });
}

extern "C" int twog_transition_counts(const int64_t* targets, int bs, int T_tgt, int E, int n_classes, int stride,
                                      int64_t ignore_index, int64_t* counts, void* stream) {
    if (bs < 0 || T_tgt < 0 || E < 1 || n_classes < 1 || stride < 1) return -1;
    if (n_classes > LC_MAX_CLASSES) return -2;
    const int n_pairs = T_tgt > 0 ? (T_tgt - 1) / stride : 0;
    const int64_t n = (int64_t)bs * n_pairs * E;
    if (n == 0) return 0;
    const int grid = (int)((n + 255) / 256 < TRANS_GRID_CAP ? (n + 255) / 256 : TRANS_GRID_CAP);
    hipLaunchKernelGGL(transition_counts_kernel, dim3(grid), dim3(256), (size_t)n_classes * n_classes * sizeof(unsigned),
                       (hipStream_t)stream, reinterpret_cast<const long long*>(targets), n_pairs, n, T_tgt, E, n_classes,
                       stride, (long long)ignore_index, reinterpret_cast<long long*>(counts));
    TWOG_CHECK_LAUNCH();
    return 0;
}
