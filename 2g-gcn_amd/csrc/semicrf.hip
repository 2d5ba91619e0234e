// Semi-Markov CRF loss: the sequence negative log-likelihood over whole segments with learned duration scores, forward and
// backward. It is the sum-product twin of segdecode.hip; the reference project has no such term, the
// definition is the numpy specification tests/semicrf_ref.py, restated at twog_semicrf_nll_fwd in include/twog_gcn.h.
//
// The recursion kernels have the shape of label_chain.h (one wave per sequence, lane c owns class c, the slab staged in
// chunks, the labels of a chunk one per lane as in crf.hip). Removed steps drop out, so everything below counts kept steps k.
//   forward : e_k is the CRF forward's logsumexp over the other lanes' d_{k-1} (column A[:, c] in registers); d_k walks the
//             segment lengths on segdecode.hip's ring of the last Dr = min(D, T) kept steps of (e, x) in LDS, twice: once for
//             the maximum, once for the sum. (e, d) of every kept step go to the workspace, and one mark per step says where
//             the gold segmentation starts a piece.
//   backward: the kept steps descend on a ring of (bd, x): be_k walks the same lengths forward in time, which on a ring
//             filled in descending order is the same walk. The second pass of the walk also adds the segment marginals
//             mu(k, l, c) to the wave's ddur sums, which sit in LDS in the lane's own column. Lane c' holds the row A[c', :]
//             and its dA sums in registers, as crf_bwd_kernel does. The coverage sum of d input is the recurrence
//             cov_k = cov_{k+1} + End_k - Start_{k+1}; d input leaves through LDS in the slab's layout, zeros at removed steps.
// Every logsumexp subtracts its maximum, or 0 when that maximum is -inf: all-(-inf) terms give -inf and never NaN, and a
// -inf entry of A, pi or dur gets exp(-inf) = 0 as its gradient. No floating-point atomics: second-stage kernels sum the
// per-sequence values in index order in fp64.
#include "twog_common.h"
#include "label_chain.h"

namespace {

constexpr int SCRF_BLOCK = 8;         // segment lengths whose ring and dur reads are in flight together (SEG_BLOCK of segdecode.hip)
// Backward, beyond 32 classes: one wave per SIMD, so that a lane's two rows of 64 values stay in registers (crf.hip).
constexpr int SCRF_BWD_WAVES_WIDE = 4;
__host__ __device__ constexpr int scrf_bwd_max_waves(int classes) { return classes > 32 ? SCRF_BWD_WAVES_WIDE : LC_MAX_WAVES; }

inline size_t scrf_fwd_lds(int C, int Dr, int waves) {      // rings of (e, x), dur, staging in
    return (size_t)waves * Dr * C * sizeof(float2) + (size_t)Dr * C * sizeof(float) + 2 * (size_t)C * lc_row(waves) * sizeof(float);
}
inline size_t scrf_bwd_lds(int C, int Dr, int waves) {      // rings of (bd, x) and the ddur sums, dur, staging in and out
    return (size_t)waves * Dr * C * (sizeof(float2) + sizeof(float)) + (size_t)Dr * C * sizeof(float) +
           4 * (size_t)C * lc_row(waves) * sizeof(float);
}
static_assert((size_t)TWOG_SEGDEC_MAX_DURATION * LC_MAX_CLASSES * (sizeof(float2) + 2 * sizeof(float)) +
                      4 * (size_t)LC_MAX_CLASSES * (LC_CHUNK + 1) * sizeof(float) <= LC_LDS_LIMIT,
              "one backward wave at the largest C and D fits the LDS budget");

struct ScrfPlan {
    int cmax, Dr;
    LcGeometry gf, gb;                // forward, backward
    size_t lds_f, lds_b;
    size_t ed_bytes, marks_bytes, seq_bytes, partial_bytes;
    int64_t partial_words;            // per sequence
};

// The one statement of the launches and the workspaces: twog_semicrf_plan reports it, the launchers use it. The waves of a
// workgroup are as many entities as the LDS budget holds rings for; fewer of them only means more workgroups.
inline ScrfPlan scrf_plan(int bs, int C, int T, int E, int D) {
    ScrfPlan p;
    p.cmax = lc_dispatch_classes(C, [](auto cmax) { return (int)decltype(cmax)::value; });
    p.Dr = D < T ? D : T;
    int wf = E < LC_MAX_WAVES ? E : LC_MAX_WAVES;
    while (wf > 1 && scrf_fwd_lds(C, p.Dr, wf) > LC_LDS_LIMIT) --wf;
    int wb = E < scrf_bwd_max_waves(C) ? E : scrf_bwd_max_waves(C);
    while (wb > 1 && scrf_bwd_lds(C, p.Dr, wb) > LC_LDS_LIMIT) --wb;
    p.gf = lc_geometry(C, E, wf);
    p.gb = lc_geometry(C, E, wb);
    p.lds_f = scrf_fwd_lds(C, p.Dr, wf);
    p.lds_b = scrf_bwd_lds(C, p.Dr, wb);
    const size_t n_seq = (size_t)bs * E;
    p.ed_bytes = n_seq * T * C * sizeof(float2);
    p.marks_bytes = n_seq * T * sizeof(int32_t);
    p.seq_bytes = n_seq * LC_SEQ_WORDS * sizeof(float);
    p.partial_words = (int64_t)C * (C + 1 + p.Dr);
    p.partial_bytes = n_seq * p.partial_words * sizeof(float);
    return p;
}

// The lengths l = 1 .. n of the lane's column, ascending: f(l, cand_l) with acc_l = acc_(l-1) + x of the entry l - 1 steps
// back (acc_0 = 0) and cand_l = (first member of that entry + dur[l-1]) + acc_l. l = 1 is (head, x) from registers, the
// others come from the ring, walking back from `slot`. As in segdecode.hip the walk is cut where the ring wraps, and each
// piece into blocks of SCRF_BLOCK lengths whose reads are all issued before the first is used.
template <class F>
__device__ __forceinline__ void scrf_walk(const float2* ring, const float* dur_s, int C, int col, int Dr, int slot, int n,
                                          float head, float x, F&& f) {
    float acc = 0.0f + x;
    f(1, (head + dur_s[col]) + acc);
    int s = __builtin_amdgcn_readfirstlane(slot);
    int l = 2;
    while (l <= n) {
        if (s == 0) s = Dr;
        const int run = n - l + 1 < s ? n - l + 1 : s;     // lengths l .. l + run - 1 sit at s - 1, s - 2, .. s - run
        const float2* rp = ring + (s - 1) * C + col;
        const float* dp = dur_s + (l - 1) * C + col;
        auto block = [&](int k, int cnt, auto whole) {
            float2 v[SCRF_BLOCK];
            float du[SCRF_BLOCK];
#pragma unroll
            for (int j = 0; j < SCRF_BLOCK; ++j) {
                const int kj = k + ((decltype(whole)::value || j < cnt) ? j : 0);
                v[j] = rp[-kj * C];
                du[j] = dp[kj * C];
            }
#pragma unroll
            for (int j = 0; j < SCRF_BLOCK; ++j) {
                if (decltype(whole)::value || j < cnt) {
                    acc = acc + v[j].y;
                    f(l + k + j, (v[j].x + du[j]) + acc);
                }
            }
        };
        int k = 0;
        for (; k + SCRF_BLOCK <= run; k += SCRF_BLOCK) block(k, SCRF_BLOCK, std::true_type{});
        if (k < run) block(k, run - k, std::false_type{});
        s -= run;
        l += run;
    }
}

// what a logsumexp subtracts: its maximum, 0 when every term is -inf
__device__ __forceinline__ float scrf_shift(float m) { return m == -__builtin_inff() ? 0.0f : m; }

// grid (groups, bs), 64 * EW threads: wave w runs entity blockIdx.x * EW + w of clip blockIdx.y.
// LDS: ring[EW][Dr][C] float2 (e, x), dur_s[Dr][C], stage[2][C][lc_row(EW)] floats.
// ed [bs * E][T][C] float2: (e, d) of kept step k at [k]. marks [bs * E][T]: 1 where a gold piece starts, by step t.
template <int CMAX>
__global__ __launch_bounds__(64 * LC_MAX_WAVES) void scrf_fwd_kernel(
    const float* __restrict__ logp, int C, int T, int E, const float* __restrict__ A, const float* __restrict__ pi,
    const float* __restrict__ dur, int D, int Dr, const long long* __restrict__ target, long long ignore,
    float2* __restrict__ ed_ws, int* __restrict__ marks_ws, float* __restrict__ seq, int EW) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int R = CMAX / 4;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nthreads = 64 * EW;
    const int b = blockIdx.y, e0 = blockIdx.x * EW, e = e0 + w;
    const bool runs = e < E;                          // wave-uniform; a wave without an entity still stages
    const int row = lc_row(EW);
    const int buf_floats = C * row;
    float2* ring = reinterpret_cast<float2*>(smem) + (size_t)w * Dr * C;
    float* dur_s = smem + (size_t)2 * EW * Dr * C;
    float* stage = dur_s + (size_t)Dr * C;

    for (int idx = tid; idx < C * Dr; idx += nthreads) {          // dur[c][l-1] -> dur_s[l-1][c]; visible after the first barrier
        const int c = idx / Dr, l = idx - c * Dr;
        dur_s[l * C + c] = dur[(int64_t)c * D + l];
    }

    LcStager S;
    S.init(tid, C, T, E, EW, e0);
    const float* base = logp + (int64_t)b * C * T * E + e0;
    float pre[R];
    const long long* labels = target + (int64_t)b * T * E + (runs ? e : 0);
    auto fetch_label = [&](int t0) {
        return (runs && lane < LC_CHUNK && t0 + lane < T) ? lc_chain_label(labels[(int64_t)(t0 + lane) * E], ignore, C) : -1;
    };

    const float NEG_INF = -__builtin_inff();
    const bool owns = lane < C;
    const int col = owns ? lane : 0;                  // a lane without a class reads column 0 and writes nothing
    float a[CMAX];
#pragma unroll
    for (int cp = 0; cp < CMAX; ++cp) a[cp] = cp < C ? A[cp * C + col] : NEG_INF;
    const float pi_c = pi[col];
    const int my_row = col * row + w;
    const int64_t s_idx = (int64_t)b * E + (runs ? e : 0);
    float2* ed_out = ed_ws + s_idx * T * C;
    int* marks_out = marks_ws + s_idx * T;

    float d = NEG_INF, gold = 0.0f;
    int K = 0, y_prev = 0, pos = 0, slot = 0;         // pos: steps of the open gold piece; slot = K mod Dr
    const int n_chunks = (T + LC_CHUNK - 1) / LC_CHUNK;
    S.fetch<R>(base, 0, T, pre);
    int lab_pre = fetch_label(0);
    for (int ch = 0; ch < n_chunks; ++ch) {
        const int buf = ch & 1, t0 = ch * LC_CHUNK;
        S.commit<R>(stage + buf * buf_floats, pre);   // buffer `buf` was last read in chunk ch - 2, which every wave left before the barrier of ch - 1
        __syncthreads();
        const int lab = lab_pre;
        if (ch + 1 < n_chunks) {                          // in flight while this chunk is consumed
            S.fetch<R>(base, t0 + LC_CHUNK, T, pre);
            lab_pre = fetch_label(t0 + LC_CHUNK);
        }
        if (!runs) continue;
        const float* mine = stage + buf * buf_floats + my_row;
        const int n_here = T - t0 < LC_CHUNK ? T - t0 : LC_CHUNK;
        int mark = 0;
        for (int tt = 0; tt < n_here; ++tt) {
            const int y = __builtin_amdgcn_readlane(lab, tt);
            if (y < 0) continue;                          // a removed step: not part of the chain
            const float x = mine[tt * EW];
            const float x_y = lane_value(x, y);
            // the gold segmentation: a piece starts at the first step, at a change of label and after D steps of one label
            const bool starts = K == 0 || y != y_prev || pos == D;
            if (starts) {
                if (K > 0) gold = (gold + dur_s[(pos - 1) * C + y_prev]) + A[y_prev * C + y];
                else gold = gold + pi[y];
                pos = 0;
            }
            ++pos;
            gold = gold + x_y;
            if (lane == tt) mark = starts ? 1 : 0;

            float ev = pi_c;
            if (K > 0) {
                float m = NEG_INF;
#pragma unroll
                for (int cp = 0; cp < CMAX; ++cp) m = fmaxf(m, lane_value(d, cp) + a[cp]);
                m = scrf_shift(m);
                float s = 0.0f;
#pragma unroll
                for (int cp = 0; cp < CMAX; ++cp) s += expf((lane_value(d, cp) + a[cp]) - m);
                ev = m + logf(s);
            }
            if (owns) ring[slot * C + lane] = make_float2(ev, x);
            const int n = K + 1 < Dr ? K + 1 : Dr;
            float m = NEG_INF;
            scrf_walk(ring, dur_s, C, col, Dr, slot, n, ev, x, [&](int, float cand) { m = fmaxf(m, cand); });
            m = scrf_shift(m);
            float s = 0.0f;
            scrf_walk(ring, dur_s, C, col, Dr, slot, n, ev, x, [&](int, float cand) { s += expf(cand - m); });
            const float dv = m + logf(s);
            d = owns ? dv : NEG_INF;
            if (owns) ed_out[(int64_t)K * C + lane] = make_float2(ev, dv);
            slot = slot + 1 == Dr ? 0 : slot + 1;
            y_prev = y;
            ++K;
        }
        if (lane < n_here) marks_out[t0 + lane] = mark;
    }
    if (!runs) return;
    float logZ = 0.0f;
    if (K > 0) {
        gold = gold + dur_s[(pos - 1) * C + y_prev];
        const float m = scrf_shift(wave_max(d));
        const float s = wave_sum(owns ? expf(d - m) : 0.0f);
        logZ = m + logf(s);
    }
    if (lane == 0) {
        float* o = seq + s_idx * LC_SEQ_WORDS;
        o[0] = logZ;
        o[1] = gold;
        o[2] = logZ - gold;
        o[3] = __int_as_float(K);
    }
}

// Same geometry with the backward's waves, the kept steps walked from the last to the first.
// LDS: ring[EW][Dr][C] float2 (bd, x), dur_s[Dr][C], sums[EW][Dr][C] (the wave's ddur sums, row l - 1), stage[2][C][row],
// out[2][C][row] floats.
// partials (NULL: the parameters need no gradient) [bs * E][C + 1 + Dr][C]: rows 0 .. C-1 = the expected joins minus the
// gold ones, row C = Start_0 - indicator, rows C + 1 .. = the expected pieces of length l minus the gold ones (row l - 1,
// column c), all before the factor g.
template <int CMAX>
__global__ __launch_bounds__(64 * scrf_bwd_max_waves(CMAX)) void scrf_bwd_kernel(
    const float* __restrict__ logp, int C, int T, int E, const float* __restrict__ A, const float* __restrict__ dur, int D,
    int Dr, const long long* __restrict__ target, long long ignore, const float2* __restrict__ ed_ws,
    const int* __restrict__ marks_ws, const float* __restrict__ seq, const double* __restrict__ stats,
    const float* __restrict__ dloss, float weight, float* __restrict__ dinput, int accumulate, float* __restrict__ partials,
    int EW) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int R = CMAX / 4;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nthreads = 64 * EW;
    const int b = blockIdx.y, e0 = blockIdx.x * EW, e = e0 + w;
    const bool runs = e < E;
    const int row = lc_row(EW);
    const int buf_floats = C * row;
    float2* ring = reinterpret_cast<float2*>(smem) + (size_t)w * Dr * C;
    float* dur_s = smem + (size_t)2 * EW * Dr * C;
    float* sums = dur_s + (size_t)Dr * C + (size_t)w * Dr * C;
    float* stage = dur_s + (size_t)(EW + 1) * Dr * C;
    float* out = stage + 2 * buf_floats;

    for (int idx = tid; idx < C * Dr; idx += nthreads) {
        const int c = idx / Dr, l = idx - c * Dr;
        dur_s[l * C + c] = dur[(int64_t)c * D + l];
    }

    const double cnt = stats[1];
    const float g = cnt > 0.0 ? weight * dloss[0] / (float)cnt : 0.0f;

    LcStager S;
    S.init(tid, C, T, E, EW, e0);
    const float* base = logp + (int64_t)b * C * T * E + e0;
    float* dbase = dinput ? dinput + (int64_t)b * C * T * E + e0 : nullptr;
    float pre[R];
    auto flush = [&](int buf, int t0) {                   // the d input of a finished chunk, in the layout it was fetched in
#pragma unroll
        for (int k = 0; k < R; ++k) {
            if (!S.has(k) || t0 + S.tt >= T) continue;
            float* dst = dbase + (int64_t)t0 * E + S.goff(k);
            const float v = out[buf * buf_floats + S.soff(k)];
            *dst = accumulate ? *dst + v : v;
        }
    };
    const int64_t s_idx = (int64_t)b * E + (runs ? e : 0);
    const long long* labels = target + (int64_t)b * T * E + (runs ? e : 0);
    const int* marks = marks_ws + s_idx * T;
    auto fetch_label = [&](int t0) {
        return (runs && lane < LC_CHUNK && t0 + lane < T) ? lc_chain_label(labels[(int64_t)(t0 + lane) * E], ignore, C) : -1;
    };
    auto fetch_mark = [&](int t0) { return (runs && lane < LC_CHUNK && t0 + lane < T) ? marks[t0 + lane] : 0; };

    const float NEG_INF = -__builtin_inff();
    const bool owns = lane < C;
    const int col = owns ? lane : 0;
    const bool sums_wanted = partials != nullptr && owns;
    // row A[c', :]; a lane without a class takes row 0 (finite sums, dropped), a column without a class is 0 under be = -inf
    float ar[CMAX], acc[CMAX];
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
        ar[c] = c < C ? A[col * C + c] : 0.0f;
        acc[c] = 0.0f;
    }
    if (owns)
        for (int l = 0; l < Dr; ++l) sums[l * C + lane] = 0.0f;   // the lane's own column: no barrier
    const int my_row = col * row + w;
    const float2* ed_in = ed_ws + s_idx * T * C + col;
    const float logZ = seq[s_idx * LC_SEQ_WORDS];
    const int K_seq = __builtin_amdgcn_readfirstlane(__float_as_int(seq[s_idx * LC_SEQ_WORDS + 3]));
    const int K = K_seq < T ? K_seq : T;                  // whatever the word holds, no index leaves the workspace

    int kk = runs ? K - 1 : -1;                           // the kept step the walk visits next
    float be_next = NEG_INF, start_next = 0.0f, cov = 0.0f, first_d = 0.0f;
    int y_next = -1;                                      // the label of step kk + 1, -1: nothing visited yet
    int piece = 0, slot = 0;                              // steps of the open gold piece (from its end); slot = visited mod Dr
    bool joined = false;                                  // step kk + 1 starts a gold piece
    const int n_chunks = (T + LC_CHUNK - 1) / LC_CHUNK;
    S.fetch<R>(base, (n_chunks - 1) * LC_CHUNK, T, pre);
    int lab_pre = fetch_label((n_chunks - 1) * LC_CHUNK), mark_pre = fetch_mark((n_chunks - 1) * LC_CHUNK);
    float2 ed_pre = kk >= 0 ? ed_in[(int64_t)kk * C] : make_float2(0.0f, 0.0f);   // one kept step ahead of its use
    for (int it = 0; it < n_chunks; ++it) {
        const int buf = it & 1, t0 = (n_chunks - 1 - it) * LC_CHUNK;
        S.commit<R>(stage + buf * buf_floats, pre);
        __syncthreads();      // stage[buf] is whole, and every wave has left the chunk before: out[buf ^ 1] is whole
        if (dinput && it > 0) flush(buf ^ 1, t0 + LC_CHUNK);
        const int lab = lab_pre, mk = mark_pre;
        if (it + 1 < n_chunks) {
            S.fetch<R>(base, t0 - LC_CHUNK, T, pre);
            lab_pre = fetch_label(t0 - LC_CHUNK);
            mark_pre = fetch_mark(t0 - LC_CHUNK);
        }
        if (!runs) continue;
        const float* mine = stage + buf * buf_floats + my_row;
        float* mine_out = out + buf * buf_floats + my_row;
        const int n_here = T - t0 < LC_CHUNK ? T - t0 : LC_CHUNK;
        for (int tt = n_here - 1; tt >= 0; --tt) {
            const int y = __builtin_amdgcn_readlane(lab, tt);
            float dval = 0.0f;
            if (y >= 0 && kk >= 0) {
                const bool starts = __builtin_amdgcn_readlane(mk, tt) != 0;
                const float e_k = ed_pre.x, d_k = owns ? ed_pre.y : NEG_INF;
                if (kk > 0) ed_pre = ed_in[(int64_t)(kk - 1) * C];
                const float x = mine[tt * EW];
                const float ind = lane == y ? 1.0f : 0.0f;
                // bd_k from be_{k+1} of the other lanes, and the joins k -> k + 1 into the lane's row of dA
                float bd = 0.0f;
                if (y_next >= 0) {
                    float m = NEG_INF;
#pragma unroll
                    for (int c = 0; c < CMAX; ++c) m = fmaxf(m, ar[c] + lane_value(be_next, c));
                    m = scrf_shift(m);
                    const float scale = expf((d_k + m) - logZ);
                    const float gold_join = joined ? ind : 0.0f;
                    float s = 0.0f;
#pragma unroll
                    for (int c = 0; c < CMAX; ++c) {
                        const float ex = expf((ar[c] + lane_value(be_next, c)) - m);
                        s += ex;
                        acc[c] += ex * scale - (c == y_next ? gold_join : 0.0f);
                    }
                    bd = m + logf(s);
                }
                if (owns) ring[slot * C + lane] = make_float2(bd, x);
                // be_k over the lengths, and mu(k, l, c) into the ddur sums
                const int visited = K - kk;
                const int n = visited < Dr ? visited : Dr;
                float m = NEG_INF;
                scrf_walk(ring, dur_s, C, col, Dr, slot, n, bd, x, [&](int, float cand) { m = fmaxf(m, cand); });
                m = scrf_shift(m);
                const float scale = expf((e_k + m) - logZ);
                float s = 0.0f;
                scrf_walk(ring, dur_s, C, col, Dr, slot, n, bd, x, [&](int l, float cand) {
                    const float ex = expf(cand - m);
                    s += ex;
                    if (sums_wanted) sums[(l - 1) * C + lane] += ex * scale;
                });
                const float be = m + logf(s);
                ++piece;
                if (starts) {
                    if (sums_wanted && lane == y && piece <= Dr) sums[(piece - 1) * C + lane] -= 1.0f;
                    piece = 0;
                }
                joined = starts;
                const float start_k = expf((e_k + be) - logZ), end_k = expf((d_k + bd) - logZ);
                cov = (cov + end_k) - start_next;
                start_next = start_k;
                first_d = start_k - ind;
                dval = g * (cov - ind);
                be_next = owns ? be : NEG_INF;
                y_next = y;
                slot = slot + 1 == Dr ? 0 : slot + 1;
                --kk;
            }
            if (dinput && owns) mine_out[tt * EW] = dval;
        }
    }
    if (dinput) {
        __syncthreads();
        flush((n_chunks - 1) & 1, 0);
    }
    if (!runs || !partials || !owns) return;
    float* p = partials + s_idx * ((int64_t)C * (C + 1 + Dr));
#pragma unroll
    for (int c = 0; c < CMAX; ++c)
        if (c < C) p[lane * C + c] = acc[c];
    p[C * C + lane] = first_d;
    for (int l = 0; l < Dr; ++l) p[(C + 1 + l) * C + lane] = sums[l * C + lane];
}

// Element j of (dA, dpi, ddur) summed over the sequences in index order in fp64, times g, rounded once. A duration beyond
// Dr = min(D, T) cannot occur: its gradient is 0.
__global__ __launch_bounds__(256) void scrf_param_kernel(const float* __restrict__ partials, int64_t n_seq, int C, int D, int Dr,
                                                          const double* __restrict__ stats, const float* __restrict__ dloss,
                                                          float weight, float* dA, float* dpi, float* ddur, int accumulate) {
    const int j = blockIdx.x * 256 + threadIdx.x, n_chain = (C + 1) * C, n = n_chain + C * D;
    if (j >= n) return;
    const double cnt = stats[1];
    const float g = cnt > 0.0 ? weight * dloss[0] / (float)cnt : 0.0f;
    const int64_t words = (int64_t)C * (C + 1 + Dr);
    int src = j;                                           // where element j sits in a sequence's partials, -1: nowhere
    if (j >= n_chain) {
        const int c = (j - n_chain) / D, l = (j - n_chain) - c * D;
        src = l < Dr ? n_chain + l * C + c : -1;
    }
    double sum = 0.0;
    if (src >= 0)
        for (int64_t s = 0; s < n_seq; ++s) sum += (double)partials[s * words + src];
    const float v = (float)((double)g * sum);
    float* dst = j < C * C ? dA + j : (j < n_chain ? dpi + (j - C * C) : ddur + (j - n_chain));
    *dst = accumulate ? *dst + v : v;
}

inline bool scrf_duration_ok(int D) { return D <= TWOG_SEGDEC_MAX_DURATION; }

}  // namespace

extern "C" int twog_semicrf_limits(int* max_classes, int* max_steps, int* max_duration) {
    return twog_segdecode_limits(max_classes, max_steps, max_duration);
}

extern "C" int twog_semicrf_plan(int bs, int n_classes, int T, int E, int D, int32_t* out, size_t* bytes) {
    if (!lc_shape_ok(bs, n_classes, T, E) || D < 1) return -1;
    if (!lc_launchable(bs, n_classes, T, E) || !scrf_duration_ok(D)) return -2;
    const ScrfPlan p = scrf_plan(bs, n_classes, T, E, D);
    if (out) {
        out[0] = p.cmax;
        out[1] = p.gf.waves;
        out[2] = p.gf.groups;
        out[3] = p.gb.waves;
        out[4] = p.gb.groups;
    }
    if (bytes) {
        bytes[0] = p.ed_bytes;
        bytes[1] = p.marks_bytes;
        bytes[2] = p.seq_bytes;
        bytes[3] = p.partial_bytes;
    }
    return 0;
}

extern "C" int twog_semicrf_nll_fwd(const float* input, const int64_t* target, int bs, int n_classes, int T, int E,
                                    const float* A, const float* pi, const float* dur, int D, int64_t ignore_index,
                                    float weight, float* ed, int32_t* marks, float* seq, double* stats, float* loss,
                                    void* stream) {
    const int C = n_classes;
    if (!lc_shape_ok(bs, C, T, E) || D < 1) return -1;
    if (!lc_launchable(bs, C, T, E) || !scrf_duration_ok(D)) return -2;
    if (!A || !pi || !dur || !stats || !loss || (bs > 0 && (!input || !target || !ed || !marks || !seq))) return -3;
    if (bs > 0) {
        const ScrfPlan p = scrf_plan(bs, C, T, E, D);
        const int rc = lc_dispatch_classes(C, [&](auto cmax) {
            return lc_launch<scrf_fwd_kernel<decltype(cmax)::value>>(
                p.gf, bs, p.lds_f, stream, input, C, T, E, A, pi, dur, D, p.Dr, reinterpret_cast<const long long*>(target),
                (long long)ignore_index, reinterpret_cast<float2*>(ed), reinterpret_cast<int*>(marks), seq, p.gf.waves);
        });
        if (rc) return rc;
    }
    hipLaunchKernelGGL(lc_nll_final_kernel, dim3(1), dim3(LC_FINAL_THREADS), 0, (hipStream_t)stream, seq, (int64_t)bs * E,
                       weight, stats, loss);
    TWOG_CHECK_LAUNCH();
    return 0;
}

extern "C" int twog_semicrf_nll_bwd(const float* input, const int64_t* target, int bs, int n_classes, int T, int E,
                                    const float* A, const float* dur, int D, int64_t ignore_index, float weight,
                                    const float* ed, const int32_t* marks, const float* seq, const double* stats,
                                    const float* dloss, float* dinput, int accumulate, float* partials, float* dA, float* dpi,
                                    float* ddur, int accumulate_params, void* stream) {
    const int C = n_classes;
    if (!lc_shape_ok(bs, C, T, E) || D < 1) return -1;
    if (!lc_launchable(bs, C, T, E) || !scrf_duration_ok(D)) return -2;
    if (!A || !dur || !stats || !dloss || (bs > 0 && (!input || !target || !ed || !marks || !seq))) return -3;
    if ((dA == nullptr) != (dpi == nullptr) || (dA == nullptr) != (ddur == nullptr) || (dA && bs > 0 && !partials)) return -3;
    if (!dinput && !dA) return 0;
    const ScrfPlan p = scrf_plan(bs, C, T, E, D);
    if (bs > 0) {
        float* part = dA ? partials : nullptr;
        const int rc = lc_dispatch_classes(C, [&](auto cmax) {
            return lc_launch<scrf_bwd_kernel<decltype(cmax)::value>>(
                p.gb, bs, p.lds_b, stream, input, C, T, E, A, dur, D, p.Dr, reinterpret_cast<const long long*>(target),
                (long long)ignore_index, reinterpret_cast<const float2*>(ed), reinterpret_cast<const int*>(marks), seq, stats,
                dloss, weight, dinput, accumulate, part, p.gb.waves);
        });
        if (rc) return rc;
    }
    if (dA) {
        const int n = (C + 1) * C + C * D;
        hipLaunchKernelGGL(scrf_param_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, partials,
                           (int64_t)bs * E, C, D, p.Dr, stats, dloss, weight, dA, dpi, ddur, accumulate_params);
        TWOG_CHECK_LAUNCH();
    }
    return 0;
}
