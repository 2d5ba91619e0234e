// Linear-chain CRF loss: the sequence negative log-likelihood of the frame labels under learned transition scores, forward
// and backward. The reference project has no such term; the definition is the numpy specification
// tests/crf_ref.py, restated at twog_crf_nll_fwd in include/twog_gcn.h.
//
// The recursion kernels have the shape of label_chain.h (one wave per sequence, lane c owns class c, the slab staged in
// chunks). The labels of a chunk are fetched the same way, one per lane, so a step reads its label from a register and the
// kept / removed decision is wave-uniform.
//   forward : lane c holds the column A[:, c]; alpha of the previous kept step comes from the other lanes by v_readlane.
//   backward: lane c' holds the row A[c', :] and its row of sum_k (xi_k - indicator) in registers; u = x + beta of the next
//             kept step comes from the other lanes by v_readlane. d input goes through a second pair of LDS buffers and
//             leaves in the layout the slab was fetched in, so a removed step costs one zero per class and nothing is
//             cleared beforehand.
// Every logsumexp is taken in the log domain with the maximum subtracted (expf / logf of the device library, not the
// fast forms): finite A and pi of any size are in contract, nothing can underflow as a whole.
// No floating-point atomics: the sums over sequences are made by second-stage kernels in index order in fp64.
#include "twog_common.h"
#include "label_chain.h"

namespace {

// Entities of one clip per workgroup: LC_MAX_WAVES, and beyond 32 classes one wave per SIMD, so that a lane's two rows of 64
// values (backward: A[c', :] and its sums) stay in the register file with no scratch.
constexpr int CRF_MAX_WAVES_WIDE = 4;
__host__ __device__ constexpr int crf_max_waves(int classes) { return classes > 32 ? CRF_MAX_WAVES_WIDE : LC_MAX_WAVES; }

struct CrfPlan {
    LcGeometry g;
    size_t alpha_bytes, seq_bytes, partial_bytes;
};

// The one statement of the workspaces: twog_crf_workspace reports it, the launchers use it.
inline CrfPlan crf_plan(int bs, int C, int T, int E) {
    CrfPlan p;
    p.g = lc_geometry(C, E, crf_max_waves(C));
    const size_t n_seq = (size_t)bs * E;
    p.alpha_bytes = n_seq * T * C * sizeof(float);
    p.seq_bytes = n_seq * TWOG_CRF_SEQ_WORDS * sizeof(float);
    p.partial_bytes = n_seq * C * (C + 1) * sizeof(float);
    return p;
}

// grid (groups, bs), 64 * EW threads: wave w runs entity blockIdx.x * EW + w of clip blockIdx.y.
// LDS: stage[2][C][lc_row(EW)] floats.
// alpha [bs * E][T][C]: written at the kept steps only. seq [bs * E][TWOG_CRF_SEQ_WORDS]: logZ, gold, nll, K (int bits).
template <int CMAX>
__global__ __launch_bounds__(64 * crf_max_waves(CMAX)) void crf_fwd_kernel(
    const float* __restrict__ logp, int C, int T, int E, const float* __restrict__ A, const float* __restrict__ pi,
    const long long* __restrict__ target, long long ignore, float* __restrict__ alpha_ws, float* __restrict__ seq, int EW) {
    extern __shared__ float smem[];
    constexpr int R = CMAX / 4;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int b = blockIdx.y, e0 = blockIdx.x * EW, e = e0 + w;
    const bool runs = e < E;                          // wave-uniform; a wave without an entity still stages
    const int row = lc_row(EW);
    const int buf_floats = C * row;
    float* stage = smem;

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
    // column A[:, c]; a lane without a class takes column 0 (finite values: its sums stay finite and are dropped)
    float a[CMAX];
#pragma unroll
    for (int cp = 0; cp < CMAX; ++cp) a[cp] = cp < C ? A[cp * C + (owns ? lane : 0)] : NEG_INF;
    const float pi_c = pi[owns ? lane : 0];
    const int my_row = (owns ? lane : 0) * row + w;
    const int64_t s_idx = (int64_t)b * E + (runs ? e : 0);
    float* alpha_out = alpha_ws + s_idx * T * C;

    float alpha = NEG_INF, gold = 0.0f;
    int K = 0, y_prev = 0;
    const int n_chunks = (T + LC_CHUNK - 1) / LC_CHUNK;
    S.fetch(base, 0, T, pre);
    int lab_pre = fetch_label(0);
    for (int ch = 0; ch < n_chunks; ++ch) {
        const int buf = ch & 1, t0 = ch * LC_CHUNK;
        // buffer `buf` was last read in chunk ch - 2, which every wave left before the barrier of ch - 1
        S.commit(stage + buf * buf_floats, pre);
        __syncthreads();
        const int lab = lab_pre;
        if (ch + 1 < n_chunks) {                          // in flight while this chunk is consumed
            S.fetch(base, t0 + LC_CHUNK, T, pre);
            lab_pre = fetch_label(t0 + LC_CHUNK);
        }
        if (!runs) continue;
        const float* mine = stage + buf * buf_floats + my_row;
        const int n_here = T - t0 < LC_CHUNK ? T - t0 : LC_CHUNK;
        for (int tt = 0; tt < n_here; ++tt) {
            const int y = __builtin_amdgcn_readlane(lab, tt);
            if (y < 0) continue;                          // a removed step: not part of the chain
            const float x = mine[tt * EW];
            const float x_y = lane_value(x, y);
            if (K == 0) {
                alpha = pi_c + x;
                gold = pi[y] + x_y;
            } else {
                float m = NEG_INF;
#pragma unroll
                for (int cp = 0; cp < CMAX; ++cp) m = fmaxf(m, lane_value(alpha, cp) + a[cp]);
                float s = 0.0f;
#pragma unroll
                for (int cp = 0; cp < CMAX; ++cp) s += expf((lane_value(alpha, cp) + a[cp]) - m);
                alpha = x + (m + logf(s));
                gold = gold + (A[y_prev * C + y] + x_y);
            }
            if (!owns) alpha = NEG_INF;
            else alpha_out[(int64_t)(t0 + tt) * C + lane] = alpha;
            y_prev = y;
            ++K;
        }
    }
    if (!runs) return;
    float logZ = 0.0f;
    if (K > 0) {
        const float m = wave_max(alpha);
        const float s = wave_sum(owns ? expf(alpha - m) : 0.0f);
        logZ = m + logf(s);
    } else {
        gold = 0.0f;
    }
    if (lane == 0) {
        float* o = seq + s_idx * TWOG_CRF_SEQ_WORDS;
        o[0] = logZ;
        o[1] = gold;
        o[2] = logZ - gold;
        o[3] = __int_as_float(K);
    }
}

// Same geometry as crf_fwd_kernel, the kept steps walked from the last to the first.
// LDS: stage[2][C][row] floats, then (dinput != NULL) out[2][C][row] floats.
// partials (NULL: the parameters need no gradient) [bs * E][C + 1][C]: rows 0 .. C-1 = sum_k (xi_k - indicator) of the
// sequence, row C = gamma_0 - indicator, all before the factor g.
template <int CMAX>
__global__ __launch_bounds__(64 * crf_max_waves(CMAX)) void crf_bwd_kernel(
    const float* __restrict__ logp, int C, int T, int E, const float* __restrict__ A, const long long* __restrict__ target,
    long long ignore, const float* __restrict__ alpha_ws, const float* __restrict__ seq, const double* __restrict__ stats,
    const float* __restrict__ dloss, float weight, float* __restrict__ dinput, int accumulate, float* __restrict__ partials,
    int EW) {
    extern __shared__ float smem[];
    constexpr int R = CMAX / 4;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int b = blockIdx.y, e0 = blockIdx.x * EW, e = e0 + w;
    const bool runs = e < E;
    const int row = lc_row(EW);
    const int buf_floats = C * row;
    float* stage = smem;
    float* out = smem + 2 * buf_floats;

    const double cnt = stats[1];
    const float g = cnt > 0.0 ? weight * dloss[0] / (float)cnt : 0.0f;

    LcStager S;
    S.init(tid, C, T, E, EW, e0);
    const float* base = logp + (int64_t)b * C * T * E + e0;
    float* dbase = dinput ? dinput + (int64_t)b * C * T * E + e0 : nullptr;
    float pre[R];
    // The staging loops are written out here on the stager's index arithmetic, not called as its members: in this kernel the
    // member form costs three SGPRs, the allocator then rebuilds the expf / logf constants inside the step loop, and the
    // launches at 9 to 16 classes run 1 % longer.
    auto fetch = [&](int t0) {
#pragma unroll
        for (int k = 0; k < R; ++k)
            pre[k] = (S.has(k) && t0 + S.tt < T) ? base[(int64_t)t0 * E + S.goff0 + k * S.gstep] : 0.0f;
    };
    auto commit = [&](int buf) {
#pragma unroll
        for (int k = 0; k < R; ++k)
            if (S.has(k)) stage[buf * buf_floats + S.soff0 + k * S.sstep] = pre[k];
    };
    auto flush = [&](int buf, int t0) {                   // the d input of a finished chunk, in the layout it was fetched in
#pragma unroll
        for (int k = 0; k < R; ++k) {
            if (!S.has(k) || t0 + S.tt >= T) continue;
            float* dst = dbase + (int64_t)t0 * E + S.goff0 + k * S.gstep;
            const float v = out[buf * buf_floats + S.soff0 + k * S.sstep];
            *dst = accumulate ? *dst + v : v;
        }
    };
    const long long* labels = target + (int64_t)b * T * E + (runs ? e : 0);
    auto fetch_label = [&](int t0) {
        return (runs && lane < LC_CHUNK && t0 + lane < T) ? lc_chain_label(labels[(int64_t)(t0 + lane) * E], ignore, C) : -1;
    };

    const float NEG_INF = -__builtin_inff();
    const bool owns = lane < C;
    // row A[c', :]; a lane without a class takes row 0 (finite sums, dropped), a column without a class is 0 under u = -inf
    float ar[CMAX], acc[CMAX];
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
        ar[c] = c < C ? A[(owns ? lane : 0) * C + c] : 0.0f;
        acc[c] = 0.0f;
    }
    const int my_row = (owns ? lane : 0) * row + w;
    const int64_t s_idx = (int64_t)b * E + (runs ? e : 0);
    const float* alpha_in = alpha_ws + s_idx * T * C + (owns ? lane : 0);
    const float logZ = seq[s_idx * TWOG_CRF_SEQ_WORDS];

    float u = NEG_INF, first_d = 0.0f;                    // u = x + beta of the next kept step; first_d = gamma_0 - indicator
    int y_next = -1;                                      // its label, -1: no kept step behind this one yet
    const int n_chunks = (T + LC_CHUNK - 1) / LC_CHUNK;
    fetch((n_chunks - 1) * LC_CHUNK);
    int lab_pre = fetch_label((n_chunks - 1) * LC_CHUNK);
    float alpha_pre = alpha_in[(int64_t)(T - 1) * C];     // one step ahead of its use; a removed step's slot is read, never used
    for (int it = 0; it < n_chunks; ++it) {
        const int buf = it & 1, t0 = (n_chunks - 1 - it) * LC_CHUNK;
        commit(buf);
        __syncthreads();      // stage[buf] is whole, and every wave has left the chunk before: out[buf ^ 1] is whole
        if (dinput && it > 0) flush(buf ^ 1, t0 + LC_CHUNK);
        const int lab = lab_pre;
        if (it + 1 < n_chunks) {
            fetch(t0 - LC_CHUNK);
            lab_pre = fetch_label(t0 - LC_CHUNK);
        }
        if (!runs) continue;
        const float* mine = stage + buf * buf_floats + my_row;
        float* mine_out = out + buf * buf_floats + my_row;
        const int n_here = T - t0 < LC_CHUNK ? T - t0 : LC_CHUNK;
        for (int tt = n_here - 1; tt >= 0; --tt) {
            const int t = t0 + tt;
            const float alpha_t = owns ? alpha_pre : NEG_INF;
            if (t > 0) alpha_pre = alpha_in[(int64_t)(t - 1) * C];
            const int y = __builtin_amdgcn_readlane(lab, tt);
            float d = 0.0f;
            if (y >= 0) {
                const float x = mine[tt * EW];
                float beta = 0.0f;
                if (y_next >= 0) {
                    float m = NEG_INF;
#pragma unroll
                    for (int c = 0; c < CMAX; ++c) m = fmaxf(m, ar[c] + lane_value(u, c));
                    const float scale = expf((alpha_t + m) - logZ);          // xi[c', c] = exp(w[c] - m) * scale
                    const float ind = lane == y ? 1.0f : 0.0f;
                    float s = 0.0f;
#pragma unroll
                    for (int c = 0; c < CMAX; ++c) {
                        const float ex = expf((ar[c] + lane_value(u, c)) - m);
                        s += ex;
                        acc[c] += ex * scale - (c == y_next ? ind : 0.0f);
                    }
                    beta = m + logf(s);
                }
                const float gamma = expf((alpha_t + beta) - logZ);
                first_d = gamma - (lane == y ? 1.0f : 0.0f);
                d = g * first_d;
                u = owns ? x + beta : NEG_INF;
                y_next = y;
            }
            if (dinput && owns) mine_out[tt * EW] = d;
        }
    }
    if (dinput) {
        __syncthreads();
        flush((n_chunks - 1) & 1, 0);
    }
    if (!runs || !partials || !owns) return;
    float* p = partials + s_idx * (C + 1) * C;
#pragma unroll
    for (int c = 0; c < CMAX; ++c)
        if (c < C) p[lane * C + c] = y_next >= 0 ? acc[c] : 0.0f;
    p[C * C + lane] = y_next >= 0 ? first_d : 0.0f;
}

// Element j of the (C + 1, C) partial rows summed over the sequences in index order in fp64, times g, rounded once:
// j < C * C goes to dA, the rest to dpi.
__global__ __launch_bounds__(256) void crf_param_kernel(const float* __restrict__ partials, int64_t n_seq, int C,
                                                         const double* __restrict__ stats, const float* __restrict__ dloss,
                                                         float weight, float* dA, float* dpi, int accumulate) {
    const int j = blockIdx.x * 256 + threadIdx.x, n = (C + 1) * C;
    if (j >= n) return;
    const double cnt = stats[1];
    const float g = cnt > 0.0 ? weight * dloss[0] / (float)cnt : 0.0f;
    double sum = 0.0;
    for (int64_t s = 0; s < n_seq; ++s) sum += (double)partials[s * n + j];
    const float v = (float)((double)g * sum);
    float* dst = j < C * C ? dA + j : dpi + (j - C * C);
    *dst = accumulate ? *dst + v : v;
}

}  // namespace

extern "C" int twog_crf_limits(int* max_classes, int* max_steps) {
    if (max_classes) *max_classes = LC_MAX_CLASSES;
    if (max_steps) *max_steps = LC_MAX_STEPS;
    return 0;
}

extern "C" int twog_crf_workspace(int bs, int n_classes, int T, int E, size_t* alpha_bytes, size_t* seq_bytes,
                                  size_t* partial_bytes) {
    if (!lc_shape_ok(bs, n_classes, T, E)) return -1;
    if (!lc_launchable(bs, n_classes, T, E)) return -2;
    const CrfPlan p = crf_plan(bs, n_classes, T, E);
    if (alpha_bytes) *alpha_bytes = p.alpha_bytes;
    if (seq_bytes) *seq_bytes = p.seq_bytes;
    if (partial_bytes) *partial_bytes = p.partial_bytes;
    return 0;
}

extern "C" int twog_crf_nll_fwd(const float* input, const int64_t* target, int bs, int n_classes, int T, int E,
                                const float* A, const float* pi, int64_t ignore_index, float weight, float* alpha,
                                float* seq, double* stats, float* loss, void* stream) {
    const int C = n_classes;
    if (!lc_shape_ok(bs, C, T, E)) return -1;
    if (!lc_launchable(bs, C, T, E)) return -2;
    if (!A || !pi || !stats || !loss || (bs > 0 && (!input || !target || !alpha || !seq))) return -3;
    hipStream_t st = (hipStream_t)stream;
    if (bs > 0) {
        const CrfPlan p = crf_plan(bs, C, T, E);
        const int rc = lc_dispatch_classes(C, [&](auto cmax) {
            return lc_launch<crf_fwd_kernel<decltype(cmax)::value>>(
                p.g, bs, 2 * p.g.buf_floats * sizeof(float), stream, input, C, T, E, A, pi,
                reinterpret_cast<const long long*>(target), (long long)ignore_index, alpha, seq, p.g.waves);
        });
        if (rc) return rc;
    }
    hipLaunchKernelGGL(lc_nll_final_kernel, dim3(1), dim3(LC_FINAL_THREADS), 0, st, seq, (int64_t)bs * E, weight, stats, loss);
    TWOG_CHECK_LAUNCH();
    return 0;
}

extern "C" int twog_crf_nll_bwd(const float* input, const int64_t* target, int bs, int n_classes, int T, int E,
                                const float* A, int64_t ignore_index, float weight, const float* alpha, const float* seq,
                                const double* stats, const float* dloss, float* dinput, int accumulate, float* partials,
                                float* dA, float* dpi, int accumulate_params, void* stream) {
    const int C = n_classes;
    if (!lc_shape_ok(bs, C, T, E)) return -1;
    if (!lc_launchable(bs, C, T, E)) return -2;
    if (!A || !stats || !dloss || (bs > 0 && (!input || !target || !alpha || !seq))) return -3;
    if ((dA == nullptr) != (dpi == nullptr) || (dA && bs > 0 && !partials)) return -3;
    if (!dinput && !dA) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (bs > 0) {
        const CrfPlan p = crf_plan(bs, C, T, E);
        float* part = dA ? partials : nullptr;
        const int rc = lc_dispatch_classes(C, [&](auto cmax) {
            return lc_launch<crf_bwd_kernel<decltype(cmax)::value>>(
                p.g, bs, (dinput ? 4 : 2) * p.g.buf_floats * sizeof(float), stream, input, C, T, E, A,
                reinterpret_cast<const long long*>(target), (long long)ignore_index, alpha, seq, stats, dloss, weight, dinput,
                accumulate, part, p.g.waves);
        });
        if (rc) return rc;
    }
    if (dA) {
        const int n = (C + 1) * C;
        hipLaunchKernelGGL(crf_param_kernel, dim3((n + 255) / 256), dim3(256), 0, st, partials, (int64_t)bs * E, C, stats, dloss,
                           weight, dA, dpi, accumulate_params);
        TWOG_CHECK_LAUNCH();
    }
    return 0;
}
