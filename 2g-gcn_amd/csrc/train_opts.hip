// Training-step options of the reference's trainer on the fused step (include/twog_gcn.h, "Training-step options"):
// the global gradient norm of clip_grad_norm_ (pyrutils/torch/train_utils.py:149-153), Adam reading the clip coefficient
// from device memory, and the multi-task loss learner's weighting (pyrutils/torch/multi_task.py:10-75). Further down: Adam
// with its step state on the device (twog_optim_prepare / twog_optim_apply: checkpoints, NaN skip, AdamW, EMA).
//
// The norm is the only one with a cost: one read of the model's flat gradient buffer (45.5 M floats = 182 MB for the
// headline model). Each workgroup of the first launch sums fp64 squares of a fixed set of float4 groups (four loads in flight
// per thread) and writes one partial; the second launch adds the partials in a fixed order. Nothing depends on scheduling, so
// the result is the same bit for bit on every run, and fp64 keeps the sum finite for every finite fp32 input.
#include "twog_common.h"

namespace {

// fixed-order block sum (256 threads): waves by shuffle, then wave 0 adds the four wave sums in index order
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
    v = wave_sum_f64(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) red[w] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += red[i];
    return t;
}

__device__ __forceinline__ double sq4(const float4 a) {
    const double x = a.x, y = a.y, z = a.z, w = a.w;
    return x * x + y * y + z * z + w * w;
}

constexpr int NORM_THREADS = 256;
constexpr int NORM_UNROLL = 4;

__global__ __launch_bounds__(NORM_THREADS) void norm_partials_kernel(const float* __restrict__ buf, const twog_ranges_t R,
                                                                      double* __restrict__ partials) {
    __shared__ double red[NORM_THREADS / 64];
    const int64_t tid = (int64_t)blockIdx.x * NORM_THREADS + threadIdx.x;
    const int64_t nthr = (int64_t)gridDim.x * NORM_THREADS;
    double acc = 0.0;
    for (int r = 0; r < R.n_ranges; ++r) {
        const int64_t b = R.begin[r], e = R.end[r];
        int64_t a0 = (b + 3) & ~(int64_t)3;   // first 16-byte aligned element (buf itself is 16-byte aligned)
        if (a0 > e) a0 = e;
        const int64_t n4 = (e - a0) >> 2, a1 = a0 + n4 * 4;
        const float4* p4 = reinterpret_cast<const float4*>(buf + a0);
        int64_t i = tid;
        for (; i + (NORM_UNROLL - 1) * nthr < n4; i += NORM_UNROLL * nthr) {
            float4 v[NORM_UNROLL];
#pragma unroll
            for (int u = 0; u < NORM_UNROLL; ++u) v[u] = p4[i + u * nthr];
#pragma unroll
            for (int u = 0; u < NORM_UNROLL; ++u) acc += sq4(v[u]);
        }
        for (; i < n4; i += nthr) acc += sq4(p4[i]);
        // at most three elements in front of the aligned body and three behind it
        if (tid < a0 - b) { const double x = buf[b + tid]; acc += x * x; }
        if (tid < e - a1) { const double x = buf[a1 + tid]; acc += x * x; }
    }
    const double t = block_sum_f64(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

__global__ __launch_bounds__(NORM_THREADS) void norm_finish_kernel(const double* __restrict__ partials, int n_partials,
                                                                    float scale, float max_norm, float* __restrict__ out) {
    __shared__ double red[NORM_THREADS / 64];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n_partials; i += NORM_THREADS) acc += partials[i];
    const double s = block_sum_f64(acc, red);
    if (threadIdx.x == 0) {
        const float norm = (float)(sqrt(s) * fabs((double)scale));
        // torch: max_norm / (total_norm + 1e-6) on an fp32 tensor = (total_norm + 1e-6).reciprocal() * max_norm
        const float inv = __fdiv_rn(1.f, __fadd_rn(norm, 1e-6f));
        out[0] = norm;
        out[1] = __fmul_rn(inv, max_norm);
    }
}

// adam_kernel of misc.hip with a clip coefficient read on the device. k == 1 (no clipping, or a NaN coefficient) runs the
// same source expression as adam_kernel, so it compiles to the same arithmetic and gives the same bits.
__global__ __launch_bounds__(256) void adam_coef_kernel(float* p, const float* g, float* m, float* v, int64_t n, float lr,
                                                        float b1, float b2, float eps, float wd, float bc1, float bc2s,
                                                        float gscale, const float* __restrict__ coef) {
    const float c = coef[0];
    const float k = c < 1.f ? c : 1.f;
    if (k == 1.f) {
        for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
            float gi = g[i] * gscale;
            if (wd != 0.f) gi += wd * p[i];
            const float mi = b1 * m[i] + (1.f - b1) * gi;
            const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
            m[i] = mi;
            v[i] = vi;
            p[i] -= (lr / bc1) * mi / (sqrtf(vi) / bc2s + eps);
        }
        return;
    }
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float gi = __fmul_rn(__fmul_rn(g[i], gscale), k);   // fl(fl(g * grad_scale) * k): never contracted
        if (wd != 0.f) gi += wd * p[i];
        const float mi = b1 * m[i] + (1.f - b1) * gi;
        const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        p[i] -= (lr / bc1) * mi / (sqrtf(vi) / bc2s + eps);
    }
}

inline int grid_for(int64_t n, int block = 256, int cap = 4096) {
    int64_t g = (n + block - 1) / block;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (int)g;
}

// The learner's weight of one term and the factor of its derivative, in torch's order of operations
// (multi_task.py:63-71: exp(-2 s), 0.5 * exp(-2 s), sqrt(2) * exp(-s)); e = the exp, a = the constant in front of it,
// d = d(exponent)/ds. Products and sums are rounded one by one (no contraction), as the reference's separate ATen ops.
struct TermWeight { float w, e, a, d; };
__device__ __forceinline__ TermWeight term_weight(int kind, float s) {
    TermWeight t;
    if (kind == TWOG_MTL_MAE) {
        t.e = expf(-s);
        t.a = 1.41421356237309515f;   // math.sqrt(2.0) as an fp32 scalar
        t.d = -1.f;
        t.w = __fmul_rn(t.a, t.e);
    } else {
        t.e = expf(__fmul_rn(-2.f, s));
        t.a = kind == TWOG_MTL_MSE ? 0.5f : 1.f;
        t.d = -2.f;
        t.w = kind == TWOG_MTL_MSE ? __fmul_rn(0.5f, t.e) : t.e;
    }
    return t;
}

__global__ __launch_bounds__(64) void mtl_fwd_kernel(const twog_mtl_t spec, const float* __restrict__ losses,
                                                     const float* __restrict__ log_sds, float* __restrict__ out) {
    const int i = threadIdx.x;
    if (i >= spec.n) return;
    const float L = losses[i];
    if (spec.kind[i] == TWOG_MTL_PASS) {
        out[i] = L;
        return;
    }
    const float s = log_sds[i];
    const TermWeight t = term_weight(spec.kind[i], s);
    out[i] = __fadd_rn(__fmul_rn(t.w, L), s);
}

__global__ __launch_bounds__(64) void mtl_bwd_kernel(const twog_mtl_t spec, const float* __restrict__ losses,
                                                     const float* __restrict__ log_sds, const float* __restrict__ dout,
                                                     float* __restrict__ dlosses, float* __restrict__ dlog_sds,
                                                     int accumulate) {
    const int i = threadIdx.x;
    if (i >= spec.n) return;
    const float go = dout[i];
    if (spec.kind[i] == TWOG_MTL_PASS) {
        if (dlosses) dlosses[i] = go;
        if (!accumulate) dlog_sds[i] = 0.f;
        return;
    }
    const float L = losses[i], s = log_sds[i];
    const TermWeight t = term_weight(spec.kind[i], s);
    if (dlosses) dlosses[i] = __fmul_rn(go, t.w);
    // d/ds (w L + s) through w = a * exp(d * s): ((go * L) * a) * e * d, plus go from the "+ s"
    float gw = __fmul_rn(go, L);
    if (t.a != 1.f) gw = __fmul_rn(gw, t.a);
    const float ds = __fadd_rn(__fmul_rn(__fmul_rn(gw, t.e), t.d), go);
    dlog_sds[i] = accumulate ? __fadd_rn(dlog_sds[i], ds) : ds;
}

bool mtl_spec_ok(const twog_mtl_t* spec) {
    if (!spec || spec->n < 0 || spec->n > TWOG_MTL_MAX_TERMS) return false;
    for (int i = 0; i < spec->n; ++i)
        if (spec->kind[i] < TWOG_MTL_PASS || spec->kind[i] > TWOG_MTL_MAE) return false;
    return true;
}

// ---------------------------------------------------------------------------------------------------------------------
// Adam with its step state on the device (include/twog_gcn.h states the arithmetic; tests/optim_state_ref.py is its numpy form).
// One rounding per operation is the contract. hipcc contracts a * b + c into a fused multiply-add by default, the __f*_rn
// functions of its headers included (they are the plain operators), so the functions below switch contraction off for their own
// statements; fp32 division and square root are correctly rounded by default.
__global__ __launch_bounds__(64) void optim_prepare_kernel(twog_optim_state_t* st, const twog_optim_hyper_t h, float lr,
                                                           const float* lr_ptr, const float* norm0, const float* norm1,
                                                           const float* coef, int flags) {
#pragma clang fp contract(off)
    if (threadIdx.x != 0) return;
    bool finite = true;
    if (norm0) finite = finite && isfinite(norm0[0]);
    if (norm1) finite = finite && isfinite(norm1[0]);
    if ((flags & TWOG_OPTIM_SKIP_NONFINITE) && !finite) {
        st->skipped += 1;
        st->apply = 0;
        return;
    }
    const double b1p = st->beta1_pow * (double)h.beta1, b2p = st->beta2_pow * (double)h.beta2;
    if (lr_ptr) lr = lr_ptr[0];
    const float bc1 = (float)(1.0 - b1p);
    float k = 1.f;
    if (coef) {
        const float c = coef[0];
        if (c < 1.f) k = c;
    }
    st->step += 1;
    st->beta1_pow = b1p;
    st->beta2_pow = b2p;
    st->lr = lr;
    st->step_size = lr / bc1;
    st->bc2s = (float)__builtin_sqrt(1.0 - b2p);
    st->clip_k = k;
    st->decay_mul = 1.f - lr * h.weight_decay;
    st->apply = 1;
}

struct OptimStep {
    float b1, b2, omb1, omb2, eps, wd, gscale, d, omd, step_size, bc2s, clip_k, decay_mul;
    int flags;
};

template <bool EMA>
__device__ __forceinline__ void optim_elem(float& p, float g, float& m, float& v, float& ema, const OptimStep& s) {
#pragma clang fp contract(off)
    g = g * s.gscale;
    if (s.flags & TWOG_OPTIM_CLIP) g = g * s.clip_k;
    float p0 = p;
    if (s.flags & TWOG_OPTIM_DECOUPLED) {
        p0 = p * s.decay_mul;
    } else if (s.wd != 0.f) {
        const float wp = s.wd * p;
        g = g + wp;
    }
    const float m0 = s.b1 * m, m1 = s.omb1 * g;
    m = m0 + m1;
    const float gg = g * g, v0 = s.b2 * v, v1 = s.omb2 * gg;
    v = v0 + v1;
    const float num = s.step_size * m, den = __builtin_sqrtf(v) / s.bc2s + s.eps;   // (the sum's operand is a quotient)
    p = p0 - num / den;
    if (EMA) {
        const float e0 = s.d * ema, e1 = s.omd * p;
        ema = e0 + e1;
    }
}

template <bool EMA>
__global__ __launch_bounds__(TWOG_STREAM_THREADS) void optim_apply_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                                          float* __restrict__ m, float* __restrict__ v,
                                                                          float* __restrict__ ema, int64_t n, int head,
                                                                          const twog_optim_hyper_t h, int flags,
                                                                          const twog_optim_state_t* __restrict__ st) {
    if (st->apply == 0) return;   // a skipped step: nothing is written
    OptimStep s;
    {
#pragma clang fp contract(off)
        s.b1 = h.beta1, s.b2 = h.beta2, s.omb1 = 1.f - h.beta1, s.omb2 = 1.f - h.beta2;
        s.eps = h.eps, s.wd = h.weight_decay, s.gscale = h.grad_scale, s.d = h.ema_decay, s.omd = 1.f - h.ema_decay;
    }
    s.step_size = st->step_size, s.bc2s = st->bc2s, s.clip_k = st->clip_k, s.decay_mul = st->decay_mul, s.flags = flags;
    const int64_t tid = (int64_t)blockIdx.x * TWOG_STREAM_THREADS + threadIdx.x;
    const int64_t nthr = (int64_t)gridDim.x * TWOG_STREAM_THREADS;
    // [0, head) in front of the first 16-byte boundary (head <= 3, head <= n), n4 groups of four, then [a1, n) (at most 3)
    const int64_t n4 = (n - head) >> 2, a1 = head + n4 * 4;
    float4* p4 = reinterpret_cast<float4*>(p + head);
    const float4* g4 = reinterpret_cast<const float4*>(g + head);
    float4* m4 = reinterpret_cast<float4*>(m + head);
    float4* v4 = reinterpret_cast<float4*>(v + head);
    float4* e4 = EMA ? reinterpret_cast<float4*>(ema + head) : nullptr;
    for (int64_t i = tid; i < n4; i += nthr) {
        float4 P = p4[i], M = m4[i], V = v4[i], E = EMA ? e4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 G = g4[i];
        optim_elem<EMA>(P.x, G.x, M.x, V.x, E.x, s);
        optim_elem<EMA>(P.y, G.y, M.y, V.y, E.y, s);
        optim_elem<EMA>(P.z, G.z, M.z, V.z, E.z, s);
        optim_elem<EMA>(P.w, G.w, M.w, V.w, E.w, s);
        p4[i] = P, m4[i] = M, v4[i] = V;
        if (EMA) e4[i] = E;
    }
    float dummy = 0.f;
    if (tid < head) optim_elem<EMA>(p[tid], g[tid], m[tid], v[tid], EMA ? ema[tid] : dummy, s);
    if (tid < n - a1) optim_elem<EMA>(p[a1 + tid], g[a1 + tid], m[a1 + tid], v[a1 + tid], EMA ? ema[a1 + tid] : dummy, s);
}

}  // namespace

extern "C" int twog_grad_norm(const float* buf, const twog_ranges_t* ranges, float scale, float max_norm, double* partials,
                              float* out, void* stream) {
    if (!ranges || !partials || !out || ranges->n_ranges < 0 || ranges->n_ranges > TWOG_NORM_MAX_RANGES) return -2;
    int64_t n4 = 0;
    for (int r = 0; r < ranges->n_ranges; ++r) {
        if (ranges->begin[r] < 0 || ranges->end[r] < ranges->begin[r]) return -2;
        n4 += (ranges->end[r] - ranges->begin[r] + 3) / 4;
    }
    if (n4 > 0 && (!buf || (reinterpret_cast<uintptr_t>(buf) & 15) != 0)) return -2;
    // the grid depends on the sizes only: the same ranges always give the same summation order
    const int blocks = grid_for((n4 + NORM_UNROLL - 1) / NORM_UNROLL, NORM_THREADS, TWOG_NORM_BLOCKS);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(norm_partials_kernel, dim3(blocks), dim3(NORM_THREADS), 0, st, buf, *ranges, partials);
    TWOG_CHECK_LAUNCH();
    hipLaunchKernelGGL(norm_finish_kernel, dim3(1), dim3(NORM_THREADS), 0, st, partials, blocks, scale, max_norm, out);
    TWOG_CHECK_LAUNCH();
    return 0;
}

extern "C" int twog_adam_step_coef(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                                   float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                                   const float* coef, void* stream) {
    if (n <= 0) return 0;
    if (!coef) return -2;
    const float bc1 = 1.f - powf(beta1, (float)step);     // as twog_adam_step (misc.hip)
    const float bc2s = sqrtf(1.f - powf(beta2, (float)step));
    hipLaunchKernelGGL(adam_coef_kernel, dim3(grid_for(n, 256, 2048)), dim3(256), 0, (hipStream_t)stream, param, grad,
                       exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, bc1, bc2s, grad_scale, coef);
    TWOG_CHECK_LAUNCH();
    return 0;
}

extern "C" int twog_mtl_weight_fwd(const twog_mtl_t* spec, const float* losses, const float* log_sds, float* out,
                                   void* stream) {
    if (!mtl_spec_ok(spec)) return -2;
    if (spec->n == 0) return 0;
    if (!losses || !log_sds || !out) return -2;
    hipLaunchKernelGGL(mtl_fwd_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, *spec, losses, log_sds, out);
    TWOG_CHECK_LAUNCH();
    return 0;
}

extern "C" int twog_mtl_weight_bwd(const twog_mtl_t* spec, const float* losses, const float* log_sds, const float* dout,
                                   float* dlosses, float* dlog_sds, int accumulate, void* stream) {
    if (!mtl_spec_ok(spec)) return -2;
    if (spec->n == 0) return 0;
    if (!losses || !log_sds || !dout || !dlog_sds) return -2;
    hipLaunchKernelGGL(mtl_bwd_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, *spec, losses, log_sds, dout, dlosses,
                       dlog_sds, accumulate);
    TWOG_CHECK_LAUNCH();
    return 0;
}

extern "C" int twog_optim_prepare(twog_optim_state_t* state, const twog_optim_hyper_t* hyper, float lr, const float* lr_ptr,
                                  const float* const* norms, int n_norms, const float* coef, int flags, void* stream) {
    if (!state || !hyper || n_norms < 0 || n_norms > 2 || (n_norms > 0 && !norms)) return -2;
    for (int j = 0; j < n_norms; ++j)
        if (!norms[j]) return -2;
    hipLaunchKernelGGL(optim_prepare_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, *hyper, lr, lr_ptr,
                       n_norms > 0 ? norms[0] : nullptr, n_norms > 1 ? norms[1] : nullptr, coef, flags);
    TWOG_CHECK_LAUNCH();
    return 0;
}

extern "C" int twog_optim_apply(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                                const twog_optim_hyper_t* hyper, int flags, const twog_optim_state_t* state, void* stream) {
    if (!state || !hyper || !param || !grad || !exp_avg || !exp_avg_sq || n < 0) return -2;
    if (ema && !(hyper->ema_decay > 0.f && hyper->ema_decay < 1.f)) return -2;
    const uintptr_t a = reinterpret_cast<uintptr_t>(param) & 15;
    if ((a & 3) != 0) return -2;
    for (const void* q : {(const void*)grad, (const void*)exp_avg, (const void*)exp_avg_sq, (const void*)(ema ? ema : param)})
        if ((reinterpret_cast<uintptr_t>(q) & 15) != a) return -2;
    if (n == 0) return 0;
    int64_t head = ((16 - (int64_t)a) & 15) >> 2;
    if (head > n) head = n;
    const int grid = twog_stream_blocks(TWOG_STREAM_OPTIM, n);
    if (ema)
        hipLaunchKernelGGL(optim_apply_kernel<true>, dim3(grid), dim3(TWOG_STREAM_THREADS), 0, (hipStream_t)stream, param, grad,
                           exp_avg, exp_avg_sq, ema, n, (int)head, *hyper, flags, state);
    else
        hipLaunchKernelGGL(optim_apply_kernel<false>, dim3(grid), dim3(TWOG_STREAM_THREADS), 0, (hipStream_t)stream, param, grad,
                           exp_avg, exp_avg_sq, ema, n, (int)head, *hyper, flags, state);
    TWOG_CHECK_LAUNCH();
    return 0;
}
