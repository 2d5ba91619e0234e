// Training-step options of the reference's trainer on the fused step (include/twog_gcn.h, "Training-step options"):
// the global gradient norm of clip_grad_norm_ (pyrutils/torch/train_utils.py:149-153), Adam reading the clip coefficient
// from device memory, and the multi-task loss learner's weighting (pyrutils/torch/multi_task.py:10-75).
//
// The norm is the only one with a cost: one read of the model's flat gradient buffer (45.5 M floats = 182 MB for the
// headline model). Each workgroup of the first launch sums fp64 squares of a fixed set of float4 groups (four loads in flight
// per thread) and writes one partial; the second launch adds the partials in a fixed order. Nothing depends on scheduling, so
// the result is the same bit for bit on every run, and fp64 keeps the sum finite for every finite fp32 input.
#include "twog_common.h"

namespace {

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

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
