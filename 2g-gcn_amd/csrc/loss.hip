// Multi-task loss of the 2G-GCN training step, all terms in one launch.
//
// Reference: vhoi/losses.py:8-70 (select_loss builds the term list: budget, BCE-with-ignore, and 4 or 8 NLL terms),
// pyrutils/torch/losses.py:7-51 (binary_cross_entropy_loss, budget_loss, multi_task_loss), F.nll_loss(ignore_index=-1,
// reduction='mean'). The reference runs 6-12 small torch kernels per term and one host sync per BCE / budget term
// (mask.sum().item()); here every term is a column of a (blocks, terms) grid: lane-contiguous reads, fp64 partial
// sums reduced in a fixed order (bit-reproducible), the per-term {sum, count} kept on the device for the backward
// launch, which writes d(input) of every term in one pass (for NLL: -w/count at the target class, 0 elsewhere).
// Second half of the file: the temporal smoothing terms (truncated MSE between adjacent steps), one more launch per direction;
// then the same criterion with class weights (NLL) and the positive-class weight (BCE), twog_weighted_loss_fwd / _bwd.
#include "twog_common.h"

namespace {

struct Terms { twog_loss_t t[TWOG_LOSS_MAX_TERMS]; };

// {sum, count} of a 256-thread block -> partials[term = blockIdx.y][block = blockIdx.x], in a fixed order
__device__ __forceinline__ void block_partial(double sum, double cnt, double* partials) {
    __shared__ double red[2][4];
    sum = wave_sum_f64(sum);
    cnt = wave_sum_f64(cnt);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { red[0][w] = sum; red[1][w] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double* p = partials + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 2;
        p[0] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        p[1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    }
}

__global__ __launch_bounds__(256) void loss_partial_kernel(const Terms T, double* partials) {
    const twog_loss_t& L = T.t[blockIdx.y];
    const int64_t n = L.outer * L.inner;
    double sum = 0.0, cnt = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        if (L.kind == 0) {
            const int64_t tgt = reinterpret_cast<const int64_t*>(L.target)[e];
            if (twog_label_kept(tgt, (int64_t)L.ignore_value, L.n_classes)) {
                const int64_t o = e / L.inner, i = e - o * L.inner;
                sum -= (double)L.input[(o * L.n_classes + tgt) * L.inner + i];
                cnt += 1.0;
            }
        } else {
            const float t = reinterpret_cast<const float*>(L.target)[e];
            if (t != L.ignore_value) {
                const float x = L.input[e];
                if (L.kind == 1) sum -= (double)(t * fmaxf(logf(x), -100.f) + (1.f - t) * fmaxf(logf(1.f - x), -100.f));
                else sum += (double)x;
                cnt += 1.0;
            }
        }
    }
    block_partial(sum, cnt, partials);
}

// One thread per term adds the term's block partials in block order: {sum, count} (weighted criterion: {sum, kept weight})
// into stats, weight * mean into losses. Shared by loss_final_kernel and wloss_final_kernel (TermT = twog_loss_t / twog_wloss_t);
// it holds no multiply that feeds an add, so it reads the same on either side of the contraction pragma below.
// SOFT_ONLY (smooth_final_kernel, whose terms have no kind): every term takes the branch of the BCE / budget terms.
template <bool SOFT_ONLY = false, class TermT>
__device__ __forceinline__ void final_body(const TermT* terms, int n_terms, int n_blocks, const double* partials, double* stats,
                                           float* losses) {
    const int term = blockIdx.x * blockDim.x + threadIdx.x;
    if (term >= n_terms) return;
    double sum = 0.0, cnt = 0.0;
    for (int b = 0; b < n_blocks; ++b) {
        sum += partials[((int64_t)term * n_blocks + b) * 2];
        cnt += partials[((int64_t)term * n_blocks + b) * 2 + 1];
    }
    stats[term * 2] = sum;
    stats[term * 2 + 1] = cnt;
    const TermT& L = terms[term];
    bool soft = true;
    if constexpr (!SOFT_ONLY) soft = L.kind != 0;
    // NLL: 0 / 0 -> NaN like torch's mean over an empty selection (F.nll_loss(weight=): no kept weight)
    const double v = soft ? (cnt > 0.0 ? sum / cnt : 0.0) : sum / cnt;
    losses[term] = L.weight * (float)v;
}

__global__ void loss_final_kernel(const Terms T, int n_terms, int n_blocks, const double* partials, double* stats,
                                  float* losses) {
    final_body(T.t, n_terms, n_blocks, partials, stats, losses);
}

__global__ __launch_bounds__(256) void loss_bwd_kernel(const Terms T, const double* stats, const float* dlosses) {
    const twog_loss_t& L = T.t[blockIdx.y];
    if (!L.dinput) return;
    const int64_t n = L.outer * L.inner;
    const double cnt = stats[blockIdx.y * 2 + 1];
    const float g = cnt > 0.0 ? L.weight * dlosses[blockIdx.y] / (float)cnt : 0.f;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        if (L.kind == 0) {
            const int64_t tgt = reinterpret_cast<const int64_t*>(L.target)[e];
            const bool valid = twog_label_kept(tgt, (int64_t)L.ignore_value, L.n_classes);
            const int64_t o = e / L.inner, i = e - o * L.inner;
            float* d = L.dinput + o * L.n_classes * L.inner + i;
            for (int c = 0; c < L.n_classes; ++c) d[(int64_t)c * L.inner] = (valid && c == tgt) ? -g : 0.f;
        } else {
            const float t = reinterpret_cast<const float*>(L.target)[e];
            float d = 0.f;
            if (t != L.ignore_value) {
                if (L.kind == 1) {
                    const float x = L.input[e];
                    d = g * (x - t) / fmaxf((1.f - x) * x, 1e-12f);  // torch's binary_cross_entropy backward
                } else {
                    d = g;
                }
            }
            L.dinput[e] = d;
        }
    }
}

template <class TermT>   // twog_loss_t, and the part of twog_wloss_t it shares
inline bool terms_ok(const TermT* t, int n) {
    if (n < 0 || n > TWOG_LOSS_MAX_TERMS) return false;
    for (int i = 0; i < n; ++i) {
        if (t[i].kind < 0 || t[i].kind > 2 || t[i].outer < 0 || t[i].inner < 0) return false;
        if (t[i].kind == 0 && t[i].n_classes < 1) return false;
    }
    return true;
}

// ------------------------------------------------------------------------------------------------------------------
// Temporal smoothing loss (truncated MSE between the log-probabilities of adjacent steps; the definition is at
// twog_smooth_loss_t in include/twog_gcn.h). One thread per (o, t, e) along the contiguous t * E + e axis, a loop over
// the classes: the predecessor is E floats back, mostly in the same cache lines.
// The definition fixes every fp32 rounding (the difference, g, the product g * 2 D, the addition into the buffer), so from
// here to the end of the file no multiplication is fused with an addition.
#pragma clang fp contract(off)

struct SmoothTerms { twog_smooth_loss_t t[TWOG_LOSS_MAX_TERMS]; };

__device__ __forceinline__ bool smooth_step_kept(const twog_smooth_loss_t& L, int64_t y) {
    return twog_label_kept(y, (int64_t)L.ignore_value, L.n_classes);
}

__global__ __launch_bounds__(256) void smooth_partial_kernel(const SmoothTerms T, double* partials) {
    const twog_smooth_loss_t& L = T.t[blockIdx.y];
    const int64_t inner = L.steps * L.entities, n = L.outer * inner;
    const double tau2 = (double)L.tau * (double)L.tau;
    double sum = 0.0, cnt = 0.0;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
        const int64_t o = p / inner, r = p - o * inner;
        if (r < L.entities) continue;   // step 0 has no predecessor
        if (!smooth_step_kept(L, L.target[p]) || !smooth_step_kept(L, L.target[p - L.entities])) continue;
        const float* x = L.input + o * L.n_classes * inner + r;
        for (int c = 0; c < L.n_classes; ++c) {
            const float d = x[(int64_t)c * inner] - x[(int64_t)c * inner - L.entities];
            sum += fmin((double)d * (double)d, tau2);
        }
        cnt += (double)L.n_classes;
    }
    block_partial(sum, cnt, partials);
}

__global__ void smooth_final_kernel(const SmoothTerms T, int n_terms, int n_blocks, const double* partials, double* stats,
                                    float* losses) {
    final_body<true>(T.t, n_terms, n_blocks, partials, stats, losses);
}

__global__ __launch_bounds__(256) void smooth_bwd_kernel(const SmoothTerms T, const double* stats, const float* dlosses) {
    const twog_smooth_loss_t& L = T.t[blockIdx.y];
    if (!L.dinput) return;
    const int64_t inner = L.steps * L.entities, n = L.outer * inner;
    const double tau2 = (double)L.tau * (double)L.tau;
    const double cnt = stats[blockIdx.y * 2 + 1];
    const float g = cnt > 0.0 ? L.weight * dlosses[blockIdx.y] / (float)cnt : 0.f;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
        const int64_t o = p / inner, r = p - o * inner;
        const bool kept = r >= L.entities && smooth_step_kept(L, L.target[p]) &&
                          smooth_step_kept(L, L.target[p - L.entities]);
        if (!kept && L.accumulate) continue;
        const float* x = L.input + o * L.n_classes * inner + r;
        float* dx = L.dinput + o * L.n_classes * inner + r;
        for (int c = 0; c < L.n_classes; ++c) {
            float v = 0.f;
            if (kept) {
                const float d = x[(int64_t)c * inner] - x[(int64_t)c * inner - L.entities];
                if ((double)d * (double)d <= tau2) v = g * (2.f * d);
            }
            if (!L.accumulate) dx[(int64_t)c * inner] = v;
            else if (v != 0.f) dx[(int64_t)c * inner] += v;
        }
    }
}

inline bool smooth_terms_ok(const twog_smooth_loss_t* t, int n) {
    if (n < 0 || n > TWOG_LOSS_MAX_TERMS) return false;
    for (int i = 0; i < n; ++i)
        if (!(t[i].tau > 0.f) || t[i].outer < 0 || t[i].steps < 0 || t[i].entities < 0 || t[i].n_classes < 1) return false;
    return true;
}

// ------------------------------------------------------------------------------------------------------------------
// The criterion with class weights (NLL) and the positive-class weight (BCE): twog_wloss_t in include/twog_gcn.h states
// every operation. The kernels above are left as they are (their multiply-adds may be fused; these are not), so the
// per-element arithmetic is written out again here; the launch shape, the block reduction and the final sums are shared. With cw == 1 and
// p <= 1 every partial sum below is the one loss_partial_kernel forms: sum + 1.0 * (-x) == sum - x.
struct WTerms { twog_wloss_t t[TWOG_LOSS_MAX_TERMS]; };

__device__ __forceinline__ bool wloss_positive(const twog_wloss_t& L, float t) {
    return t == 1.0f && L.positive_class_weight > 1.f;
}

__global__ __launch_bounds__(256) void wloss_partial_kernel(const WTerms T, double* partials) {
    const twog_wloss_t& L = T.t[blockIdx.y];
    const int64_t n = L.outer * L.inner;
    double sum = 0.0, den = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        if (L.kind == 0) {
            const int64_t tgt = reinterpret_cast<const int64_t*>(L.target)[e];
            if (twog_label_kept(tgt, (int64_t)L.ignore_value, L.n_classes)) {
                const int64_t o = e / L.inner, i = e - o * L.inner;
                const double cw = L.class_weight ? (double)L.class_weight[tgt] : 1.0;
                sum += cw * (double)(-L.input[(o * L.n_classes + tgt) * L.inner + i]);
                den += cw;
            }
        } else {
            const float t = reinterpret_cast<const float*>(L.target)[e];
            if (t != L.ignore_value) {
                const float x = L.input[e];
                float v;
                if (L.kind == 2) v = x;
                else if (wloss_positive(L, t)) v = -fmaxf(L.positive_class_weight * logf(x), -100.f);
                else v = -(t * fmaxf(logf(x), -100.f) + (1.f - t) * fmaxf(logf(1.f - x), -100.f));
                sum += (double)v;
                den += 1.0;
            }
        }
    }
    block_partial(sum, den, partials);
}

__global__ void wloss_final_kernel(const WTerms T, int n_terms, int n_blocks, const double* partials, double* stats,
                                   float* losses) {
    final_body(T.t, n_terms, n_blocks, partials, stats, losses);
}

__global__ __launch_bounds__(256) void wloss_bwd_kernel(const WTerms T, const double* stats, const float* dlosses) {
    const twog_wloss_t& L = T.t[blockIdx.y];
    if (!L.dinput) return;
    const int64_t n = L.outer * L.inner;
    const double den = stats[blockIdx.y * 2 + 1];
    const float g = den > 0.0 ? L.weight * dlosses[blockIdx.y] / (float)den : 0.f;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        if (L.kind == 0) {
            const int64_t tgt = reinterpret_cast<const int64_t*>(L.target)[e];
            const bool valid = twog_label_kept(tgt, (int64_t)L.ignore_value, L.n_classes);
            const int64_t o = e / L.inner, i = e - o * L.inner;
            float v = 0.f;
            if (valid) v = L.class_weight ? -(g * L.class_weight[tgt]) : -g;
            float* d = L.dinput + o * L.n_classes * L.inner + i;
            for (int c = 0; c < L.n_classes; ++c) d[(int64_t)c * L.inner] = (valid && c == tgt) ? v : 0.f;
        } else {
            const float t = reinterpret_cast<const float*>(L.target)[e];
            float d = 0.f;
            if (t != L.ignore_value) {
                if (L.kind == 1) {
                    const float x = L.input[e];
                    d = g * (x - t) / fmaxf((1.f - x) * x, 1e-12f);  // torch's binary_cross_entropy backward
                    if (wloss_positive(L, t)) d = d * L.positive_class_weight;
                } else {
                    d = g;
                }
            }
            L.dinput[e] = d;
        }
    }
}

inline bool wterms_ok(const twog_wloss_t* t, int n) {
    if (!terms_ok(t, n)) return false;
    for (int i = 0; i < n; ++i)
        if (!(t[i].positive_class_weight >= 0.f) || !(t[i].positive_class_weight <= 3.402823466e38f)) return false;
    return true;
}

// The forward launches of one criterion (TermsT = Terms / SmoothTerms / WTerms; ok = its argument check): copy the terms into
// the by-value struct, then the partial and the final sums.
template <class TermsT, class TermT, class PartialK, class FinalK>
int launch_fwd(bool ok, const TermT* terms, int n_terms, PartialK partial_kernel, FinalK final_kernel, double* partials,
               double* stats, float* losses, void* stream) {
    if (!ok) return -1;
    if (n_terms == 0) return 0;
    TermsT T;
    for (int i = 0; i < n_terms; ++i) T.t[i] = terms[i];
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(partial_kernel, dim3(TWOG_LOSS_BLOCKS, n_terms), dim3(256), 0, st, T, partials);
    TWOG_CHECK_LAUNCH();
    hipLaunchKernelGGL(final_kernel, dim3(1), dim3(64), 0, st, T, n_terms, TWOG_LOSS_BLOCKS, partials, stats, losses);
    TWOG_CHECK_LAUNCH();
    return 0;
}

// the backward launch of one criterion
template <class TermsT, class TermT, class BwdK>
int launch_bwd(bool ok, const TermT* terms, int n_terms, BwdK bwd_kernel, const double* stats, const float* dlosses,
               void* stream) {
    if (!ok) return -1;
    if (n_terms == 0) return 0;
    TermsT T;
    for (int i = 0; i < n_terms; ++i) T.t[i] = terms[i];
    hipLaunchKernelGGL(bwd_kernel, dim3(TWOG_LOSS_BLOCKS * 4, n_terms), dim3(256), 0, (hipStream_t)stream, T, stats, dlosses);
    TWOG_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" int twog_weighted_loss_fwd(const twog_wloss_t* terms, int n_terms, double* partials, double* stats,
                                      float* losses, void* stream) {
    return launch_fwd<WTerms>(wterms_ok(terms, n_terms), terms, n_terms, wloss_partial_kernel, wloss_final_kernel, partials,
                              stats, losses, stream);
}

extern "C" int twog_weighted_loss_bwd(const twog_wloss_t* terms, int n_terms, const double* stats, const float* dlosses,
                                      void* stream) {
    return launch_bwd<WTerms>(wterms_ok(terms, n_terms), terms, n_terms, wloss_bwd_kernel, stats, dlosses, stream);
}

extern "C" int twog_smooth_loss_fwd(const twog_smooth_loss_t* terms, int n_terms, double* partials, double* stats,
                                    float* losses, void* stream) {
    return launch_fwd<SmoothTerms>(smooth_terms_ok(terms, n_terms), terms, n_terms, smooth_partial_kernel, smooth_final_kernel,
                                   partials, stats, losses, stream);
}

extern "C" int twog_smooth_loss_bwd(const twog_smooth_loss_t* terms, int n_terms, const double* stats, const float* dlosses,
                                    void* stream) {
    return launch_bwd<SmoothTerms>(smooth_terms_ok(terms, n_terms), terms, n_terms, smooth_bwd_kernel, stats, dlosses, stream);
}

extern "C" int twog_multitask_loss_fwd(const twog_loss_t* terms, int n_terms, double* partials, double* stats,
                                       float* losses, void* stream) {
    return launch_fwd<Terms>(terms_ok(terms, n_terms), terms, n_terms, loss_partial_kernel, loss_final_kernel, partials, stats,
                             losses, stream);
}

extern "C" int twog_multitask_loss_bwd(const twog_loss_t* terms, int n_terms, const double* stats, const float* dlosses,
                                       void* stream) {
    return launch_bwd<Terms>(terms_ok(terms, n_terms), terms, n_terms, loss_bwd_kernel, stats, dlosses, stream);
}
