// Entity pooling + concatenation of the two baseline models (include/twog_gcn.h, twog_entity_pool_*).
//
// Reference: BimanualBaseline.forward / CAD120Baseline.forward (vhoi/models.py:59-68, :132-154):
//   human head input  [hfr_h | sum_o mask_o ofr_o / max(sum_o mask_o, 1)]          (objects -> humans, masked mean)
//   object head input [ofr_o | sum_h hfr_h]                                        (humans -> objects, CAD-120 only)
// MI355X design: memory-bound. A thread owns one column group (4 floats when the row width allows 16-byte accesses, else
// 1) of one (clip, frame): it reduces the entities of that frame in a fixed order (o = 0, 1, ...; no atomics: a step is
// bit-reproducible) and then broadcasts the pooled value to every receiving row, so each pooled vector is reduced once
// per frame. Consecutive threads take consecutive column groups of the same rows (coalesced); when a row is narrower than
// the workgroup, one workgroup covers several frames.
#include "twog_common.h"

namespace {

template <int V>
struct Vec;
template <>
struct Vec<1> {
    typedef float T;
    static __device__ __forceinline__ T zero() { return 0.f; }
};
template <>
struct Vec<4> {
    typedef f32x4 T;
    static __device__ __forceinline__ T zero() { return T{0.f, 0.f, 0.f, 0.f}; }
};

template <int V>
__device__ __forceinline__ typename Vec<V>::T ld(const float* p) {
    return *reinterpret_cast<const typename Vec<V>::T*>(p);
}
template <int V>
__device__ __forceinline__ void st(float* p, typename Vec<V>::T v) {
    *reinterpret_cast<typename Vec<V>::T*>(p) = v;
}

// (frame, column group) of this thread; false when it has none
__device__ __forceinline__ bool frame_col(int64_t n_frames, int groups, int64_t& f, int& c) {
    if (groups >= (int)blockDim.x) {   // wide rows: one frame per workgroup, the columns in strides of blockDim.x
        f = blockIdx.x / ((groups + blockDim.x - 1) / blockDim.x);
        c = (int)(blockIdx.x % ((groups + blockDim.x - 1) / blockDim.x)) * blockDim.x + threadIdx.x;
    } else {                           // narrow rows: blockDim.x / groups frames per workgroup
        const int fpb = blockDim.x / groups;
        const int lf = threadIdx.x / groups;
        if (lf >= fpb) return false;
        f = (int64_t)blockIdx.x * fpb + lf;
        c = threadIdx.x - lf * groups;
    }
    return f < n_frames && c < groups;
}

__device__ __forceinline__ float mask_count(const float* mask, int O) {
    float n = 0.f;
    for (int o = 0; o < O; ++o) n += mask[o];
    return fmaxf(n, 1.0f);
}

template <int V>
__global__ __launch_bounds__(256) void pool_fwd_kernel(const twog_entity_pool_t p) {
    typedef typename Vec<V>::T vt;
    const int W = p.W, groups = W / V;
    int64_t f;
    int c;
    if (!frame_col((int64_t)p.bs * p.T, groups, f, c)) return;
    const int j = c * V;
    const float* mask = p.mask + (f / p.T) * p.O;
    const float* hfr = p.hfr + f * p.H * W;
    const float* ofr = p.ofr + f * p.O * W;
    float* hin = p.hin + f * p.H * 2 * W;
    // objects -> humans: masked mean over the objects of the frame
    vt acc = Vec<V>::zero();
    for (int o = 0; o < p.O; ++o) acc += mask[o] * ld<V>(ofr + (int64_t)o * W + j);
    const vt pooled = acc / mask_count(mask, p.O);
    vt hsum = Vec<V>::zero();
    for (int h = 0; h < p.H; ++h) {
        const vt x = ld<V>(hfr + (int64_t)h * W + j);
        hsum += x;
        st<V>(hin + (int64_t)h * 2 * W + j, x);
        st<V>(hin + (int64_t)h * 2 * W + W + j, pooled);
    }
    if (p.oin) {   // humans -> objects: plain sum over the humans, every object (masked or not) receives it
        float* oin = p.oin + f * p.O * 2 * W;
        for (int o = 0; o < p.O; ++o) {
            st<V>(oin + (int64_t)o * 2 * W + j, ld<V>(ofr + (int64_t)o * W + j));
            st<V>(oin + (int64_t)o * 2 * W + W + j, hsum);
        }
    }
}

template <int V>
__global__ __launch_bounds__(256) void pool_bwd_kernel(const twog_entity_pool_bwd_t p) {
    typedef typename Vec<V>::T vt;
    const int W = p.W, groups = W / V;
    int64_t f;
    int c;
    if (!frame_col((int64_t)p.bs * p.T, groups, f, c)) return;
    const int j = c * V;
    const float* mask = p.mask + (f / p.T) * p.O;
    const float* dhin = p.d_hin + f * p.H * 2 * W;
    const float* doin = p.d_oin ? p.d_oin + f * p.O * 2 * W : nullptr;
    float* dhfr = p.d_hfr + f * p.H * W;
    float* dofr = p.d_ofr + f * p.O * W;
    // gradient of the broadcast halves: sum over the receivers, fixed order
    vt dpool = Vec<V>::zero();
    for (int h = 0; h < p.H; ++h) dpool += ld<V>(dhin + (int64_t)h * 2 * W + W + j);
    vt dhsum = Vec<V>::zero();
    if (doin)
        for (int o = 0; o < p.O; ++o) dhsum += ld<V>(doin + (int64_t)o * 2 * W + W + j);
    for (int h = 0; h < p.H; ++h) {
        vt d = ld<V>(dhin + (int64_t)h * 2 * W + j);
        if (doin) d += dhsum;
        st<V>(dhfr + (int64_t)h * W + j, d);
    }
    const float cnt = mask_count(mask, p.O);
    for (int o = 0; o < p.O; ++o) {
        vt d = (mask[o] / cnt) * dpool;
        if (doin) d += ld<V>(doin + (int64_t)o * 2 * W + j);
        st<V>(dofr + (int64_t)o * W + j, d);
    }
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline dim3 grid_of(int64_t n_frames, int groups) {
    if (groups >= 256) return dim3((unsigned)(n_frames * ((groups + 255) / 256)));
    const int fpb = 256 / groups;
    return dim3((unsigned)((n_frames + fpb - 1) / fpb));
}

}  // namespace

extern "C" int twog_entity_pool_fwd(const twog_entity_pool_t* p, void* stream) {
    if (!p || p->bs < 0 || p->T < 0 || p->H < 1 || p->O < 1 || p->W < 1 || !p->hfr || !p->ofr || !p->mask || !p->hin)
        return -1;
    const int64_t n_frames = (int64_t)p->bs * p->T;
    if (n_frames == 0) return 0;
    const bool vec = (p->W & 3) == 0 && al16(p->hfr) && al16(p->ofr) && al16(p->hin) && (!p->oin || al16(p->oin));
    if (vec) hipLaunchKernelGGL(pool_fwd_kernel<4>, grid_of(n_frames, p->W / 4), dim3(256), 0, (hipStream_t)stream, *p);
    else hipLaunchKernelGGL(pool_fwd_kernel<1>, grid_of(n_frames, p->W), dim3(256), 0, (hipStream_t)stream, *p);
    TWOG_CHECK_LAUNCH();
    return 0;
}

extern "C" int twog_entity_pool_bwd(const twog_entity_pool_bwd_t* p, void* stream) {
    if (!p || p->bs < 0 || p->T < 0 || p->H < 1 || p->O < 1 || p->W < 1 || !p->d_hin || !p->mask || !p->d_hfr || !p->d_ofr)
        return -1;
    const int64_t n_frames = (int64_t)p->bs * p->T;
    if (n_frames == 0) return 0;
    const bool vec = (p->W & 3) == 0 && al16(p->d_hin) && (!p->d_oin || al16(p->d_oin)) && al16(p->d_hfr) && al16(p->d_ofr);
    if (vec) hipLaunchKernelGGL(pool_bwd_kernel<4>, grid_of(n_frames, p->W / 4), dim3(256), 0, (hipStream_t)stream, *p);
    else hipLaunchKernelGGL(pool_bwd_kernel<1>, grid_of(n_frames, p->W), dim3(256), 0, (hipStream_t)stream, *p);
    TWOG_CHECK_LAUNCH();
    return 0;
}
