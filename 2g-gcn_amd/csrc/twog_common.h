// Shared device helpers for the gfx950 kernels of the 2G-GCN hot path.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include <cstdlib>
#include "../../include/twog_gcn.h"

#define TWOG_WAVE 64

typedef float f32x4 __attribute__((ext_vector_type(4)));  // native vector: loads/stores stay in registers (SROA)

#define TWOG_CHECK_LAUNCH()                         \
    do {                                            \
        hipError_t e_ = hipGetLastError();          \
        if (e_ != hipSuccess) return -(int)e_;      \
    } while (0)

// An integer switch of the environment: atoi of the variable when it is set (set but empty reads as 0), dflt when it is not.
// Reads on every call; a site that wants one reading per process keeps the result in a `static const`.
inline int twog_env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}

// compute units of the current device
inline hipError_t twog_device_cus(int* n) {
    int dev = 0;
    const hipError_t e = hipGetDevice(&dev);
    return e != hipSuccess ? e : hipDeviceGetAttribute(n, hipDeviceAttributeMultiprocessorCount, dev);
}

// Raises a kernel's dynamic-LDS limit once per device (function attributes are per device; the flag word is one bit per
// device ordinal, so a process that drives several GPUs -- or several host threads -- stays correct).
template <class K>
inline void twog_allow_dynamic_lds(K kernel, int bytes, std::atomic<uint32_t>& done) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); dev = 0; }
    const uint32_t bit = 1u << (dev & 31);
    if (done.load(std::memory_order_acquire) & bit) return;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    done.fetch_or(bit, std::memory_order_release);
}

// library-internal (gemm_f32.hip): grouped C += A B launch whose epilogue runs the GRU gate backward of the next chain step
// chain_ws / chain_ws_bytes: the chain workspace of twog_gemm_f32_chain (NULL: the reduction is never split over workgroups)
int twog_internal_gemm_gate_bwd(const twog_gemm_t* problems, int n, const twog_gru_step_bwd_t* gates,
                                float* const* du_part, int dry_run, void* chain_ws, size_t chain_ws_bytes, void* stream);

// library-internal (gemm_f32.hip): one launch for the W_hh (and message) products of a forward chain step AND its gates
int twog_internal_gemm_gru_fwd(const twog_gemm_t* gh, const twog_gemm_t* gim, const twog_gru_step_t* steps, int n,
                               int dry_run, void* stream);

int twog_internal_gru_fwd_mode(void);   // TWOG_GRU_FWD_FUSION (part of the chains' hipGraph keys: it changes what is captured)

// library-internal: the launch geometry of the geometric-level GCN kernels, out = {grid, frames per group, dynamic LDS bytes,
// variant}. The launchers launch with exactly these numbers and twog_gcn_launch_plan (geo_gcn.hip) reports them; < 0 = the
// launcher's own error code. geo_fused.hip / geo_attn_mfma.hip (kernel = TWOG_GCN_PLAN_ATTN2_FWD or _BWD) / geo_gcn.hip.
int twog_internal_plan_fused_fwd(int n_frames, int n_nodes, int out[4]);
int twog_internal_plan_attn2(int kernel, int n_frames, int n_nodes, int out[4]);

// the wide family of the geometric-level GCN (geo_wide.hip; its per-row kernels are the second instantiation of geo_gcn.hip's)
constexpr int TWOG_GCN_WIDE_MAX_NODES = 256;
int twog_internal_embed1_fwd_grid(int64_t rows);   // geo_gcn.hip: the grid of embed1_fwd_kernel, for both families

// The capped grid of a grid-stride streaming kernel (TWOG_STREAM_* of include/twog_gcn.h) for `work` items: the launchers of
// misc.hip / gate.hip / posfeat.hip launch with exactly this number and twog_stream_grid (misc.hip) reports it. -2 = unknown.
inline int twog_stream_blocks(int kernel, int64_t work) {
    if (work < 0) return -2;
    int64_t items = work, cap;
    switch (kernel) {
        case TWOG_STREAM_RELU_BWD_VEC: items = work / 4; cap = 4096; break;
        case TWOG_STREAM_RELU_BWD:
        case TWOG_STREAM_ADD_ROWS:
        case TWOG_STREAM_RANK1: cap = 4096; break;
        case TWOG_STREAM_RANK1_VEC: items = work / 4; cap = 8192; break;
        case TWOG_STREAM_ROWOPS: cap = 1024; break;
        case TWOG_STREAM_ADAM: cap = 2048; break;
        case TWOG_STREAM_MUL:
        case TWOG_STREAM_SCALE_ROWS: cap = 8192; break;
        case TWOG_STREAM_COPY_BLOCKS: items = (work + 3) / 4; cap = 512; break;
        case TWOG_STREAM_FILL_ZERO: items = work / 16; cap = 4096; break;
        case TWOG_STREAM_OPTIM: items = work / 4; cap = 2048; break;   // 8 workgroups per CU, one float4 of each buffer per thread and trip
        default: return -2;
    }
    int64_t g = (items + TWOG_STREAM_THREADS - 1) / TWOG_STREAM_THREADS;
    if (g > cap) g = cap;
    return (int)(g < 1 ? 1 : g);
}

// address of row r in a twog_rows_t (see include/twog_gcn.h)
__device__ __forceinline__ int64_t twog_row_off(const twog_rows_t& m, int r) {
    if (m.inner <= 1) return (int64_t)r * m.ld_outer;
    const int o = r / m.inner;
    return (int64_t)o * m.ld_outer + (int64_t)(r - o * m.inner) * m.ld_inner;
}
__device__ __forceinline__ float* twog_row_ptr(const twog_rows_t& m, int r) { return m.ptr + twog_row_off(m, r); }
// host: every row of m starts on 16 bytes, what the kernels with 16-byte accesses ask of an operand. An absent operand
// (null pointer) passes.
inline bool twog_rows_on_16_bytes(const twog_rows_t& m) {
    if (!m.ptr) return true;
    return (reinterpret_cast<uintptr_t>(m.ptr) & 15) == 0 && (m.ld_outer & 3) == 0 && (m.inner <= 1 || (m.ld_inner & 3) == 0);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// block-wide sum for blockDim.x a multiple of 64, <= 1024; `red` is >= 16 floats of LDS. All threads get the result.
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    float t = 0.f;
    for (int i = 0; i < nw; ++i) t += red[i];
    return t;
}

// v of lane `lane` (wave-uniform, a constant where the loop around it is unrolled) in every lane: one v_readlane
__device__ __forceinline__ float lane_value(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// The NLL terms' rule: a label takes part when it is not the ignore value and names a class. The criterion, the smoothing
// and CRF losses and the count kernels all keep or drop a label by this one test.
__device__ __forceinline__ bool twog_label_kept(int64_t y, int64_t ignore, int n_classes) {
    return y != ignore && y >= 0 && y < n_classes;
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + __expf(-x)); }
