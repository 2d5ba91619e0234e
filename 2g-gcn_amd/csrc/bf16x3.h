// The bf16x3 arithmetic of the bf16 matrix-core paths (the X3 GEMMs of gemm_f32.hip, the persistent BiGRU of gru_persist.hip,
// the persistent segment recurrence of seg_persist.hip): one definition of the exact three-way split, of the six-product
// MFMA sequence built on it, and of the vector types and sc1 buffer accesses those kernels share.
//
// Every fp32 operand element is split EXACTLY into three bf16 values, x = h + m + l: h = x truncated to its top 8
// significant bits, m = (x - h) truncated, l = x - h - m (at most 8 significant bits are left: no rounding anywhere,
// the 24-bit significand is three 8-bit chunks). A product a b = sum of nine chunk products; the six with weight
// >= 2^-16 -- hh, hm, mh, mm, hl, lh -- run on v_mfma_f32_32x32x16_bf16 (bf16 x bf16 products are exact in the fp32
// accumulator); the three dropped ones (ml, lm, ll) are <= 2^-21 |a b| in the worst case and ~2^-24 |a b| on average,
// i.e. of the order of the rounding the fp32 accumulation applies to every partial sum anyway: measured against fp64
// products the kernel's error equals the native fp32-MFMA kernel's on every shape of tools/gemm_x3_bench.py (0.7-2.5e-6
// of the largest output for K = 512 ... 61 440); adding the two products m l and l m (exact to 2^-30) changes no digit of
// that error and costs 15 % (TWOG_X3_PRODUCTS=8 at build time; the shipped default is 6). The truncating split makes the
// dropped terms carry the sign of a b -- a bias towards zero of ~2^-24 |a b| per product, far below what the accumulate
// itself does (see TTMP in compute() of gemm_f32.hip). Six bf16 MFMAs of 16 k-steps cost 192 cycles per
// 32x32 block where the fp32 MFMA (32x32x2) needs 512: 2.67x the matrix rate for the same result to fp32 rounding.
#pragma once
#include "twog_common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((__vector_size__(4 * sizeof(unsigned))));

__device__ __forceinline__ uint32_t pack_hi16(uint32_t lo, uint32_t hi) {   // {hi[31:16], lo[31:16]}
    return __builtin_amdgcn_perm(hi, lo, 0x07060302);
}
// (Non-finite operands: NaN stays NaN; an operand of +-Inf gives NaN where an fp32 multiply would give +-Inf, because the
// split subtracts Inf - Inf. The path's GEMM operands are activations, weights and gradients -- finite in any run that is
// not already broken; the masked softmax's -inf lives inside the attention kernels, never in a GEMM operand.)
// four consecutive fp32 values -> their three bf16 planes (4 x 2 bytes each), by truncation: h = the top 8 significant bits,
// m = the top 8 of x - h, l = x - h - m. Exact (both subtractions are, and at most 8 significant bits are left for l), never
// overflows (a rounding split -- v_cvt_pk_bf16_f32 -- measured 5-8 % slower with the same end-to-end error).
__device__ __forceinline__ void split3(const f32x4 v, i32x2& ph, i32x2& pm, i32x2& pl) {
    uint32_t x[4], r1[4], r2[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float f0 = v[i];   // (a scalar copy: __builtin_bit_cast applied to the vector ELEMENT v[i] reads element 0)
        x[i] = __float_as_uint(f0);
        const float f1 = f0 - __uint_as_float(x[i] & 0xffff0000u);
        r1[i] = __float_as_uint(f1);
        r2[i] = __float_as_uint(f1 - __uint_as_float(r1[i] & 0xffff0000u));
    }
    ph = i32x2{(int)pack_hi16(x[0], x[1]), (int)pack_hi16(x[2], x[3])};
    pm = i32x2{(int)pack_hi16(r1[0], r1[1]), (int)pack_hi16(r1[2], r1[3])};
    pl = i32x2{(int)pack_hi16(r2[0], r2[1]), (int)pack_hi16(r2[2], r2[3])};
}

// eight consecutive fp32 values -> the three bf16 planes of an MFMA fragment (element j = value j), by truncation: exact.
// (Two functions for the two widths: an 8-wide split over a staged float[8], which a width-templated core would need, changes
// the register allocation of the persistent kernels.)
struct Planes { bf16x8 h, m, l; };
__device__ __forceinline__ Planes split8(const f32x4 a, const f32x4 b) {
    uint32_t x[8], r1[8], r2[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float f0 = i < 4 ? a[i] : b[i - 4];
        x[i] = __float_as_uint(f0);
        const float f1 = f0 - __uint_as_float(x[i] & 0xffff0000u);
        r1[i] = __float_as_uint(f1);
        r2[i] = __float_as_uint(f1 - __uint_as_float(r1[i] & 0xffff0000u));
    }
    Planes p;
    p.h = __builtin_bit_cast(bf16x8, i32x4{(int)pack_hi16(x[0], x[1]), (int)pack_hi16(x[2], x[3]), (int)pack_hi16(x[4], x[5]), (int)pack_hi16(x[6], x[7])});
    p.m = __builtin_bit_cast(bf16x8, i32x4{(int)pack_hi16(r1[0], r1[1]), (int)pack_hi16(r1[2], r1[3]), (int)pack_hi16(r1[4], r1[5]), (int)pack_hi16(r1[6], r1[7])});
    p.l = __builtin_bit_cast(bf16x8, i32x4{(int)pack_hi16(r2[0], r2[1]), (int)pack_hi16(r2[2], r2[3]), (int)pack_hi16(r2[4], r2[5]), (int)pack_hi16(r2[6], r2[7])});
    return p;
}

struct Acc { f32x4 hi, lo; };
__device__ __forceinline__ void acc_zero(Acc& c) { c.hi = f32x4{0.f, 0.f, 0.f, 0.f}; c.lo = f32x4{0.f, 0.f, 0.f, 0.f}; }
// c += A B with A, B given as planes: h.h into `hi`, the five small products into `lo`
__device__ __forceinline__ void mac6(Acc& c, const Planes& a, const Planes& b) {
    c.hi = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.h, b.h, c.hi, 0, 0, 0);
    c.lo = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.h, b.m, c.lo, 0, 0, 0);
    c.lo = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.m, b.h, c.lo, 0, 0, 0);
    c.lo = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.m, b.m, c.lo, 0, 0, 0);
    c.lo = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.h, b.l, c.lo, 0, 0, 0);
    c.lo = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.l, b.h, c.lo, 0, 0, 0);
}

// the same six products into ONE accumulator
__device__ __forceinline__ void mac6_one(f32x4& c, const Planes& a, const Planes& b) {
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.h, b.h, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.h, b.m, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.m, b.h, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.m, b.m, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.h, b.l, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.l, b.h, c, 0, 0, 0);
}

// 16-byte buffer accesses with sc1 (write-through stores / L2-served loads): the hand-offs of the persistent launches
constexpr int SC1 = 16;          // aux bits of the buffer instructions: sc1
__device__ __forceinline__ f32x4 ld_sc1(const __amdgpu_buffer_rsrc_t rs, uint32_t byte_off) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)byte_off, 0, SC1));
}
__device__ __forceinline__ void st_sc1(const __amdgpu_buffer_rsrc_t rs, uint32_t byte_off, const f32x4 v) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rs, (int)byte_off, 0, SC1);
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc_of(const float* p) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p), 0, 0xffffffff, 0x00020000);
}
