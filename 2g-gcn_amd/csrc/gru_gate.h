// The element-wise GRU step (gates r, z, n, the blend with h_prev, the segment gate u) and its backward: ONE definition for
// every kernel that runs it -- the step kernels of gru.hip, the fused epilogues of gemm_f32.hip and the persistent launches
// of gru_persist.hip and seg_persist.hip. torch.nn.GRU's gate order r, z, n; h = u * GRUCell(x, h_prev) + (1 - u) * h_prev.
//
// Why the rounding is written out. The step contains sums of two products: (1 - z) n + z h0, u g + (1 - u) h0 and, backward,
// (1 - u) d + (u d) z. Left to the compiler each of them becomes an fma on the first product, an fma on the second, or two
// rounded products and an add, depending on the code AROUND the expression (the vectorizer packs two multiplies into a
// v_pk_mul_f32, which no longer contracts with the add); the kernels then disagree in the last bit. Here every multiply-add
// is an explicit fmaf or rounded separately (contraction off), chosen by a template argument, and a caller gets the same bits
// wherever it is inlined. The kernels do NOT all round alike: each named variant below is what the compiler had made of one
// site before the sites shared this header (read off the gfx950 assembly), kept so that no result changed. A new fused gate
// site calls one of them; it does not copy the expressions.
#pragma once
#include "twog_common.h"

// a * b + c * d: how many roundings, and which product is the exact one inside the fma
enum class MulAdd {
    rounded,  // round(round(a b) + round(c d))
    fma_ab,   // fma(a, b, round(c d))
    fma_cd,   // fma(c, d, round(a b))
};
template <MulAdd R>
__device__ __forceinline__ float mul_add2(float a, float b, float c, float d) {
#pragma clang fp contract(off)
    if constexpr (R == MulAdd::fma_ab) return fmaf(a, b, c * d);
    else if constexpr (R == MulAdd::fma_cd) return fmaf(c, d, a * b);
    else return a * b + c * d;
}

// ---- forward. ir / iz / in_: the input-side sums (W_ih x + b_ih, plus the message products where there are any); hr / hz /
// hn: the hidden-side sums (W_hh h_prev + b_hh). hn is handed back as it came: the backward pass wants it saved next to the gates.
// n = tanh(fma(rg, hn, in_)) in every variant. G rounds (1 - z) n + z h0, U rounds u g + (1 - u) h0 (has_u only).
struct GruFwdUnit { float h, rg, z, n, hn; };
template <class R>
__device__ __forceinline__ GruFwdUnit gru_fwd_unit(float ir, float iz, float in_, float hr, float hz, float hn, float h0, float uu,
                                                  bool has_u) {
#pragma clang fp contract(off)
    GruFwdUnit e;
    e.rg = 1.0f / (1.0f + expf(-(ir + hr)));
    e.z = 1.0f / (1.0f + expf(-(iz + hz)));
    e.n = tanhf(fmaf(e.rg, hn, in_));
    e.hn = hn;
    const float gnew = mul_add2<R::G>(1.0f - e.z, e.n, e.z, h0);
    e.h = has_u ? mul_add2<R::U>(uu, gnew, 1.0f - uu, h0) : gnew;
    return e;
}
// The variants. A name spells, for G and then U, the product that stays exact inside an fma: Zn = (1 - z) n, Zh = z h0,
// Ug = u g, Uh = (1 - u) h0; Rounded = two rounded products and an add.
// gru_step_fwd_kernel and gru_step_fwd_vec_kernel (gru.hip)
struct GruFwdZhUg { static constexpr MulAdd G = MulAdd::fma_cd, U = MulAdd::fma_ab; };
// both epilogues of gemm_gru_fwd_kernel (gemm_f32.hip) and bigru_persist_fwd_kernel (gru_persist.hip): the compiler had
// packed the products of both blends
struct GruFwdRounded { static constexpr MulAdd G = MulAdd::rounded, U = MulAdd::rounded; };
// p2_step of seg_persist.hip, a lane's four units: the compiler had packed the u products of units 0 and 1 and contracted
// those of units 2 and 3. Both forms are kept, by unit, because the states of a whole sequence depend on them.
struct GruFwdZnRounded { static constexpr MulAdd G = MulAdd::fma_ab, U = MulAdd::rounded; };
struct GruFwdZnUh { static constexpr MulAdd G = MulAdd::fma_ab, U = MulAdd::fma_cd; };

// ---- backward. d: the gradient arriving at h; rg, z, n, hn: what the forward step saved; h0 the previous state.
// dr_pre / dz_pre / dn_pre: gradients of the three pre-activations on the input side (d_gi), the hidden side (d_gh) takes
// dr_pre, dz_pre and dn_rg = dn_pre * rg; dprev: the direct path into h_prev; du: d * (g - h0), the gradient of the segment gate.
// 1 - n n is fma(-n, n, 1) in every variant. G rounds g = (1 - z) n + z h0 (read by du alone); P rounds dprev =
// (u d) z + (1 - u) d, a = (u d, z), c = (1 - u, d), without u: (u d) z + 0 under rounded and fma_ab; DU_FMA: du is
// fma(d, g - h0, du_acc), the site's running sum; otherwise the rounded product (du_acc is not read).
// A site without u passes has_u = false as a constant and ignores du: the compiler drops what only du reads.
struct GruBwdUnit { float dr_pre, dz_pre, dn_pre, dn_rg, dprev, du; };
template <class R>
__device__ __forceinline__ GruBwdUnit gru_bwd_unit(float d, float rg, float z, float n, float hn, float h0, float uu, bool has_u,
                                                  float du_acc = 0.f) {
#pragma clang fp contract(off)
    GruBwdUnit e;
    const float gnew = mul_add2<R::G>(1.0f - z, n, z, h0);
    e.du = R::DU_FMA ? fmaf(d, gnew - h0, du_acc) : d * (gnew - h0);
    const float dg = has_u ? uu * d : d;
    if constexpr (R::P == MulAdd::fma_cd) e.dprev = has_u ? fmaf(1.0f - uu, d, dg * z) : dg * z;
    else {
        const float dskip = has_u ? (1.0f - uu) * d : 0.f;
        e.dprev = R::P == MulAdd::fma_ab ? fmaf(dg, z, dskip) : dskip + dg * z;
    }
    const float dn = dg * (1.0f - z);
    const float dz = dg * (h0 - n);
    e.dn_pre = dn * fmaf(-n, n, 1.0f);
    e.dr_pre = e.dn_pre * hn * rg * (1.0f - rg);
    e.dz_pre = dz * z * (1.0f - z);
    e.dn_rg = e.dn_pre * rg;
    return e;
}
// The variants. A name spells, for G and then P, the product that stays exact inside an fma: Zn = (1 - z) n, Zh = z h0,
// Dz = (u d) z, Ud = (1 - u) d; Rounded as above; Sum: du is the running sum (DU_FMA).
// gru_step_bwd_kernel (gru.hip). bigru_persist_bwd_kernel (gru_persist.hip) calls it too: it has no u and reads the three
// pre-activation gradients only (its direct path d z is fused into the carry's sum there).
struct GruBwdZnDzSum { static constexpr MulAdd G = MulAdd::fma_ab, P = MulAdd::fma_ab; static constexpr bool DU_FMA = true; };
// the dword gate epilogue of gemm_tile (gemm_f32.hip): du is a product, the row sums are taken by shuffles
struct GruBwdZnDz { static constexpr MulAdd G = MulAdd::fma_ab, P = MulAdd::fma_ab; static constexpr bool DU_FMA = false; };
// the 16-byte gate epilogue of gemm_tile: the compiler had packed the products of dprev. The same bits as GruBwdZnDz where u is
// absent, 0 or 1 (with (1 - u) d or (u d) z zero the fma rounds once, like the add); tests/test_chain_epilogue_vec_gpu.py
// compares the two epilogues bit for bit at such gates.
struct GruBwdZnRounded { static constexpr MulAdd G = MulAdd::fma_ab, P = MulAdd::rounded; static constexpr bool DU_FMA = false; };
// bwd_step of seg_persist.hip
struct GruBwdZhUdSum { static constexpr MulAdd G = MulAdd::fma_cd, P = MulAdd::fma_cd; static constexpr bool DU_FMA = true; };
