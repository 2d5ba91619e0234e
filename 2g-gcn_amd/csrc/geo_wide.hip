// Geometric-level GCN for 1 <= n_nodes <= 256: the wide kernel family ("complete, not tuned"; the tuned kernels of
// geo_fused.hip / geo_attn_mfma.hip stop at 64 nodes because a receiver's score row lives in four accumulator tiles there and
// the backward kernel keeps three N x N planes of a frame in LDS).
//
// Reference: Geo_gcn.forward (pyrutils/torch/models_gcn.py:30-37) = norm_data (:45-50), embed (:72-74, :57-63),
// compute_similarity (:95-100) with the two projections folded (P = X M + d, see geo_attn_mfma.hip) and the adjacency
// product (:33-34). Exact fp32 on v_mfma_f32_16x16x4_f32, the arithmetic of the tuned kernels.
//
// One frame per workgroup trip, 8 waves. The frame's X [NP][68] (NP = N rounded up to 16, the rows behind N exact zeros), Mt and
// d live in LDS; everything N x N exists only as strips of 16 receiver rows in the accumulators of ONE wave (up to 16 column
// tiles = 64 VGPRs) and travels tile by tile through a [16][20] staging area of that wave to reach the operand layout.
//   forward  A  X = relu(relu(W1 x^ + b1) W2^T + b2) of the frame's rows -> LDS (+ global), as phase A of geo_fused.hip
//            B  per strip: P rows -> scores over all column tiles -> row max / sum over all tiles in registers, 16-lane DPP
//               -> adjacency rows -> global; Z = S X tile by tile -> global
//   backward 1  per strip of receivers i: dA = dZ X^T tile by tile for t_i = sum_j S dA, the tiles again for dS = S (dA - t) and
//               dP = dS X, dX_i = dP Mt (to global), dMt += dP^T X_i and dd += colsum dP in the wave's registers; t -> LDS
//            2  per strip of senders j (the roles of rows and columns exchanged): over all row tiles i the dA tile again (the
//               same bits), S and dS tiles transposed through the staging area, dX_j += S^T dZ + (dS^T X) Mt + (colsum_i dS) d
//               [= dS^T P with P = X M + d not materialised]
//            the eight waves' dMt / dd meet in LDS in wave order: fixed summation order, no atomics, bit-reproducible.
// S, dZ rows needed as operands come straight from global memory (the frame's 64 KB + N^2 floats are L2-resident).
// MFMA ignores EXEC: short tiles are padded with zeros SELECTED into the operand, the wave / strip indices are scalar.
#include "twog_common.h"

namespace {

constexpr int LDK = 68;      // row stride of [row][64 features] LDS arrays (= 4 mod 16 words)
constexpr int LDT = 20;      // row stride of a wave's 16 x 16 staging tile
constexpr int NWAVES = 8;
constexpr int FWD_PRIV = 16 * LDK;                 // per wave: P rows / Z rows; the staging tile lies over it
constexpr int BWD_PRIV = 16 * LDK + 2 * 16 * LDT;  // per wave: dP (G) rows + two staging tiles
constexpr int MAX_GRID = 256;

__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
// the 64-deep operand fragment of geo_fused.hip: lane group g takes k = 16c + 4g + j for step 4c + j
__device__ __forceinline__ void frag64(const float* row, int g, float (&f)[16]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float4 v = *reinterpret_cast<const float4*>(row + 16 * c + 4 * g);
        f[4 * c] = v.x; f[4 * c + 1] = v.y; f[4 * c + 2] = v.z; f[4 * c + 3] = v.w;
    }
}
__device__ __forceinline__ void frag64_or_zero(const float* row, bool on, int g, float (&f)[16]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (on) v = *reinterpret_cast<const float4*>(row + 16 * c + 4 * g);
        f[4 * c] = v.x; f[4 * c + 1] = v.y; f[4 * c + 2] = v.z; f[4 * c + 3] = v.w;
    }
}
__device__ __forceinline__ f32x4 mm64(const float (&a)[16], const float (&b)[16], f32x4 acc) {
#pragma unroll
    for (int i = 0; i < 16; ++i) acc = mfma16(a[i], b[i], acc);
    return acc;
}
template <int CTRL>
__device__ __forceinline__ float dpp_ror(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ float max16(float v) {
    v = fmaxf(v, dpp_ror<0x128>(v));
    v = fmaxf(v, dpp_ror<0x124>(v));
    v = fmaxf(v, dpp_ror<0x122>(v));
    v = fmaxf(v, dpp_ror<0x121>(v));
    return v;
}
__device__ __forceinline__ float sum16(float v) {
    v += dpp_ror<0x128>(v);
    v += dpp_ror<0x124>(v);
    v += dpp_ror<0x122>(v);
    v += dpp_ror<0x121>(v);
    return v;
}

// S[row][col] of the frame at row r0, exact zero for padding rows / columns: the address is clamped into the frame and the value
// selected, so the load sits in no branch
__device__ __forceinline__ float adj_or_zero(const float* adj, int64_t r0, int row, int col, int N) {
    const float v = adj[(r0 + min(row, N - 1)) * N + min(col, N - 1)];
    return (row < N && col < N) ? v : 0.f;
}

// stage Mt [64][LDK] and d [64] of md [65][64]
__device__ __forceinline__ void stage_md(const float* md, float* sMt, float* sd) {
    for (int i = threadIdx.x; i < 64 * 16; i += blockDim.x) {
        const int r = i >> 4, c = (i & 15) * 4;
        *reinterpret_cast<float4*>(sMt + r * LDK + c) = *reinterpret_cast<const float4*>(md + r * 64 + c);
    }
    if (threadIdx.x < 64) sd[threadIdx.x] = md[64 * 64 + threadIdx.x];
}

// NTC: column tiles a strip can hold in its accumulators (4, 8, 12 or 16); nt = ceil(N / 16) <= NTC of them are computed
template <int NTC>
__global__ __launch_bounds__(64 * NWAVES, 1) void gcn_wide_fwd_kernel(const float* x, int64_t fstride, int n_frames, int N,
                                                                      const float* ab, const float* w1, const float* b1,
                                                                      const float* w2, const float* b2, const float* md,
                                                                      float* xout, float* adj, float* z) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int nt = (N + 15) >> 4, NP = nt * 16, nch = 4 * N;
    float* sMt = sm;                  // [64][LDK]
    float* sd = sMt + 64 * LDK;       // [64]
    float* sb2 = sd + 64;             // [64]
    float* sw1 = sb2 + 64;            // [64][4]
    float* sb1 = sw1 + 256;           // [64]
    float* sX = sb1 + 64;             // [NP][LDK]
    const int lane = threadIdx.x & 63, i16 = lane & 15, g = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float* priv = sX + NP * LDK + wv * FWD_PRIV;
    stage_md(md, sMt, sd);
    if (threadIdx.x < 64) {
        sb2[threadIdx.x] = b2[threadIdx.x];
        sb1[threadIdx.x] = b1[threadIdx.x];
        *reinterpret_cast<float4*>(sw1 + threadIdx.x * 4) = *reinterpret_cast<const float4*>(w1 + threadIdx.x * 4);
    }
    const int c0 = (wv & 1) * 2;
    for (int f = blockIdx.x; f < n_frames; f += gridDim.x) {
        const int64_t r0 = (int64_t)f * N;
        __syncthreads();   // the previous frame is done with sX; first trip: the weights are staged
        // ---- A: X of the frame; item = (16-row tile, pair of 16-column tiles). Rows N .. NP-1 become exact zeros.
        for (int rt = wv >> 1; rt < nt; rt += NWAVES / 2) {
            const int n = rt * 16 + i16;
            float4 xh = make_float4(0.f, 0.f, 0.f, 0.f);
            if (n < N) {   // (the fused multiply-adds of embed1_fwd_kernel, geo_gcn.hip: the backward pass recomputes e1 there)
                const float4 v = *reinterpret_cast<const float4*>(x + (int64_t)f * fstride + n * 4);
                xh.x = fmaf(ab[n], v.x, ab[nch + n]);
                xh.y = fmaf(ab[N + n], v.y, ab[nch + N + n]);
                xh.z = fmaf(ab[2 * N + n], v.z, ab[nch + 2 * N + n]);
                xh.w = fmaf(ab[3 * N + n], v.w, ab[nch + 3 * N + n]);
            }
            float ae[16];
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) {
                const int k = 16 * (kk >> 2) + 4 * g + (kk & 3);
                const float4 w = *reinterpret_cast<const float4*>(sw1 + k * 4);
                float acc = sb1[k];
                acc = fmaf(w.x, xh.x, acc);
                acc = fmaf(w.y, xh.y, acc);
                acc = fmaf(w.z, xh.z, acc);
                acc = fmaf(w.w, xh.w, acc);
                ae[kk] = fmaxf(acc, 0.f);
            }
#pragma unroll
            for (int cc = 0; cc < 2; ++cc) {
                const int ct = c0 + cc;
                float bf[16];
                frag64(w2 + (ct * 16 + i16) * 64, g, bf);
                const f32x4 acc = mm64(ae, bf, f32x4{0.f, 0.f, 0.f, 0.f});
                const int col = ct * 16 + i16;
                const float bias = sb2[col];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = rt * 16 + 4 * g + r;
                    sX[row * LDK + col] = row < N ? fmaxf(acc[r] + bias, 0.f) : 0.f;
                }
            }
        }
        __syncthreads();
        if (xout) {
            for (int i = threadIdx.x; i < N * 16; i += blockDim.x) {
                const int r = i >> 4, c = (i & 15) * 4;
                *reinterpret_cast<float4*>(xout + (r0 + r) * 64 + c) = *reinterpret_cast<const float4*>(sX + r * LDK + c);
            }
        }
        // ---- B: a strip of 16 receivers from start to end in one wave; the only LDS it writes is its own scratch
        for (int rt = wv; rt < nt; rt += NWAVES) {
            const int base = rt * 16;
            {   // P = X M + d of the strip -> scratch [16][LDK]
                float af[16];
                frag64(sX + (base + i16) * LDK, g, af);
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) {
                    float bf[16];
                    frag64(sMt + (ct * 16 + i16) * LDK, g, bf);
                    const f32x4 acc = mm64(af, bf, f32x4{0.f, 0.f, 0.f, 0.f});
                    const int col = ct * 16 + i16;
                    const float dv = sd[col];
#pragma unroll
                    for (int r = 0; r < 4; ++r) priv[(4 * g + r) * LDK + col] = acc[r] + dv;
                }
            }
            f32x4 sc[NTC];
            {
                float af[16];
                frag64(priv + i16 * LDK, g, af);
#pragma unroll
                for (int ct = 0; ct < NTC; ++ct) {
                    sc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (ct < nt) {
                        float bf[16];
                        frag64(sX + (ct * 16 + i16) * LDK, g, bf);
                        sc[ct] = mm64(af, bf, sc[ct]);
                    }
                }
            }
            // row softmax over the N real columns of ALL tiles: row 4g + r lives on the 16 lanes of group g, one column per lane
            // and tile. Padding columns take no part in the max or the sum and become exact zeros.
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float m = -INFINITY;
#pragma unroll
                for (int ct = 0; ct < NTC; ++ct)
                    if (ct < nt && ct * 16 + i16 < N) m = fmaxf(m, sc[ct][r]);
                m = max16(m);
                float s = 0.f;
#pragma unroll
                for (int ct = 0; ct < NTC; ++ct) {
                    const float e = (ct < nt && ct * 16 + i16 < N) ? __expf(sc[ct][r] - m) : 0.f;
                    sc[ct][r] = e;
                    s += e;
                }
                const float inv = 1.0f / sum16(s);
#pragma unroll
                for (int ct = 0; ct < NTC; ++ct) sc[ct][r] *= inv;
            }
            // adjacency rows -> global (16 lanes write 64 contiguous bytes of a row); Z = S X tile by tile: the tile goes through
            // the staging area (P is dead) from the accumulator layout [row 4g + r][col i16] to the operand layout [row i16][k]
            f32x4 zc[4];
#pragma unroll
            for (int oc = 0; oc < 4; ++oc) zc[oc] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ct = 0; ct < NTC; ++ct) {
                if (ct < nt) {
                    const int col = ct * 16 + i16;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = base + 4 * g + r;
                        if (row < N && col < N) adj[(r0 + row) * N + col] = sc[ct][r];
                        priv[(4 * g + r) * LDT + i16] = sc[ct][r];
                    }
                    float sa[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) sa[j] = priv[i16 * LDT + g + 4 * j];
                    // (rows N .. NP-1 of sX are exact zeros and so are the padding columns of S: nothing to select here)
#pragma unroll
                    for (int oc = 0; oc < 4; ++oc) {
                        const float* pb = sX + (ct * 16 + g) * LDK + oc * 16 + i16;
#pragma unroll
                        for (int j = 0; j < 4; ++j) zc[oc] = mfma16(sa[j], pb[j * 4 * LDK], zc[oc]);
                    }
                }
            }
#pragma unroll
            for (int oc = 0; oc < 4; ++oc)
#pragma unroll
                for (int r = 0; r < 4; ++r) priv[(4 * g + r) * LDK + oc * 16 + i16] = zc[oc][r];
            const int nr = min(16, N - base);
            float* dst = z + (r0 + base) * 64;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = lane + 64 * j, r = i >> 4, c = (i & 15) * 4;
                if (r < nr) *reinterpret_cast<float4*>(dst + r * 64 + c) = *reinterpret_cast<const float4*>(priv + r * LDK + c);
            }
        }
    }
}

// Backward per frame (dZ given):  dA = dZ X^T;  dS = S o (dA - rowsum(S o dA));  dP = dS X;
//   dX = S^T dZ + dS^T P + dP Mt;   dMt += dP^T X;   dd += colsum(dP)       (P = X M + d, used as (dS^T X) Mt + colsum(dS) d)
__global__ __launch_bounds__(64 * NWAVES, 1) void gcn_wide_bwd_kernel(const float* xin, const float* md, const float* adj,
                                                                      const float* dz, int n_frames, int N, float* dx,
                                                                      float* partials) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int nt = (N + 15) >> 4, NP = nt * 16;
    float* sMt = sm;                  // [64][LDK]   (at the end: the sum of the waves' dMt)
    float* sd = sMt + 64 * LDK;       // [64]        (at the end: the sum of the waves' dd)
    float* st = sd + 64;              // [256]  t_i = sum_j S_ij dA_ij
    float* sX = st + TWOG_GCN_WIDE_MAX_NODES;   // [NP][LDK]
    const int lane = threadIdx.x & 63, i16 = lane & 15, g = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float* rowsP = sX + NP * LDK + wv * BWD_PRIV;   // [16][LDK]: dP rows (pass 1), G rows (pass 2)
    float* tA = rowsP + 16 * LDK;                   // [16][LDT] staging tile
    float* tB = tA + 16 * LDT;                      // [16][LDT] staging tile
    stage_md(md, sMt, sd);
    f32x4 accM[16];   // this wave's share of dMt: tile (n tile, k tile) = accM[4 nt + kt]
#pragma unroll
    for (int u = 0; u < 16; ++u) accM[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    float dd_acc = 0.f;   // lane n: this wave's share of dd[n]
    for (int f = blockIdx.x; f < n_frames; f += gridDim.x) {
        const int64_t r0 = (int64_t)f * N;
        __syncthreads();
        for (int i = threadIdx.x; i < NP * 16; i += blockDim.x) {   // X of the frame, rows N .. NP-1 zero
            const int r = i >> 4, c = (i & 15) * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < N) v = *reinterpret_cast<const float4*>(xin + (r0 + r) * 64 + c);
            *reinterpret_cast<float4*>(sX + r * LDK + c) = v;
        }
        __syncthreads();
        // ---- pass 1: strips of receivers
        for (int it = wv; it < nt; it += NWAVES) {
            const int base = it * 16;
            // The strip's N x N rows are never held: a first sweep over the column tiles computes the dA tiles for t_i alone, a
            // second one computes them again (same operands, same order: same bits), forms dS and feeds it to dP = dS X through
            // the staging area. (Keeping 16 tiles = 64 VGPRs beside the 64 of dMt spills.) S of padding rows / columns is
            // selected to zero, so dS is zero there.
            float af[16];
            frag64_or_zero(dz + (r0 + base + i16) * 64, base + i16 < N, g, af);
            float tr[4] = {0.f, 0.f, 0.f, 0.f};
            for (int ct = 0; ct < nt; ++ct) {
                float bf[16];
                frag64(sX + (ct * 16 + i16) * LDK, g, bf);
                const f32x4 da = mm64(af, bf, f32x4{0.f, 0.f, 0.f, 0.f});
                const int col = ct * 16 + i16;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = base + 4 * g + r;
                    const float sv = adj_or_zero(adj, r0, row, col, N);
                    tr[r] = fmaf(sv, da[r], tr[r]);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                tr[r] = sum16(tr[r]);
                if (i16 == 0) st[base + 4 * g + r] = tr[r];
            }
            f32x4 dp[4];
#pragma unroll
            for (int oc = 0; oc < 4; ++oc) dp[oc] = f32x4{0.f, 0.f, 0.f, 0.f};
            for (int ct = 0; ct < nt; ++ct) {
                float bf[16];
                frag64(sX + (ct * 16 + i16) * LDK, g, bf);
                const f32x4 da = mm64(af, bf, f32x4{0.f, 0.f, 0.f, 0.f});
                const int col = ct * 16 + i16;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = base + 4 * g + r;
                    const float sv = adj_or_zero(adj, r0, row, col, N);
                    tA[(4 * g + r) * LDT + i16] = sv * (da[r] - tr[r]);
                }
                float sa[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) sa[j] = tA[i16 * LDT + g + 4 * j];
#pragma unroll
                for (int oc = 0; oc < 4; ++oc) {
                    const float* pb = sX + (ct * 16 + g) * LDK + oc * 16 + i16;
#pragma unroll
                    for (int j = 0; j < 4; ++j) dp[oc] = mfma16(sa[j], pb[j * 4 * LDK], dp[oc]);
                }
            }
#pragma unroll
            for (int oc = 0; oc < 4; ++oc)
#pragma unroll
                for (int r = 0; r < 4; ++r) rowsP[(4 * g + r) * LDK + oc * 16 + i16] = dp[oc][r];
            {   // dX_i = dP Mt (the rest is added in pass 2 by the same lanes): k = n runs in the fragment order of frag64
                float af[16];
                frag64(rowsP + i16 * LDK, g, af);
#pragma unroll
                for (int oc = 0; oc < 4; ++oc) {
                    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int kk = 0; kk < 16; ++kk) {
                        const int k = 16 * (kk >> 2) + 4 * g + (kk & 3);
                        acc = mfma16(af[kk], sMt[k * LDK + oc * 16 + i16], acc);
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = base + 4 * g + r;
                        if (row < N) dx[(r0 + row) * 64 + oc * 16 + i16] = acc[r];
                    }
                }
            }
            // dMt += dP^T X_i (k = the strip's 16 receivers; padding rows of dP and of sX are exact zeros); dd += colsum dP
#pragma unroll
            for (int nt4 = 0; nt4 < 4; ++nt4) {
                float a[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) a[j] = rowsP[(g + 4 * j) * LDK + nt4 * 16 + i16];
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) {
                    const float* pb = sX + (base + g) * LDK + kt * 16 + i16;
#pragma unroll
                    for (int j = 0; j < 4; ++j) accM[nt4 * 4 + kt] = mfma16(a[j], pb[j * 4 * LDK], accM[nt4 * 4 + kt]);
                }
            }
            {
                float s = 0.f;
#pragma unroll
                for (int i = 0; i < 16; ++i) s += rowsP[i * LDK + lane];
                dd_acc += s;
            }
        }
        __syncthreads();   // t of every receiver is in LDS
        // ---- pass 2: strips of senders j; the tile (i tile, j strip) of dA is computed again (same operands, same order: same bits)
        for (int jt = wv; jt < nt; jt += NWAVES) {
            const int jbase = jt * 16, col = jbase + i16;
            float bx[16];
            frag64(sX + (jbase + i16) * LDK, g, bx);
            f32x4 acc1[4], accG[4];
#pragma unroll
            for (int oc = 0; oc < 4; ++oc) acc1[oc] = accG[oc] = f32x4{0.f, 0.f, 0.f, 0.f};
            float csp = 0.f;   // this lane's share of colsum_i dS[i][col]
            for (int it = 0; it < nt; ++it) {
                const int ibase = it * 16;
                float af[16];
                frag64_or_zero(dz + (r0 + ibase + i16) * 64, ibase + i16 < N, g, af);
                const f32x4 da = mm64(af, bx, f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = ibase + 4 * g + r;
                    const float sv = adj_or_zero(adj, r0, row, col, N);
                    const float ds = sv * (da[r] - st[row]);
                    tA[(4 * g + r) * LDT + i16] = sv;
                    tB[(4 * g + r) * LDT + i16] = ds;
                    csp += ds;
                }
                // operands S^T, dS^T: [row j = i16][k = i = g + 4 j4]
                float aS[4], aD[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    aS[j] = tA[(g + 4 * j) * LDT + i16];
                    aD[j] = tB[(g + 4 * j) * LDT + i16];
                }
#pragma unroll
                for (int oc = 0; oc < 4; ++oc) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int irow = ibase + g + 4 * j;
                        // dZ rows behind the frame belong to the next frame: selected to zero, not multiplied by a zero weight (the
                        // load itself is clamped into the frame, so that it needs no branch and the loads of a tile go out together)
                        const float bzl = dz[(r0 + min(irow, N - 1)) * 64 + oc * 16 + i16];
                        const float bz = irow < N ? bzl : 0.f;
                        acc1[oc] = mfma16(aS[j], bz, acc1[oc]);
                        accG[oc] = mfma16(aD[j], sX[irow * LDK + oc * 16 + i16], accG[oc]);
                    }
                }
            }
            // colsum_i dS of the strip's 16 senders: the four lane groups' shares meet in the staging tile, added in fixed order
            tA[g * 16 + i16] = csp;
            float cs[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int jl = 4 * g + r;
                cs[r] = (tA[jl] + tA[16 + jl]) + (tA[32 + jl] + tA[48 + jl]);
            }
            // G = dS^T X -> operand layout; dX_j = [dP Mt of pass 1] + S^T dZ + G Mt + colsum(dS) d
#pragma unroll
            for (int oc = 0; oc < 4; ++oc)
#pragma unroll
                for (int r = 0; r < 4; ++r) rowsP[(4 * g + r) * LDK + oc * 16 + i16] = accG[oc][r];
            float ag[16];
            frag64(rowsP + i16 * LDK, g, ag);
#pragma unroll
            for (int oc = 0; oc < 4; ++oc) {
                float bf[16];
                frag64(sMt + (oc * 16 + i16) * LDK, g, bf);
                const f32x4 acc2 = mm64(ag, bf, f32x4{0.f, 0.f, 0.f, 0.f});
                const float dv = sd[oc * 16 + i16];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = jbase + 4 * g + r;
                    if (row < N) {
                        float* p = dx + (r0 + row) * 64 + oc * 16 + i16;   // written by this very lane in pass 1
                        *p = (*p + acc1[oc][r]) + (acc2[r] + cs[r] * dv);
                    }
                }
            }
        }
    }
    // the waves' shares of dMt and dd, added in wave order (Mt and d are dead)
    for (int w = 0; w < NWAVES; ++w) {
        __syncthreads();
        if (wv == w) {
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int n4 = u >> 2, kt = u & 3;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float* p = sMt + (n4 * 16 + 4 * g + r) * LDK + kt * 16 + i16;
                    *p = w == 0 ? accM[u][r] : *p + accM[u][r];
                }
            }
            sd[lane] = w == 0 ? dd_acc : sd[lane] + dd_acc;
        }
    }
    __syncthreads();
    float* out = partials + (int64_t)blockIdx.x * (65 * 64);
    for (int i = threadIdx.x; i < 64 * 64; i += blockDim.x) out[i] = sMt[(i >> 6) * LDK + (i & 63)];
    if (threadIdx.x < 64) out[64 * 64 + threadIdx.x] = sd[threadIdx.x];
}

inline int ntc_of(int N) { const int nt = (N + 15) / 16; return nt <= 4 ? 4 : nt <= 8 ? 8 : nt <= 12 ? 12 : 16; }
inline size_t fwd_lds(int N) {
    const int NP = (N + 15) & ~15;
    return sizeof(float) * (size_t)(64 * LDK + 64 + 64 + 256 + 64 + NP * LDK + NWAVES * FWD_PRIV);
}
inline size_t bwd_lds(int N) {
    const int NP = (N + 15) & ~15;
    return sizeof(float) * (size_t)(64 * LDK + 64 + TWOG_GCN_WIDE_MAX_NODES + NP * LDK + NWAVES * BWD_PRIV);
}
inline int frame_grid(int n_frames) { return n_frames < MAX_GRID ? (n_frames > 0 ? n_frames : 1) : MAX_GRID; }

}  // namespace

extern "C" int twog_gcn_wide_max_nodes(void) { return TWOG_GCN_WIDE_MAX_NODES; }

extern "C" int twog_gcn_wide_launch_plan(int kernel, int n_frames, int n_nodes, int out[4]) {
    if (!out) return -2;
    if (n_nodes > TWOG_GCN_WIDE_MAX_NODES || n_nodes < 1) return -1;
    if (n_frames < 0) n_frames = 0;
    out[1] = 1;
    switch (kernel) {
        case TWOG_GCN_WIDE_PLAN_FWD:
            out[0] = frame_grid(n_frames); out[2] = (int)fwd_lds(n_nodes); out[3] = ntc_of(n_nodes);
            return 0;
        case TWOG_GCN_WIDE_PLAN_BWD:
            out[0] = frame_grid(n_frames); out[2] = (int)bwd_lds(n_nodes); out[3] = 0;
            return 0;
        case TWOG_GCN_WIDE_PLAN_EMBED1_FWD: {
            const int grid = twog_internal_embed1_fwd_grid((int64_t)n_frames * n_nodes);
            out[0] = grid > 0 ? grid : 1; out[2] = 0; out[3] = 0;
            return 0;
        }
        default: return -2;
    }
}

extern "C" int twog_gcn_wide_fwd(const float* x_geo, int64_t frame_stride, int n_frames, int n_nodes, const float* ab,
                                 const float* w1, const float* b1, const float* w2, const float* b2, const float* md,
                                 float* x_out, float* adj, float* z, void* stream) {
    int plan[4];
    const int rc = twog_gcn_wide_launch_plan(TWOG_GCN_WIDE_PLAN_FWD, n_frames, n_nodes, plan);
    if (rc < 0) return rc;
    if (n_frames <= 0) return 0;
    const int grid = plan[0];
    const size_t lds = (size_t)plan[2];
    static std::atomic<uint32_t> done4{0}, done8{0}, done12{0}, done16{0};
#define TWOG_WIDE_LAUNCH(NTC_, FLAG_)                                                                                    \
    do {                                                                                                                 \
        twog_allow_dynamic_lds(gcn_wide_fwd_kernel<NTC_>, 160 * 1024, FLAG_);                                            \
        hipLaunchKernelGGL(gcn_wide_fwd_kernel<NTC_>, dim3(grid), dim3(64 * NWAVES), lds, (hipStream_t)stream, x_geo,    \
                           frame_stride, n_frames, n_nodes, ab, w1, b1, w2, b2, md, x_out, adj, z);                     \
    } while (0)
    switch (plan[3]) {
        case 4: TWOG_WIDE_LAUNCH(4, done4); break;
        case 8: TWOG_WIDE_LAUNCH(8, done8); break;
        case 12: TWOG_WIDE_LAUNCH(12, done12); break;
        default: TWOG_WIDE_LAUNCH(16, done16); break;
    }
#undef TWOG_WIDE_LAUNCH
    TWOG_CHECK_LAUNCH();
    return 0;
}

extern "C" int twog_gcn_wide_bwd(const float* x, const float* md, const float* adj, const float* dz, int n_frames,
                                 int n_nodes, float* dx_att, float* partials, int n_blocks, void* stream) {
    int plan[4];
    const int rc = twog_gcn_wide_launch_plan(TWOG_GCN_WIDE_PLAN_BWD, n_frames, n_nodes, plan);
    if (rc < 0) return rc;
    if (n_frames <= 0) return 0;
    if (n_blocks != plan[0]) return -2;
    const size_t lds = (size_t)plan[2];
    static std::atomic<uint32_t> lds_attr_done{0};
    twog_allow_dynamic_lds(gcn_wide_bwd_kernel, 160 * 1024, lds_attr_done);
    hipLaunchKernelGGL(gcn_wide_bwd_kernel, dim3(n_blocks), dim3(64 * NWAVES), lds, (hipStream_t)stream, x, md, adj, dz,
                       n_frames, n_nodes, dx_att, partials);
    TWOG_CHECK_LAUNCH();
    return 0;
}
