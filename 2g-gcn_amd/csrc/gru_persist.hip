// Frame-level bidirectional GRU recurrence as ONE persistent launch with the recurrent weights resident on the chip.
//
// Reference: _process_frame_level_rnn (vhoi/models.py:983-1002): nn.GRU(h, h, bidirectional) per entity type, all
// entities of a type batched as rows; gate order r, z, n. Same inputs, outputs and saved tensors as twog_bigru_fwd
// (gru.hip), which issues one launch per time step (gemm_gru_fwd_kernel: each of its 176 tiles re-reads a 384 KB slice
// of W_hh every step).
//
// Here the chip is partitioned once: a workgroup (one per CU, 4 waves, one per SIMD) owns, for the whole sequence, a
// slice of 16 hidden units x 3 gates of ONE (entity type, direction) weight and a chunk of at most 16 of that type's
// 16-row tiles. The slice's 48 x h weights are split ONCE into their three bf16 planes and kept in LDS as ready MFMA B
// fragments (lane-linear 1 KB blocks per (k-block, gate, plane): 144 KB at h = 512); every wave owns up to four row
// tiles and runs the whole reduction for them (exact 3 x bf16 split of the streamed states, 6 of 9 products on
// v_mfma_f32_16x16x32_bf16, fp32 accumulate, the h.h product and the five small ones in separate accumulators like
// the 64x64 class), each B fragment it reads serving all its tiles; then the input projection, the gate math, and the
// tile's 16 columns of h_t. No partial sums cross waves: a row tile's chain lives in one wave.
//
// Steps are ordered inside the launch. A row tile of step s needs all h / 16 slices of that tile from step s - 1 --
// nothing else: the wave w of every workgroup of a (group, chunk) combination works the same tiles, so the hand-off is
// between same-numbered waves of those workgroups, per the agent-scope rules of gfx950 (per-XCD L2s are not coherent):
// states stored write-through (16-byte sc1 stores), the storing wave drains them (s_waitcnt vmcnt(0)) and one of its
// lanes adds to the combination's wave counter (agent scope); the consuming wave polls that counter with sc1 loads and
// reads the states with sc1 loads only. Every spin is bounded: a grid that is not fully resident (another tenant holds
// compute units) ends with the error word set and every wave gone -- no trap, no hang; the host then re-runs the pass on
// the launch-per-step path (kernels.py).
// With 8 combinations (the bench shape) the 32 workgroups of a combination share blockIdx mod 8, i.e. an XCD: their
// exchange stays in that XCD's L2 -- a matter of speed, never of correctness. Bit-reproducible: fixed summation order.
#include "bf16x3.h"
#include "gru_gate.h"
#include "persist_common.h"

namespace {

constexpr int MAXG = 8;     // (entity type, direction) groups
constexpr int MAXC = 32;    // (group, row chunk) combinations, each worked by hidden / 16 workgroups
constexpr int MAXTW = 4;    // row tiles per wave at most: a chunk has at most 4 * MAXTW tiles

struct PGroup {
    const float* gi;     // [bs][T][E][6h]
    const float* w_hh;   // [3h][h] of this direction
    const float* b_hh;   // [3h] or nullptr
    float* out;          // [bs][T][E][2h]
    float* save;         // [2][bs][T][E][4h]
    int E, dir, rows;    // rows = bs * E
};
struct PCombo { int group, rt0, rt1, tw; };   // row tiles [rt0, rt1): wave w owns tiles rt0 + w * tw ... + tw - 1
struct PArgs {
    PGroup g[MAXG];
    PCombo c[MAXC];
    unsigned* pub;       // [MAXC][4] zero at launch: arrivals (workgroups x steps) of each wave's tiles
    unsigned* error;     // set to 1 when a spin bound is exceeded: every wave then leaves the kernel (wait_counter)
    int n_combos, bs, T;
    int spin_limit;
};

// The exact 3 x bf16 split of the weights and the streamed states (bf16x3.h), behind this file's timing probe.
__device__ __forceinline__ Planes split_gp(const f32x4 a, const f32x4 b) {
#ifdef TWOG_GP_PROBE_NOSPLIT   // timing probe only (wrong results): what the per-wave split of the streamed states costs
    { Planes q; q.h = __builtin_bit_cast(bf16x8, a); q.m = __builtin_bit_cast(bf16x8, b); q.l = q.h; return q; }
#endif
    return split8(a, b);
}

// four floats of the transposition scratch, read AS floats: a load through a vector-typed pointer does not alias the
// float stores as far as the compiler's type-based analysis goes, and the next block's stores were moved in front of it
__device__ __forceinline__ f32x4 row4(const float* p) { return f32x4{p[0], p[1], p[2], p[3]}; }
// The scratch transposes a tile between lanes of ONE wave. At the ISA level a wave's LDS operations run in order; at the
// language level the lanes are independent threads, and the compiler may thread a lane-dependent branch (the masked
// store behind the read) through the scratch writes, so that the masked-out lanes write AFTER the others have read
// (seen: wrong columns exactly where a quad of rows was partly valid). A convergent wave barrier on both sides of the
// exchange pins writes, reads and the next writes in program order for all lanes.
__device__ __forceinline__ void lanes_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ f32x4 mfma(const bf16x8 a, const bf16x8 b, const f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// NKB k-blocks of 32: hidden = 32 * NKB. TWC: row tiles per wave at most (of all combinations); D: k-blocks of states in
// flight per wave beside the one being multiplied -- with one tile per wave (small batches: the step is a latency chain)
// the whole row of states is requested at once.
template <int NKB, int TWC>
__global__ __launch_bounds__(256, 1) void bigru_persist_fwd_kernel(const PArgs P) {
    constexpr int TW = TWC;
#ifndef TWOG_GP_D4
#define TWOG_GP_D4 3
#endif
    constexpr int D = TWC == 1 ? NKB : (TWC == 2 ? (NKB < 8 ? NKB : 8) : (NKB < TWOG_GP_D4 ? NKB : TWOG_GP_D4));
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int h = 32 * NKB, n_wg = h / 16;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), i16 = lane & 15, g4 = lane >> 4;
    const int combo = (int)blockIdx.x % P.n_combos, slice = (int)blockIdx.x / P.n_combos;
    const PCombo& C = P.c[combo];
    const PGroup& G = P.g[C.group];
    const int T = P.T, E = G.E, dir = G.dir;
    const float inv_e = 1.0f / (float)E;
    unsigned* pub = P.pub + combo * 4 + wave;
    const int t0 = C.rt0 + wave * C.tw;
    const int nt = max(0, min(C.tw, C.rt1 - t0));   // this wave's tiles: t0 ... t0 + nt - 1
    // LDS: the weight slice as B fragments [k-block][gate][plane][64 lanes] x 16 bytes, then a [16][20] float scratch per wave
    i32x4* wfrag = reinterpret_cast<i32x4*>(smem);
    float* scratch = reinterpret_cast<float*>(smem + NKB * 9 * 1024) + wave * 16 * 20;
    // lane l of a fragment holds W[gate c][unit 16 slice + (l & 15)][k = 32 kb + 8 (l >> 4) + j], j = 0..7
    for (int f = wave; f < NKB * 3; f += 4) {
        const int kb = f / 3, c = f - kb * 3;
        const float* w = G.w_hh + (int64_t)(c * h + slice * 16 + i16) * h + kb * 32 + 8 * g4;
        const Planes p = split_gp(*reinterpret_cast<const f32x4*>(w), *reinterpret_cast<const f32x4*>(w + 4));
        wfrag[((kb * 3 + c) * 3 + 0) * 64 + lane] = __builtin_bit_cast(i32x4, p.h);
        wfrag[((kb * 3 + c) * 3 + 1) * 64 + lane] = __builtin_bit_cast(i32x4, p.m);
        wfrag[((kb * 3 + c) * 3 + 2) * 64 + lane] = __builtin_bit_cast(i32x4, p.l);
    }
    float bias[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) bias[c] = G.b_hh ? G.b_hh[c * h + slice * 16 + i16] : 0.f;
    __syncthreads();
    if (nt == 0) return;   // (a wave without tiles neither waits nor is waited for: the counters are per wave)
    const __amdgpu_buffer_rsrc_t rs_out = rsrc_of(G.out);
    const int col = slice * 16 + i16;
    // byte offset of (row, column 0 of this direction) at time x in `out`: rows (b, e) of [bs][T][E][2h]
    auto out_off = [&](int row, int x) -> uint32_t {
        const int b = (int)(((float)row + 0.5f) * inv_e), e = row - b * E;
        return 4u * (uint32_t)((((int64_t)b * T + x) * E + e) * (2 * h) + dir * h);
    };

    for (int s = 0; s < T; ++s) {
        const int t = dir == 0 ? s : T - 1 - s, tp = dir == 0 ? t - 1 : t + 1;
        // the input projections of this wave's outputs: independent of the chain, requested before the wait
        float gi[TW][4][3];
#pragma unroll
        for (int i = 0; i < TW; ++i)
            if (i < nt) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = min((t0 + i) * 16 + 4 * g4 + r, G.rows - 1);
                    const int b = (int)(((float)row + 0.5f) * inv_e), e = row - b * E;
                    const float* p = G.gi + ((((int64_t)b * T + t) * E + e) * 6 + dir * 3) * h + col;
                    gi[i][r][0] = p[0]; gi[i][r][1] = p[h]; gi[i][r][2] = p[2 * h];
                }
            }
        f32x4 hi[TW][3], lo[TW][3];
#pragma unroll
        for (int i = 0; i < TW; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) { hi[i][c] = f32x4{0.f, 0.f, 0.f, 0.f}; lo[i][c] = f32x4{0.f, 0.f, 0.f, 0.f}; }
        float h0[TW][4];
#pragma unroll
        for (int i = 0; i < TW; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) h0[i][r] = 0.f;
        if (s > 0) {
            // every slice has published step s - 1 of this wave's tiles
            if (!twog_wait_counter(pub, (unsigned)s * (unsigned)n_wg, P.error, P.spin_limit, lane)) return;
            uint32_t abase[TW];
#pragma unroll
            for (int i = 0; i < TW; ++i) {
                const int row = min((t0 + min(i, nt - 1)) * 16 + i16, G.rows - 1);
                abase[i] = out_off(row, tp) + 4u * (uint32_t)(8 * g4);
            }
#pragma unroll
            for (int i = 0; i < TW; ++i)
                if (i < nt) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = min((t0 + i) * 16 + 4 * g4 + r, G.rows - 1);
                        h0[i][r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_out, (int)(out_off(row, tp) + 4u * (uint32_t)col), 0, SC1));
                    }
                }
            auto load_a = [&](int kb, f32x4 (&a)[TW][2]) {
#pragma unroll
                for (int i = 0; i < TW; ++i) {
                    a[i][0] = ld_sc1(rs_out, abase[i] + 128u * kb);
                    a[i][1] = ld_sc1(rs_out, abase[i] + 128u * kb + 16u);
                }
            };
            auto mac = [&](int kb, const f32x4 (&a)[TW][2]) {
                Planes A[TW];
#pragma unroll
                for (int i = 0; i < TW; ++i) A[i] = split_gp(a[i][0], a[i][1]);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    Planes W;
                    W.h = __builtin_bit_cast(bf16x8, wfrag[((kb * 3 + c) * 3 + 0) * 64 + lane]);
                    W.m = __builtin_bit_cast(bf16x8, wfrag[((kb * 3 + c) * 3 + 1) * 64 + lane]);
                    W.l = __builtin_bit_cast(bf16x8, wfrag[((kb * 3 + c) * 3 + 2) * 64 + lane]);
#pragma unroll
                    for (int i = 0; i < TW; ++i)
                        if (i < nt) {
                            // (mac6 of bf16x3.h written out: with the accumulators as Acc[TW][3] instead of these two arrays
                            // every instantiation of this kernel gets another register allocation)
                            hi[i][c] = mfma(A[i].h, W.h, hi[i][c]);
                            lo[i][c] = mfma(A[i].h, W.m, lo[i][c]);
                            lo[i][c] = mfma(A[i].m, W.h, lo[i][c]);
                            lo[i][c] = mfma(A[i].m, W.m, lo[i][c]);
                            lo[i][c] = mfma(A[i].h, W.l, lo[i][c]);
                            lo[i][c] = mfma(A[i].l, W.h, lo[i][c]);
                        }
                }
            };
            // D k-blocks in flight beside the one being multiplied (straight-line code: the compiler counts its waits)
            f32x4 ring[D][TW][2];
#pragma unroll
            for (int kb = 0; kb < D; ++kb) load_a(kb, ring[kb]);
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb) {
                mac(kb, ring[kb % D]);
                if (kb + D < NKB) load_a(kb + D, ring[kb % D]);
            }
        }
        // ---- gates; the states first (write-through), then the signal, then what only the backward pass reads
        float rg[TW][4], zz[TW][4], nn[TW][4], hn4[TW][4];
#pragma unroll
        for (int i = 0; i < TW; ++i) {
            if (i < nt) {
                const int rt = t0 + i;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float hr = hi[i][0][r] + lo[i][0][r] + bias[0], hz = hi[i][1][r] + lo[i][1][r] + bias[1];
                    const GruFwdUnit e = gru_fwd_unit<GruFwdRounded>(gi[i][r][0], gi[i][r][1], gi[i][r][2], hr, hz,
                                                                     hi[i][2][r] + lo[i][2][r] + bias[2], h0[i][r], 1.0f, false);
                    rg[i][r] = e.rg; zz[i][r] = e.z; nn[i][r] = e.n; hn4[i][r] = e.hn;
                    scratch[(4 * g4 + r) * 20 + i16] = e.h;
                }
                lanes_sync();
                // the tile's 16 x 16 states: one 16-byte write-through store per lane (row = lane / 4, 4 units)
                const int srow = lane >> 2, sc = (lane & 3) * 4;
                const f32x4 v = row4(scratch + srow * 20 + sc);   // same wave wrote it: LDS operations of a wave run in order
                const int row = rt * 16 + srow;
                if (row < G.rows)   // (longhand: st_sc1 here changes the register allocation of the four-tile instantiations)
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rs_out,
                                                           (int)(out_off(row, t) + 4u * (uint32_t)(slice * 16 + sc)), 0, SC1);
                lanes_sync();
            }
        }
        // publish step s of this wave's tiles: the wave drains its stores, then one lane signals
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        twog_jitter();
        if (lane == 0) __hip_atomic_fetch_add(pub, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int i = 0; i < TW; ++i) {
            if (i < nt) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = (t0 + i) * 16 + 4 * g4 + r;
                    if (row < G.rows) {
                        const int b = (int)(((float)row + 0.5f) * inv_e), e = row - b * E;
                        float* sv = G.save + ((((int64_t)dir * P.bs + b) * T + t) * E + e) * (4 * h) + col;
                        sv[0] = rg[i][r]; sv[h] = zz[i][r]; sv[2 * h] = nn[i][r]; sv[3 * h] = hn4[i][r];
                    }
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Backward through time, small-batch form (one 16-row tile per wave at most). A workgroup owns 16 hidden units of one
// (type, direction): the carried gradient of those units lives in registers for the whole sequence, and the 3h x 16
// slice of W_hh that produces it (d h_prev[:, u] = sum_k d_gh[:, k] W_hh[k][u], k over the 3h gate rows) in LDS as
// B fragments. Per step: gate backward of the own units (gru_gate.h) -> d_gi, d_gh columns (d_gh
// write-through: it is the next product's operand for EVERY slice) -> signal -> wait for all slices -> the complete
// d_gh rows x the slice -> carried gradient of the next step. Same hand-off rules as the forward kernel.
// ---------------------------------------------------------------------------------------------------------------
struct BGroup {
    const float* d_out;  // [bs][T][E][2h]
    const float* save;   // [2][bs][T][E][4h]
    const float* out;    // [bs][T][E][2h]
    const float* w_hh;   // [3h][h] of this direction
    float* d_gi;         // [bs][T][E][6h]
    float* d_gh;         // [bs][T][E][6h]
    int E, dir, rows;
};
struct BArgs {
    BGroup g[MAXG];
    PCombo c[MAXC];
    unsigned* pub;
    unsigned* error;
    int n_combos, bs, T;
    int spin_limit;
};

template <int NKH>   // hidden = 32 * NKH; the reduction runs over 3h = 96 * NKH, i.e. 3 * NKH k-blocks
__global__ __launch_bounds__(256, 1) void bigru_persist_bwd_kernel(const BArgs P) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int h = 32 * NKH, n_wg = h / 16, NKB = 3 * NKH;
    constexpr int D = NKB < 24 ? NKB : 24;   // k-blocks of d_gh in flight
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), i16 = lane & 15, g4 = lane >> 4;
    const int combo = (int)blockIdx.x % P.n_combos, slice = (int)blockIdx.x / P.n_combos;
    const PCombo& C = P.c[combo];
    const BGroup& G = P.g[C.group];
    const int T = P.T, E = G.E, dir = G.dir;
    const float inv_e = 1.0f / (float)E;
    unsigned* pub = P.pub + combo * 4 + wave;
    const int rt = C.rt0 + wave;            // tw = 1: this wave's tile, if any
    const bool mine = rt < C.rt1;
    i32x4* wfrag = reinterpret_cast<i32x4*>(smem);   // [k-block][plane][64 lanes] x 16 bytes
    float* scratch = reinterpret_cast<float*>(smem + NKB * 3 * 1024) + wave * 16 * 20;
    // lane l of a fragment holds W_hh[k = 32 kb + 8 (l >> 4) + j][unit 16 slice + (l & 15)], j = 0..7 (k-major operand)
    for (int kb = wave; kb < NKB; kb += 4) {
        const float* w = G.w_hh + (int64_t)(kb * 32 + 8 * g4) * h + slice * 16 + i16;
        f32x4 a, b;
#pragma unroll
        for (int j = 0; j < 4; ++j) { a[j] = w[(int64_t)j * h]; b[j] = w[(int64_t)(j + 4) * h]; }
        const Planes p = split_gp(a, b);
        wfrag[(kb * 3 + 0) * 64 + lane] = __builtin_bit_cast(i32x4, p.h);
        wfrag[(kb * 3 + 1) * 64 + lane] = __builtin_bit_cast(i32x4, p.m);
        wfrag[(kb * 3 + 2) * 64 + lane] = __builtin_bit_cast(i32x4, p.l);
    }
    __syncthreads();
    if (!mine) return;
    const __amdgpu_buffer_rsrc_t rs_dgh = rsrc_of(G.d_gh);
    const int col = slice * 16 + i16;
    // element offset of row (b, e) at time x in a [bs][T][E][width] tensor
    auto row_off = [&](int row, int x, int width) -> int64_t {
        const int b = (int)(((float)row + 0.5f) * inv_e), e = row - b * E;
        return (((int64_t)b * T + x) * E + e) * width;
    };
    float carry[4] = {0.f, 0.f, 0.f, 0.f};   // d h_t[rows 4 g4 + r][unit col] arriving from step s + 1
    int rows4[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) rows4[r] = rt * 16 + 4 * g4 + r;
    const int srow = lane >> 2, sc = (lane & 3) * 4;   // the 16-byte store form: row = lane / 4, 4 units
    const int row_s = rt * 16 + srow;

    // what the gate backward of a step reads (nothing of it depends on the chain): requested one step ahead, under the
    // previous step's product
    struct GateIn { float d[4], rg[4], z[4], n[4], hn[4], h0[4]; };
    auto fetch_gate = [&](int s, GateIn& X) {
        const int t = dir == 0 ? s : T - 1 - s, tp = dir == 0 ? t - 1 : t + 1;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = min(rows4[r], G.rows - 1);
            const float* sv = G.save + (int64_t)dir * P.bs * T * E * 4 * h + row_off(row, t, 4 * h) + col;
            X.d[r] = G.d_out[row_off(row, t, 2 * h) + dir * h + col];
            X.rg[r] = sv[0]; X.z[r] = sv[h]; X.n[r] = sv[2 * h]; X.hn[r] = sv[3 * h];
            X.h0[r] = s > 0 ? G.out[row_off(row, tp, 2 * h) + dir * h + col] : 0.f;
        }
    };
    GateIn cur, nxt;
    fetch_gate(T - 1, cur);
    for (int s = T - 1; s >= 0; --s) {
        const int t = dir == 0 ? s : T - 1 - s;
        // ---- gate backward of the own 4 x 1 outputs per lane (gru_gate.h)
        float dgi_[3][4], dgh_[3][4], dd[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float d = cur.d[r] + carry[r];
            const GruBwdUnit e = gru_bwd_unit<GruBwdZnDzSum>(d, cur.rg[r], cur.z[r], cur.n[r], cur.hn[r], cur.h0[r], 1.0f, false);
            dgi_[0][r] = e.dr_pre; dgi_[1][r] = e.dz_pre; dgi_[2][r] = e.dn_pre;
            dgh_[0][r] = e.dr_pre; dgh_[1][r] = e.dz_pre; dgh_[2][r] = e.dn_rg;
            dd[r] = d;
        }
        // d_gh first (write-through: the other slices wait for it), then d_gi: 16 x 16 blocks through the wave's scratch,
        // one 16-byte store per lane and gate
        const int64_t o6 = row_off(min(row_s, G.rows - 1), t, 6 * h) + dir * 3 * h + slice * 16 + sc;
#pragma unroll
        for (int gte = 0; gte < 3; ++gte) {
#pragma unroll
            for (int r = 0; r < 4; ++r) scratch[(4 * g4 + r) * 20 + i16] = dgh_[gte][r];
            lanes_sync();
            const f32x4 v = row4(scratch + srow * 20 + sc);
            if (row_s < G.rows)   // (longhand: st_sc1 here changes the register allocation of the h = 512 instantiation)
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rs_dgh, (int)(4 * (o6 + (int64_t)gte * h)), 0, SC1);
            lanes_sync();
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        twog_jitter();
        if (lane == 0) __hip_atomic_fetch_add(pub, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int gte = 0; gte < 3; ++gte) {
#pragma unroll
            for (int r = 0; r < 4; ++r) scratch[(4 * g4 + r) * 20 + i16] = dgi_[gte][r];
            lanes_sync();
            const f32x4 v = row4(scratch + srow * 20 + sc);
            if (row_s < G.rows) *reinterpret_cast<f32x4*>(G.d_gi + o6 + (int64_t)gte * h) = v;
            lanes_sync();
        }
        if (s == 0) break;   // no state before the first step
        fetch_gate(s - 1, nxt);
        // ---- every slice has published its d_gh columns of this step
        if (!twog_wait_counter(pub, (unsigned)(T - s) * (unsigned)n_wg, P.error, P.spin_limit, lane)) return;
        // ---- carry = direct + d_gh[rows][0 : 3h] . W_hh[:, own units]
        const uint32_t abase = (uint32_t)(4 * (row_off(min(rt * 16 + i16, G.rows - 1), t, 6 * h) + dir * 3 * h + 8 * g4));
        Acc acc;
        acc_zero(acc);
        auto load_a = [&](int kb, f32x4 (&a)[2]) {
            a[0] = ld_sc1(rs_dgh, abase + 128u * kb);
            a[1] = ld_sc1(rs_dgh, abase + 128u * kb + 16u);
        };
        auto mac = [&](int kb, const f32x4 (&a)[2]) {
            const Planes A = split_gp(a[0], a[1]);   // (before the fragment reads: the other order is another register allocation)
            Planes W;
            W.h = __builtin_bit_cast(bf16x8, wfrag[(kb * 3 + 0) * 64 + lane]);
            W.m = __builtin_bit_cast(bf16x8, wfrag[(kb * 3 + 1) * 64 + lane]);
            W.l = __builtin_bit_cast(bf16x8, wfrag[(kb * 3 + 2) * 64 + lane]);
            mac6(acc, A, W);
        };
        f32x4 ring[D][2];
#pragma unroll
        for (int kb = 0; kb < D; ++kb) load_a(kb, ring[kb]);
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
            mac(kb, ring[kb % D]);
            if (kb + D < NKB) load_a(kb + D, ring[kb % D]);
        }
        // (the direct path d z, dprev of gru_gate.h, stays exact inside the sum: what the compiler had made of direct + (hi + lo))
#pragma unroll
        for (int r = 0; r < 4; ++r) carry[r] = fmaf(dd[r], cur.z[r], acc.hi[r] + acc.lo[r]);
        cur = nxt;
    }
}

}  // namespace

// Plans the partition for (n_types entity counts E, bs, hidden) on n_cus compute units: per (type, direction) group the
// number of row-tile chunks (every chunk is worked by hidden / 16 workgroups, one per slice of 16 units), growing the
// group with the longest chunk while the grid still fits. Returns the number of (group, chunk) combinations or -1 when
// the shape is not served: hidden not 64 / 128 / 256 / 512, more combinations x slices than compute units, or a chunk of
// more than 16 row tiles (four per wave).
static int plan(const int* E_of_type, int n_types, int bs, int hidden, int n_cus, PCombo* combos) {
    if (hidden != 64 && hidden != 128 && hidden != 256 && hidden != 512) return -1;
    const int slices = hidden / 16, n_groups = 2 * n_types;
    if (n_groups > MAXG || n_groups * slices > n_cus) return -1;
    int total = n_groups, rt[MAXG], chunks[MAXG];
    for (int g = 0; g < n_groups; ++g) {
        chunks[g] = 1;
        rt[g] = (bs * E_of_type[g / 2] + 15) / 16;
        if (rt[g] == 0) return -1;
    }
    for (;;) {
        int best = -1, longest = 1;
        for (int g = 0; g < n_groups; ++g) {
            const int len = (rt[g] + chunks[g] - 1) / chunks[g];
            if (len > longest && chunks[g] < rt[g]) { longest = len; best = g; }
        }
        if (best < 0 || (total + 1) * slices > n_cus || total + 1 > MAXC) break;
        ++chunks[best];
        ++total;
    }
    int n = 0;
    for (int g = 0; g < n_groups; ++g)
        for (int c = 0; c < chunks[g]; ++c) {
            PCombo& C = combos[n++];
            C.group = g;
            C.rt0 = c * rt[g] / chunks[g];
            C.rt1 = (c + 1) * rt[g] / chunks[g];
            const int tiles = C.rt1 - C.rt0;
            if (tiles > 4 * MAXTW) return -1;
            C.tw = (tiles + 3) / 4;
        }
    return n;
}

// Everything the two launches take from the partition: what they launch with, what the two *_supported functions rate, and
// what twog_bigru_persistent_plan reports. One place: there is no second copy of this arithmetic.
struct PLaunch {
    int n_combos;   // (group, chunk) combinations, > 0
    int nkb, twc;   // the forward instance bigru_persist_fwd_kernel<nkb, twc>: hidden / 32, and the largest tiles-per-wave of
                    // any combination rounded up to an instance that exists (1, 2, 4)
    int grid;       // workgroups of either launch: n_combos x hidden / 16
    int lds_fwd;    // dynamic LDS bytes, forward: the slice's B fragments [hidden / 32][3 gates][3 planes] x 1 KB + the waves' scratch
    int lds_bwd;    // backward: [3 hidden / 32][3 planes] x 1 KB + the waves' scratch
    int bwd_served; // 1 when no wave owns more than one tile: the backward kernel has no other form
};
constexpr int SCRATCH_BYTES = 4 * 16 * 20 * 4;   // a [16][20] float transposition scratch per wave
static_assert(TWOG_BIGRU_PLAN_MAX_COMBOS == MAXC, "the report of include/twog_gcn.h holds every combination");

// plan() and what follows from it. Returns the number of combinations, or -1 (L and combos undefined) when the shape is not served.
static int launch_plan(const int* E_of_type, int n_types, int bs, int hidden, int n_cus, PCombo* combos, PLaunch& L) {
    if (n_types <= 0 || n_types > MAXG / 2) return -1;
    const int n = plan(E_of_type, n_types, bs, hidden, n_cus, combos);
    if (n <= 0) return -1;
    int tw = 1;
    for (int i = 0; i < n; ++i)
        if (combos[i].tw > tw) tw = combos[i].tw;
    L.n_combos = n;
    L.nkb = hidden / 32;
    L.twc = tw > 2 ? 4 : tw;
    L.grid = n * (hidden / 16);
    L.lds_fwd = (hidden / 32) * 9 * 1024 + SCRATCH_BYTES;
    L.lds_bwd = (3 * hidden / 32) * 3 * 1024 + SCRATCH_BYTES;
    L.bwd_served = tw == 1;
    return n;
}

// The partition and the launch numbers of (E_of_type[n_types], bs, hidden) on n_cus compute units (<= 0: those of the current
// device), without a launch; with n_cus > 0 without any device call. Layout of `out`: include/twog_gcn.h.
extern "C" int twog_bigru_persistent_plan(const int32_t* E_of_type, int n_types, int bs, int hidden, int n_cus, int32_t* out) {
    if (!out || (n_types > 0 && !E_of_type)) return -2;
    if (n_cus <= 0) {
        const hipError_t e = twog_device_cus(&n_cus);
        if (e != hipSuccess) return -(int)e;
    }
    for (int i = 0; i < TWOG_BIGRU_PLAN_INTS; ++i) out[i] = 0;
    out[0] = -1;
    out[7] = n_cus;
    PCombo combos[MAXC];
    PLaunch L;
    int Es[MAXG / 2];
    for (int k = 0; k < n_types && k < MAXG / 2; ++k) Es[k] = E_of_type[k];
    if (launch_plan(Es, n_types, bs, hidden, n_cus, combos, L) < 0) return 0;
    out[0] = L.n_combos; out[1] = L.nkb; out[2] = L.twc; out[3] = L.grid;
    out[4] = L.lds_fwd; out[5] = L.lds_bwd; out[6] = L.bwd_served;
    for (int i = 0; i < L.n_combos; ++i) {
        int32_t* c = out + TWOG_BIGRU_PLAN_HEAD + 4 * i;
        c[0] = combos[i].group; c[1] = combos[i].rt0; c[2] = combos[i].rt1; c[3] = combos[i].tw;
    }
    return 0;
}

// 2 if twog_bigru_fwd_persistent serves this shape on the current device AND is the faster path (every wave owns at
// most one row tile: the small-batch regime, where a step is a latency chain -- 9.2 us per step against 17.4 at 8
// clips; with more tiles per wave the launch-per-step path wins: 48 against 31 us at 64 clips, see profiles/HISTORY.md);
// 1 if it is served but slower; 0 if it is not served.
extern "C" int twog_bigru_persistent_supported(const twog_bigru_t* types, int n_types, int bs, int hidden) {
    int n_cus = 0;
    if (n_types <= 0 || n_types > MAXG / 2) return 0;
    if (twog_device_cus(&n_cus) != hipSuccess) return 0;
    PCombo combos[MAXC];
    PLaunch L;
    int Es[MAXG / 2];
    for (int k = 0; k < n_types; ++k) Es[k] = types[k].E;
    if (launch_plan(Es, n_types, bs, hidden, n_cus, combos, L) < 0) return 0;
    return L.twc > 1 ? 1 : 2;
}

// Same contract as twog_bigru_fwd (tmp_gh and zeros unused). sync: device memory, >= 1024 uint32, ZERO at launch
// ([0, 128) the waves' arrival counters, [128] the error word: non-zero after the launch = a wait ran out, the outputs are
// incomplete and the caller must re-run the pass with twog_bigru_fwd). Returns TWOG_PERSIST_NOT_RESIDENT (-3), nothing
// launched, when the runtime's occupancy figure says the grid cannot be resident at once.
extern "C" int twog_bigru_fwd_persistent(const twog_bigru_t* types, int n_types, int bs, int T, int hidden, void* sync,
                                         void* stream) {
    if (n_types <= 0 || T <= 0) return 0;
    if (n_types > MAXG / 2) return -2;
    int n_cus = 0;
    const hipError_t e = twog_device_cus(&n_cus);
    if (e != hipSuccess) return -(int)e;
    PArgs P;
    PLaunch L;
    int Es[MAXG / 2];
    for (int k = 0; k < n_types; ++k) Es[k] = types[k].E;
    const int n_combos = launch_plan(Es, n_types, bs, hidden, n_cus, P.c, L);
    if (n_combos <= 0 || !sync) return -2;
    for (int k = 0; k < n_types; ++k)
        for (int dir = 0; dir < 2; ++dir) {
            PGroup& G = P.g[2 * k + dir];
            const twog_bigru_t& Y = types[k];
            G.gi = Y.gi; G.w_hh = dir == 0 ? Y.w_hh_f : Y.w_hh_r; G.b_hh = dir == 0 ? Y.b_hh_f : Y.b_hh_r;
            G.out = Y.out; G.save = Y.save; G.E = Y.E; G.dir = dir; G.rows = bs * Y.E;
        }
    P.pub = static_cast<unsigned*>(sync);
    P.error = P.pub + MAXC * 4;
    P.n_combos = n_combos; P.bs = bs; P.T = T;
    P.spin_limit = twog_persist_spin_limit();
    twog_jitter_configure();   // (no-op in the shipped library)
    const int grid = L.grid, twc = L.twc;
    const size_t lds = (size_t)L.lds_fwd;
    hipStream_t st = (hipStream_t)stream;
#define TWOG_GP_LAUNCH(NKB_, TWC_)                                                                              \
    do {                                                                                                        \
        static std::atomic<uint32_t> done{0};                                                                   \
        twog_allow_dynamic_lds(bigru_persist_fwd_kernel<NKB_, TWC_>, 160 * 1024, done);                         \
        if (!twog_persist_grid_fits(bigru_persist_fwd_kernel<NKB_, TWC_>, grid, lds, n_cus))                    \
            return TWOG_PERSIST_NOT_RESIDENT;                                                                   \
        hipLaunchKernelGGL((bigru_persist_fwd_kernel<NKB_, TWC_>), dim3(grid), dim3(256), lds, st, P);          \
    } while (0)
#define TWOG_GP_LAUNCH_H(NKB_)                                                                                  \
    do {                                                                                                        \
        if (twc == 1) TWOG_GP_LAUNCH(NKB_, 1);                                                                  \
        else if (twc == 2) TWOG_GP_LAUNCH(NKB_, 2);                                                             \
        else TWOG_GP_LAUNCH(NKB_, 4);                                                                           \
    } while (0)
    switch (L.nkb) {
        case 2: TWOG_GP_LAUNCH_H(2); break;
        case 4: TWOG_GP_LAUNCH_H(4); break;
        case 8: TWOG_GP_LAUNCH_H(8); break;
        default: TWOG_GP_LAUNCH_H(16); break;
    }
#undef TWOG_GP_LAUNCH_H
#undef TWOG_GP_LAUNCH
    TWOG_CHECK_LAUNCH();
    return 0;
}

// 2 if twog_bigru_bwd_persistent serves this shape (at most one row tile per wave), else 0.
extern "C" int twog_bigru_bwd_persistent_supported(const twog_bigru_bwd_t* types, int n_types, int bs, int hidden) {
    int n_cus = 0;
    if (n_types <= 0 || n_types > MAXG / 2) return 0;
    if (twog_device_cus(&n_cus) != hipSuccess) return 0;
    PCombo combos[MAXC];
    PLaunch L;
    int Es[MAXG / 2];
    for (int k = 0; k < n_types; ++k) Es[k] = types[k].E;
    if (launch_plan(Es, n_types, bs, hidden, n_cus, combos, L) < 0) return 0;
    return L.bwd_served ? 2 : 0;
}

extern "C" int twog_bigru_bwd_persistent(const twog_bigru_bwd_t* types, int n_types, int bs, int T, int hidden, void* sync,
                                         void* stream) {
    if (n_types <= 0 || T <= 0) return 0;
    if (n_types > MAXG / 2) return -2;
    int n_cus = 0;
    const hipError_t e = twog_device_cus(&n_cus);
    if (e != hipSuccess) return -(int)e;
    BArgs P;
    PLaunch L;
    int Es[MAXG / 2];
    for (int k = 0; k < n_types; ++k) Es[k] = types[k].E;
    const int n_combos = launch_plan(Es, n_types, bs, hidden, n_cus, P.c, L);
    if (n_combos <= 0 || !sync || !L.bwd_served) return -2;
    for (int k = 0; k < n_types; ++k)
        for (int dir = 0; dir < 2; ++dir) {
            BGroup& G = P.g[2 * k + dir];
            const twog_bigru_bwd_t& Y = types[k];
            G.d_out = Y.d_out; G.save = Y.save; G.out = Y.out; G.w_hh = dir == 0 ? Y.w_hh_f : Y.w_hh_r;
            G.d_gi = Y.d_gi; G.d_gh = Y.d_gh; G.E = Y.E; G.dir = dir; G.rows = bs * Y.E;
        }
    P.pub = static_cast<unsigned*>(sync);
    P.error = P.pub + MAXC * 4;
    P.n_combos = n_combos; P.bs = bs; P.T = T;
    P.spin_limit = twog_persist_spin_limit();
    twog_jitter_configure();   // (no-op in the shipped library)
    const int grid = L.grid;
    const size_t lds = (size_t)L.lds_bwd;
    hipStream_t st = (hipStream_t)stream;
#define TWOG_GPB_LAUNCH(NKH_)                                                                       \
    do {                                                                                            \
        static std::atomic<uint32_t> done{0};                                                       \
        twog_allow_dynamic_lds(bigru_persist_bwd_kernel<NKH_>, 160 * 1024, done);                   \
        if (!twog_persist_grid_fits(bigru_persist_bwd_kernel<NKH_>, grid, lds, n_cus))              \
            return TWOG_PERSIST_NOT_RESIDENT;                                                       \
        hipLaunchKernelGGL(bigru_persist_bwd_kernel<NKH_>, dim3(grid), dim3(256), lds, st, P);      \
    } while (0)
    switch (L.nkb) {
        case 2: TWOG_GPB_LAUNCH(2); break;
        case 4: TWOG_GPB_LAUNCH(4); break;
        case 8: TWOG_GPB_LAUNCH(8); break;
        default: TWOG_GPB_LAUNCH(16); break;
    }
#undef TWOG_GPB_LAUNCH
    TWOG_CHECK_LAUNCH();
    return 0;
}
