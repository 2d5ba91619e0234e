/*
 * twog_gcn.h -- C ABI of lib2ggcn_hip.so: the MI355X (gfx950) kernels of the 2G-GCN hot path.
 *
 * The reference (tanqiu98/2G-GCN) is pure Python/PyTorch and has no FFI of its own; its hot path is TGGCN.forward
 * (vhoi/models.py:584-933) and the ATen ops that forward dispatches. Each entry point below replaces one group of
 * those ops (cited per function; all citations are relative to the reference tree). Conventions:
 *   - every pointer is a DEVICE pointer to fp32 unless stated, owned by the caller, and must stay alive until the work
 *     enqueued on `stream` has completed (torch autograd's saved tensors guarantee that on the Python side);
 *   - no entry point allocates, synchronises the device, or keeps global mutable state (re-entrant per stream);
 *   - return value: 0 on success, a negative hipError_t / negative argument-error code otherwise; nothing throws;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).
 *
 * Strided rows: most kernels address matrix rows through `twog_rows_t`, so a (clip, entity) row set living inside a
 * larger (clip, time, entity, feature) tensor is used in place, with no gather/cat copy:
 *      address(row r, col c) = ptr + (r / inner) * ld_outer + (r % inner) * ld_inner + c        (c contiguous)
 */
#ifndef TWOG_GCN_H
#define TWOG_GCN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    float* ptr;
    int64_t ld_outer; /* elements between consecutive outer groups    */
    int64_t ld_inner; /* elements between consecutive rows in a group */
    int32_t inner;    /* rows per outer group (<= 1: plain row stride = ld_outer) */
    int32_t pad_;
} twog_rows_t;

/* Human-readable build/info string (arch, tile sizes). */
const char* twog_version(void);

/* ===============================================================================================================
 * Dense projections on fp32 MFMA (v_mfma_f32_32x32x2_f32). Replaces every nn.Linear of build_mlp
 * (pyrutils/torch/models.py:31-36), the GRU/GRUCell input and hidden projections (vhoi/models.py:267-320), the
 * message MLPs (:323-520), the label heads (:552-580), the 1x1 convolutions of Geo_gcn (pyrutils/torch/
 * models_gcn.py:57-63, :95-96, :35) and, with the k-major operand forms, all their backward passes.
 *      C[m][n] = act( sum_k A(m,k) * B(n,k) + bias[n] ) (+ C[m][n] if accumulate)
 * a_kmajor = 0: A stored [M rows][K contiguous];            1: A stored [K rows][M contiguous].
 * b_kmajor = 0: B stored [N rows][K contiguous] (nn.Linear weight); 1: B stored [K rows][N contiguous].
 * The strided index of each operand goes through twog_rows_t. All problems of one call share the layout flags and run
 * as grouped launches. `workspace` (may be NULL) enables deterministic split-K for tall-reduction/small-output shapes:
 * caller-owned scratch whose first 16 KB are reserved (ZERO when it is first handed over, afterwards left to the library);
 * the k-slices of a tile write partial tiles (slabs) behind them and an ordered-reduce launch adds them in slice order
 * (bit-reproducible) and runs the epilogue. One workspace must not be used by launches that can run concurrently
 * (different streams): give each stream its own.
 * =============================================================================================================== */
typedef struct {
    twog_rows_t A, B, C;
    const float* bias;  /* [N] or NULL */
    int32_t M, N, K;
    int32_t act;        /* 0 none, 1 relu */
    int32_t accumulate; /* 0: C = ..., 1: C += ... */
    int32_t batch;      /* >= 1 independent problems of this shape; operand of batch i = ptr + i * *_batch_stride */
    int64_t a_batch_stride, b_batch_stride, c_batch_stride;
    float* a_colsum;            /* NULL, or [M]: a_colsum[m] (+)= sum_k A(m,k) from the same pass over A -- the bias gradient that
                                   belongs to a weight gradient dW = dY^T X (nn.Linear / GRU input projection backward:
                                   pyrutils/torch/models.py:31-36, vhoi/models.py:267-320). Served only where
                                   twog_gemm_colsum_fused() says so; asked for elsewhere the call returns -5, nothing launched */
    int32_t a_colsum_accumulate; /* 0: a_colsum = ..., 1: a_colsum += ... */
    int32_t pad2_;
} twog_gemm_t;
int twog_gemm_f32(const twog_gemm_t* problems, int n_problems, int a_kmajor, int b_kmajor, void* workspace,
                  size_t workspace_bytes, void* stream);
/* 1 if twog_gemm_f32 with these arguments computes the a_colsum of every problem that asks for one inside the GEMM launch
 * (k-major A and B, the bf16x3 128x128 class: aligned operands, M % 4 == 0, whole 16-deep k-tiles, plain or grouped rows),
 * 0 if the caller has to take the column sums with twog_colsum / twog_colsum_n instead. No launch. */
int twog_gemm_colsum_fused(const twog_gemm_t* problems, int n_problems, int a_kmajor, int b_kmajor, void* workspace,
                           size_t workspace_bytes);

/* Which kernel variant the calling thread's most recent twog_gemm_f32 chunk (or fused gate launch) selected -- lets a
 * test assert that it exercised the variant it was written for. Bit field: */
#define TWOG_GEMM_CLASS_TILE128 1  /* 128x128 tiles (else 64x64)                        */
#define TWOG_GEMM_CLASS_WAVES8  2  /* 8-wave workgroups (else 4)                        */
#define TWOG_GEMM_CLASS_KG      4  /* k-major operand with (outer, inner) grouped rows  */
#define TWOG_GEMM_CLASS_SPLITK  8  /* deterministic split-K + ordered reduce            */
#define TWOG_GEMM_CLASS_GATE    16 /* gate backward fused into the epilogue             */
#define TWOG_GEMM_CLASS_KSPLIT  32 /* 64x64 tiles, 8 waves, k-split inside the workgroup */
#define TWOG_GEMM_CLASS_GRUFWD  64 /* 64 x (64 units x 3 gates) tiles, GRU forward step in the epilogue */
#define TWOG_GEMM_CLASS_ROWS32  128 /* 32 x 64 tiles (chain launches of small batches)           */
#define TWOG_GEMM_CLASS_XSPLIT  256 /* reduction split over workgroups, combined inside the launch (last arriver) */
#define TWOG_GEMM_CLASS_X3      512 /* on the bf16 matrix cores: fp32 operands split exactly into 3 bf16, 6 products (128x128 class; 64x64 class when K >= 256) */
#define TWOG_GEMM_CLASS_P3      1024 /* beside X3, 128x128 class: the 'high' instantiation ran (two planes, 3 products)   */
#define TWOG_GEMM_CLASS_P1      2048 /* beside X3, 128x128 class: the 'medium' instantiation ran (one plane, 1 product)  */
int twog_gemm_last_class(void);

/* Opt-in matmul precision of the bf16x3 128x128 class (the dense projections and weight gradients), per calling thread;
 * the names follow torch.set_float32_matmul_precision. HIGHEST (the default): three bf16 planes per operand, six products,
 * fp32 results. HIGH: two planes rounded to nearest (h = rne(x), m = rne(x - h)), the products h h + h m + m h:
 * |error| <= (2 + 2^-6) 2^-16 sum |a||b|. MEDIUM: one plane h = rne(x), the product h h: |error| <= (2^-7 + 2^-16) sum |a||b|.
 * Both accumulate in fp32. Every other GEMM class (64x64, chain, gate- and GRU-fused, persistent), the split-accumulator TT
 * launches (TWOG_X3_DW_SPLIT_ACC=1) and the native fp32 kernels (TWOG_GEMM_X3=0) ignore the setting.
 * twog_gemm_set_precision returns the previous value, or -1 (nothing changed) for an unknown p. The setting belongs to the
 * thread that made it -- a backward pass on autograd's thread has its own -- and applies to every launch that thread issues,
 * the library's own loops and tape replays included. */
#define TWOG_GEMM_PRECISION_HIGHEST 0
#define TWOG_GEMM_PRECISION_HIGH    1
#define TWOG_GEMM_PRECISION_MEDIUM  2
int twog_gemm_set_precision(int p);
int twog_gemm_get_precision(void);

/* The dependent launches of the recurrent chains (vhoi/models.py:983-1002 frame-level BiGRUs, :785-880 segment loop:
 * few output tiles, K = h ... 3h, every launch waiting for the previous one). `chain_ws` is a caller-owned scratch of
 * twog_chain_workspace_bytes() bytes whose first 16 KB (arrival tickets) are ZERO when it is first handed over and are
 * afterwards left to the library (every launch returns them to zero); with it the library may split the reduction of
 * such a launch over workgroups and combine the partial tiles inside the launch -- each workgroup publishes its partial
 * write-through and draws a ticket, the last arriver adds the partials in slice order (bit-reproducible) and runs the
 * epilogue; no grid barrier, no waiting. NULL: never split. One chain workspace must not be used by launches that can
 * run concurrently (different streams): give each stream its own. */
size_t twog_chain_workspace_bytes(void);
int twog_gemm_f32_chain(const twog_gemm_t* problems, int n_problems, int a_kmajor, int b_kmajor, void* chain_ws,
                        size_t chain_ws_bytes, void* stream);

/* ===============================================================================================================
 * Geometric-level GCN (pyrutils/torch/models_gcn.py:6-100; called at vhoi/models.py:640-645).
 * x_geo = x_human + 2048 (geometry of human 0, vhoi/models.py:636-639), frame f at x_geo + f*frame_stride, node n,
 * feature c at [n*4 + c]; BatchNorm channel = c*N + n (models_gcn.py:47).
 * =============================================================================================================== */
int twog_gcn_max_nodes(void);
/* The launch geometry the kernels below use for (n_frames, n_nodes): out = {grid (workgroups), frames a workgroup takes per
 * trip of its loop, dynamic LDS bytes, variant}. Host arithmetic only -- no GPU call; the launchers take their grid, group size
 * and LDS size from the same code, so the answer is what is launched. A workgroup makes ceil(ceil(n_frames / out[1]) / grid)
 * trips (embed1: rows = n_frames * n_nodes, 4 rows per workgroup and trip). variant: FUSED_FWD -> NT = ceil(n_nodes / 16), the
 * kernel instance; ATTN2_BWD -> 1 when the M copy fits the LDS (n_nodes <= 48), else 0; otherwise 0. Returns 0, -1 for
 * n_nodes outside 1 .. twog_gcn_max_nodes(), -2 for an unknown kernel, -3 when the kernel's LDS does not fit. */
#define TWOG_GCN_PLAN_FUSED_FWD 0   /* twog_gcn_fused_fwd */
#define TWOG_GCN_PLAN_ATTN2_FWD 1   /* twog_gcn_attn2_fwd */
#define TWOG_GCN_PLAN_ATTN2_BWD 2   /* twog_gcn_attn2_bwd (grid = twog_gcn_attn2_bwd_blocks) */
#define TWOG_GCN_PLAN_EMBED1_FWD 3  /* twog_gcn_embed1_fwd */
#define TWOG_GCN_PLAN_ATTN_FWD 4    /* twog_gcn_attn_fwd */
#define TWOG_GCN_PLAN_ATTN_BWD 5    /* twog_gcn_attn_bwd */
int twog_gcn_launch_plan(int kernel, int n_frames, int n_nodes, int out[4]);
/* norm_data train-mode batch statistics (models_gcn.py:43-49): per-block fp64 partial sums
 * partials[n_blocks][2][4N] (sum, sum of squares; channel order). */
int twog_bn_stats(const float* x_geo, int64_t frame_stride, int n_frames, int n_nodes, double* partials, int n_blocks,
                  void* stream);
/* Folds BatchNorm into x^ = a*x + b per channel: ab[2][4N]; mean_invstd[2][4N] is kept for the backward pass.
 * training != 0: batch statistics (biased variance), running stats updated with momentum 0.1 / unbiased variance,
 * num_batches_tracked += 1 (torch BatchNorm1d semantics); training == 0: running statistics. */
int twog_bn_finalize(const double* partials, int n_blocks, int n_frames, int n_nodes, const float* gamma,
                     const float* beta, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                     int training, float* ab, float* mean_invstd, const float* wq, const float* wk, const float* bq,
                     float* md_out, void* stream);
/* (md_out != NULL: the same launch folds the two similarity projections of compute_similarity, models_gcn.py:95-100, for
 * twog_gcn_fused_fwd: wq, wk [128][64] = get_s.s1 / s2 weights, bq [128] = get_s.s1 bias -> md_out [65][64] = [Mt | d],
 * Mt[n][k] = sum_o wk[o][n] wq[o][k], d[n] = sum_o wk[o][n] bq[o].) */
/* embed layer 1 (models_gcn.py:57-59): e1[(f,n)][64] = relu(W1 (a*x+b) + b1), W1 [64][4]. */
int twog_gcn_embed1_fwd(const float* x_geo, int64_t frame_stride, int n_frames, int n_nodes, const float* ab,
                        const float* w1, const float* b1, float* e1, void* stream);
/* Backward of layer 1 given de1 (already ReLU-masked): dw1[64][4], db1[64], dgamma[4N], dbeta[4N].
 * partials: scratch [n_blocks][320 + 8N] floats. */
int twog_gcn_embed1_bwd(const float* x_geo, int64_t frame_stride, int n_frames, int n_nodes, const float* ab,
                        const float* mean_invstd, const float* w1, const float* de1, float* partials, int n_blocks,
                        float* dw1, float* db1, float* dgamma, float* dbeta, void* stream);
/* Gradient of the geometry INPUT (the split at vhoi/models.py:636-639, norm_data and the first 1x1 conv at
 * models_gcn.py:45-59), given the same ReLU-masked de1 as twog_gcn_embed1_bwd: per (frame, node)
 *   dx^[c] = sum_j de1[j] w1[j][c];   training == 0: dx[c] = a[ch] dx^[c]   (ch = c*N + n, a = ab[0][ch]);
 *   training != 0: dx[c] = a[ch] (dx^[c] - dbeta[ch]/M - x_n[c] dgamma[ch]/M), x_n = (x - mean) invstd, M = n_frames --
 * dgamma / dbeta are the sums twog_gcn_embed1_bwd produced over the SAME n_frames (run it first, on the same stream;
 * NULL ok with training == 0, as is mean_invstd). dx_geo = the gradient of x_human + 2048, laid out like x_geo; human h of
 * a frame at + h*human_stride. Human 0's 4N geometry columns get dx, those of the humans 1 .. n_humans-1 get zeros (only
 * human 0's geometry is read). Grid = n_blocks workgroups of 256 threads, each trip of a workgroup
 * takes 64 (frame, node) rows. Bit-reproducible. Returns -1 for n_nodes outside 1 .. twog_gcn_max_nodes(), -2 for a NULL or
 * misaligned pointer, strides that are not whole float4s or overlap, n_humans < 1 or n_blocks < 1 -- nothing is launched. */
int twog_gcn_input_bwd(const float* x_geo, int64_t frame_stride, int n_frames, int n_nodes, int n_humans,
                       int64_t human_stride, const float* ab, const float* mean_invstd, const float* w1,
                       const float* de1, const float* dgamma, const float* dbeta, int training, float* dx_geo,
                       int n_blocks, void* stream);
/* The forward pass up to the aggregation as ONE kernel (csrc/geo_fused.hip): x^ = a*x+b (norm_data folded, :45-50),
 * e1 = relu(W1 x^ + b1) (:57-59, never stored), X = relu(W2 e1 + b2) (:60-63), S = softmax_j(x_i^T M x_j + d . x_j) -- the
 * similarity of compute_similarity (:95-100) with M = Wq^T Wk, d = Wk^T bq folded by the caller into md [65][64] =
 * [Mt | d] -- and Z = S X (:33-34). w1 [64][4], b1 [64], w2 [64][64], b2 [64]. Outputs: x_out [(f,n)][64] (NULL ok: only the
 * backward pass reads it), adj [f][N][N], z [(f,n)][64]. */
int twog_gcn_fused_fwd(const float* x_geo, int64_t frame_stride, int n_frames, int n_nodes, const float* ab,
                       const float* w1, const float* b1, const float* w2, const float* b2, const float* md,
                       float* x_out, float* adj, float* z, void* stream);
/* compute_similarity + aggregation per frame (models_gcn.py:95-100, :33-34): qk [(f,n)][256] = [theta(x) | phi(x)],
 * x [(f,n)][64]; s_out [f][N][N] = softmax_j(q_i . k_j) (no 1/sqrt(d)); z [(f,n)][64] = S x. */
int twog_gcn_attn_fwd(const float* qk, const float* x, int n_frames, int n_nodes, float* s_out, float* z,
                      void* stream);
/* Backward: dx_att [(f,n)][64] = S^T dz ; dqk [(f,n)][256] = [dP k | dP^T q], dP = S*(dS - rowsum(dS*S)), dS = dz x^T. */
int twog_gcn_attn_bwd(const float* qk, const float* x, const float* s, const float* dz, int n_frames, int n_nodes,
                      float* dx_att, float* dqk, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * The wide family of the geometric-level GCN (csrc/geo_wide.hip): the same functions for 1 <= n_nodes <=
 * twog_gcn_wide_max_nodes() = 256. The reference's Geo_gcn(N, 4, 128) takes any N (models_gcn.py:6-100: conv2d, matmul and
 * softmax only); the tuned kernels above stop at twog_gcn_max_nodes() = 64. Complete, not tuned: one frame per workgroup trip.
 * Every entry point returns -1 for n_nodes outside 1 .. twog_gcn_wide_max_nodes() before anything is launched. */
int twog_gcn_wide_max_nodes(void);
/* As twog_gcn_launch_plan for the wide kernels: out = {grid, frames per trip (1), dynamic LDS bytes, variant}; variant of FWD =
 * the column tiles of 16 senders a strip of receivers can hold in its accumulators (4, 8, 12 or 16: the kernel instance),
 * otherwise 0; EMBED1_FWD: {grid, 1, 0, 0}. Host arithmetic only; the launchers use the same code. Returns 0, -1 for n_nodes outside
 * 1 .. twog_gcn_wide_max_nodes(), -2 for an unknown kernel. */
#define TWOG_GCN_WIDE_PLAN_FWD 0         /* twog_gcn_wide_fwd */
#define TWOG_GCN_WIDE_PLAN_BWD 1         /* twog_gcn_wide_bwd (grid = the n_blocks it must be given) */
#define TWOG_GCN_WIDE_PLAN_EMBED1_FWD 2  /* twog_gcn_wide_embed1_fwd */
int twog_gcn_wide_launch_plan(int kernel, int n_frames, int n_nodes, int out[4]);
/* twog_bn_stats for up to 256 nodes (norm_data, models_gcn.py:43-49): partials[n_blocks][2][4N], fp64. */
int twog_gcn_wide_bn_stats(const float* x_geo, int64_t frame_stride, int n_frames, int n_nodes, double* partials,
                           int n_blocks, void* stream);
/* twog_bn_finalize for up to 256 nodes = 1024 BatchNorm channels (models_gcn.py:43-50; torch BatchNorm1d running-statistics
 * rules; md_out != NULL: the fold of compute_similarity, models_gcn.py:95-100, in the same launch). */
int twog_gcn_wide_bn_finalize(const double* partials, int n_blocks, int n_frames, int n_nodes, const float* gamma,
                              const float* beta, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                              int training, float* ab, float* mean_invstd, const float* wq, const float* wk,
                              const float* bq, float* md_out, void* stream);
/* twog_gcn_embed1_fwd for up to 256 nodes (models_gcn.py:57-59). */
int twog_gcn_wide_embed1_fwd(const float* x_geo, int64_t frame_stride, int n_frames, int n_nodes, const float* ab,
                             const float* w1, const float* b1, float* e1, void* stream);
/* twog_gcn_embed1_bwd for up to 256 nodes (backward of models_gcn.py:45-59); partials: scratch [n_blocks][320 + 8N]. */
int twog_gcn_wide_embed1_bwd(const float* x_geo, int64_t frame_stride, int n_frames, int n_nodes, const float* ab,
                             const float* mean_invstd, const float* w1, const float* de1, float* partials, int n_blocks,
                             float* dw1, float* db1, float* dgamma, float* dbeta, void* stream);
/* twog_gcn_input_bwd for up to 256 nodes (the split at vhoi/models.py:636-639, models_gcn.py:45-59), train and eval forms,
 * same argument checks and return codes. */
int twog_gcn_wide_input_bwd(const float* x_geo, int64_t frame_stride, int n_frames, int n_nodes, int n_humans,
                            int64_t human_stride, const float* ab, const float* mean_invstd, const float* w1,
                            const float* de1, const float* dgamma, const float* dbeta, int training, float* dx_geo,
                            int n_blocks, void* stream);
/* The contract of twog_gcn_fused_fwd (models_gcn.py:30-34, :45-50, :57-63, :95-100): BN fold, 4 -> 64 ReLU, 64 -> 64 ReLU,
 * P = X Mt + d, S = softmax_j (no 1/sqrt(d)), Z = S X. Outputs x_out [(f,n)][64] (NULL ok), adj [f][N][N], z [(f,n)][64]. */
int twog_gcn_wide_fwd(const float* x_geo, int64_t frame_stride, int n_frames, int n_nodes, const float* ab,
                      const float* w1, const float* b1, const float* w2, const float* b2, const float* md, float* x_out,
                      float* adj, float* z, void* stream);
/* The contract of twog_gcn_attn2_bwd (backward of models_gcn.py:95-100, :33-34): dx_att [(f,n)][64] and per-workgroup sums
 * partials [n_blocks][65*64] of (dMt | dd), n_blocks = out[0] of twog_gcn_wide_launch_plan(TWOG_GCN_WIDE_PLAN_BWD) (-2
 * otherwise); the caller column-sums them (twog_colsum). Fixed summation order, no atomics: bit-reproducible. */
int twog_gcn_wide_bwd(const float* x, const float* md, const float* adj, const float* dz, int n_frames, int n_nodes,
                      float* dx_att, float* partials, int n_blocks, void* stream);

/* ===============================================================================================================
 * GRU gate math (torch.nn.GRU / GRUCell semantics, gate order r,z,n) for the frame-level BiGRUs
 * (vhoi/models.py:983-1002) and the gated segment-level step h_t = u*GRUCell(x,h) + (1-u)*h (vhoi/models.py:1535-1564).
 * gi / gh are the input / hidden projections (biases included) produced by twog_gemm_f32.
 * =============================================================================================================== */
typedef struct {
    twog_rows_t gi;     /* [rows][3h]  W_ih x + b_ih                                      */
    twog_rows_t gi2;    /* optional second addend of gi (ptr NULL if unused)              */
    twog_rows_t gh;     /* [rows][3h]  W_hh h_prev + b_hh                                 */
    twog_rows_t h_prev; /* [rows][h]   (ptr NULL => zeros)                                */
    twog_rows_t h_out;  /* [rows][h]                                                      */
    twog_rows_t save;   /* [rows][4h]  r, z, n, (W_hn h + b_hn) for backward (ptr NULL ok) */
    const float* u;     /* gate per row or NULL (plain GRU): u[(r/u_inner)*u_ld_outer + (r%u_inner)*u_ld_inner] */
    int64_t u_ld_outer, u_ld_inner;
    int32_t u_inner;
    int32_t rows, hidden;
    int32_t pad_;
} twog_gru_step_t;
int twog_gru_step_fwd(const twog_gru_step_t* steps, int n_steps, void* stream);
/* What the most recent twog_gru_step_fwd call of this thread launched (host-side decisions, taken per chunk of 8 descriptors
 * over all descriptors of the chunk); tests assert it, so that a case written for the 16-byte kernel cannot silently move to
 * the scalar one. Bit 0 and the workgroup size describe the last chunk that launched; the launch count is the whole call's
 * (chunks whose descriptors all have rows == 0 launch nothing). A call that launches nothing leaves 0. */
#define TWOG_GRU_STEP_PATH_VEC             1  /* four hidden units per thread, 16-byte accesses (else one unit per thread) */
#define TWOG_GRU_STEP_PATH_THREADS_SHIFT   4  /* workgroup size = (word >> 4) & 0xfff                                      */
#define TWOG_GRU_STEP_PATH_LAUNCHES_SHIFT  16 /* launches of the call = word >> 16                                         */
int twog_gru_step_last_path(void);

typedef struct {
    twog_rows_t dh;      /* [rows][h] gradient wrt h_out of this step                                  */
    twog_rows_t dh2;     /* optional second addend of dh (carried gradient; ptr NULL if unused)         */
    twog_rows_t save;    /* [rows][4h] from the forward step                                            */
    twog_rows_t h_prev;  /* [rows][h] (ptr NULL => zeros)                                               */
    twog_rows_t dgi;     /* out [rows][3h]                                                              */
    twog_rows_t dgh;     /* out [rows][3h]                                                              */
    twog_rows_t dh_prev; /* out [rows][h]: direct path (1-u)*dh + u*dh*z; the W_hh path is added by a GEMM */
    const float* u;      /* as in twog_gru_step_t                                                       */
    float* du;           /* += sum_j dh_j*(gru_j - h_prev_j) per row (atomic add), addressed like u; NULL ok */
    int64_t u_ld_outer, u_ld_inner;
    int32_t u_inner;
    int32_t rows, hidden;
    int32_t dh_prev_accumulate; /* 1: dh_prev += */
} twog_gru_step_bwd_t;
int twog_gru_step_bwd(const twog_gru_step_bwd_t* steps, int n_steps, void* stream);

/* Frame-level bidirectional GRU recurrence (vhoi/models.py:983-1002), all entities of a type batched as rows,
 * both directions and up to 4 entity types advancing in the same launches. */
typedef struct {
    const float* gi;     /* [bs][T][E][6h] W_ih x + b_ih: cols [0,3h) forward direction, [3h,6h) reverse */
    const float* w_hh_f; /* [3h][h] weight_hh_l0          */
    const float* b_hh_f; /* [3h]                          */
    const float* w_hh_r; /* [3h][h] weight_hh_l0_reverse  */
    const float* b_hh_r;
    float* out;          /* [bs][T][E][2h] (forward | reverse), = h_fr of the reference                  */
    float* save;         /* [2][bs][T][E][4h]                                                            */
    float* tmp_gh;       /* scratch [2][bs*E][3h]                                                        */
    float* zeros;        /* [bs*E][h] zeros (initial state)                                              */
    int32_t E;
    int32_t pad_;
} twog_bigru_t;
int twog_bigru_fwd(const twog_bigru_t* types, int n_types, int bs, int T, int hidden, void* chain_ws,
                   size_t chain_ws_bytes, void* stream); /* chain_ws: see twog_gemm_f32_chain (NULL ok) */
/* The same recurrence as ONE persistent launch (csrc/gru_persist.hip): a workgroup per compute unit owns 16 hidden
 * units x 3 gates of one (type, direction) weight for the whole sequence -- split once into bf16 planes, resident in
 * LDS as MFMA fragments -- and a chunk of the type's 16-row tiles, up to four per wave; the steps are ordered inside
 * the launch by agent-scope counters between same-numbered waves. Same inputs, outputs and saved tensors as
 * twog_bigru_fwd (tmp_gh / zeros unused). sync: device memory, >= 1024 uint32, ZERO when the launch starts.
 * twog_bigru_persistent_supported: 0 = shape not served (hidden not 64 / 128 / 256 / 512, or the (type, direction, chunk) x
 * hidden / 16 workgroups do not fit the device), 1 = served, 2 = served and the faster path (at most one tile per
 * wave: small batches).
 * Residency (both persistent entry points, forward and backward): every workgroup of the grid must be resident at once.
 * The launch first asks the runtime (hipOccupancyMaxActiveBlocksPerMultiprocessor x compute units >= grid) and returns
 * TWOG_PERSIST_NOT_RESIDENT (-3) WITHOUT launching when the device cannot hold the grid. What the runtime cannot see --
 * another tenant of the GPU holding compute units -- is caught inside the launch: every wait is bounded
 * (TWOG_PERSIST_SPIN_LIMIT spins, default 2^24 ~ seconds); when a bound runs out the launch sets sync[128] != 0 and every
 * wave leaves (no trap, the context survives). After the launch the CALLER reads sync[128]: non-zero means the outputs are
 * incomplete and the pass must be re-run with the launch-per-step entry point (twog_bigru_fwd / twog_bigru_bwd: same
 * buffers, written in place, so the re-run is idempotent). kernels.py does exactly that. */
#define TWOG_PERSIST_NOT_RESIDENT (-3)
int twog_bigru_persistent_supported(const twog_bigru_t* types, int n_types, int bs, int hidden);
int twog_bigru_fwd_persistent(const twog_bigru_t* types, int n_types, int bs, int T, int hidden, void* sync, void* stream);

typedef struct {
    const float* d_out;  /* [bs][T][E][2h] gradient wrt out                                              */
    const float* save;
    const float* out;
    const float* w_hh_f;
    const float* w_hh_r;
    float* d_gi;         /* out [bs][T][E][6h] gradient wrt gi                                           */
    float* d_gh;         /* out [bs][T][E][6h] gradient wrt (W_hh h_prev + b_hh)                         */
    float* carry;        /* scratch [2][bs*E][h]                                                         */
    int32_t E;
    int32_t pad_;
} twog_bigru_bwd_t;
int twog_bigru_bwd(const twog_bigru_bwd_t* types, int n_types, int bs, int T, int hidden, void* chain_ws,
                   size_t chain_ws_bytes, void* stream);
/* Backward through time as ONE persistent launch, the small-batch form (at most one 16-row tile per wave: the shapes
 * for which twog_bigru_bwd_persistent_supported returns 2): a workgroup owns 16 hidden units of one (type, direction),
 * keeps the 3h x 16 slice of W_hh that produces THEIR carried gradient in LDS as bf16x3 MFMA fragments and the carried
 * gradient itself in registers; per step it runs the gate backward of its units, publishes their d_gh columns
 * (write-through) and multiplies the complete d_gh rows -- all workgroups' columns -- with its slice. Same outputs as
 * twog_bigru_bwd (carry unused). sync: device memory, >= 1024 uint32, ZERO when the launch starts. */
int twog_bigru_bwd_persistent_supported(const twog_bigru_bwd_t* types, int n_types, int bs, int hidden);
int twog_bigru_bwd_persistent(const twog_bigru_bwd_t* types, int n_types, int bs, int T, int hidden, void* sync, void* stream);
/* What the two persistent launches would launch with for entity counts E_of_type[n_types] at this batch and width on n_cus
 * compute units (n_cus <= 0: those of the current device): host arithmetic only, nothing is launched, and with n_cus > 0 no
 * device is touched. The launchers and the two *_supported functions take their numbers from the same code. out: int32
 * [TWOG_BIGRU_PLAN_INTS], written whole:
 *   out[0]  number of (group, chunk) combinations, or -1: the shape is not served (n_types not 1 .. 4, hidden not 64 / 128 /
 *           256 / 512, a type without rows, more workgroups than compute units, a chunk of more than 16 row tiles); every
 *           field below except out[7] is then 0
 *   out[1]  NKB, out[2] TWC: the forward launch runs bigru_persist_fwd_kernel<NKB, TWC>; NKB = hidden / 32, TWC = the most row
 *           tiles any wave owns, rounded up to 1, 2 or 4. twog_bigru_persistent_supported = 2 iff TWC == 1, 1 iff TWC > 1
 *   out[3]  grid of either launch: combinations x hidden / 16 workgroups of 256 threads
 *   out[4]  dynamic LDS bytes of the forward launch, out[5] of the backward launch
 *   out[6]  1 when the backward launch serves the shape (no wave owns more than one tile: twog_bigru_bwd_persistent_supported
 *           = 2), else 0
 *   out[7]  the compute-unit count the plan was made for
 *   out[TWOG_BIGRU_PLAN_HEAD + 4 i ...], i < out[0]: {group, rt0, rt1, tw} of combination i -- group = 2 x type + direction
 *           (0 forward, 1 reverse), the combination's 16-row tiles [rt0, rt1) of that group's bs x E rows, tw = ceil((rt1 - rt0)
 *           / 4) tiles per wave: wave w of each of its hidden / 16 workgroups owns tiles rt0 + w tw ... and leaves at once
 *           when that is not below rt1. Workgroup b works combination b % out[0], unit slice b / out[0].
 * Returns 0 (also for a shape that is not served), -2 for a NULL argument, or the negative HIP error of the device query. */
#define TWOG_BIGRU_PLAN_HEAD 8
#define TWOG_BIGRU_PLAN_MAX_COMBOS 32
#define TWOG_BIGRU_PLAN_INTS (TWOG_BIGRU_PLAN_HEAD + 4 * TWOG_BIGRU_PLAN_MAX_COMBOS)
int twog_bigru_persistent_plan(const int32_t* E_of_type, int n_types, int bs, int hidden, int n_cus, int32_t* out);

/* Single-direction frame recurrence: nn.GRU(bidirectional=False) applied per entity slice by the baseline models'
 * _process_frame_level_rnn (vhoi/models.py:70-87, :157-175; modules :25-28, :102-105). The same descriptors and the
 * same per-step machinery as twog_bigru_fwd / twog_bigru_bwd with the forward direction only, so every row is h (not 2h)
 * wide and the reverse weights are not read (w_hh_r / b_hh_r may be NULL):
 *   twog_bigru_t:     gi [bs][T][E][3h], out [bs][T][E][h], save [bs][T][E][4h], tmp_gh [bs*E][3h], zeros [bs*E][h]
 *   twog_bigru_bwd_t: d_out [bs][T][E][h], d_gi / d_gh [bs][T][E][3h], carry [bs*E][h]
 * There is no persistent form. */
int twog_gru_seq_fwd(const twog_bigru_t* types, int n_types, int bs, int T, int hidden, void* chain_ws,
                     size_t chain_ws_bytes, void* stream);
int twog_gru_seq_bwd(const twog_bigru_bwd_t* types, int n_types, int bs, int T, int hidden, void* chain_ws,
                     size_t chain_ws_bytes, void* stream);

/* Entity pooling + concatenation of the baseline models (vhoi/models.py:59-68 BimanualBaseline, :132-154 CAD120Baseline):
 *   hin[b][t][h] = [ hfr[b][t][h] | sum_o mask[b][o] ofr[b][t][o] / max(sum_o mask[b][o], 1) ]            [2W]
 *   oin[b][t][o] = [ ofr[b][t][o] | sum_h hfr[b][t][h] ]      (CAD-120 only: oin NULL skips it)         [2W]
 * hfr [bs][T][H][W], ofr [bs][T][O][W] (W = directions x hidden), mask [bs][O]. One launch; fixed-order reductions, no
 * atomics. H >= 1, O >= 1, any W >= 1. */
typedef struct {
    const float* hfr;
    const float* ofr;
    const float* mask;
    float* hin;
    float* oin;
    int32_t bs, T, H, O, W;
    int32_t pad_;
} twog_entity_pool_t;
int twog_entity_pool_fwd(const twog_entity_pool_t* p, void* stream);
/* Backward of the above: d_hfr = d_hin[:, :W] (+ sum_o d_oin[o][W:]),
 * d_ofr[o] = (d_oin[o][:W]) + mask[o] / max(sum mask, 1) * sum_h d_hin[h][W:]   (the d_oin terms only if d_oin != NULL).
 * Both outputs are written, not accumulated. */
typedef struct {
    const float* d_hin;
    const float* d_oin;
    const float* mask;
    float* d_hfr;
    float* d_ofr;
    int32_t bs, T, H, O, W;
    int32_t pad_;
} twog_entity_pool_bwd_t;
int twog_entity_pool_bwd(const twog_entity_pool_bwd_t* p, void* stream);

/* ===============================================================================================================
 * Fusion-level attention message passing (vhoi/models.py:1004-1475, :1693-1754) for message_type 'v2', granularity
 * 'v1' (generic), aggregation 'att', attention styles 'v2'/'v3' (dot / scaled dot product).
 * One instance = one (clip, frame) at frame level, one clip at segment level; entities: H humans, O objects, plus the
 * single-sender geometry relations. Per instance and relation with receiver r and senders s:
 *      w_rs = softmax_s( q_r . k_s * scale ) over non-virtual senders (objects_mask), NaN -> 0 (:1750-1753)
 *      out_r = [recv_mask_r] * sum_s w_rs * msg_s
 * relations: hh (human<-other humans), oh (human<-objects), sh (human<-geometry), ho (object<-humans),
 *            so (object<-geometry), oo (object<-other objects). A relation is off when its msg ptr is NULL.
 * =============================================================================================================== */
typedef struct {
    twog_rows_t feat_h;  /* [inst*H][D] query/key features of humans */
    twog_rows_t feat_o;  /* [inst*O][D] of objects                   */
    twog_rows_t msg_hh, msg_ho; /* [inst*H][hidden] messages sent BY humans (to humans / to objects)          */
    twog_rows_t msg_oh, msg_oo; /* [inst*O][hidden] messages sent BY objects (to humans / to objects)         */
    twog_rows_t msg_so, msg_sh; /* [inst][hidden]   messages sent by the geometry node (to objects / humans)  */
    twog_rows_t out_hh, out_oh, out_sh; /* [inst*H][hidden] received by humans  */
    twog_rows_t out_ho, out_so, out_oo; /* [inst*O][hidden] received by objects */
    const float* obj_mask; /* [clips][O], clip = inst / inst_per_clip; NULL => all real */
    float* att;            /* saved weights [inst][H*H + H*O + O*H + O*O] (hh, oh, ho, oo); NULL ok in forward */
    int32_t n_inst, inst_per_clip, H, O, D, hidden;
    float scale;           /* 1 ('v2') or 1/sqrt(D) ('v3', :1745) */
    int32_t recv_mask_ho;  /* 1: out_ho and out_so are multiplied by obj_mask of the receiver (frame level,
                              vhoi/models.py:720,729); 0: not (segment level, :841-843) */
} twog_attn_t;
int twog_attn_fwd(const twog_attn_t* a, int n, void* stream);
int twog_attn_limits(int* max_h, int* max_o);

typedef struct {
    twog_attn_t f;       /* the forward descriptor (features, messages, saved att; out_* unused) */
    twog_rows_t dout_hh, dout_oh, dout_sh, dout_ho, dout_so, dout_oo; /* incoming gradients wrt out_*         */
    twog_rows_t dmsg_hh, dmsg_ho, dmsg_oh, dmsg_oo, dmsg_so, dmsg_sh; /* out: gradient wrt sender messages    */
    twog_rows_t dfeat_h, dfeat_o; /* out: gradient wrt features [..][D]                                       */
    const float* dw_extra;        /* optional [n_inst][natt]: added to dL/d(weights) before the softmax backward (the
                                     part of the gradient that reaches the weights outside this kernel: twog_ssp_bwd) */
    int32_t dfeat_accumulate;     /* 1: dfeat += */
    int32_t relu_mask_dmsg;       /* 1: dmsg *= (msg > 0), i.e. gradient wrt the pre-ReLU activation of the message MLP */
} twog_attn_bwd_t;
int twog_attn_bwd(const twog_attn_bwd_t* a, int n, void* stream);

/* Code path the most recent twog_attn_fwd / twog_attn_bwd launch of this thread selected (host-side decisions, taken
 * over all descriptors of the launch); tests assert it, so that a case written for one path cannot silently move to
 * another when a boundary changes. A call that launches nothing (no instances, an error) leaves the word as it was. */
#define TWOG_ATTN_PATH_STAGED          1  /* latency regime: message / gradient rows staged in LDS, two workgroups per instance */
#define TWOG_ATTN_PATH_GRAM_COLUMNS    2  /* forward: Gram matrix column-parallel from global memory (<= 10 entities)   */
#define TWOG_ATTN_PATH_DW_COLUMNS      4  /* backward, streaming: dL/dw column-parallel, one relation after the other  */
#define TWOG_ATTN_PATH_DW_WAVE_GROUPS  8  /* backward, staged: every descriptor takes the wave-group dL/dw (H <= 2, O <= 8) */
#define TWOG_ATTN_PATH_BACKWARD        16 /* written by twog_attn_bwd (else by twog_attn_fwd)                           */
#define TWOG_ATTN_PATH_THREADS_SHIFT   16 /* workgroup size = word >> 16                                                */
int twog_attn_last_path(void);

/* ===============================================================================================================
 * Segment-level gated bidirectional recurrence with message passing (vhoi/models.py:785-880, :1535-1564,
 * :1051, :1145, :1239, :1334). Buffers are (clip, time, entity)-ordered; [2] = direction (0 forward, 1 backward).
 * nsh/nso = number of enabled sender MLPs on human/object states ((hh|ho) / (oh|oo)); nmh/nmo = number of message
 * blocks received by a human/object ((hh|oh) / (ho|oo)).
 * =============================================================================================================== */
typedef struct {
    int32_t bs, T, H, O, hidden;
    int32_t msg_segment;                    /* message_segment */
    int32_t rel_hh, rel_ho, rel_oh, rel_oo; /* enabled relations */
    float att_scale;
    int32_t pad_;
    const float* gi_h;     /* [bs][T][H][6h] frame part of W_ih x + b_ih: fcell cols [0,3h), bcell [3h,6h) */
    const float* gi_o;     /* [bs][T][O][6h] */
    const float* u_h;      /* hard gates [bs][T][H] */
    const float* u_o;      /* [bs][T][O] */
    const float* obj_mask; /* [bs][O] */
    const float* w_hh_h[2]; const float* b_hh_h[2]; /* human_segment_rnn_{f,b}cell.weight_hh [3h][h], bias_hh */
    const float* w_hh_o[2]; const float* b_hh_o[2];
    const float* w_ihm_h[2]; /* &weight_ih[0][first message column] of the human cells, row stride ld_ih_h */
    const float* w_ihm_o[2];
    int64_t ld_ih_h, ld_ih_o;
    const float* w_smsg_h; const float* b_smsg_h; /* packed sender MLPs on human states [(nsh*h)][h], [(nsh*h)] */
    const float* w_smsg_o; const float* b_smsg_o; /* packed sender MLPs on object states */
    float* hs_h;    /* out [bs][T][H][2h] (forward | backward states) */
    float* hs_o;    /* out [bs][T][O][2h] */
    float* save_h;  /* [2][bs][T][H][4h] */
    float* save_o;  /* [2][bs][T][O][4h] */
    float* msrc_h;  /* [2][bs][T][H][nsh*h] post-ReLU sender messages from humans */
    float* msrc_o;  /* [2][bs][T][O][nso*h] */
    float* mg_h;    /* [2][bs][T][H][nmh*h] aggregated messages received by humans */
    float* mg_o;    /* [2][bs][T][O][nmo*h] */
    float* att;     /* [2][T][bs][H*H + 2*H*O + O*O] */
    float* tmp_gim_h; /* scratch [2][bs*H][3h] */
    float* tmp_gim_o; /* scratch [2][bs*O][3h] */
    float* tmp_gh_h;  /* scratch [2][bs*H][3h] */
    float* tmp_gh_o;  /* scratch [2][bs*O][3h] */
    float* zeros;     /* [bs*max(H,O)][h] zeros */
} twog_segrnn_t;
int twog_segrnn_fwd(const twog_segrnn_t* desc, void* chain_ws, size_t chain_ws_bytes, void* stream); /* chain_ws: see twog_gemm_f32_chain */
/* The same forward recurrence as ONE persistent launch (csrc/seg_persist.hip; small batches): per (direction, clip chunk)
 * and slice of 16 hidden units four workgroups -- P1a / P1b: sender MLPs, attention weights (the chunk's Gram matrix on the
 * matrix cores), aggregated messages received by humans / objects and W_hh h_prev; P2h / P2o: W_ih[:, messages] on the
 * complete message rows, gate math, h_t -- two in-launch hand-offs per step (agent-scope counters, write-through stores,
 * sc1 loads). Same inputs, outputs and saved tensors as twog_segrnn_fwd (tmp_gim_* / zeros unused, tmp_gh_* carries
 * W_hh h_prev between the roles). twog_segrnn_persistent_supported: 2 = served on the current device (message_segment with
 * all four relations, hidden 64 / 128 / 256 / 512, a chunk of clips fits one 16-row tile of humans and at most two of
 * objects, 2 x chunks x 4 x hidden / 16 workgroups fit the device), 0 = not served. sync: device memory,
 * twog_segrnn_persistent_sync_bytes(), ZERO at launch; its last 128-byte line is the error word (uint32 index
 * bytes / 4 - 32). Residency and soft failure: exactly as twog_bigru_fwd_persistent (TWOG_PERSIST_NOT_RESIDENT; error word
 * != 0 after the launch -> re-run the pass with twog_segrnn_fwd on the same buffers). */
int twog_segrnn_persistent_supported(const twog_segrnn_t* desc);
size_t twog_segrnn_persistent_sync_bytes(void);
int twog_segrnn_fwd_persistent(const twog_segrnn_t* desc, void* sync, void* stream);

typedef struct {
    const float* d_hs_h; /* [bs][T][H][2h] gradient wrt hs_h */
    const float* d_hs_o;
    float* d_gi_h;  /* out [bs][T][H][6h] gradient wrt the full W_ih x + b_ih (frame + message part) */
    float* d_gi_o;
    float* d_gh_h;  /* out [bs][T][H][6h] gradient wrt W_hh h_prev + b_hh */
    float* d_gh_o;
    float* d_u_h;   /* += [bs][T][H] gradient wrt the hard gates (caller zeroes) */
    float* d_u_o;
    float* d_pre_h; /* out [2][bs][T][H][nsh*h] gradient wrt the pre-ReLU sender-MLP activations */
    float* d_pre_o;
    float* carry_h; /* scratch [2][bs*H][h] */
    float* carry_o; /* scratch [2][bs*O][h] */
    float* tmp_dmg_h; /* scratch [2][bs*H][nmh*h] */
    float* tmp_dmg_o; /* scratch [2][bs*O][nmo*h] */
    float* trash;     /* scratch [bs*max(H,O)][h] */
    /* scratch [2][T][16][bs*H] / [2][T][16][bs*O] or NULL. When both are given, the gate backward of chain step s-1 runs
     * in the epilogue of the last GEMM of step s (no separate gate launches) and parks its per-row partial sums of
     * d_u here; they are added into d_u_* in fixed order after the loop (bit-reproducible). NULL: separate launches. */
    float* du_part_h;
    float* du_part_o;
} twog_segrnn_bwd_t;
int twog_segrnn_bwd(const twog_segrnn_t* desc, const twog_segrnn_bwd_t* bdesc, void* chain_ws, size_t chain_ws_bytes,
                    void* stream);
/* Backward through time as ONE persistent launch (csrc/seg_persist.hip; the shapes twog_segrnn_persistent_supported
 * serves): per slice of 16 columns Q2h / Q2o keep the carried state gradient of their units in registers, run the gate
 * backward and publish d_gi / d_gh columns; Q1h / Q1o turn the complete d_gi rows into the gradients of the aggregated
 * messages, and those -- with the SAVED attention weights -- into d_pre columns and their slice's share of the score
 * gradients; two in-launch hand-offs per step. Same outputs as twog_segrnn_bwd (carry_*, tmp_dmg_*, trash, du_part_* unused).
 * scratch: twog_segrnn_bwd_persistent_scratch_bytes(desc) bytes of device memory, contents undefined. sync, residency and
 * soft failure as for twog_segrnn_fwd_persistent (after a launch that gave up d_u_* are untouched). */
size_t twog_segrnn_bwd_persistent_scratch_bytes(const twog_segrnn_t* desc);
int twog_segrnn_bwd_persistent(const twog_segrnn_t* desc, const twog_segrnn_bwd_t* bdesc, void* scratch, size_t scratch_bytes,
                               void* sync, void* stream);
/* What the two persistent launches would launch with for the SHAPE of *desc -- bs, T, H, O, hidden, msg_segment, rel_* -- on
 * n_cus compute units (n_cus <= 0: those of the current device): host arithmetic only, nothing is launched, and with n_cus > 0
 * no device is touched. The launchers, twog_segrnn_persistent_supported and twog_segrnn_bwd_persistent_scratch_bytes take their
 * numbers from the same code. A pure shape query: no pointer of *desc is read or tested (they may all be NULL); the report says
 * what a launch with valid buffers does, where the launchers themselves also refuse a descriptor without gi_* / u_*.
 * out: int32 [TWOG_SEGRNN_PLAN_INTS], written whole:
 *   out[0]  1 = served, 0 = not served (hidden not 64 / 128 / 256 / 512, message_segment or a relation off, H not 1 .. 4, O not
 *           1 .. 12, a chunk of clips beyond one 16-row tile of humans or two of objects, fewer than 8 x hidden / 16 compute
 *           units); every field below except out[15] is then 0
 *   out[1]  cpc, clips per chunk; out[2] n_chunks, chunks per direction: chunk c holds clips [c cpc, min(bs, (c + 1) cpc));
 *           out[3] clips of the last chunk (< cpc: ragged)
 *   out[4]  mh, out[5] mo: 16-row tiles of a chunk's human / object rows -- the forward launch runs seg_persist_fwd_kernel
 *           <mh, mo>, the backward seg_persist_bwd_kernel<mh, mo, x3q1>
 *   out[6]  pair_mask: bit (8 i + j), i <= j, set when Gram tile (i, j) of the chunk's row tiles (humans first) holds two rows
 *           of one clip; the other tiles are not computed
 *   out[7]  grid of either launch: 2 directions x n_chunks x 4 roles x hidden / 16 workgroups of 256 threads
 *   out[8]  dynamic LDS bytes of the forward launch, out[9] of the backward launch
 *   out[10] x3q1: 1 when the backward instance multiplies Q1's products with the 3 x bf16 split (hidden >= 256)
 *   out[11] dw_pad: floats of a slice's parked dL/dw share per (direction, step, chunk, kind)
 *   out[12] uint32 words of `sync` the counters use (2 x n_chunks x 4 lines of 32); they end below the error word
 *   out[13], out[14] bytes of the backward launch's scratch (twog_segrnn_bwd_persistent_scratch_bytes): out[13] + 2^31 out[14]
 *   out[15] the compute-unit count the plan was made for
 * Returns 0 (also for a shape that is not served), -2 for a NULL argument, or the negative HIP error of the device query. */
#define TWOG_SEGRNN_PLAN_INTS 16
int twog_segrnn_persistent_plan(const twog_segrnn_t* desc, int n_cus, int32_t* out);
/* hipGraph cache of the time loops (twog_bigru_*, twog_segrnn_*): number of captured loops and of hash-bucket hits whose
 * descriptor bytes differed (each was resolved by the byte compare; see csrc/graph_cache.h). Diagnostics / tests. */
int twog_graph_cache_stats(int64_t* entries, int64_t* collisions);

/* ===============================================================================================================
 * Optional position features and the less common gate strategies (disabled in every shipped configuration).
 * twog_pos_embed_fwd: out[(b,t,e)][hidden] = relu(w * s + b) (positional_encoding_style 'e': time_position_mlp /
 *   segment_length_mlp = build_mlp([1, h], ['relu']), vhoi/models.py:259-264) or the periodic embedding
 *   [sin(s / w_k) | cos(s / w_k)], w_k = 1e4^(k / (h/2 - 1)) (make_periodic_embedding, :1778-1794). The scalar s of row
 *   (b,t,e) is s[row] when `s` is given, else the time feature (t + 1) (/ steps[b] when `divide`;
 *   _assemble_time_tensor, :935-952). s_out (optional) receives the scalars [bs*T*E] for the backward pass.
 * twog_periodic_embed_bwd: ds[row] of the periodic embedding (the 'e' style uses a GEMM and twog_colsum).
 * twog_seglen_fwd / _bwd: _assemble_segment_length_tensor (:954-981): per (clip, entity) scan over time of the hard
 *   gates u [bs][T][E]; the backward ADDS into du.
 * twog_mul: out[i] = a[i] * b[i] (+ out[i] if accumulate): 'conditional_on_human' object gates (:1531-1532).
 * twog_scale_rows: x[r][:] *= s[r] (receiver mask of a relational message, :720/:729).
 * =============================================================================================================== */
int twog_pos_embed_fwd(const float* s, const float* steps, int bs, int T, int E, int divide, const float* w,
                       const float* b, int periodic, int hidden, twog_rows_t out, float* s_out, void* stream);
int twog_periodic_embed_bwd(twog_rows_t dout, const float* s, int rows, int hidden, float* ds, void* stream);
int twog_seglen_fwd(const float* u, const float* steps, int bs, int T, int E, int divide, float* s_out, void* stream);
int twog_seglen_bwd(const float* u, const float* steps, int bs, int T, int E, int divide, const float* ds, float* du,
                    void* stream);
int twog_mul(const float* a, const float* b, float* out, int64_t n, int accumulate, void* stream);
int twog_scale_rows(twog_rows_t x, const float* s, int rows, int cols, void* stream);

/* ===============================================================================================================
 * Sender-side projection of aggregated messages. The objects' segment-level GRUCells read
 * cat[h_f, m_ho, m_so, m_oo] (vhoi/models.py:748) through W_ih; m_ho[k] = mask_k sum_h att[k][h] msg_h (:1099-1143, :720)
 * and m_so[k] = mask_k msg_s (:1384-1429, :729) are linear in the senders' messages, so the caller projects the H + 1
 * sender rows of a frame (GEMM) and these kernels scatter / gather them over the O receivers:
 *   fwd: gi[(inst,k)][:] += mask[clip][k] * ( sum_h att[inst][att_off + k*H + h] * ph[(inst,h)][:] + ps[inst][:] )
 *   bwd: qh[(inst,h)][:] = sum_k mask_k att[k][h] dgi[(inst,k)][:]   qs[inst][:] = sum_k mask_k dgi[(inst,k)][:]
 *        dw[inst][att_off + k*H + h] = mask_k <dgi[(inst,k)], ph[(inst,h)]>   (feeds twog_attn_bwd's dw_extra)
 * ph / ps / qh / qs may be NULL (relation off). cols % 4 == 0, H <= 4, O <= 16.
 * =============================================================================================================== */
int twog_ssp_fwd(float* gi, const float* ph, const float* ps, const float* att, const float* mask, int n_inst,
                 int inst_per_clip, int H, int O, int cols, int natt, int att_off, void* stream);
/* gather alone, with arbitrary placement: qh[(inst,h)][c] = sum_k att(inst)[att_off + k*H + h] * dgi[(inst*O + k)*dgi_ld + c],
 * att(inst) = att + clip*att_ld_clip + frame*att_ld_frame. Used for the segment-level human->object message block of the
 * objects' W_ih gradient (its weights are stored [time][clip][natt], the two directions share the d_gi rows). */
int twog_ssp_gather(const float* dgi, int64_t dgi_ld, const float* att, int64_t att_ld_clip, int64_t att_ld_frame,
                    int att_off, float* qh, int n_inst, int inst_per_clip, int H, int O, int cols, void* stream);
int twog_ssp_bwd(const float* dgi, const float* ph, const float* att, const float* mask, float* qh, float* qs, float* dw,
                 int n_inst, int inst_per_clip, int H, int O, int cols, int natt, int att_off, void* stream);

/* ===============================================================================================================
 * General message passing of ONE relation (receiver set R, sender set S per instance): the message / aggregation forms
 * of the reference beyond the shipped one (twog_attn_* covers sender-only messages + dot-product attention for the
 * four entity relations at once): relational messages (compute_relational_message, vhoi/models.py:1667-1690),
 * 'specific' granularity (:1712-1713), attention styles 'concat' / 'general' (:1739-1746), distance-based attention
 * (:1757-1775) and mean pooling (:1034-1037). Linear layers on cat[receiver, sender] are split by the caller into a
 * receiver and a sender projection (GEMMs); this kernel combines them per pair:
 *      out[r] = recv_mask[r] * sum_s w[r][s] * M(r, s)
 *      M(r, s) = msg[s]                              (TWOG_REL_MSG_SENDER)
 *              = relu(p_r[r] + p_s[s])               (TWOG_REL_MSG_PAIR)
 *      w[r][.] = send_mask[s]                        (TWOG_REL_SUM: masked sum, relational)
 *              = softmax_s(scale <q[r], k[s]> + score_bias [relu])   (TWOG_REL_DOT; 'general': k = A k precomputed)
 *              = softmax_s(relu(a_r[r] + c_s[s]))    (TWOG_REL_ADDITIVE: 'concat')
 *              = softmax_s(1 / (dist[r][s] + 1e-7)), dist == 0 excluded     (TWOG_REL_DISTANCE)
 *              = 1 / max(#valid senders, 1)          (TWOG_REL_MEAN)
 * over the valid senders (send_mask != 0, and s != r when exclude_self); no valid sender -> all-zero weights (the
 * reference's NaN -> 0). Rows of one instance must be equally strided (inner <= 1 or inner == R resp. S).
 * No receivers (R == 0, or n_inst <= 0): a descriptor that passes the checks is a no-op in every entry point below, also
 * inside a multi-descriptor call: no buffer is read or written, gradient buffers that do not accumulate are NOT cleared.
 * =============================================================================================================== */
#define TWOG_REL_SUM 0
#define TWOG_REL_DOT 1
#define TWOG_REL_ADDITIVE 2
#define TWOG_REL_DISTANCE 3
#define TWOG_REL_MEAN 4
#define TWOG_REL_MSG_SENDER 0
#define TWOG_REL_MSG_PAIR 1
typedef struct {
    twog_rows_t q, k;        /* [inst*R][D], [inst*S][D]      (TWOG_REL_DOT) */
    twog_rows_t msg;         /* [inst*S][hidden]              (TWOG_REL_MSG_SENDER) */
    twog_rows_t p_r, p_s;    /* [inst*R][hidden], [inst*S][hidden] (TWOG_REL_MSG_PAIR) */
    twog_rows_t out;         /* [inst*R][hidden] */
    const float* a_r;        /* [inst*R] (TWOG_REL_ADDITIVE; the layer's bias folded in) */
    const float* c_s;        /* [inst*S] */
    const float* dist;       /* element (inst, r, s) at inst*dist_ld_inst + r*dist_ld_r + s*dist_ld_s (TWOG_REL_DISTANCE) */
    int64_t dist_ld_inst, dist_ld_r, dist_ld_s;
    const float* send_mask;  /* [clip][S] or NULL */
    const float* recv_mask;  /* [clip][R] or NULL */
    float* att;              /* out (fwd): weights [inst][R][S], or NULL */
    const float* score_bias; /* device scalar added to the dot score (the Bilinear bias of 'general'), or NULL */
    float scale;
    int32_t score_mode, msg_mode, relu_scores, exclude_self;
    int32_t n_inst, inst_per_clip, R, S, D, hidden;
    int32_t pad_;
} twog_relation_t;
int twog_relation_limits(void); /* max R, S */
int twog_relation_fwd(const twog_relation_t* rel, void* stream);
typedef struct {
    twog_relation_t f;
    twog_rows_t dout;        /* [inst*R][hidden] gradient wrt out */
    twog_rows_t dmsg;        /* out [inst*S][hidden] (MSG_SENDER; NULL = not needed) */
    twog_rows_t dp_r, dp_s;  /* out (MSG_PAIR) */
    twog_rows_t dq, dk;      /* out [..][D] (DOT; NULL = not needed) */
    float* da_r;             /* out [inst*R] (ADDITIVE) */
    float* dc_s;             /* out [inst*S] */
    float* dscore_sum;       /* out [inst]: sum over the pairs of d(raw score) = d score_bias per instance (DOT), or NULL */
    int32_t dq_accumulate, dk_accumulate; /* add into dq / dk instead of overwriting */
    int32_t relu_mask_dmsg;  /* dmsg *= (msg > 0): the sender MLP's ReLU folded in */
    int32_t pad_;
} twog_relation_bwd_t;
int twog_relation_bwd(const twog_relation_bwd_t* rel, void* stream);
/* n relations per call, several descriptors per launch: the general segment-level loop (vhoi/models.py:785-880 with the
 * message forms above) issues all relations of both directions of a chain step together. The descriptors of one call
 * must not ACCUMULATE into the same rows (dq / dk with *_accumulate set): they run concurrently. */
int twog_relation_fwd_n(const twog_relation_t* rels, int n, void* stream);
int twog_relation_bwd_n(const twog_relation_bwd_t* rels, int n, void* stream);

/* ===============================================================================================================
 * Segment-boundary gates (vhoi/models.py:1477-1533, :1620-1627; pyrutils/torch/distributions.py:4-53) with
 * discrete_networks_num_layers == 1: p = sigmoid(w . [column blocks of the entity row] + b); 'gs': Gumbel-sigmoid
 * with PRE-DRAWN noise, 'st' (noise == NULL): straight-through; hard = soft > thr; last step forced to 1 (:701-702).
 * Rows are (b, t, e)-ordered; hard/soft/p_save are [bs][T][E].
 * =============================================================================================================== */
typedef struct {
    twog_rows_t x;        /* entity rows; gate input = concat of n_seg column blocks of width `hidden` */
    int32_t seg_col[8];   /* starting column in x of weight block i */
    int32_t n_seg, hidden;
    const float* w;       /* [n_seg*hidden] */
    const float* b;       /* [1] or NULL    */
    const float* noise;   /* Gumbel noise [T][noise_entities][bs][2] (reference call order) or NULL ('st') */
    float* hard;
    float* soft;
    float* p_save;
    int32_t bs, T, E;
    int32_t noise_entities, noise_offset; /* this type's entity e uses noise slot noise_offset + e */
    int32_t force_last;   /* 1: hard[:, T-1, :] = 1 and no gradient through it */
    float threshold;
    int32_t pad_;
} twog_gate_t;
int twog_gate_fwd(const twog_gate_t* g, void* stream);
/* dlogit[row] = (d_soft[row] + d_hard[row]*st_mask[row]) * d soft / d logit. d_soft, d_hard, st_mask may be NULL
 * (st_mask NULL => 1; with force_last the last step's d_hard is dropped). */
int twog_gate_bwd(const twog_gate_t* g, const float* d_hard, const float* d_soft, const float* st_mask, float* dlogit,
                  void* stream);
/* twog_gumbel_noise_fill: the 'gs' noise drawn on the device instead of on the host's default generator (the reference's
 * sample_gumbel / gumbel_sigmoid, pyrutils/torch/distributions.py:4-36: g = -log(-log(u)), one (bs, 2) draw per gate call).
 * Fills noise[T][noise_entities][bs][2], the layout twog_gate_t.noise is read in. The pair at (t, slot, b) is a pure function
 * of (seed, calls, clip_offset + b, t, slot) and of nothing else -- not of bs, T, noise_entities, the launch geometry or the
 * rank that holds the clip -- through Philox4x32-10 (Salmon et al., SC'11; 10 rounds):
 *   multipliers M0 = 0xD2511F53, M1 = 0xCD9E8D57; Weyl constants W0 = 0x9E3779B9, W1 = 0xBB67AE85;
 *   one round: c' = [hi(M1*c2) ^ c1 ^ k0, lo(M1*c2), hi(M0*c0) ^ c3 ^ k1, lo(M0*c0)], then k0 += W0, k1 += W1;
 *   key     = (low, high 32 bits of state[0])                                   -- the seed
 *   counter = (calls low, calls high, clip_offset + b, t * 256 + slot)          -- calls = state[1]
 *   output words w0, w1 (w2, w3 unused): u_i = ((w_i >> 9) + 0.5f) * 2^-23, exact in fp32 and inside [2^-24, 1 - 2^-24];
 *   g_i = -logf(-logf(u_i)): finite by construction, about [-2.81, 16.64].
 * state: two DEVICE int64 words [seed, calls]. The fill reads both from the device and the same call then advances calls by
 * one, behind the fill in stream order (a second, one-thread launch): the host neither reads nor writes the call number, so
 * the two launches captured into a graph draw the next call's noise at every replay. clip_offset: index of this buffer's clip 0
 * in the global batch (data parallel: rank * bs). words_or_null: when non-NULL also receives the raw Philox output
 * [T][noise_entities][bs][4] (the generator checked bit for bit; 16-byte aligned). noise must be 8-byte aligned.
 * Returns -1 for state == NULL, noise_entities > 256, T >= 2^24, a negative size or a misaligned buffer, -2 for
 * T * noise_entities * bs >= 2^31. */
int twog_gumbel_noise_fill(float* noise, int T, int noise_entities, int bs, uint32_t clip_offset, int64_t* state,
                           uint32_t* words_or_null, void* stream);
/* twog_augment_inputs: random augmentation of a batch's inputs, in place, on the device. No counterpart in the reference
 * trainer (its loaders hand the stored features over unchanged); SGN, the model Geo_gcn is taken from, rotates its skeletons
 * at random in its loader. Two parts, each skipped when its options are neutral:
 *   geometry  one similarity transform per clip of the (x, y, vx, vy) nodes in the last 4 * N floats of every x_human row
 *             (the layout data_loading._pos_vel writes for all three data sets);
 *   features  uniform jitter and dropout of the first geo_offset channels of the human rows and of all F_o channels of the
 *             object rows.
 * A clip's draw is a pure function of (seed, epoch, clip id, element) and of nothing else -- not of the batch's composition or
 * size, the rank that holds the clip or the launch geometry -- through Philox4x32-10 (constants and round: see
 * twog_gumbel_noise_fill) keyed apart from the Gumbel noise and per part:
 *   key     = (seed low, seed high ^ TAG),  TAG = TWOG_AUGMENT_TAG_GEOMETRY / _HUMAN / _OBJECT      -- seed  = state[0]
 *   counter = (epoch low, epoch high, clip id, index)                                                -- epoch = state[1]
 *   a word w becomes r = 2u - 1 with u = ((w >> 9) + 0.5f) * 2^-23: exact in fp32 (an odd numerator below 2^23), |r| < 1.
 * Every operation below is one fp32 operation rounded once (no contraction, correctly rounded division, no transcendentals),
 * so that a numpy restatement (tests/augment_ref.py) gives the same bits.
 * Geometry: index 0, words -> r0..r3; the rotation is drawn through the tangent of the half angle:
 *   t = tan_half_max * r0;  q = t * t;  c = (1 - q) / (1 + q);  s = (t + t) / (1 + q);  g = 1 + scale_max * r1;
 *   a = g * c;  b = g * s;  tx = shift_max * r2;  ty = shift_max * r3;
 * for every human row, every frame t < steps[b] and every node with x != 0 or y != 0 (a node at exactly (0, 0) is a missing
 * object or a padded frame and stays zero), with dx = x - cx, dy = y - cy:
 *   x' = ((a * dx - b * dy) + cx) + tx;   y' = ((b * dx + a * dy) + cy) + ty;   vx' = a * vx - b * vy;   vy' = b * vx + a * vy
 * (velocities take the linear part only, so v = (p_next - p_cur) * 100 stays true; all H human rows carry the same context
 * block and get the same transform). The distance tensors of the batch are NOT touched: they are normalised by the image size
 * per axis, so no similarity transform maps onto them.
 * Features: frames t < steps[b] only, objects with objects_mask > 0 only. Element e = (t * E + entity) * F + channel is numbered
 * over the whole row block of the clip (E = H, F = F_h, the geometry tail included / E = O, F = F_o), whatever the access
 * width; it uses index = e >> 1 and the words 2 * (e & 1) (dropout) and 2 * (e & 1) + 1 (jitter):
 *   keep = (w_drop >> 8) >= drop_threshold;   x' = keep ? (x + amp * r) * keep_scale : 0
 * with drop_threshold = round(p * 2^24) < 2^24, amp = noise_std * sqrt(3) (uniform jitter of the variance the option names)
 * and keep_scale = 1 / (1 - p) made by the caller in fp64 and passed as fp32.
 * Neutral options issue nothing: tan_half_max = scale_max = shift_max = 0 -> no geometry launch; amp = 0 and
 * drop_threshold = 0 -> no feature launch. At most three launches: the parameters (only with params_out), geometry, features.
 * state: two DEVICE int64 words [seed, epoch], read by the kernels and never by the host (a captured launch draws anew after the
 * epoch has moved on); clip_ids: DEVICE int64 [bs], 0 <= id < 2^32 (the low 32 bits are the counter word).
 * Returns -1 for a NULL descriptor, a negative size, geo_offset + 4 * N != F_h, drop_threshold >= 2^24, a pointer that is not
 * aligned to its element (4 bytes; 8 for clip_ids and state), a missing clip_ids / state / x_human or 2^62 elements and more;
 * -2 for a clip whose row block T * H * F_h or T * O * F_o exceeds 2^33 elements (e >> 1 is a 32-bit counter word).
 * The 16-byte form of the feature pass serves a tensor whose base is 16-byte aligned and whose F (and geo_offset) is a multiple
 * of 4, the scalar form any other. */
#define TWOG_AUGMENT_TAG_GEOMETRY 0x47454F4Du   /* 'GEOM' */
#define TWOG_AUGMENT_TAG_HUMAN    0x48554D4Eu   /* 'HUMN' */
#define TWOG_AUGMENT_TAG_OBJECT   0x4F424A53u   /* 'OBJS' */
typedef struct {
    float* x_human;              /* [bs][T][H][F_h], contiguous, written in place */
    float* x_objects;            /* [bs][T][O][F_o], contiguous, written in place; NULL = no objects */
    const int64_t* clip_ids;     /* [bs] */
    const float* steps;          /* [bs] frames per clip (the loader's steps_per_example) or NULL = T */
    const float* objects_mask;   /* [bs][O] or NULL = all present */
    const int64_t* state;        /* [2] = (seed, epoch) */
    float* params_out;           /* [bs][4] = (a, b, tx, ty) per clip or NULL: a test hook */
    int32_t bs, T, H, O, F_h, F_o;
    int32_t N, geo_offset;       /* nodes; F_h - 4 * N */
    float tan_half_max, scale_max, shift_max, cx, cy;
    float amp, keep_scale;
    uint32_t drop_threshold;
} twog_augment_t;
int twog_augment_inputs(const twog_augment_t* a, void* stream);
/* The grid of the two capped launches of twog_augment_inputs, host arithmetic only: workgroups for `work` workgroup-sized
 * items = (clip, frame, entity) rows of the feature pass, which takes one row per workgroup and trip, or groups of 256 nodes of
 * the geometry pass. A workgroup makes a second trip exactly when work exceeds the answer. -2 for negative work. */
int twog_augment_grid(int64_t work);
/* dst[r][c] += s[r] * v[c]  (gate input gradient, one call per column block) */
int twog_rank1_update(twog_rows_t dst, const float* s, const float* v, int rows, int cols, void* stream);
/* out[c] (+)= sum_r rowscale[r] * x[r][c] (rowscale NULL => 1): bias gradients and gate weight gradients.
 * Deterministic two-pass reduction; partials: scratch [n_blocks][cols]. */
int twog_colsum(twog_rows_t x, const float* rowscale, int rows, int cols, float* out, int accumulate,
                float* partials, int n_blocks, void* stream);
/* Several column sums in one pair of launches (the bias gradients of a backward stage collected by the host: 45 per training
 * step). Problem i: out[c] (+)= sum_r rowscale[r] * x[r][c] with the arithmetic -- and so, bit for bit, the results -- of its own
 * twog_colsum call with the default row slicing. partials: scratch of twog_colsum_n_partial_floats(ops, n) floats (the chunks of
 * TWOG_COLSUM_MAX problems of one call run one after the other and share it). */
#define TWOG_COLSUM_MAX 16
typedef struct {
    twog_rows_t x;
    const float* rowscale;  /* [rows] or NULL */
    float* out;             /* [cols] */
    int32_t rows, cols;
    int32_t accumulate;
    int32_t pad_;
} twog_colsum_t;
size_t twog_colsum_n_partial_floats(const twog_colsum_t* ops, int n);
int twog_colsum_n(const twog_colsum_t* ops, int n, float* partials, size_t partial_floats, void* stream);

/* filter_soft_decisions (vhoi/models.py:1637-1664): local-maximum filter on soft gates [bs][T][E];
 * grad_mask = d hard / d soft (0 or 1) under the reference's straight-through + clamp semantics. */
int twog_filter_fwd(const float* soft, float* hard, float* grad_mask, int bs, int T, int E, float threshold,
                    void* stream);

/* reorder_hidden_states (vhoi/models.py:1567-1586) without the host sync: out[b,t,e,:] = hx[b,idx,e,:], idx = first
 * frame >= t whose gate is non-zero (t itself if none). hx/out: [bs][T][E][cols], gate: [bs][T][E]. */
int twog_reorder_fwd(const float* hx, const float* gate, float* out, int bs, int T, int E, int cols, void* stream);
int twog_reorder_bwd(const float* dout, const float* gate, float* dhx, int bs, int T, int E, int cols, void* stream);

/* Label-head epilogue (vhoi/models.py:909-917): log_softmax over classes of logits [(b,t,e)][C] + the
 * permute(0,3,1,2) store to [bs][C][T][E]; backward returns dlogits [(b,t,e)][C]. */
int twog_logsoftmax_permute_fwd(const float* logits, float* out, int bs, int T, int E, int C, void* stream);
int twog_logsoftmax_permute_bwd(const float* out, const float* dout, float* dlogits, int bs, int T, int E, int C,
                                void* stream);

/* Elementwise helpers between GEMMs in the backward pass: dx = dy * (y > 0) (ReLU'), dst += src. */
int twog_relu_bwd(twog_rows_t dy, twog_rows_t y, twog_rows_t dx, int rows, int cols, void* stream);
int twog_add_rows(twog_rows_t src, twog_rows_t dst, int rows, int cols, void* stream);
/* Several of these small row-wise operations in one launch (same callers as twog_relu_bwd / twog_add_rows /
 * twog_rank1_update, issued once per dependency level by the general segment-level loop). No two operations of one call
 * may write the same rows. */
enum { TWOG_ROWOP_RELU_BWD = 0, TWOG_ROWOP_ADD = 1, TWOG_ROWOP_RANK1 = 2 };
typedef struct {
    twog_rows_t a, b, dst; /* RELU_BWD: dst = a * (b > 0);  ADD: dst += a;  RANK1: dst[r][c] += s[r] * v[c] */
    const float* s;        /* RANK1: [rows] */
    const float* v;        /* RANK1: [cols] */
    int32_t kind, rows, cols, pad_;
} twog_rowop_t;
int twog_rowops(const twog_rowop_t* ops, int n_ops, void* stream);

/* ===============================================================================================================
 * Replay of a recorded call sequence for the further steps of a loop (the general segment-level loop,
 * vhoi/models.py:785-880 with the message forms of twog_relation_*): the host composes two consecutive chain steps a, b
 * as lists of calls (kind, flags, descriptor array in HOST memory) without issuing them; every 64-bit word w of every
 * descriptor of step a + k is  w(a) + k * (w(b) - w(a))  -- per-step operands live in consecutive slots of per-step
 * buffers, everything else is equal in a and b. Runs steps k_begin <= k < k_end in order (k = 0 is step a itself);
 * the calls are exactly the entry points above. workspace: the split-K scratch handed to twog_gemm_f32.
 * =============================================================================================================== */
enum { TWOG_TAPE_GEMM = 0, TWOG_TAPE_RELATION_FWD = 1, TWOG_TAPE_RELATION_BWD = 2, TWOG_TAPE_GRU_STEP_FWD = 3,
       TWOG_TAPE_GRU_STEP_BWD = 4, TWOG_TAPE_ROWOPS = 5 };
typedef struct {
    int32_t kind;     /* TWOG_TAPE_* */
    int32_t n;        /* descriptors in the call */
    int32_t flags;    /* GEMM: bit 0 a_kmajor, bit 1 b_kmajor */
    int32_t pad_;
    const void* desc; /* host array of n descriptors of the kind's type */
} twog_tape_entry_t;
int twog_tape_run(const twog_tape_entry_t* step_a, const twog_tape_entry_t* step_b, int n_entries, int k_begin, int k_end,
                  void* workspace, size_t workspace_bytes, void* stream);

/* Fused Adam on one flat fp32 parameter buffer (torch.optim.Adam semantics; reference train.py:39). The gradient is
 * multiplied by grad_scale first (1/world_size after a sum all-reduce). */
/* Zero fill of `nbytes` bytes at `p` (any alignment) on `stream`: the step's workspace / gradient clears (torch.zeros and
 * Tensor.zero_() on the reference's path, e.g. optimizer.zero_grad(), pyrutils/torch/train_utils.py:146). */
int twog_fill_zero(void* p, size_t nbytes, void* stream);
/* Diagnostics (tests): n_blocks workgroups of 256 threads holding lds_bytes of LDS each spin for `usec` microseconds --
 * the co-tenant a persistent launch must survive (see TWOG_PERSIST_NOT_RESIDENT). No reference counterpart. */
int twog_debug_occupy(int n_blocks, int lds_bytes, int usec, void* stream);

/* Persistent launches checked at the end of a pass (see twog_bigru_fwd_persistent): `words` are the host-pinned copies of
 * their error words (device-readable), filled by asynchronous copies enqueued before this call. If any is non-zero, every
 * `out[i]` (n[i] floats) is overwritten with NaN -- the pass's results can then not be consumed silently while the host
 * check (which raises) is left for the end of the backward pass. Host plumbing; no counterpart in the reference. */
#define TWOG_GUARD_MAX 16
typedef struct {
    const uint32_t* words[TWOG_GUARD_MAX];
    float* out[TWOG_GUARD_MAX];
    int64_t n[TWOG_GUARD_MAX];
    int32_t n_words, n_out;
} twog_guard_t;
int twog_guard_outputs(const twog_guard_t* g, void* stream);

/* A stream restricted to n_cus compute units (hipExtStreamCreateWithCUMask; the low n_cus mask bits = n_cus / 8 CUs on each
 * XCD). Host plumbing of this library's own backward pass (weight-gradient GEMMs beside a launch-per-step recurrence that
 * leaves those CUs idle); no counterpart in the reference. Returns 0, or < 0 when the runtime refuses. */
int twog_stream_create_masked(int n_cus, void** stream_out);
/* A stream of the LOWEST priority the device offers (hipDeviceGetStreamPriorityRange / hipStreamCreateWithPriority): the side
 * stream of the same backward pass (TWOG_SIDE_PRIORITY=low) -- its GEMM workgroups then yield free compute units to the
 * launch-per-step recurrence on the caller's stream. Returns 0, or < 0 when the runtime refuses. */
int twog_stream_create_low_priority(void** stream_out);
int twog_stream_destroy(void* stream);
/* n_blocks <= TWOG_COPY_MAX copies dst[i] = src[i], i < n floats, of contiguous fp32 blocks in ONE launch. The host uses it
 * to rebuild, at EVERY forward call, the packed operands the time loops read (w_smsg_* / b_smsg_* of twog_segrnn_t: the
 * reference applies the four segment-level sender MLPs one by one, vhoi/models.py:1051-1098, :1145-1190, :1239-1285,
 * :1334-1383; here two of them share a GEMM). Nothing derived from a parameter is kept across calls. */
#define TWOG_COPY_MAX 16
typedef struct {
    const float* src;
    float* dst;
    int64_t n;
} twog_copy_t;
int twog_copy_blocks(const twog_copy_t* blocks, int n_blocks, void* stream);
int twog_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                   float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale, void* stream);

/* The launch geometry of the small streaming kernels that launch a CAPPED grid of TWOG_STREAM_THREADS-thread workgroups and
 * stride over the rest of the work. Host arithmetic only -- no GPU call; the launchers take their grid from the same function,
 * so the answer is what is launched. Returns the number of workgroups along x for `work` items: elements (rows * cols, the
 * largest operation of a twog_rowops call, the largest block of a twog_copy_blocks call) or, for FILL_ZERO, bytes. A thread
 * takes `per` = one element per trip, four in the _VEC kernels and COPY_BLOCKS, 16 bytes in FILL_ZERO. Some thread of the main
 * loop is SURE to make a second trip when  grid * TWOG_STREAM_THREADS * per  <  work - slack:  slack = 0 for the one-element
 * kernels (there the condition is also necessary); 3 for the _VEC kernels and COPY_BLOCKS, which stride over whole groups of
 * four (work / 4, rounded down; the n % 4 tail of a copy is a loop of its own); 30 for FILL_ZERO, whose 16-byte body excludes
 * up to 15 head bytes in front of the first 16-byte boundary and the bytes behind the last. A copy whose source or destination
 * is not 16-byte aligned takes one float per thread and trip on the same grid, so it makes further trips from a quarter of
 * that size on. `cols` is read by TWOG_STREAM_REORDER only: work = (clip, entity) pairs, the result = the column chunks
 * (gridDim.y) of twog_reorder_fwd / _bwd (1 for no pairs). -2 for an unknown kernel, negative work, or, with
 * TWOG_STREAM_REORDER, work or cols beyond INT32_MAX or negative cols. */
#define TWOG_STREAM_THREADS 256
#define TWOG_STREAM_RELU_BWD_VEC 0  /* twog_relu_bwd, 16-byte form (cols % 4 == 0, aligned rows) */
#define TWOG_STREAM_RELU_BWD 1      /* twog_relu_bwd, scalar form */
#define TWOG_STREAM_ADD_ROWS 2      /* twog_add_rows */
#define TWOG_STREAM_RANK1_VEC 3     /* twog_rank1_update, 16-byte form */
#define TWOG_STREAM_RANK1 4         /* twog_rank1_update, scalar form */
#define TWOG_STREAM_ROWOPS 5        /* twog_rowops (per launch of up to 16 operations) */
#define TWOG_STREAM_ADAM 6          /* twog_adam_step */
#define TWOG_STREAM_MUL 7           /* twog_mul */
#define TWOG_STREAM_SCALE_ROWS 8    /* twog_scale_rows */
#define TWOG_STREAM_COPY_BLOCKS 9   /* twog_copy_blocks */
#define TWOG_STREAM_FILL_ZERO 10    /* twog_fill_zero */
#define TWOG_STREAM_REORDER 11      /* twog_reorder_fwd / twog_reorder_bwd: column chunks */
/* (12 is not assigned: the launch-free plan's test keeps it as its example of an unknown id)
 * twog_optim_apply: a _VEC kernel over the 16-byte aligned body of the range. The body starts up to 3 elements into the range,
 * so with pointers that are not 16-byte aligned the slack is 6 instead of 3. */
#define TWOG_STREAM_OPTIM 13
int twog_stream_grid(int kernel, int64_t work, int64_t cols);

/* Adjacency attention of Geo_gcn (compute_similarity + s.matmul(x), pyrutils/torch/models_gcn.py:86-100, :30-34) on the
 * matrix cores with the theta / phi projections folded: md = [65][64] = Mt (Mt[n][k] = sum_o Wk[o][n] Wq[o][k]) followed
 * by d = Wk^T bq; per frame P = X M + d, adj = softmax_j(P X^T), z = adj X (identical to softmax(theta phi^T) X: the
 * dropped terms are constant along j). x: [n_frames*N][64], adj: [n_frames][N][N], z: [n_frames*N][64].
 * Backward: dx_att = d/dX through adj and z (X's own ReLU/W2 path excluded), partials[n_blocks][65*64] = per-workgroup
 * sums of (dMt | dd), n_blocks = twog_gcn_attn2_bwd_blocks(n_frames); the caller column-sums them (twog_colsum). */
int twog_gcn_attn2_fwd(const float* x, const float* md, int n_frames, int n_nodes, float* adj, float* z, void* stream);
int twog_gcn_attn2_bwd_blocks(int n_frames);
int twog_gcn_attn2_bwd(const float* x, const float* md, const float* adj, const float* dz, int n_frames, int n_nodes,
                       float* dx_att, float* partials, int n_blocks, void* stream);

/* ===============================================================================================================
 * Multi-task loss: the criterion the training loop applies to the model's output list
 * (vhoi/losses.py:8-70 select_loss; pyrutils/torch/losses.py:7-51 multi_task_loss, binary_cross_entropy_loss,
 * budget_loss; F.nll_loss with ignore_index, reduction 'mean'). All terms of the list run in ONE forward and ONE
 * backward launch; sums are fp64 and ordered (deterministic); nothing syncs with the host (the reference calls
 * mask.sum().item() per term).
 *   kind 0  NLL:    input [outer][C][inner] log-probabilities, target int64 [outer][inner];
 *                   loss = w * sum_{target != ignore} -input[o][target][i] / count            (count 0 -> NaN, as torch)
 *   kind 1  BCE:    input, target float [inner] (outer = C = 1); m = target != ignore;
 *                   loss = w * sum_m -(t*max(log x,-100) + (1-t)*max(log(1-x),-100)) / count   (count 0 -> 0)
 *   kind 2  budget: loss = w * sum_m x / count                                                 (count 0 -> 0)
 * stats[term] = {sum, count} is written by the forward call and read by the backward call, which stores
 * d(loss_total)/d(input) = dlosses[term] * d(loss_term)/d(input) into terms[i].dinput (skipped where dinput is NULL).
 * =============================================================================================================== */
typedef struct {
    int32_t kind;
    int32_t n_classes;
    int64_t outer, inner;
    const float* input;
    const void* target;
    float* dinput;
    float weight;
    float ignore_value;
} twog_loss_t;
#define TWOG_LOSS_MAX_TERMS 16
#define TWOG_LOSS_BLOCKS 64
/* partials: workspace of n_terms * TWOG_LOSS_BLOCKS * 2 doubles; losses: [n_terms] floats. */
int twog_multitask_loss_fwd(const twog_loss_t* terms, int n_terms, double* partials, double* stats, float* losses,
                            void* stream);
int twog_multitask_loss_bwd(const twog_loss_t* terms, int n_terms, const double* stats, const float* dlosses,
                            void* stream);

/* ===============================================================================================================
 * The same criterion with the two imbalance options: per-class weights on the NLL terms (F.nll_loss(weight=)) and the
 * positive-class weight of the BCE terms (pyrutils/torch/losses.py:17-18). A second pair of entry points with a struct of
 * its own; twog_loss_t and twog_multitask_loss_* above are unchanged. Same launch shape: a (TWOG_LOSS_BLOCKS, terms) grid,
 * TWOG_LOSS_BLOCKS fp64 partial sums per term added in a fixed order, then one sequential pass; stats[term] = {sum, den}
 * stays on the device for the backward call. Up to TWOG_LOSS_MAX_TERMS terms of all three kinds in one launch per direction.
 * No multiplication below is fused with an addition; (double) and (float) are conversions, fl() is one fp32 rounding.
 *
 * kind 0, NLL, class_weight cw ([n_classes] device floats; NULL: every cw = 1):
 *   an element (o, i) with target y is kept when y != ignore && 0 <= y < C (the rule of twog_loss_t)
 *   sum  = sum over kept of (double)cw[y] * (double)(-x[o][y][i])     (the product of two fp32 values is exact in fp64)
 *   den  = sum over kept of (double)cw[y]                            (NULL: the count of kept elements)
 *   loss = w * (float)(sum / den); 0 / 0 gives NaN, as torch gives for weight= with no kept weight
 *   g = w * dloss / (float)den in fp32, 0 when den <= 0
 *   d x[o][y][i] = -fl(g * cw[y]) at kept elements (NULL: -g); every other element of dinput is stored as 0
 *   Negative, infinite or NaN class weights: whatever IEEE arithmetic gives; not specified.
 * kind 1, BCE, positive_class_weight p; an element is kept when t != ignore; den = the count of kept elements:
 *   where t == 1.0f && p > 1:   term = -fmaxf(fl(p * logf(x)), -100.f)
 *   everywhere else:            term = -fl(fl(t * fmaxf(logf(x), -100.f)) + fl(fl(1.f - t) * fmaxf(logf(fl(1.f - x)), -100.f)))
 *   sum = sum over kept of (double)term;  loss = w * (float)(sum / den), 0 when den == 0
 *   g as above;  d0 = fl(fl(g * fl(x - t)) / fmaxf(fl(fl(1.f - x) * x), 1e-12f))   (torch's binary_cross_entropy backward)
 *   d x = fl(d0 * p) where t == 1.0f && p > 1, d0 at every other kept element, 0 at ignored ones
 *   p <= 1 changes nothing, and neither does a target other than exactly 1.0 (a smoothed 0.5, say), as in the reference.
 *   The reference raises the input to the power p (x' = x ** p) and hands x' to F.binary_cross_entropy. log(x ** p) and
 *   p * log x are clamped at -100 on the same inputs and differ by the fp32 rounding of x ** p only: on x in
 *   [1e-3, 1 - 1e-3], p in {1.5, 2, 2.5, 3} the fp64 form of this definition is within 1.5e-7 relative of the reference's
 *   loss and 2.4e-7 of its input gradient, the reference's own fp32 rounding. Outside that domain -- where x ** p leaves
 *   fp32's range (underflows to 0 or to a subnormal) or (1 - x') x' < 1e-12 -- THIS definition holds, not torch's
 *   composition: x = 0 at t = 1 gives term 100 and d x = fl(-g * 1e12 * p); x = 1 gives 0 and 0.
 * kind 2, budget: no option; as in twog_loss_t.
 * With class_weight NULL (or all ones) and p <= 1 the results equal twog_multitask_loss_* bit for bit whenever the BCE
 * targets are 0, 1 or ignored (with those, a fused and a separate multiply-add cannot differ).
 * Both return -1 on what twog_multitask_loss_* rejects and on a positive_class_weight that is negative or not finite.
 * =============================================================================================================== */
typedef struct {
    int32_t kind;
    int32_t n_classes;
    int64_t outer, inner;
    const float* input;
    const void* target;
    float* dinput;
    float weight;
    float ignore_value;
    const float* class_weight;
    float positive_class_weight;
    int32_t pad0_;
} twog_wloss_t;
/* partials: workspace of n_terms * TWOG_LOSS_BLOCKS * 2 doubles; stats: [n_terms][2] doubles; losses: [n_terms] floats. */
int twog_weighted_loss_fwd(const twog_wloss_t* terms, int n_terms, double* partials, double* stats, float* losses,
                           void* stream);
int twog_weighted_loss_bwd(const twog_wloss_t* terms, int n_terms, const double* stats, const float* dlosses,
                           void* stream);

/* ===============================================================================================================
 * Temporal smoothing loss: the truncated mean-squared error between the log-probabilities of adjacent steps (T-MSE,
 * Farha & Gall, MS-TCN, CVPR 2019), the training-side companion of the segmental metrics (F1@k, edit score): it acts on
 * predictions that flicker between labels for a few steps. Not part of the reference; csrc/loss.hip.
 * Per term:
 *   input x    fp32 log-probabilities [outer][C][T][E] (steps are E elements apart, classes T*E), outputs of a log-softmax
 *   target y   int64 [outer][T][E];  tau > 0 (MS-TCN: 4);  w the weight;  ignore the ignored target value
 *   a step is kept under the NLL term's rule: y != ignore && 0 <= y < C;
 *   a pair (o, t, e), t >= 1, is kept when steps t and t-1 of (o, e) are both kept;
 *   D = x[o][c][t][e] - x[o][c][t-1][e] in fp32 (one rounding);  v = min((double)D * (double)D, (double)tau * (double)tau)
 *   sum   = sum of v over the kept pairs and all C classes, added in fp64 in a fixed order (TWOG_LOSS_BLOCKS partial sums
 *           per term, then one sequential pass);  count = (kept pairs) * C
 *   stats = {sum, count};  loss = w * (float)(sum / count), 0 when count == 0 (a clip of one step, or every target ignored,
 *           has nothing to smooth: 0 like the BCE and budget terms, not NaN)
 *   the predecessor is a constant (MS-TCN's .detach()): only step t of a pair receives a gradient. With
 *   g = w * dloss / (float)count in fp32 (0 when count == 0):
 *     d x[o][c][t][e] = fl(g * (2 D))  where the pair is kept and D*D <= tau*tau (boundary included, as torch.clamp), else 0.
 *   The product is rounded to fp32 before it is stored or added (no fused multiply-add into the buffer), so both store
 *   modes are reproducible bit for bit. NaN / infinite inputs: whatever IEEE arithmetic gives; not specified.
 * twog_smooth_loss_fwd: up to TWOG_LOSS_MAX_TERMS terms in one launch pair, a (TWOG_LOSS_BLOCKS, terms) grid; partials is a
 *   workspace of n_terms * TWOG_LOSS_BLOCKS * 2 doubles; stats [n_terms][2] and losses [n_terms] are plain pointers (the
 *   tail of the criterion's own tensors). twog_smooth_loss_bwd: one launch; per term, accumulate == 0 stores every element
 *   of dinput (zeros included), accumulate != 0 adds the non-zero contributions into dinput and leaves every other element
 *   untouched (the buffer an earlier launch on the same stream filled); a NULL dinput skips the term. No two terms of one
 *   call may share a dinput. Both return -1 on a malformed term (tau <= 0, a negative size, n_classes < 1).
 * =============================================================================================================== */
typedef struct {
    int32_t n_classes;
    int32_t pad0_;
    int64_t outer, steps, entities;
    const float* input;
    const int64_t* target;
    float* dinput;
    float weight;
    float tau;
    float ignore_value;
    int32_t accumulate;
} twog_smooth_loss_t;
int twog_smooth_loss_fwd(const twog_smooth_loss_t* terms, int n_terms, double* partials, double* stats, float* losses,
                         void* stream);
int twog_smooth_loss_bwd(const twog_smooth_loss_t* terms, int n_terms, const double* stats, const float* dlosses,
                         void* stream);

/* ===============================================================================================================
 * Training-step options of the reference's trainer on the fused step (pyrutils/torch/train_utils.py:149-153,
 * train.py:42-46; csrc/train_opts.hip).
 *
 * twog_grad_norm: the global L2 norm of clip_grad_norm_(model.parameters(), max_norm) over the flat gradient buffer `buf`
 *   restricted to ranges [begin[r], end[r]) (element indices), of the gradient g * scale (scale: the step's 1 / world_size):
 *     norm = fp32( sqrt( sum_r sum_i (double) buf[i]^2 ) * |scale| )      (fp64 sum: finite for every finite fp32 input)
 *     coef = max_norm * (1 / (norm + 1e-6))                                (fp32, torch's max_norm / (total_norm + 1e-6))
 *   out[0] = norm, out[1] = coef. The sum has a fixed order (TWOG_NORM_BLOCKS partial sums in `partials`, then one
 *   workgroup): bit-identical results from run to run; no atomics. Two launches, no host synchronisation.
 * twog_adam_step_coef: twog_adam_step with every gradient read as fl(fl(g * grad_scale) * k), k = coef[0] if coef[0] < 1
 *   else 1 (a NaN coefficient does not clip: the rule of the reference's torch 1.5.1). k = 1 gives exactly
 *   twog_adam_step's result. A sub-range is stepped by offsetting the four pointers.
 * twog_mtl_weight_fwd / _bwd: the multi-task loss learner (Kendall et al.; pyrutils/torch/multi_task.py:10-75) over the
 *   n loss scalars in one launch each. Per term i, with s = log_sds[i], L = losses[i]:
 *     kind SOFTMAX  w = exp(-2 s)        MSE  w = 0.5 exp(-2 s)        MAE  w = sqrt(2) exp(-s)
 *     forward   out[i] = w L + s                      (kind PASS: out[i] = L, the term is not learned)
 *     backward  dlosses[i] = dout[i] w,  dlog_sds[i] (+)= dout[i] (w' L + 1)   (PASS: dlosses[i] = dout[i], dlog_sds 0)
 *   dlog_sds is accumulated into when `accumulate` is non-zero (the flat gradient buffer), stored otherwise; dlosses may be
 *   NULL.
 * =============================================================================================================== */
#define TWOG_NORM_MAX_RANGES 8
#define TWOG_NORM_BLOCKS 2048
typedef struct {
    int64_t begin[TWOG_NORM_MAX_RANGES];
    int64_t end[TWOG_NORM_MAX_RANGES];
    int32_t n_ranges;
    int32_t pad_;
} twog_ranges_t;
/* partials: workspace of TWOG_NORM_BLOCKS doubles; out: 2 floats. */
int twog_grad_norm(const float* buf, const twog_ranges_t* ranges, float scale, float max_norm, double* partials, float* out,
                   void* stream);
int twog_adam_step_coef(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                        float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                        const float* coef, void* stream);
enum { TWOG_MTL_PASS = 0, TWOG_MTL_SOFTMAX = 1, TWOG_MTL_MSE = 2, TWOG_MTL_MAE = 3 };
#define TWOG_MTL_MAX_TERMS 16
typedef struct {
    int32_t kind[TWOG_MTL_MAX_TERMS];
    int32_t n;
    int32_t pad_;
} twog_mtl_t;
int twog_mtl_weight_fwd(const twog_mtl_t* spec, const float* losses, const float* log_sds, float* out, void* stream);
int twog_mtl_weight_bwd(const twog_mtl_t* spec, const float* losses, const float* log_sds, const float* dout, float* dlosses,
                        float* dlog_sds, int accumulate, void* stream);

/* ===============================================================================================================
 * Adam with its step state on the device (csrc/train_opts.hip): the step number, the bias corrections, the clip coefficient
 * and the decision to apply or skip the step live in one 64-byte block and are advanced by a launch, so that a checkpointable,
 * NaN-skipping, decoupled-decay (AdamW), weight-averaging (EMA) step reads nothing on the host. fl() = one fp32 rounding;
 * nothing is contracted into a fused multiply-add, so tests/optim_state_ref.py reproduces both launches bit for bit in numpy.
 *
 * twog_optim_prepare: one workgroup, one active lane, plain stores. norms: HOST array of n_norms (0, 1 or 2) DEVICE pointers,
 *   each to an fp32 norm written by twog_grad_norm; lr_ptr / coef: device fp32 scalars or NULL.
 *     finite = every *norms[j] is finite;   apply = !((flags & SKIP_NONFINITE) && !finite)
 *     not apply:  skipped += 1, apply = 0, nothing else changes
 *     apply:      step += 1;  beta1_pow *= (double)beta1;  beta2_pow *= (double)beta2       (fp64 running products, no pow)
 *                 lr = lr_ptr ? *lr_ptr : lr
 *                 step_size = fl(lr / fl32(1.0 - beta1_pow))           (fp64 subtraction, rounded to fp32, fp32 division)
 *                 bc2s      = fl32(sqrt(1.0 - beta2_pow))              (fp64 subtraction and square root, rounded to fp32)
 *                 clip_k    = (coef && *coef < 1) ? *coef : 1          (a NaN coefficient does not clip: twog_adam_step_coef's rule)
 *                 decay_mul = fl(1 - fl(lr * weight_decay))
 * twog_optim_apply: the element-wise update of n elements; every thread reads the block first and returns when apply == 0
 *   (then no buffer is written). Per element, with b1 / b2 / eps / wd / d = beta1 / beta2 / eps / weight_decay / ema_decay:
 *     g  = fl(grad * grad_scale);            if (flags & CLIP) g = fl(g * clip_k)
 *     p0 = p
 *     if (flags & DECOUPLED)  p0 = fl(p * decay_mul)
 *     else if (wd != 0)       g  = fl(g + fl(wd * p))
 *     m' = fl(fl(b1 * m) + fl(fl(1 - b1) * g))
 *     v' = fl(fl(b2 * v) + fl(fl(1 - b2) * fl(g * g)))
 *     p' = fl(p0 - fl(fl(step_size * m') / fl(fl(sqrt(v') / bc2s) + eps)))               (adam_kernel's order of divisions)
 *     if (ema) ema' = fl(fl(d * ema) + fl(fl(1 - d) * p'))
 *   ema may be NULL. The pointers must be 4-byte aligned and congruent modulo 16 (the same sub-range of equally aligned buffers:
 *   a sub-range is stepped by offsetting all of them): up to 3 elements in front of the first 16-byte boundary and up to 3
 *   behind the last are taken one by one, the body in 16-byte loads and stores on the capped grid of TWOG_STREAM_OPTIM.
 * Both return -2 before any launch for NULL state / hyper / param / grad / exp_avg / exp_avg_sq, n < 0, n_norms outside 0..2
 * or a NULL among norms, an ema_decay outside (0, 1) when ema is given, and pointers that are not congruent; n == 0 launches
 * nothing.
 * =============================================================================================================== */
typedef struct {
    int64_t step, skipped;         /* applied steps so far, skipped steps so far */
    double beta1_pow, beta2_pow;   /* beta^step (1.0 at step 0) */
    float lr, step_size, bc2s, clip_k, decay_mul;   /* the scalars of the CURRENT step, written by twog_optim_prepare */
    int32_t apply;
    int64_t reserved_;             /* 64 bytes */
} twog_optim_state_t;
typedef struct {
    float beta1, beta2, eps, weight_decay, grad_scale, ema_decay;
} twog_optim_hyper_t;
enum { TWOG_OPTIM_CLIP = 1, TWOG_OPTIM_DECOUPLED = 2, TWOG_OPTIM_SKIP_NONFINITE = 4 };
int twog_optim_prepare(twog_optim_state_t* state, const twog_optim_hyper_t* hyper, float lr, const float* lr_ptr,
                       const float* const* norms, int n_norms, const float* coef, int flags, void* stream);
int twog_optim_apply(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                     const twog_optim_hyper_t* hyper, int flags, const twog_optim_state_t* state, void* stream);

/* ===============================================================================================================
 * Inference post-processing on the device.
 * twog_predict_labels: predict.py:64-70 (repeat_interleave by `downsampling` along time, match_shape :95-116 to T_out
 *   steps) + :195-201 (argmax over classes; ties -> first index): logp [bs][C][T][E] -> labels int64 [bs][T_out][E],
 *   labels[b][t][e] = argmax_c logp[b][c][min(t / downsampling, T - 1)][e].
 * twog_f1_at_k: pyrutils/metrics.py:7-81. y_true / y_pred int64 [n_seq][n_steps]; steps with y_true == ignore_value
 *   are dropped from both (use_ignore); f1[s] = F1@overlap of sequence s, valid[s] = 0 for sequences left empty (the
 *   reference skips them); the batch metric is sum(f1) / sum(valid). scratch: n_seq * n_steps bytes.
 * twog_eval_update: predict.py:205-226 (evaluate_predictions: the label pairs sklearn's precision_recall_fscore_support /
 *   classification_report count) fused with the label step above, plus the index selection of :136-156
 *   (downsample_bad_bimanual_videos) and :159-183 (summarize_frames_into_segments). One pass over one output, no labels
 *   tensor in between. logp [bs][C][T][E]; target int64 [bs][T_tgt][E] (-1 = ignored); step_index int32 [bs][S] or
 *   NULL. Position (b, s, e), s < S (s < T_tgt without step_index), evaluates t' = step_index[b][s] (t' = s):
 *   t' < 0 is padding (nothing counted, label 0 / target -1 in the optional outputs); otherwise label = argmax_c
 *   logp[b][c][min(t' / downsampling, T - 1)][e] against target[b][t'][e]. ADDS to counts int64 [C][C] (row = true,
 *   column = predicted) and to flags int64 [2]: [0] positions whose target is outside [-1, C), [1] positions whose
 *   step_index entry is >= T_tgt; neither kind is counted, the second is never read. labels_out / targets_out int64
 *   [bs][S or T_tgt][E] or NULL. Integer atomics: counts is bit-identical from run to run. Returns -2 for
 *   C > the max_classes of twog_eval_limits (a C x C histogram of 32-bit counters per workgroup in LDS).
 * twog_confusion_counts: the same histogram over two int64 label arrays of n elements (predict.py:208-211, :224);
 *   a prediction outside [0, C) whose target is not -1 is counted in flags[0] too.
 * twog_eval_limits: max_classes, and the positions one trip of the capped grid covers (more than that and the
 *   grid-stride loop of the two kernels above runs again).
 * twog_segment_f1: the same metric as twog_f1_at_k for up to max_overlaps thresholds from ONE matching, one workgroup per
 *   sequence. Sequence s of y_true / y_pred (int64, compared as int64) is read in place: entities == 0 is sequence-major
 *   [n_seq][n_steps]; entities == E > 0 is [n_seq / E][n_steps][E] as twog_eval_update writes labels (s = b * E + e, step
 *   stride E). Per sequence and overlap k: tp / fp / fn int32 [n_seq][K] (the counts of metrics.py:40-48) and f1 fp64
 *   [n_seq][K] (precision, recall and F1 with the reference's zero-denominator rules, in the reference's own fp64
 *   expressions); valid int32 [n_seq] is 0 for a sequence with no kept step, whose rows are all zero. `overlaps` is a HOST
 *   array of n_overlaps doubles, read before the call returns. Integer counting and LDS bit-OR only: results are
 *   bit-identical from run to run. Returns -1 for an overlap <= 0 or NaN (there a zero IoU can match and only the
 *   sequential matching of twog_f1_at_k is right) and for n_overlaps outside [1, max_overlaps]; -2 for n_steps > max_steps.
 * twog_segment_f1_accumulate: one workgroup; f1_sums[k] += sum_s f1[s][k] and valid_sums[k] += sum_s valid[s] (device
 *   fp64, k < n_overlaps), in a fixed order.
 * twog_segment_f1_limits: the longest sequence the LDS layout of twog_segment_f1 holds, and its largest n_overlaps.
 * twog_segment_edit: the segmental edit score, one workgroup per sequence, labels read in place in the two layouts of
 *   twog_segment_f1 (int64, compared as int64). Per sequence: steps with y_true == ignore_value are dropped from both
 *   sequences (use_ignore) BEFORE the run-length encoding, so two runs of one label that an ignored stretch separated are
 *   one segment; with use_bg the segments labelled bg_label are then removed from both segment lists WITHOUT merging the
 *   neighbours this brings together (A bg A gives [A, A]); distance int32 [n_seq] is the Levenshtein distance between the
 *   two lists of n_true = m and n_pred = n segment labels (unit insertion, deletion and substitution), and score fp64
 *   [n_seq] = (1.0 - (double)distance / (double)max(m, n)) * 100.0, each of the three operations rounded once. valid
 *   int32 [n_seq] is 0, and the other four outputs are zero, for a sequence with no kept step or with max(m, n) == 0; the
 *   batch metric is sum(score) / sum(valid) (twog_segment_f1_accumulate with n_overlaps == 1 adds both). Integer
 *   arithmetic in LDS only, no atomics: bit-identical from run to run. Returns -1 for a negative size or n_seq not a
 *   multiple of entities; -2 for n_steps > max_steps; 0 without a launch for n_seq == 0. n_steps == 0 writes the
 *   all-zero rows, as twog_segment_f1 does.
 * twog_segment_edit_limits: the longest sequence twog_segment_edit takes: the max_steps of twog_segment_f1_limits.
 * =============================================================================================================== */
int twog_predict_labels(const float* logp, int bs, int n_classes, int T, int E, int downsampling, int T_out,
                        int64_t* labels, void* stream);
int twog_f1_at_k(const int64_t* y_true, const int64_t* y_pred, int n_seq, int n_steps, int num_classes, double overlap,
                 int64_t ignore_value, int use_ignore, unsigned char* scratch, float* f1, float* valid, void* stream);
int twog_eval_update(const float* logp, int bs, int n_classes, int T, int E, int downsampling, const int64_t* target,
                     int T_tgt, const int32_t* step_index, int S, int64_t* counts, int64_t* flags, int64_t* labels_out,
                     int64_t* targets_out, void* stream);
int twog_confusion_counts(const int64_t* y_true, const int64_t* y_pred, int64_t n, int n_classes, int64_t* counts,
                          int64_t* flags, void* stream);
int twog_eval_limits(int* max_classes, int* positions_per_trip);
int twog_segment_f1(const int64_t* y_true, const int64_t* y_pred, int n_seq, int n_steps, int entities, int num_classes,
                    const double* overlaps, int n_overlaps, int64_t ignore_value, int use_ignore, int32_t* tp, int32_t* fp,
                    int32_t* fn, double* f1, int32_t* valid, void* stream);
int twog_segment_f1_accumulate(const double* f1, const int32_t* valid, int n_seq, int n_overlaps, double* f1_sums,
                               double* valid_sums, void* stream);
int twog_segment_f1_limits(int* max_steps, int* max_overlaps);
int twog_segment_edit(const int64_t* y_true, const int64_t* y_pred, int n_seq, int n_steps, int entities,
                      int64_t ignore_value, int use_ignore, int64_t bg_label, int use_bg, double* score, int32_t* distance,
                      int32_t* n_true, int32_t* n_pred, int32_t* valid, void* stream);
int twog_segment_edit_limits(int* max_steps);
/* twog_class_counts: ADDS, per class c, the number of targets[i] == c among n int64 labels to counts[c] (int64 [n_classes]),
 * under the rule of the NLL term: a label is counted when it is != ignore_index and 0 <= label < n_classes; every other
 * label is skipped (twog_confusion_counts ignores -1 only and reports the rest as errors, so it cannot stand in). An LDS
 * histogram per workgroup and one integer atomic per non-empty class per workgroup: the totals do not depend on the order.
 * Returns -1 on n < 0 or n_classes < 1, -2 on more than TWOG_CLASS_COUNTS_MAX classes. */
#define TWOG_CLASS_COUNTS_MAX 4096
int twog_class_counts(const int64_t* targets, int64_t n, int n_classes, int64_t ignore_index, int64_t* counts, void* stream);

/* ===============================================================================================================
 * Viterbi decoding of frame labels under a label-transition model (the reference project has no
 * such decode, tests/viterbi_ref.py is the specification). For one sequence = one (clip b, entity e), with
 * logp[t][c] = logp[b][c][t][e] at the model's own step rate, L the decoded length, A fp32 [C][C] transition scores
 * (row = from, column = to) and pi fp32 [C] initial scores (NULL: all zero). All arithmetic is fp32, one rounding per
 * add, nothing fused or reordered:
 *     d[0][c] = logp[0][c] + pi[c]
 *     m[t][c] = max over c' of (d[t-1][c'] + A[c'][c])     psi[t][c] = the SMALLEST c' that attains it
 *     d[t][c] = m[t][c] + logp[t][c]                       (t = 1 .. L-1)
 *     y[L-1]  = the smallest c attaining max d[L-1][.]     y[t-1] = psi[t][y[t]]     score = max d[L-1][.]
 * A candidate replaces the running best only when it is strictly greater: that is the tie-break (among paths of equal
 * score the smallest one compared from the last step backwards) and it decides what -inf does; -inf entries of A
 * (forbidden transitions) are in contract. NaN is out of contract, but never gives a label outside [0, C) or an access
 * outside the buffers.
 * lengths: int64 [bs] on the device, in model steps, clamped by the kernel to [0, T]; NULL means T. A length of 0 writes
 *   label 0 everywhere and score 0.0.
 * labels int64 [bs][T_out][E]: labels[b][t'][e] = y[min(t' / downsampling, L - 1)], the upsampling of twog_predict_labels;
 *   score fp32 [bs][E].
 * Back-pointers are one byte per (t, c). twog_viterbi_workspace (launch-free) returns the route of a shape:
 *   TWOG_VITERBI_ROUTE_LDS, *bytes = 0: they fit in LDS beside the staging buffers, `workspace` is not touched;
 *   TWOG_VITERBI_ROUTE_WORKSPACE: they go to `workspace`, *bytes of device memory (256-byte aligned) that the call may
 *   overwrite and whose content means nothing afterwards.
 * The time axis is staged through LDS in chunks of TWOG_VITERBI_CHUNK steps. The result does not depend on the route, the
 * chunking or the batch a sequence is decoded in, bit for bit.
 * twog_viterbi_limits: the largest C (64) and T (4096). Returns: -1 for a bad size, -2 beyond the limits (or C * T * E
 * >= 2^31, bs > 65535), -3 for a workspace that is NULL or too small on the workspace route.
 *
 * twog_transition_counts: ADDS to counts int64 [C][C] (row = from, column = to) one for every (b, e, k) with
 *   (k + 1) * stride < T_tgt whose labels targets[b][k * stride][e] and targets[b][(k + 1) * stride][e] (int64
 *   [bs][T_tgt][E]) are both in [0, C) and both != ignore_index: the statistics at the model's rate (stride = the
 *   loader's downsampling). LDS histograms and integer atomics: the totals do not depend on the order. -2 for C > 64.
 * =============================================================================================================== */
#define TWOG_VITERBI_CHUNK 16
#define TWOG_VITERBI_ROUTE_LDS 0
#define TWOG_VITERBI_ROUTE_WORKSPACE 1
int twog_viterbi_limits(int* max_classes, int* max_steps);
int twog_viterbi_workspace(int bs, int n_classes, int T, int E, size_t* bytes);
int twog_viterbi_decode(const float* logp, int bs, int n_classes, int T, int E, const float* A, const float* pi,
                        const int64_t* lengths, int downsampling, int T_out, int64_t* labels, float* score,
                        void* workspace, size_t workspace_bytes, void* stream);
int twog_transition_counts(const int64_t* targets, int bs, int T_tgt, int E, int n_classes, int stride,
                           int64_t ignore_index, int64_t* counts, void* stream);

/* ===============================================================================================================
 * Segmental (semi-Markov) decoding: Viterbi over whole segments with a per-class duration score (DESIGN section 4.16;
 * the reference project has no such decode, tests/segdecode_ref.py is the specification). One sequence = one (clip b,
 * entity e), with logp[t][c] = logp[b][c][t][e], L the decoded length, A fp32 [C][C] scores between consecutive
 * segments (row = from, column = to), pi fp32 [C] (NULL: all zero) and dur fp32 [C][D]: dur[c][l-1] is the score of a
 * class-c segment that lasts l steps, l = 1 .. D. All arithmetic is fp32, each add rounds once in the order written,
 * nothing is fused or reordered, and a candidate replaces the running best only when it is strictly greater:
 *     e[0][c] = pi[c]
 *     e[t][c] = max over c' = 0..C-1 of (d[t-1][c'] + A[c'][c]),  prev[t][c] = the smallest c' attaining it    (t >= 1)
 *     for l = 1 .. min(D, t+1), ascending:   acc_l = acc_(l-1) + logp[t-l+1][c]   (acc_0 = 0)
 *                                            cand_l = (e[t-l+1][c] + dur[c][l-1]) + acc_l
 *     d[t][c] = max over l of cand_l,        len[t][c] = the smallest l attaining it (the running best starts as cand_1)
 *     end:  c = the smallest class attaining max d[L-1][.];  score = that maximum;  t = L-1
 *     back: l = len[t][c];  y[t-l+1 .. t] = c;  stop if t-l+1 == 0;  c = prev[t-l+1][c];  t = t - l
 * The diagonal of A is used like any other entry: a segment may be followed by one of the same class at A[c][c], which
 * is how runs longer than D are composed; a caller forbids it with -inf. -inf in A, pi and dur is in contract
 * (forbidden transitions, minimum durations). NaN is out of contract, but never gives a label outside [0, C) or an
 * access outside the buffers; the same holds when every path scores -inf.
 * lengths, downsampling, T_out, labels and score are those of twog_viterbi_decode: labels[b][t'][e] = y[min(t' /
 *   downsampling, L - 1)], and a length of 0 writes label 0 everywhere and score 0.0.
 * The working set of a wave is a ring of the last min(D, T) steps of (e, logp) in LDS, dur once per workgroup, and
 * back-pointers of two bytes per (t, c). twog_segdecode_plan (launch-free) states the launch of a shape: out[0] the class
 * template (8, 16, 32 or 64), out[1] the waves (= entities) per workgroup, out[2] the workgroups per clip, out[3] the
 * route:
 *   TWOG_SEGDEC_ROUTE_LDS, *workspace_bytes = 0: the back-pointers of at least one wave fit in LDS beside the rest; the
 *   waves are as many (up to 8) as the LDS budget holds rings and back-pointers for, `workspace` is not touched;
 *   TWOG_SEGDEC_ROUTE_WORKSPACE: they go to `workspace`, *workspace_bytes of device memory (256-byte aligned) that the
 *   call may overwrite and whose content means nothing afterwards; the waves are as many as the budget holds rings for.
 * The result does not depend on the route, the waves per workgroup, the chunking or the batch a sequence is decoded in,
 * bit for bit.
 * twog_segdecode_limits: the largest C (64), T (4096) and D (TWOG_SEGDEC_MAX_DURATION). Returns: -1 for a bad size
 * (D < 1 included), -2 beyond the limits (or C * T * E >= 2^31, bs > 65535), -3 for a workspace that is NULL or too
 * small on the workspace route.
 *
 * twog_duration_counts: ADDS to counts int64 [C][D] the run lengths of targets (int64 [bs][T_tgt][E]) read at the
 *   model's rate, targets[b][k * stride][e] for k = 0, 1, ... while k * stride < T_tgt: a maximal run of n equal labels c
 *   adds one to counts[c][min(n, D) - 1]. A label counts only if it is in [0, C) and != ignore_index; a run ends at a
 *   change of label, at a label that does not count, and at the end of the sequence. LDS histograms and integer atomics:
 *   the totals do not depend on the order. -2 for C > 64 or D > TWOG_SEGDEC_MAX_DURATION.
 * =============================================================================================================== */
#define TWOG_SEGDEC_MAX_DURATION 128
#define TWOG_SEGDEC_ROUTE_LDS 0
#define TWOG_SEGDEC_ROUTE_WORKSPACE 1
int twog_segdecode_limits(int* max_classes, int* max_steps, int* max_duration);
int twog_segdecode_plan(int bs, int n_classes, int T, int E, int D, int32_t* out, size_t* workspace_bytes);
int twog_segdecode(const float* logp, int bs, int n_classes, int T, int E, const float* A, const float* pi,
                   const float* dur, int D, const int64_t* lengths, int downsampling, int T_out,
                   int64_t* labels, float* score, void* workspace, size_t workspace_bytes, void* stream);
int twog_duration_counts(const int64_t* targets, int bs, int T_tgt, int E, int n_classes, int D, int stride,
                         int64_t ignore_index, int64_t* counts, void* stream);

/* ===============================================================================================================
 * Linear-chain CRF loss: the sequence negative log-likelihood under learned transition scores (the
 * reference project has no such term, tests/crf_ref.py at fp64 is the specification). The scores it trains go to
 * twog_viterbi_decode unchanged.
 *   input  fp32 [bs][C][T][E] log-probabilities (the model's outputs at the model's rate, as the NLL terms get them)
 *   target int64 [bs][T][E]
 *   A      fp32 [C][C] transition scores, row = from, column = to (the convention of twog_viterbi_decode); pi fp32 [C].
 *          Finite A and pi are in contract; +-inf and NaN are not.
 * A sequence is (clip b, entity e). Its kept steps t_0 < t_1 < ... < t_{K-1} are those with 0 <= target[b][t][e] < C and
 * target != ignore_index (the NLL terms' rule); every other step is removed from the chain -- padding, an absent entity and
 * a hole in the middle are the same case -- and transitions link consecutive kept steps. K = 0 contributes nothing.
 * With x_k[c] = input[b][c][t_k][e] and y_k = target[b][t_k][e]:
 *     alpha_0[c] = pi[c] + x_0[c]
 *     alpha_k[c] = x_k[c] + logsumexp_{c'} (alpha_{k-1}[c'] + A[c'][c])          k = 1 .. K-1
 *     logZ       = logsumexp_c alpha_{K-1}[c]
 *     gold       = pi[y_0] + x_0[y_0] + sum_{k>=1} (A[y_{k-1}][y_k] + x_k[y_k])
 *     nll_seq    = logZ - gold                                                    (>= 0)
 *     loss       = weight * (sum over sequences of nll_seq) / (sum over sequences of K)      (0 when no step is kept)
 * stats[0] = sum of nll_seq, stats[1] = sum of K (the count of the term: it is on the scale of the per-step NLL terms).
 * Gradients, with g = dloss * weight / stats[1] (0 when stats[1] <= 0; the caller may have replaced stats[1] by a global
 * count):
 *     beta_{K-1}[c] = 0
 *     beta_k[c']    = logsumexp_c (A[c'][c] + x_{k+1}[c] + beta_{k+1}[c])
 *     gamma_k[c]    = exp(alpha_k[c] + beta_k[c] - logZ)
 *     xi_k[c'][c]   = exp(alpha_{k-1}[c'] + A[c'][c] + x_k[c] + beta_k[c] - logZ)
 *     dinput[b][c][t_k][e] = g * (gamma_k[c] - [c = y_k]); every removed step gets 0: the tensor is written completely, with
 *                            no separate clear (accumulate != 0: the same values are ADDED to what the buffer holds)
 *     dA[c'][c] = g * sum_seq sum_{k>=1} (xi_k[c'][c] - [y_{k-1} = c', y_k = c])
 *     dpi[c]    = g * sum_seq (gamma_0[c] - [y_0 = c])
 * Arithmetic: the per-sequence recursions run in fp32, every logsumexp in the log domain with the maximum subtracted.
 * The sums over sequences (nll_seq, K, dA, dpi) are carried in fp64 in index order and rounded to fp32 once. No
 * floating-point atomics: two runs on the same inputs give the same bits, and a sequence gives the same per-sequence
 * values in any batch.
 * Workspaces (twog_crf_workspace, launch-free; all device memory, 4-byte aligned):
 *   alpha   bs * E * T * C floats: alpha of every kept step, written by the forward, read by the backward
 *   seq     bs * E * TWOG_CRF_SEQ_WORDS floats per sequence: logZ, gold, nll_seq, K (the bits of an int32)
 *   partials bs * E * (C + 1) * C floats: the backward's per-sequence sums for dA (C rows) and dpi (one row); needed only
 *           when dA / dpi are asked for
 * twog_crf_nll_fwd: two launches (recursion, sums). twog_crf_nll_bwd: the recursion (writes dinput when it is not NULL),
 * then, when dA and dpi are not NULL (both or neither), the reduction over sequences, which stores (accumulate_params == 0)
 * or adds. The time axis is staged through LDS in chunks of TWOG_CRF_CHUNK steps.
 * twog_crf_limits: the largest C (64) and T (4096), those of twog_viterbi_limits. Returns: -1 for a bad size, -2 beyond
 * the limits (or C * T * E >= 2^31, bs > 65535), -3 for a missing buffer.
 * =============================================================================================================== */
#define TWOG_CRF_CHUNK 16
#define TWOG_CRF_SEQ_WORDS 4
int twog_crf_limits(int* max_classes, int* max_steps);
int twog_crf_workspace(int bs, int n_classes, int T, int E, size_t* alpha_bytes, size_t* seq_bytes, size_t* partial_bytes);
int twog_crf_nll_fwd(const float* input, const int64_t* target, int bs, int n_classes, int T, int E, const float* A,
                     const float* pi, int64_t ignore_index, float weight, float* alpha, float* seq, double* stats,
                     float* loss, void* stream);
int twog_crf_nll_bwd(const float* input, const int64_t* target, int bs, int n_classes, int T, int E, const float* A,
                     int64_t ignore_index, float weight, const float* alpha, const float* seq, const double* stats,
                     const float* dloss, float* dinput, int accumulate, float* partials, float* dA, float* dpi,
                     int accumulate_params, void* stream);

/* ===============================================================================================================
 * Semi-Markov CRF loss: the sequence negative log-likelihood over whole segments with learned per-class duration
 * scores (the reference project has no such term, tests/semicrf_ref.py at fp64 is the
 * specification). It is the sum-product twin of twog_segdecode, and the three tables it trains go there unchanged.
 *   input  fp32 [bs][C][T][E] log-probabilities, target int64 [bs][T][E]: as for twog_crf_nll_fwd
 *   A      fp32 [C][C] scores between consecutive segments, row = from, column = to; the diagonal is an entry like any other
 *   pi     fp32 [C];   dur fp32 [C][D]: dur[c][l-1] scores a class-c segment of l steps, l = 1 .. D
 * A sequence is (clip b, entity e); its kept steps t_0 < ... < t_{K-1} follow the NLL terms' rule exactly as for the
 * linear-chain CRF: removed steps drop out of the chain, K = 0 contributes nothing. With x_k[c] = input[b][c][t_k][e],
 * y_k = target[b][t_k][e] and S_c(s, l) = x_s[c] + ... + x_{s+l-1}[c]:
 *     e_0[c]   = pi[c]
 *     e_k[c]   = logsumexp_{c'} (d_{k-1}[c'] + A[c'][c])                                    k >= 1
 *     d_k[c]   = logsumexp_{l = 1 .. min(D, k+1)} (e_{k-l+1}[c] + dur[c][l-1] + S_c(k-l+1, l))
 *     logZ     = logsumexp_c d_{K-1}[c]
 *     gold     = the score of the gold segmentation: the maximal runs of equal y over the kept steps; a run of n > D steps
 *                is cut into pieces of D steps from its start with the remainder (1 .. D steps) last, consecutive pieces
 *                joined by A[c][c]:  pi[c_1] + sum_j (dur[c_j][l_j - 1] + S_{c_j}(s_j, l_j)) + sum_{j >= 2} A[c_{j-1}][c_j]
 *     nll_seq  = logZ - gold                                                                 (>= 0)
 *     loss     = weight * (sum over sequences of nll_seq) / (sum over sequences of K)       (0 when no step is kept)
 * stats[0] = sum of nll_seq, stats[1] = sum of K, as for twog_crf_nll_fwd. Gradients, with g = dloss * weight / stats[1]
 * (0 when stats[1] <= 0; the caller may have replaced stats[1] by a global count):
 *     bd_{K-1}[c] = 0;   bd_k[c] = logsumexp_{c'} (A[c][c'] + be_{k+1}[c'])
 *     be_s[c]     = logsumexp_{l = 1 .. min(D, K-s)} (dur[c][l-1] + S_c(s, l) + bd_{s+l-1}[c])
 *     mu(s, l, c) = exp(e_s[c] + dur[c][l-1] + S_c(s, l) + bd_{s+l-1}[c] - logZ)           the segment marginal
 *     End_k[c] = exp(d_k[c] + bd_k[c] - logZ),  Start_k[c] = exp(e_k[c] + be_k[c] - logZ)
 *     cov_k    = cov_{k+1} + End_k - Start_{k+1}  (cov_K = Start_K = 0): the sum of mu over the segments that cover k
 *     dinput[b][c][t_k][e] = g * (cov_k[c] - [y_k = c]); every removed step gets 0: the tensor is written completely, with
 *                            no separate clear (accumulate != 0: the same values are ADDED to what the buffer holds)
 *     ddur[c][l-1] = g * sum_seq (sum_s mu(s, l, c) - #gold pieces of class c and length l)
 *     dA[c'][c]    = g * sum_seq (sum_{k>=1} exp(d_{k-1}[c'] + A[c'][c] + be_k[c] - logZ) - #gold joins c' -> c)
 *     dpi[c]       = g * sum_seq (exp(pi[c] + be_0[c] - logZ) - [c_1 = c])
 * -inf is in contract in A, pi and dur (a forbidden self-transition, a minimum duration): a logsumexp whose terms are all
 * -inf is -inf, never NaN, and a -inf entry gets gradient exactly 0.0. Out of contract: +inf and NaN anywhere, and a
 * sequence whose own gold score is -inf (a gold run longer than D under A[c][c] = -inf, for one): choose D at least the
 * longest labelled run, or keep the diagonal finite. Out-of-contract inputs cause no access outside the buffers; nll_seq
 * may then be +inf or NaN.
 * Arithmetic: the per-sequence recursions run in fp32, every logsumexp in the log domain with the maximum subtracted
 * (expf / logf of the device library). The sums over sequences (nll_seq, K, dA, dpi, ddur) are carried in fp64 in index
 * order and rounded to fp32 once. No floating-point atomics: two runs on the same inputs give the same bits, and a
 * sequence gives the same per-sequence values in any batch.
 * twog_semicrf_plan (launch-free) states the launches and the workspaces of a shape: out[0] the class template (8, 16, 32
 * or 64), out[1] / out[2] the waves (= entities) per workgroup and the workgroups per clip of the forward, out[3] / out[4]
 * those of the backward; the waves are as many (up to 8; backward beyond 32 classes: 4) as the 160 KB LDS budget holds
 * rings of the last min(D, T) kept steps for (forward: (e, x); backward: (bd, x) and the wave's ddur sums), beside dur and
 * the staging buffers. bytes[0 .. 3] (all device memory, 8-byte aligned):
 *   ed       bs * E * T * C float pairs: (e, d) of every kept step, indexed by k; written by the forward, read by the backward
 *   marks    bs * E * T int32: 1 where a gold piece starts, per step t; written by the forward, read by the backward
 *   seq      bs * E * TWOG_SEMICRF_SEQ_WORDS floats: logZ, gold, nll_seq, K (the bits of an int32)
 *   partials bs * E * C * (C + 1 + min(D, T)) floats: the backward's per-sequence sums for dA (C rows), dpi (one row) and
 *            ddur (min(D, T) rows of C); needed only when the parameter gradients are asked for
 * twog_semicrf_nll_fwd: two launches (recursion, sums). twog_semicrf_nll_bwd: the recursion (writes dinput when it is not
 * NULL), then, when dA, dpi and ddur are not NULL (all or none), the reduction over sequences, which stores
 * (accumulate_params == 0) or adds.
 * twog_semicrf_limits: those of twog_segdecode_limits. Returns: -1 for a bad size (D < 1 included), -2 beyond the limits
 * (or C * T * E >= 2^31, bs > 65535), -3 for a missing buffer or workspace.
 * =============================================================================================================== */
#define TWOG_SEMICRF_SEQ_WORDS 4
int twog_semicrf_limits(int* max_classes, int* max_steps, int* max_duration);
int twog_semicrf_plan(int bs, int n_classes, int T, int E, int D, int32_t* out, size_t* bytes);
int twog_semicrf_nll_fwd(const float* input, const int64_t* target, int bs, int n_classes, int T, int E, const float* A,
                         const float* pi, const float* dur, int D, int64_t ignore_index, float weight, float* ed,
                         int32_t* marks, float* seq, double* stats, float* loss, void* stream);
int twog_semicrf_nll_bwd(const float* input, const int64_t* target, int bs, int n_classes, int T, int E, const float* A,
                         const float* dur, int D, int64_t ignore_index, float weight, const float* ed,
                         const int32_t* marks, const float* seq, const double* stats, const float* dloss, float* dinput,
                         int accumulate, float* partials, float* dA, float* dpi, float* ddur, int accumulate_params,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TWOG_GCN_H */
