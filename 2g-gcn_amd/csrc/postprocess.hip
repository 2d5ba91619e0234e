// Inference post-processing on the device, so that a prediction pass hands back labels and
// the segmental metric instead of the (bs, C, T, E) log-probability tensors.
//
// Reference: predict.py:64-70 (torch.repeat_interleave of every output by the downsampling factor + match_shape
// :95-116), :195-201 (np.argmax over the class axis after a D2H copy of every output), and the segmental F1@k metric
// pyrutils/metrics.py:7-81 (run-length encoded segments, greedy IoU matching).
#include "twog_common.h"

namespace {

// first argmax_c p[c * stride]. Strict comparison: ties keep the first index, like np.argmax
__device__ __forceinline__ int first_argmax(const float* p, int C, int64_t stride) {
    float best = p[0];
    int arg = 0;
    for (int c = 1; c < C; ++c) {
        const float v = p[(int64_t)c * stride];
        if (v > best) { best = v; arg = c; }
    }
    return arg;
}

// labels[b][t'][e] = first argmax_c logp[b][c][min(t' / ds, T - 1)][e]
__global__ __launch_bounds__(256) void predict_labels_kernel(const float* logp, int bs, int C, int T, int E, int ds,
                                                             int T_out, long long* labels) {
    const int64_t n = (int64_t)bs * T_out * E;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int e = (int)(i % E);
        const int64_t bt = i / E;
        const int tp = (int)(bt % T_out), b = (int)(bt / T_out);
        const int t = min(tp / ds, T - 1);
        labels[i] = first_argmax(logp + ((int64_t)b * C * T + t) * E + e, C, (int64_t)T * E);
    }
}

// ---- confusion counts (predict.py:205-226 feeds sklearn with host copies of every label; here the C x C counts are
// built where the labels are). Every workgroup keeps a private histogram of 32-bit counters in LDS: hist[C * C] cells
// (row = true class, column = predicted class) followed by the two flag counters. A workgroup sees at most
// n / gridDim.x + 256 positions, far below 2^32 for any tensor that fits the device. The flush adds the non-zero
// cells to the int64 totals with integer atomics, so the totals do not depend on the arrival order.
constexpr int EVAL_MAX_CLASSES = 64;   // 64 * 64 * 4 B = 16 KB of LDS
constexpr int EVAL_GRID_CAP = 1024;    // workgroups of 256: every one flushes up to C * C cells

__device__ __forceinline__ void count_position(unsigned* hist, int C, long long tgt, long long pred) {
    if (tgt == -1) return;                                   // ignored (predict.py:210-211)
    if (tgt < -1 || tgt >= C || pred < 0 || pred >= C) { atomicAdd(&hist[C * C], 1u); return; }
    atomicAdd(&hist[(int)tgt * C + (int)pred], 1u);
}

__device__ __forceinline__ void clear_hist(unsigned* hist, int C) {
    for (int k = threadIdx.x; k < C * C + 2; k += 256) hist[k] = 0u;
    __syncthreads();
}

__device__ __forceinline__ void flush_hist(const unsigned* hist, int C, long long* counts, long long* flags) {
    __syncthreads();
    for (int k = threadIdx.x; k < C * C + 2; k += 256) {
        const unsigned v = hist[k];
        if (v == 0u) continue;
        long long* dst = k < C * C ? counts + k : flags + (k - C * C);
        atomicAdd(reinterpret_cast<unsigned long long*>(dst), (unsigned long long)v);
    }
}

// One pass over one model output: position (b, s, e) evaluates target step t' = step_index[b][s] (or s), whose label is
// the argmax at source step min(t' / ds, T - 1). t' < 0 is padding (label 0, target -1: what the reference's -100 /
// -1.0 rubbish rows give after argmax); t' >= T_tgt is counted in flags[1] and never read.
__global__ __launch_bounds__(256) void eval_update_kernel(const float* logp, int bs, int C, int T, int E, int ds,
                                                          const long long* target, int T_tgt, const int* step_index,
                                                          int S, long long* counts, long long* flags,
                                                          long long* labels_out, long long* targets_out) {
    extern __shared__ unsigned hist[];
    clear_hist(hist, C);
    const int64_t n = (int64_t)bs * S * E;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int e = (int)(i % E);
        const int64_t bsx = i / E;
        const int s = (int)(bsx % S), b = (int)(bsx / S);
        const int tp = step_index ? step_index[(int64_t)b * S + s] : s;
        long long label = 0, tgt = -1;
        if (tp >= T_tgt) {
            atomicAdd(&hist[C * C + 1], 1u);
        } else if (tp >= 0) {
            const int t = min(tp / ds, T - 1);
            label = first_argmax(logp + ((int64_t)b * C * T + t) * E + e, C, (int64_t)T * E);
            tgt = target[((int64_t)b * T_tgt + tp) * E + e];
            count_position(hist, C, tgt, label);
        }
        if (labels_out) labels_out[i] = label;
        if (targets_out) targets_out[i] = tgt;
    }
    flush_hist(hist, C, counts, flags);
}

__global__ __launch_bounds__(256) void confusion_counts_kernel(const long long* y_true, const long long* y_pred,
                                                               int64_t n, int C, long long* counts, long long* flags) {
    extern __shared__ unsigned hist[];
    clear_hist(hist, C);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        count_position(hist, C, y_true[i], y_pred[i]);
    flush_hist(hist, C, counts, flags);
}

// Class counts of a label tensor under the NLL terms' rule (twog_label_kept), for losses.class_counts:
// hist[C] 32-bit counters per workgroup (a workgroup sees far fewer than 2^32 positions), flushed like the cells above.
__global__ __launch_bounds__(256) void class_counts_kernel(const long long* targets, int64_t n, int C, long long ignore,
                                                           long long* counts) {
    extern __shared__ unsigned hist[];
    for (int k = threadIdx.x; k < C; k += 256) hist[k] = 0u;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const long long y = targets[i];
        if (twog_label_kept(y, ignore, C)) atomicAdd(&hist[(int)y], 1u);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < C; k += 256) {
        const unsigned v = hist[k];
        if (v != 0u) atomicAdd(reinterpret_cast<unsigned long long*>(counts + k), (unsigned long long)v);
    }
}

inline int eval_grid(int64_t n) { return (int)((n + 255) / 256 < EVAL_GRID_CAP ? (n + 255) / 256 : EVAL_GRID_CAP); }

// One thread per sequence. Steps whose target equals the ignore value are dropped from BOTH sequences before the
// run-length encoding (metrics.py:75-77). `used` is a per-sequence scratch row of n_steps bytes.
__global__ __launch_bounds__(64) void f1_at_k_kernel(const long long* y_true, const long long* y_pred, int n_seq,
                                                     int n_steps, int num_classes, double overlap, long long ignore,
                                                     int use_ignore, unsigned char* used, float* f1, float* valid) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= n_seq) return;
    const long long* yt = y_true + (int64_t)s * n_steps;
    const long long* yp = y_pred + (int64_t)s * n_steps;
    unsigned char* u = used + (int64_t)s * n_steps;
    // number of target segments in the filtered sequence
    int n_kept = 0, n_tgt = 0;
    long long prev = 0;
    for (int i = 0; i < n_steps; ++i) {
        if (use_ignore && yt[i] == ignore) continue;
        if (n_kept == 0 || yt[i] != prev) { u[n_tgt] = 0; ++n_tgt; }
        prev = yt[i];
        ++n_kept;
    }
    if (n_kept == 0) { f1[s] = 0.f; valid[s] = 0.f; return; }
    double tp = 0.0, fp = 0.0;
    // walk the predicted segments of the filtered sequence
    int pos = 0, i = 0;  // pos: index in the filtered sequence
    while (i < n_steps) {
        if (use_ignore && yt[i] == ignore) { ++i; continue; }
        const long long oid = yp[i];
        const int o0 = pos;
        while (i < n_steps) {  // extend over kept steps with the same predicted label
            if (use_ignore && yt[i] == ignore) { ++i; continue; }
            if (yp[i] != oid) break;
            ++i;
            ++pos;
        }
        const int o1 = pos;
        // IoU against every target segment; first maximum (np.argmax)
        double best = 0.0;
        int best_idx = -1;
        int tpos = 0, seg = -1, t0 = 0;
        long long tid = 0;
        bool open = false;
        for (int j = 0; j <= n_steps; ++j) {
            const bool kept = j < n_steps && !(use_ignore && yt[j] == ignore);
            if (j < n_steps && !kept) continue;
            if (open && (j == n_steps || yt[j] != tid)) {  // close target segment [t0, tpos)
                const double inter = (double)(min(o1, tpos) - max(o0, t0));
                const double uni = (double)(max(o1, tpos) - min(o0, t0));
                const double iou = (inter / uni) * (oid == tid ? 1.0 : 0.0);
                if (best_idx < 0 || iou > best) { best = iou; best_idx = seg; }
                open = false;
            }
            if (j == n_steps) break;
            if (!open) { open = true; tid = yt[j]; t0 = tpos; ++seg; }
            ++tpos;
        }
        if (oid >= num_classes) continue;
        if (best >= overlap && !u[best_idx]) { tp += 1.0; u[best_idx] = 1; }
        else fp += 1.0;
    }
    double n_used = 0.0;
    for (int k = 0; k < n_tgt; ++k) n_used += u[k];
    const double fn = (double)n_tgt - n_used;
    const double precision = tp + fp > 0.0 ? tp / (tp + fp) : 0.0;
    const double recall = tp + fn > 0.0 ? tp / (tp + fn) : 0.0;
    f1[s] = precision + recall > 0.0 ? (float)(2.0 * precision * recall / (precision + recall)) : 0.f;
    valid[s] = 1.f;
}

// ---- segmental F1@k with a workgroup per sequence, every overlap from one matching (pyrutils/metrics.py:7-65).
// The target segment a predicted segment p is matched against is argmax(iou), which does not depend on `used`. For
// overlap > 0 only a same-label target segment with a positive intersection can reach the threshold, and those are the
// same-label segments among the contiguous range holding p's first and last step. So with (best_p, idx_p) the first
// maximum of inter / union over that range:
//   TP_k = #{t : some p has idx_p == t, best_p >= k, label_p < num_classes}
//   FP_k = #{p : label_p < num_classes} - TP_k          FN_k = n_target_segments - TP_k
// which is what the greedy loop counts: of the predicted segments that reach the threshold on one target segment the
// first is a true positive and the others, like those that reach it nowhere, are false positives.
// LDS (16-bit entries, values <= SEGF1_MAX_STEPS): orig[q] the step of the q-th kept step, tseg[q] its target segment,
// tstart[t] / pstart[p] the first kept position of a segment (one entry beyond the last: n_kept); then one bitmap of
// target segments per overlap. Labels are read in place (int64) through orig[].
constexpr int SEGF1_MAX_STEPS = 4096;
constexpr int SEGF1_MAX_OVERLAPS = 8;
constexpr int SEGF1_THREADS = 256;
constexpr int SEGF1_WAVES = SEGF1_THREADS / TWOG_WAVE;

struct SegF1Overlaps { double k[SEGF1_MAX_OVERLAPS]; };

inline int segf1_round_steps(int n_steps) { return (n_steps + 63) & ~63; }
inline size_t segf1_lds_bytes(int n_steps) {   // 4 tables of (rounded + 2) 16-bit entries, K bitmaps of rounded / 32 words
    const int r = segf1_round_steps(n_steps);
    return (size_t)4 * (r + 2) * sizeof(unsigned short) + (size_t)SEGF1_MAX_OVERLAPS * (r / 32 + 1) * sizeof(unsigned);
}

// lanes of this wave below the caller whose bit is set in `mask`
__device__ __forceinline__ int lanes_below(unsigned long long mask) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// precision, recall and F1 with the reference's three zero-denominator rules (metrics.py:49-60). Every operation is one
// correctly rounded fp64 division, product or sum of the reference's own expression; no multiply feeds an add, and
// contraction is off so that it stays that way.
__device__ __forceinline__ double segment_f1_value(int tp_i, int fp_i, int fn_i) {
#pragma clang fp contract(off)
    const double tp = (double)tp_i, fp = (double)fp_i, fn = (double)fn_i;
    const double precision = tp + fp > 0.0 ? tp / (tp + fp) : 0.0;
    const double recall = tp + fn > 0.0 ? tp / (tp + fn) : 0.0;
    return precision + recall > 0.0 ? 2.0 * (precision * recall) / (precision + recall) : 0.0;
}

// Sequence s reads y[seq_off(s) + step * step_stride]: sequence-major (entities == 0: s * n_steps, stride 1) or
// entity-minor [bs][n_steps][E] (s = b * E + e: b * n_steps * E + e, stride E).
__global__ __launch_bounds__(SEGF1_THREADS) void segment_f1_kernel(
    const long long* y_true, const long long* y_pred, int n_steps, int entities, long long num_classes, SegF1Overlaps ov,
    int K, long long ignore, int use_ignore, int* tp_out, int* fp_out, int* fn_out, double* f1_out, int* valid_out) {
    extern __shared__ unsigned segf1_lds[];
    __shared__ int wave_cnt[2][SEGF1_WAVES];
    __shared__ int tp_k[SEGF1_MAX_OVERLAPS];
    const int rounded = (n_steps + 63) & ~63;
    unsigned short* orig = reinterpret_cast<unsigned short*>(segf1_lds);
    unsigned short* tseg = orig + (rounded + 2);
    unsigned short* tstart = tseg + (rounded + 2);
    unsigned short* pstart = tstart + (rounded + 2);
    unsigned* bitmap = reinterpret_cast<unsigned*>(pstart + (rounded + 2));   // 8 * (rounded + 2) bytes in: 4-byte aligned
    const int words = rounded / 32 + 1;                                       // per overlap
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = blockIdx.x;
    int64_t off, stride;
    if (entities > 0) { off = (int64_t)(s / entities) * n_steps * entities + s % entities; stride = entities; }
    else { off = (int64_t)s * n_steps; stride = 1; }
    const long long* yt = y_true + off;
    const long long* yp = y_pred + off;

    for (int w = tid; w < K * words; w += SEGF1_THREADS) bitmap[w] = 0u;

    // 1. drop the ignored steps: orig[q] = step of the q-th kept one
    int n_kept = 0;
    for (int base = 0; base < n_steps; base += SEGF1_THREADS) {
        const int i = base + tid;
        const bool kept = i < n_steps && !(use_ignore && yt[(int64_t)i * stride] == ignore);
        const unsigned long long mask = __ballot(kept);
        if (lane == 0) wave_cnt[0][wave] = __popcll(mask);
        __syncthreads();
        int before = n_kept, total = n_kept;
        for (int w = 0; w < SEGF1_WAVES; ++w) {
            const int c = wave_cnt[0][w];
            if (w < wave) before += c;
            total += c;
        }
        if (kept) orig[before + lanes_below(mask)] = (unsigned short)i;
        n_kept = total;
        __syncthreads();
    }
    if (n_kept == 0) {   // the reference skips such a sequence (metrics.py:77-78): an all-zero row, valid 0
        if (tid < K) {
            const int64_t o = (int64_t)s * K + tid;
            tp_out[o] = 0; fp_out[o] = 0; fn_out[o] = 0; f1_out[o] = 0.0;
        }
        if (tid == 0) valid_out[s] = 0;
        return;
    }

    // 2. segment starts of the filtered target and prediction, numbered by a prefix sum
    int n_tgt = 0, n_pred = 0;
    for (int base = 0; base < n_kept; base += SEGF1_THREADS) {
        const int q = base + tid;
        bool ts = false, ps = false;
        if (q < n_kept) {
            const int64_t at = (int64_t)orig[q] * stride;
            ts = ps = q == 0;
            if (q > 0) {
                const int64_t prev = (int64_t)orig[q - 1] * stride;
                ts = yt[at] != yt[prev];
                ps = yp[at] != yp[prev];
            }
        }
        const unsigned long long tmask = __ballot(ts), pmask = __ballot(ps);
        if (lane == 0) { wave_cnt[0][wave] = __popcll(tmask); wave_cnt[1][wave] = __popcll(pmask); }
        __syncthreads();
        int tbefore = n_tgt, ttotal = n_tgt, pbefore = n_pred, ptotal = n_pred;
        for (int w = 0; w < SEGF1_WAVES; ++w) {
            const int ct = wave_cnt[0][w], cp = wave_cnt[1][w];
            if (w < wave) { tbefore += ct; pbefore += cp; }
            ttotal += ct;
            ptotal += cp;
        }
        if (q < n_kept) {
            const int t = tbefore + lanes_below(tmask) + (ts ? 1 : 0) - 1;   // the segment that holds q
            tseg[q] = (unsigned short)t;
            if (ts) tstart[t] = (unsigned short)q;
            if (ps) pstart[pbefore + lanes_below(pmask)] = (unsigned short)q;
        }
        n_tgt = ttotal;
        n_pred = ptotal;
        __syncthreads();
    }
    if (tid == 0) { tstart[n_tgt] = (unsigned short)n_kept; pstart[n_pred] = (unsigned short)n_kept; }
    __syncthreads();

    // 3. one lane per predicted segment: first maximum of inter / union over its candidate range, then one bit per
    // overlap it reaches (an OR: the bitmaps do not depend on the arrival order)
    int counted = 0;
    for (int p = tid; p < n_pred; p += SEGF1_THREADS) {
        const int o0 = pstart[p], o1 = pstart[p + 1];
        const long long label = yp[(int64_t)orig[o0] * stride];
        if (label >= num_classes) continue;                     // metrics.py:38-39
        ++counted;
        const int t_first = tseg[o0], t_last = tseg[o1 - 1];
        double best = 0.0;
        int idx = -1;
        for (int t = t_first; t <= t_last; ++t) {
            const int t0 = tstart[t], t1 = tstart[t + 1];
            if (yt[(int64_t)orig[t0] * stride] != label) continue;
            const int inter = min(o1, t1) - max(o0, t0);
            const int uni = max(o1, t1) - min(o0, t0);
            const double iou = (double)inter / (double)uni;
            if (iou > best) { best = iou; idx = t; }
        }
        if (idx < 0) continue;
        for (int k = 0; k < K; ++k)
            if (best >= ov.k[k]) atomicOr(&bitmap[k * words + (idx >> 5)], 1u << (idx & 31));
    }
    counted = wave_sum_int(counted);
    if (lane == 0) wave_cnt[0][wave] = counted;
    __syncthreads();
    counted = 0;
    for (int w = 0; w < SEGF1_WAVES; ++w) counted += wave_cnt[0][w];

    // 4. TP_k = set bits of bitmap k (wave w takes k = w, w + 4)
    const int tgt_words = (n_tgt + 31) >> 5;
    for (int k = wave; k < K; k += SEGF1_WAVES) {
        int c = 0;
        for (int w = lane; w < tgt_words; w += TWOG_WAVE) c += __popc(bitmap[k * words + w]);
        c = wave_sum_int(c);
        if (lane == 0) tp_k[k] = c;
    }
    __syncthreads();
    if (tid < K) {
        const int tp = tp_k[tid], fp = counted - tp, fn = n_tgt - tp;
        const int64_t o = (int64_t)s * K + tid;
        tp_out[o] = tp; fp_out[o] = fp; fn_out[o] = fn;
        f1_out[o] = segment_f1_value(tp, fp, fn);
    }
    if (tid == 0) valid_out[s] = 1;
}

// One workgroup: sums[k] += sum_s f1[s][k], valid_sums[k] += sum_s valid[s], in fp64 and in a fixed order -- thread t adds
// rows t, t + 256, ... in that order, then a fixed tree over the 256 partial sums.
__global__ __launch_bounds__(SEGF1_THREADS) void segment_f1_accumulate_kernel(const double* f1, const int* valid, int n_seq,
                                                                              int K, double* f1_sums, double* valid_sums) {
    __shared__ double red[SEGF1_THREADS];
    const int tid = threadIdx.x;
    for (int k = 0; k <= K; ++k) {   // column K is `valid`
        double v = 0.0;
        for (int s = tid; s < n_seq; s += SEGF1_THREADS) v += k < K ? f1[(int64_t)s * K + k] : (double)valid[s];
        red[tid] = v;
        __syncthreads();
        for (int h = SEGF1_THREADS / 2; h > 0; h >>= 1) {
            if (tid < h) red[tid] += red[tid + h];
            __syncthreads();
        }
        if (tid == 0) {
            if (k < K) f1_sums[k] += red[0];
            else for (int j = 0; j < K; ++j) valid_sums[j] += red[0];
        }
        __syncthreads();
    }
}

// ---- segmental edit score with a workgroup per sequence: 100 * (1 - Levenshtein(true segments, predicted segments) /
// max(m, n)), unit costs. The ignored steps are dropped first (the rule and the compaction of segment_f1_kernel), both
// filtered sequences are run-length encoded, and a segment whose label is bg_label is left out of its list WITHOUT
// merging its neighbours: a step opens a list entry iff it starts a run and its label is not the background.
// The table D[i][j] (i <= m true segments, j <= n predicted ones) is filled over its anti-diagonals d = i + j: a cell
// needs D[i-1][j] and D[i][j-1] of diagonal d - 1 and D[i-1][j-1] of diagonal d - 2, so three rolling diagonals indexed
// by i are the whole state, with one barrier per diagonal (it orders the writes of d before the reads of d + 1, and the
// reads of d - 2 before d + 1 overwrites that buffer).
// LDS: tl[] / pl[] the two segment-label lists as int64 (labels are compared exactly, without a second look at global
// memory), then three diagonals of (rounded + 2) 16-bit entries (values <= SEGF1_MAX_STEPS). orig[] (the step of the
// q-th kept step, needed until the lists exist) lies on the first diagonal. 16 * rounded + 6 * (rounded + 2) bytes:
// 90 124 at 4096 steps, one workgroup per CU; 8 460 at the 384 an evaluation batch has.
inline size_t segedit_lds_bytes(int n_steps) {
    const int r = segf1_round_steps(n_steps);
    return (size_t)2 * r * sizeof(long long) + (size_t)3 * (r + 2) * sizeof(unsigned short);
}

__device__ __forceinline__ double segment_edit_value(int distance, int longer) {
#pragma clang fp contract(off)
    const double ratio = (double)distance / (double)longer;
    const double kept = 1.0 - ratio;
    return kept * 100.0;
}

// Diagonal d of the table: its two border cells (0, d) and (d, 0), then the inner cells i = lo + tid, lo + tid + 256, ...
// without a branch. The diagonal written is none of the four arrays read, which the qualifiers say, so that the loads of
// several cells are in flight together.
__device__ __forceinline__ void segment_edit_diagonal(unsigned short* __restrict__ cur, const unsigned short* __restrict__ p1,
                                                      const unsigned short* __restrict__ p2, const long long* __restrict__ tl,
                                                      const long long* __restrict__ pl, int d, int m, int n, int tid) {
    if (tid == 0 && d <= n) cur[0] = (unsigned short)d;
    if (tid == 1 && d <= m) cur[d] = (unsigned short)d;
    const int lo = max(1, d - n), hi = min(d - 1, m);
#pragma unroll 4
    for (int i = lo + tid; i <= hi; i += SEGF1_THREADS) {
        const int edge = min((int)p1[i - 1], (int)p1[i]) + 1;                          // deletion, insertion
        const int subst = (int)p2[i - 1] + (tl[i - 1] != pl[d - i - 1] ? 1 : 0);
        cur[i] = (unsigned short)min(edge, subst);
    }
}

__global__ __launch_bounds__(SEGF1_THREADS) void segment_edit_kernel(
    const long long* y_true, const long long* y_pred, int n_steps, int entities, long long ignore, int use_ignore,
    long long bg, int use_bg, double* score_out, int* dist_out, int* n_true_out, int* n_pred_out, int* valid_out) {
    extern __shared__ long long segedit_lds[];
    __shared__ int wave_cnt[2][SEGF1_WAVES];
    const int rounded = (n_steps + 63) & ~63;
    long long* tl = segedit_lds;
    long long* pl = tl + rounded;
    unsigned short* diag0 = reinterpret_cast<unsigned short*>(pl + rounded);
    unsigned short* diag1 = diag0 + (rounded + 2);
    unsigned short* diag2 = diag1 + (rounded + 2);
    unsigned short* orig = diag0;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = blockIdx.x;
    int64_t off, stride;
    if (entities > 0) { off = (int64_t)(s / entities) * n_steps * entities + s % entities; stride = entities; }
    else { off = (int64_t)s * n_steps; stride = 1; }
    const long long* yt = y_true + off;
    const long long* yp = y_pred + off;

    // 1. drop the ignored steps: orig[q] = step of the q-th kept one
    int n_kept = 0;
    for (int base = 0; base < n_steps; base += SEGF1_THREADS) {
        const int i = base + tid;
        const bool kept = i < n_steps && !(use_ignore && yt[(int64_t)i * stride] == ignore);
        const unsigned long long mask = __ballot(kept);
        if (lane == 0) wave_cnt[0][wave] = __popcll(mask);
        __syncthreads();
        int before = n_kept, total = n_kept;
        for (int w = 0; w < SEGF1_WAVES; ++w) {
            const int c = wave_cnt[0][w];
            if (w < wave) before += c;
            total += c;
        }
        if (kept) orig[before + lanes_below(mask)] = (unsigned short)i;
        n_kept = total;
        __syncthreads();
    }

    // 2. the two lists: one entry per run start whose label is not the background
    int m = 0, n = 0;
    for (int base = 0; base < n_kept; base += SEGF1_THREADS) {
        const int q = base + tid;
        bool ts = false, ps = false;
        long long tlab = 0, plab = 0;
        if (q < n_kept) {
            const int64_t at = (int64_t)orig[q] * stride;
            tlab = yt[at];
            plab = yp[at];
            ts = ps = q == 0;
            if (q > 0) {
                const int64_t prev = (int64_t)orig[q - 1] * stride;
                ts = tlab != yt[prev];
                ps = plab != yp[prev];
            }
            ts = ts && !(use_bg && tlab == bg);
            ps = ps && !(use_bg && plab == bg);
        }
        const unsigned long long tmask = __ballot(ts), pmask = __ballot(ps);
        if (lane == 0) { wave_cnt[0][wave] = __popcll(tmask); wave_cnt[1][wave] = __popcll(pmask); }
        __syncthreads();
        int tbefore = m, ttotal = m, pbefore = n, ptotal = n;
        for (int w = 0; w < SEGF1_WAVES; ++w) {
            const int ct = wave_cnt[0][w], cp = wave_cnt[1][w];
            if (w < wave) { tbefore += ct; pbefore += cp; }
            ttotal += ct;
            ptotal += cp;
        }
        if (ts) tl[tbefore + lanes_below(tmask)] = tlab;
        if (ps) pl[pbefore + lanes_below(pmask)] = plab;
        m = ttotal;
        n = ptotal;
        __syncthreads();
    }
    const int longer = max(m, n);
    if (longer == 0) {   // no kept step, or nothing but background: an all-zero row that the mean skips. m and n are
        if (tid == 0) {  // workgroup-uniform, and no barrier follows
            score_out[s] = 0.0; dist_out[s] = 0; n_true_out[s] = 0; n_pred_out[s] = 0; valid_out[s] = 0;
        }
        return;
    }

    // 3. the table, diagonal by diagonal (orig[] is dead: the last barrier of phase 2 is behind every read of it)
    unsigned short *cur = diag0, *p1 = diag2, *p2 = diag1;   // diagonals d, d - 1, d - 2
    for (int d = 0; d <= m + n; ++d) {
        segment_edit_diagonal(cur, p1, p2, tl, pl, d, m, n, tid);
        __syncthreads();
        unsigned short* freed = p2;
        p2 = p1; p1 = cur; cur = freed;
    }
    if (tid == 0) {   // p1 is the last diagonal written, d = m + n, whose one cell is i = m
        const int distance = p1[m];
        score_out[s] = segment_edit_value(distance, longer);
        dist_out[s] = distance; n_true_out[s] = m; n_pred_out[s] = n; valid_out[s] = 1;
    }
}

}  // namespace

extern "C" int twog_predict_labels(const float* logp, int bs, int n_classes, int T, int E, int downsampling, int T_out,
                                   int64_t* labels, void* stream) {
    if (bs < 0 || n_classes < 1 || T < 1 || E < 1 || downsampling < 1 || T_out < 0) return -1;
    const int64_t n = (int64_t)bs * T_out * E;
    if (n == 0) return 0;
    const int grid = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(predict_labels_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, logp, bs, n_classes, T, E,
                       downsampling, T_out, reinterpret_cast<long long*>(labels));
    TWOG_CHECK_LAUNCH();
    return 0;
}

extern "C" int twog_f1_at_k(const int64_t* y_true, const int64_t* y_pred, int n_seq, int n_steps, int num_classes,
                            double overlap, int64_t ignore_value, int use_ignore, unsigned char* scratch, float* f1,
                            float* valid, void* stream) {
    if (n_seq < 0 || n_steps < 0) return -1;
    if (n_seq == 0) return 0;
    hipLaunchKernelGGL(f1_at_k_kernel, dim3((n_seq + 63) / 64), dim3(64), 0, (hipStream_t)stream,
                       reinterpret_cast<const long long*>(y_true), reinterpret_cast<const long long*>(y_pred), n_seq,
                       n_steps, num_classes, overlap, (long long)ignore_value, use_ignore, scratch, f1, valid);
    TWOG_CHECK_LAUNCH();
    return 0;
}

extern "C" int twog_eval_limits(int* max_classes, int* positions_per_trip) {
    if (max_classes) *max_classes = EVAL_MAX_CLASSES;
    if (positions_per_trip) *positions_per_trip = EVAL_GRID_CAP * 256;
    return 0;
}

extern "C" int twog_eval_update(const float* logp, int bs, int n_classes, int T, int E, int downsampling,
                                const int64_t* target, int T_tgt, const int32_t* step_index, int S, int64_t* counts,
                                int64_t* flags, int64_t* labels_out, int64_t* targets_out, void* stream) {
    if (bs < 0 || n_classes < 1 || T < 1 || E < 1 || downsampling < 1 || T_tgt < 0 || (step_index && S < 0)) return -1;
    if (n_classes > EVAL_MAX_CLASSES) return -2;
    const int steps = step_index ? S : T_tgt;
    const int64_t n = (int64_t)bs * steps * E;
    if (n == 0) return 0;
    const size_t lds = ((size_t)n_classes * n_classes + 2) * sizeof(unsigned);
    hipLaunchKernelGGL(eval_update_kernel, dim3(eval_grid(n)), dim3(256), lds, (hipStream_t)stream, logp, bs, n_classes,
                       T, E, downsampling, reinterpret_cast<const long long*>(target), T_tgt, step_index, steps,
                       reinterpret_cast<long long*>(counts), reinterpret_cast<long long*>(flags),
                       reinterpret_cast<long long*>(labels_out), reinterpret_cast<long long*>(targets_out));
    TWOG_CHECK_LAUNCH();
    return 0;
}

extern "C" int twog_confusion_counts(const int64_t* y_true, const int64_t* y_pred, int64_t n, int n_classes,
                                     int64_t* counts, int64_t* flags, void* stream) {
    if (n < 0 || n_classes < 1) return -1;
    if (n_classes > EVAL_MAX_CLASSES) return -2;
    if (n == 0) return 0;
    const size_t lds = ((size_t)n_classes * n_classes + 2) * sizeof(unsigned);
    hipLaunchKernelGGL(confusion_counts_kernel, dim3(eval_grid(n)), dim3(256), lds, (hipStream_t)stream,
                       reinterpret_cast<const long long*>(y_true), reinterpret_cast<const long long*>(y_pred), n,
                       n_classes, reinterpret_cast<long long*>(counts), reinterpret_cast<long long*>(flags));
    TWOG_CHECK_LAUNCH();
    return 0;
}

extern "C" int twog_class_counts(const int64_t* targets, int64_t n, int n_classes, int64_t ignore_index, int64_t* counts,
                                 void* stream) {
    if (n < 0 || n_classes < 1) return -1;
    if (n_classes > TWOG_CLASS_COUNTS_MAX) return -2;
    if (n == 0) return 0;
    hipLaunchKernelGGL(class_counts_kernel, dim3(eval_grid(n)), dim3(256), (size_t)n_classes * sizeof(unsigned),
                       (hipStream_t)stream, reinterpret_cast<const long long*>(targets), n, n_classes,
                       (long long)ignore_index, reinterpret_cast<long long*>(counts));
    TWOG_CHECK_LAUNCH();
    return 0;
}

extern "C" int twog_segment_f1_limits(int* max_steps, int* max_overlaps) {
    if (max_steps) *max_steps = SEGF1_MAX_STEPS;
    if (max_overlaps) *max_overlaps = SEGF1_MAX_OVERLAPS;
    return 0;
}

extern "C" int twog_segment_f1(const int64_t* y_true, const int64_t* y_pred, int n_seq, int n_steps, int entities,
                               int num_classes, const double* overlaps, int n_overlaps, int64_t ignore_value,
                               int use_ignore, int32_t* tp, int32_t* fp, int32_t* fn, double* f1, int32_t* valid,
                               void* stream) {
    if (n_seq < 0 || n_steps < 0 || entities < 0 || (entities > 0 && n_seq % entities != 0)) return -1;
    if (n_overlaps < 1 || n_overlaps > SEGF1_MAX_OVERLAPS || !overlaps) return -1;
    SegF1Overlaps ov = {};
    for (int k = 0; k < n_overlaps; ++k) {
        if (!(overlaps[k] > 0.0)) return -1;   // zero, negative or NaN: only twog_f1_at_k serves those
        ov.k[k] = overlaps[k];
    }
    if (n_steps > SEGF1_MAX_STEPS) return -2;
    if (n_seq == 0) return 0;
    static_assert(4 * (SEGF1_MAX_STEPS + 2) * 2 + SEGF1_MAX_OVERLAPS * (SEGF1_MAX_STEPS / 32 + 1) * 4 + 64 <= 64 * 1024,
                  "the LDS layout at the longest sequence stays below what a launch may ask for without an attribute");
    hipLaunchKernelGGL(segment_f1_kernel, dim3(n_seq), dim3(SEGF1_THREADS), segf1_lds_bytes(n_steps), (hipStream_t)stream,
                       reinterpret_cast<const long long*>(y_true), reinterpret_cast<const long long*>(y_pred), n_steps,
                       entities, (long long)num_classes, ov, n_overlaps, (long long)ignore_value, use_ignore, tp, fp, fn,
                       f1, valid);
    TWOG_CHECK_LAUNCH();
    return 0;
}

extern "C" int twog_segment_f1_accumulate(const double* f1, const int32_t* valid, int n_seq, int n_overlaps,
                                          double* f1_sums, double* valid_sums, void* stream) {
    if (n_seq < 0 || n_overlaps < 1 || n_overlaps > SEGF1_MAX_OVERLAPS) return -1;
    if (n_seq == 0) return 0;
    hipLaunchKernelGGL(segment_f1_accumulate_kernel, dim3(1), dim3(SEGF1_THREADS), 0, (hipStream_t)stream, f1, valid, n_seq,
                       n_overlaps, f1_sums, valid_sums);
    TWOG_CHECK_LAUNCH();
    return 0;
}

extern "C" int twog_segment_edit_limits(int* max_steps) {
    if (max_steps) *max_steps = SEGF1_MAX_STEPS;
    return 0;
}

extern "C" int twog_segment_edit(const int64_t* y_true, const int64_t* y_pred, int n_seq, int n_steps, int entities,
                                 int64_t ignore_value, int use_ignore, int64_t bg_label, int use_bg, double* score,
                                 int32_t* distance, int32_t* n_true, int32_t* n_pred, int32_t* valid, void* stream) {
    if (n_seq < 0 || n_steps < 0 || entities < 0 || (entities > 0 && n_seq % entities != 0)) return -1;
    if (n_steps > SEGF1_MAX_STEPS) return -2;
    if (n_seq == 0) return 0;
    // n_steps == 0 is launched like any other length, as twog_segment_f1 does: every sequence is empty, and the kernel
    // writes its all-zero row
    constexpr int LDS_LIMIT = 2 * SEGF1_MAX_STEPS * 8 + 3 * (SEGF1_MAX_STEPS + 2) * 2;
    static_assert(LDS_LIMIT + 64 <= 160 * 1024, "the LDS layout at the longest sequence fits one CU");
    static std::atomic<uint32_t> lds_attr_done{0};
    twog_allow_dynamic_lds(segment_edit_kernel, LDS_LIMIT, lds_attr_done);
    hipLaunchKernelGGL(segment_edit_kernel, dim3(n_seq), dim3(SEGF1_THREADS), segedit_lds_bytes(n_steps),
                       (hipStream_t)stream, reinterpret_cast<const long long*>(y_true),
                       reinterpret_cast<const long long*>(y_pred), n_steps, entities, (long long)ignore_value, use_ignore,
                       (long long)bg_label, use_bg, score, distance, n_true, n_pred, valid);
    TWOG_CHECK_LAUNCH();
    return 0;
}
