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
