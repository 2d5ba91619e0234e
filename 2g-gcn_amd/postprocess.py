"""Inference post-processing on the device.

Mirror of the steps `predict.py` runs after the model: `match_shape` (:95-116), the ``repeat_interleave`` by the
downsampling factor (:64-70), `process_output`'s argmax (:186-202) and `pyrutils.metrics.f1_at_k` (:68-81) as used by
`evaluate_f1_at_k` (predict.py:229-246). The reference copies every (bs, C, T, E) log-probability tensor to the host and
does these in numpy; here the labels and the per-sequence F1@k are computed by HIP kernels and only the final scalar
(or the int64 labels, C x smaller than the log-probabilities) crosses PCIe.

The frame-wise half of the evaluation is here too: `evaluate_predictions` (predict.py:205-226: micro / macro precision,
recall and F1, the per-class report), the Bimanual 15-fps fix-up `downsample_bad_bimanual_videos` (:136-156) and
`summarize_frames_into_segments` (:159-183). The device builds C x C confusion counts (twog_eval_update,
twog_confusion_counts); every metric is a few hundred fp64 divisions on those integers, done on the host in numpy with
scikit-learn's semantics, so scikit-learn itself is not needed. `EvaluationAccumulator` keeps the counts and the F1@k
sums on the device over a whole test set and merges over ranks by a sum.

The segmental edit score (twog_segment_edit) is the third number an action-segmentation model is reported with; the
reference does not compute it, so its definition is stated at `edit_score_per_example`.

`ViterbiDecoder` replaces the per-step argmax by the best label path under a label-transition model (twog_viterbi_decode;
the reference has no such decode either, `viterbi_labels` states the definition); `transition_counts`,
`transition_log_probs` and `switch_penalty` make the model. `process_output` and `EvaluationAccumulator` take a decoder.

`SegmentalDecoder` stands in the same slot and scores whole segments: emission sum + per-class duration score +
segment-to-segment transition (twog_segdecode; `segment_decode_labels` states the definition). `duration_counts`,
`duration_log_probs` and `segment_transition_log_probs` make its model from label tensors.
"""
import math
from collections import namedtuple

import numpy as np
import torch
import torch.distributed as dist

from .kernels import get_kernels, unpack_segment_edit, unpack_segment_f1


def match_shape(out: torch.Tensor, tgt: torch.Tensor) -> torch.Tensor:
    """predict.py:95-116 (kept for callers that still want the resized log-probabilities)."""
    if out.ndim == 3:
        o, t = out.shape[-1], tgt.shape[-1]
        if o >= t:
            return out[..., :t]
        return torch.cat([out, out[..., -1:].expand(*out.shape[:-1], t - o)], dim=-1)
    if out.ndim == 4:
        o, t = out.shape[-2], tgt.shape[-2]
        if o >= t:
            return out[:, :, :t]
        return torch.cat([out, out[:, :, -1:].expand(out.shape[0], out.shape[1], t - o, out.shape[3])], dim=-2)
    return out


def predict_labels(output: torch.Tensor, target: torch.Tensor = None, downsampling: int = 1) -> torch.Tensor:
    """Labels of one model output: ``argmax(match_shape(repeat_interleave(output, downsampling, -2), target), 1)`` in one
    kernel, without materialising the upsampled tensor. output (bs, C, T, E); returns int64 (bs, T_target, E)."""
    if output.ndim != 4:
        raise RuntimeError(f'Number of dimensions for output is {output.ndim}')  # predict.py:66-67
    steps = output.shape[-2] if (downsampling <= 1 or target is None) else target.shape[-2]
    return get_kernels().predict_labels(output, max(1, int(downsampling)), steps)


def process_output(outputs, downsampling: int = 1, targets=None, index_to_name=None, decoder=None, lengths=None):
    """predict.py:186-202 for predictions: list over batches of lists of (bs, C, T, E) outputs -> {index: int64 labels
    (N, T, E) on the device} (the reference returns numpy arrays of the same values). decoder: a `ViterbiDecoder` or a
    `SegmentalDecoder` (one for every output, or a dict {key: decoder}; an output without one keeps the argmax) that
    replaces the per-step argmax; lengths: with a decoder, one int64 (bs,) device tensor of model steps per batch, or
    None."""
    per_index = {}
    for bi, output in enumerate(outputs):
        for i, tensor in enumerate(output):
            tgt = None if targets is None else targets[bi][i]
            key = index_to_name[i] if index_to_name is not None else i
            dec = decoder.get(key) if isinstance(decoder, dict) else decoder
            if dec is None:
                labels = predict_labels(tensor, tgt, downsampling)
            else:
                labels = dec(tensor, tgt, downsampling, None if lengths is None else lengths[bi])
            per_index.setdefault(key, []).append(labels)
    return {k: torch.cat(v, 0) for k, v in per_index.items()}


# --------------------------------------------------------------------------------------------------------------------
# Viterbi decode under a label-transition model (twog_viterbi_decode) and the statistics such a model is made from
def transition_counts(targets, num_classes: int, stride: int = 1, ignore_index: int = -1, out=None) -> torch.Tensor:
    """int64 (C, C) counts (row = from, column = to) of the label pairs (targets[b, k * stride, e], targets[b, (k + 1) *
    stride, e]) of a (bs, T, E) or (bs, T) label tensor on the device: the transitions at the model's rate when `stride`
    is the loader's downsampling. A pair that touches `ignore_index` or a label outside [0, C) is not counted. With `out`
    the counts are ADDED to it, so that a pass over a loader accumulates (as `losses.class_counts` does); no host
    synchronisation either way."""
    K = get_kernels()
    targets = targets.to(torch.int64)
    if targets.ndim == 2:
        targets = targets.unsqueeze(-1)
    if targets.ndim != 3:
        raise ValueError(f'labels (bs, T) or (bs, T, E) expected, not {tuple(targets.shape)}')
    if int(stride) < 1:
        raise ValueError(f'stride must be at least 1, not {stride}')
    max_classes = K.viterbi_limits()[0]
    if num_classes > max_classes:
        raise ValueError(f'transition_counts takes up to {max_classes} classes, not {num_classes}')
    if out is None:
        out = K.zeros(num_classes, num_classes, dtype=torch.int64, device=targets.device)
    return K.transition_counts(targets.contiguous(), int(num_classes), int(stride), int(ignore_index), out)


def transition_log_probs(counts, smoothing: float = 1.0) -> torch.Tensor:
    """fp32 (C, C) log((n + s) / (row sum + C * s)) of transition counts, computed in fp64 on the host from ONE copy of
    the counts and rounded to fp32 once; returned on the device of `counts`. With smoothing 0 an unseen transition is
    -inf (forbidden); a row with no counts at all (and no smoothing) is all zeros: nothing is known about leaving it."""
    device = counts.device if isinstance(counts, torch.Tensor) else None
    n = (counts.cpu().numpy() if isinstance(counts, torch.Tensor) else np.asarray(counts)).astype(np.float64)
    if n.ndim != 2 or n.shape[0] != n.shape[1]:
        raise ValueError(f'square counts expected, not {n.shape}')
    s = float(smoothing)
    den = n.sum(1, keepdims=True) + n.shape[0] * s
    with np.errstate(divide='ignore', invalid='ignore'):
        logp = np.log((n + s) / den)
    logp = np.where(den > 0, logp, 0.0).astype(np.float32)
    out = torch.from_numpy(logp)
    return out.to(device) if device is not None else out


def switch_penalty(num_classes: int, penalty: float, device=None) -> torch.Tensor:
    """fp32 (C, C) transition scores with 0 on the diagonal and -penalty elsewhere: the model that needs no training
    data; every change of label costs `penalty` nats."""
    a = np.full((num_classes, num_classes), -float(penalty), dtype=np.float32)
    np.fill_diagonal(a, 0.0)
    out = torch.from_numpy(a)
    return out.to(device) if device is not None else out


def viterbi_labels(output, transitions, initial=None, target=None, downsampling: int = 1, lengths=None):
    """(labels int64 (bs, T_target, E), score fp32 (bs, E)): the best label path of every sequence = (clip b, entity e) of
    (bs, C, T, E) log-probabilities, with T_target as `predict_labels` has it. `transitions` A fp32 (C, C) (row = from,
    column = to), `initial` pi fp32 (C,) or None (all zero), `lengths` int64 (bs,) on the device in model steps (clamped to
    [0, T]; None means T), all on the output's device. With logp[t, c] = output[b, c, t, e] and L the length, in fp32 with
    one rounding per add, nothing fused or reordered:

        d[0][c] = logp[0,c] + pi[c]
        m[t][c] = max over c' of (d[t-1][c'] + A[c',c])      psi[t][c] = the SMALLEST c' that attains it
        d[t][c] = m[t][c] + logp[t,c]                        (t = 1 .. L-1)
        y[L-1]  = the smallest c attaining max d[L-1][.]     y[t-1] = psi[t][y[t]]      score = max d[L-1][.]

    A candidate replaces the running best only when it is strictly greater: that is the tie-break (among paths of equal
    score the smallest one compared from the last step backwards) and it decides what -inf does; -inf entries of A
    (forbidden transitions) are in contract, NaN is not (it still gives labels in [0, C)). labels[b, t', e] = y[min(t' //
    downsampling, L - 1)]; a length of 0 gives label 0 everywhere and score 0.0. tests/viterbi_ref.py is this definition
    in numpy, and the kernel (twog_viterbi_decode) meets it bit for bit. ValueError beyond `kernels.viterbi_limits()`."""
    if output.ndim != 4:
        raise RuntimeError(f'Number of dimensions for output is {output.ndim}')  # predict.py:66-67
    downsampling = max(1, int(downsampling))
    steps = output.shape[-2] if (downsampling <= 1 or target is None) else target.shape[-2]   # as predict_labels
    return get_kernels().viterbi_decode(output, transitions, initial, lengths, downsampling, steps)


class ViterbiDecoder:
    """The sequence-level replacement of `predict_labels`: the best label path of every (clip, entity) under fp32 (C, C)
    transition scores (row = from, column = to; -inf forbids a transition) and optional (C,) initial scores, decoded on
    the device by twog_viterbi_decode (`viterbi_labels` states the recurrence and its tie-break). The tensors are kept
    on the device in fp32 and moved once to the device of the first output decoded.

    decoder(output, target=None, downsampling=1, lengths=None) returns what `predict_labels` returns for the same
    arguments, int64 (bs, T_target, E); lengths int64 (bs,) on the device gives the valid model steps of every clip, the
    labels behind them repeat the last decoded one. `last_score` holds the fp32 (bs, E) path scores of the last call."""

    def __init__(self, transitions, initial=None):
        as_f32 = lambda v: torch.as_tensor(v).detach().to(torch.float32).contiguous()
        self.transitions = as_f32(transitions)
        if self.transitions.ndim != 2 or self.transitions.shape[0] != self.transitions.shape[1]:
            raise ValueError(f'transitions must be (C, C), not {tuple(self.transitions.shape)}')
        self.num_classes = self.transitions.shape[0]
        self.initial = None if initial is None else as_f32(initial)
        if self.initial is not None and self.initial.shape != (self.num_classes,):
            raise ValueError(f'initial must be ({self.num_classes},), not {tuple(self.initial.shape)}')
        self.last_score = None

    def __call__(self, output: torch.Tensor, target: torch.Tensor = None, downsampling: int = 1, lengths=None):
        if output.ndim != 4:
            raise RuntimeError(f'Number of dimensions for output is {output.ndim}')  # predict.py:66-67
        downsampling = max(1, int(downsampling))
        steps = output.shape[-2] if (downsampling <= 1 or target is None) else target.shape[-2]   # as predict_labels
        return self.decode(output, downsampling, steps, lengths)

    def decode(self, output, downsampling, steps, lengths=None):
        """The labels at `steps` target steps, int64 (bs, steps, E): step t' reads model step t' // downsampling, as
        twog_eval_update evaluates it."""
        if output.shape[1] != self.num_classes:
            raise ValueError(f'the output has {output.shape[1]} classes, the transition model {self.num_classes}')
        if self.transitions.device != output.device:
            self.transitions = self.transitions.to(output.device)
            self.initial = None if self.initial is None else self.initial.to(output.device)
        if lengths is not None:
            lengths = lengths.to(device=output.device, dtype=torch.int64).contiguous()
        labels, self.last_score = get_kernels().viterbi_decode(output, self.transitions, self.initial, lengths,
                                                               int(downsampling), int(steps))
        return labels


# --------------------------------------------------------------------------------------------------------------------
# Segmental decode under a duration model (twog_segdecode) and the statistics such a model is made from
def duration_counts(targets, num_classes: int, max_duration: int, stride: int = 1, ignore_index: int = -1,
                    out=None) -> torch.Tensor:
    """int64 (C, D) counts of the run lengths of a (bs, T, E) or (bs, T) label tensor on the device, read at the model's
    rate (targets[b, k * stride, e], k = 0, 1, ...; `stride` is the loader's downsampling): a maximal run of n equal
    labels c adds one to [c, min(n, D) - 1], D = max_duration. A label counts only if it is in [0, C) and is not
    `ignore_index`; a run ends at a change of label, at a label that does not count and at the end of the sequence. With
    `out` the counts are ADDED to it, so that a pass over a loader accumulates (as `transition_counts` does); no host
    synchronisation either way."""
    K = get_kernels()
    targets = targets.to(torch.int64)
    if targets.ndim == 2:
        targets = targets.unsqueeze(-1)
    if targets.ndim != 3:
        raise ValueError(f'labels (bs, T) or (bs, T, E) expected, not {tuple(targets.shape)}')
    if int(stride) < 1:
        raise ValueError(f'stride must be at least 1, not {stride}')
    if int(max_duration) < 1:
        raise ValueError(f'max_duration must be at least 1, not {max_duration}')
    max_classes, _, longest = K.segdecode_limits()
    if num_classes > max_classes or max_duration > longest:
        raise ValueError(f'duration_counts takes up to {max_classes} classes and durations up to {longest}, '
                         f'not {num_classes} and {max_duration}')
    if out is None:
        out = K.zeros(num_classes, max_duration, dtype=torch.int64, device=targets.device)
    return K.duration_counts(targets.contiguous(), int(num_classes), int(max_duration), int(stride), int(ignore_index), out)


def _counts_on_host(counts):
    device = counts.device if isinstance(counts, torch.Tensor) else None
    n = (counts.cpu().numpy() if isinstance(counts, torch.Tensor) else np.asarray(counts)).astype(np.float64)
    return n, device


def duration_log_probs(counts, smoothing: float = 1.0, scheme: str = 'empirical') -> torch.Tensor:
    """fp32 (C, D) duration scores of `duration_counts`, column l - 1 for a segment of l steps, computed in fp64 on the host
    from ONE copy of the counts and rounded to fp32 once; returned on the device of `counts`.
    'empirical': log((n + s) / (row sum + D * s)); with smoothing 0 an unseen duration is -inf (forbidden).
    'poisson': l * log(lambda_c) - lambda_c - lgamma(l + 1) with lambda_c the mean run length of class c in the counts (a
    run of D or more counts as D); `smoothing` is not used.
    A class without runs is all zeros either way: nothing is known about how long it lasts."""
    if scheme not in ('empirical', 'poisson'):
        raise ValueError(f"scheme must be 'empirical' or 'poisson', not {scheme!r}")
    n, device = _counts_on_host(counts)
    if n.ndim != 2 or n.shape[1] < 1:
        raise ValueError(f'(C, D) counts expected, not {n.shape}')
    D = n.shape[1]
    total = n.sum(1, keepdims=True)
    lengths = np.arange(1, D + 1, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        if scheme == 'empirical':
            s = float(smoothing)
            logp = np.log((n + s) / (total + D * s))
        else:
            lam = (n * lengths).sum(1, keepdims=True) / total
            lgamma = np.asarray([math.lgamma(l + 1.0) for l in lengths])
            logp = lengths * np.log(lam) - lam - lgamma
    logp = np.where(total > 0, logp, 0.0).astype(np.float32)
    out = torch.from_numpy(logp)
    return out.to(device) if device is not None else out


def segment_transition_log_probs(counts, smoothing: float = 1.0, self_transition=None) -> torch.Tensor:
    """fp32 (C, C) scores between consecutive SEGMENTS from the frame-level `transition_counts`: the diagonal (a label
    that stays) is removed before normalising, log((n + s) / (row sum without the diagonal + (C - 1) * s)) off the
    diagonal, in fp64 on the host from ONE copy of the counts and rounded to fp32 once; a row without any count (and no
    smoothing) is all zeros. The diagonal is set to `self_transition`; None means -inf: a segment is never followed by one
    of its own class, so the decoder's `max_duration` D must then cover the longest run, since a run longer than D can only
    be composed of several segments of the class."""
    n, device = _counts_on_host(counts)
    if n.ndim != 2 or n.shape[0] != n.shape[1]:
        raise ValueError(f'square counts expected, not {n.shape}')
    Cn = n.shape[0]
    np.fill_diagonal(n, 0.0)
    s = float(smoothing)
    den = n.sum(1, keepdims=True) + (Cn - 1) * s
    with np.errstate(divide='ignore', invalid='ignore'):
        logp = np.log((n + s) / den)
    logp = np.where(den > 0, logp, 0.0)
    np.fill_diagonal(logp, -np.inf if self_transition is None else float(self_transition))
    out = torch.from_numpy(logp.astype(np.float32))
    return out.to(device) if device is not None else out


def segment_decode_labels(output, transitions, durations, initial=None, target=None, downsampling: int = 1, lengths=None):
    """(labels int64 (bs, T_target, E), score fp32 (bs, E)): the best segmentation of every sequence = (clip b, entity e) of
    (bs, C, T, E) log-probabilities, with T_target as `predict_labels` has it. `transitions` A fp32 (C, C) scores between
    consecutive segments (row = from, column = to), `durations` dur fp32 (C, D): dur[c, l-1] is the score of a class-c
    segment that lasts l steps, `initial` pi fp32 (C,) or None (all zero), `lengths` int64 (bs,) on the device in model
    steps (clamped to [0, T]; None means T), all on the output's device. With logp[t, c] = output[b, c, t, e] and L the
    length, in fp32, each add rounding once in the order written, nothing fused or reordered:

        e[0][c] = pi[c]
        e[t][c] = max over c' of (d[t-1][c'] + A[c',c])      prev[t][c] = the SMALLEST c' that attains it   (t >= 1)
        for l = 1 .. min(D, t+1), ascending:   acc_l = acc_(l-1) + logp[t-l+1,c]   (acc_0 = 0)
                                               cand_l = (e[t-l+1][c] + dur[c,l-1]) + acc_l
        d[t][c] = max over l of cand_l         len[t][c] = the SMALLEST l that attains it
        end:  c = the smallest class attaining max d[L-1][.];  score = that maximum;  t = L-1
        back: l = len[t][c];  y[t-l+1 .. t] = c;  stop if t-l+1 == 0;  c = prev[t-l+1][c];  t = t - l

    A candidate replaces the running best only when it is strictly greater. The diagonal of A is used like any other
    entry: a segment may be followed by one of its own class at A[c,c], which is how runs longer than D are composed;
    -inf forbids it. -inf in A, pi and dur (forbidden transitions, minimum durations) is in contract, NaN is not (it still
    gives labels in [0, C)). labels[b, t', e] = y[min(t' // downsampling, L - 1)]; a length of 0 gives label 0 everywhere
    and score 0.0. tests/segdecode_ref.py is this definition in numpy, and the kernel (twog_segdecode) meets it bit for
    bit. ValueError beyond `kernels.segdecode_limits()`."""
    if output.ndim != 4:
        raise RuntimeError(f'Number of dimensions for output is {output.ndim}')  # predict.py:66-67
    downsampling = max(1, int(downsampling))
    steps = output.shape[-2] if (downsampling <= 1 or target is None) else target.shape[-2]   # as predict_labels
    return get_kernels().segment_decode(output, transitions, durations, initial, lengths, downsampling, steps)


class SegmentalDecoder:
    """`ViterbiDecoder` with a duration model: the best segmentation of every (clip, entity) under fp32 (C, C) scores
    between consecutive segments (row = from, column = to; -inf forbids), fp32 (C, D) duration scores (column l - 1: a
    segment of l steps; -inf forbids a duration) and optional (C,) initial scores, decoded on the device by twog_segdecode
    (`segment_decode_labels` states the recurrence and its tie-break). `num_classes` is C and `max_duration` D. The tensors
    are kept in fp32 and moved once to the device of the first output decoded.

    decoder(output, target=None, downsampling=1, lengths=None) and decode(output, downsampling, steps, lengths=None) are
    those of `ViterbiDecoder`, so `process_output` and `EvaluationAccumulator` take either. `last_score` holds the fp32
    (bs, E) scores of the last call."""

    def __init__(self, transitions, durations, initial=None):
        as_f32 = lambda v: torch.as_tensor(v).detach().to(torch.float32).contiguous()
        self.transitions = as_f32(transitions)
        if self.transitions.ndim != 2 or self.transitions.shape[0] != self.transitions.shape[1]:
            raise ValueError(f'transitions must be (C, C), not {tuple(self.transitions.shape)}')
        self.num_classes = self.transitions.shape[0]
        self.durations = as_f32(durations)
        if self.durations.ndim != 2 or self.durations.shape[0] != self.num_classes or self.durations.shape[1] < 1:
            raise ValueError(f'durations must be ({self.num_classes}, D) with D >= 1, not {tuple(self.durations.shape)}')
        self.max_duration = self.durations.shape[1]
        self.initial = None if initial is None else as_f32(initial)
        if self.initial is not None and self.initial.shape != (self.num_classes,):
            raise ValueError(f'initial must be ({self.num_classes},), not {tuple(self.initial.shape)}')
        self.last_score = None

    def __call__(self, output: torch.Tensor, target: torch.Tensor = None, downsampling: int = 1, lengths=None):
        if output.ndim != 4:
            raise RuntimeError(f'Number of dimensions for output is {output.ndim}')  # predict.py:66-67
        downsampling = max(1, int(downsampling))
        steps = output.shape[-2] if (downsampling <= 1 or target is None) else target.shape[-2]   # as predict_labels
        return self.decode(output, downsampling, steps, lengths)

    def decode(self, output, downsampling, steps, lengths=None):
        """The labels at `steps` target steps, int64 (bs, steps, E): step t' reads model step t' // downsampling, as
        twog_eval_update evaluates it."""
        if output.shape[1] != self.num_classes:
            raise ValueError(f'the output has {output.shape[1]} classes, the transition model {self.num_classes}')
        if self.transitions.device != output.device:
            self.transitions = self.transitions.to(output.device)
            self.durations = self.durations.to(output.device)
            self.initial = None if self.initial is None else self.initial.to(output.device)
        if lengths is not None:
            lengths = lengths.to(device=output.device, dtype=torch.int64).contiguous()
        labels, self.last_score = get_kernels().segment_decode(output, self.transitions, self.durations, self.initial,
                                                               lengths, int(downsampling), int(steps))
        return labels


def f1_at_k(y_true, y_pred, num_classes: int, *, overlap: float, ignore_value: float = None) -> float:
    """pyrutils/metrics.py:68-81 for (n_seq, n_steps) label matrices (device tensors or anything torch.as_tensor takes)."""
    K = get_kernels()
    dev = y_pred.device if isinstance(y_pred, torch.Tensor) else (y_true.device if isinstance(y_true, torch.Tensor) else 'cuda')
    yt = torch.as_tensor(np.asarray(y_true) if not isinstance(y_true, torch.Tensor) else y_true).to(dev)
    yp = torch.as_tensor(np.asarray(y_pred) if not isinstance(y_pred, torch.Tensor) else y_pred).to(dev)
    f1, valid = K.f1_at_k(yt.reshape(-1, yt.shape[-1]), yp.reshape(-1, yp.shape[-1]), num_classes, overlap, ignore_value)
    return float(f1.sum() / valid.sum())  # ZeroDivisionError-equivalent: nan when nothing is valid (reference raises)


def evaluate_f1_at_k(targets: dict, outputs: dict, num_subactivities, num_affordances, overlap: float = 0.25):
    """predict.py:229-246: {index: labels (N, T) or (N, T, E)} -> {index: F1@overlap}."""
    results = {}
    for index, target in sorted(targets.items()):
        output = outputs[index]
        if target.ndim == 3:
            target, output = target.transpose(1, 2), output.transpose(1, 2)
        steps = output.shape[-1]
        num_classes = num_affordances if 'affordance' in str(index) else num_subactivities
        results[index] = f1_at_k(target.reshape(-1, steps), output.reshape(-1, steps), num_classes, overlap=overlap,
                                 ignore_value=-1.0)
    return results


# --------------------------------------------------------------------------------------------------------------------
# segmental F1@k per example: every overlap from one matching (twog_segment_f1)
SegmentF1 = namedtuple('SegmentF1', 'f1 tp fp fn valid route')
SegmentF1.__doc__ = """f1 float64 (n_seq, K); tp / fp / fn int32 (n_seq, K), None on the 'thread' route; valid int32 (n_seq,), 0
for a sequence without a kept step (its rows are zero); route: 'workgroup' (twog_segment_f1) or 'thread' (twog_f1_at_k)."""


def _positive(overlaps):
    return all(o > 0 for o in overlaps)   # False for zero, a negative value and NaN


def _label_matrices(y_true, y_pred):
    dev = y_pred.device if isinstance(y_pred, torch.Tensor) else (y_true.device if isinstance(y_true, torch.Tensor) else 'cuda')
    to = lambda y: torch.as_tensor(np.asarray(y) if not isinstance(y, torch.Tensor) else y).to(dev).to(torch.int64)
    return to(y_true), to(y_pred)


def _segment_f1(K, yt, yp, num_classes, overlaps, ignore_value, entity_minor, need_counts=False):
    """SegmentF1 plus the packed buffer (None on the 'thread' route) for int64 label tensors on one device: sequence-major
    (n_seq, n_steps), or (bs, n_steps, E) with entity_minor. twog_segment_f1 takes positive overlaps and sequences up to
    its max_steps; anything else goes through the per-thread kernel, one launch per overlap, which has no counts."""
    overlaps = [float(o) for o in overlaps]
    max_steps, max_overlaps = K.segment_f1_limits()
    fits = len(overlaps) >= 1 and _positive(overlaps) and yt.shape[1] <= max_steps
    if fits and len(overlaps) <= max_overlaps:
        f1, tp, fp, fn, valid, packed = K.segment_f1(yt, yp, num_classes, overlaps, ignore_value, entity_minor=entity_minor)
        return SegmentF1(f1, tp, fp, fn, valid, 'workgroup'), packed
    if fits:   # more overlaps than one launch takes
        parts = [_segment_f1(K, yt, yp, num_classes, overlaps[j:j + max_overlaps], ignore_value, entity_minor)[0]
                 for j in range(0, len(overlaps), max_overlaps)]
        cat = lambda field: torch.cat([getattr(p, field) for p in parts], 1)
        return SegmentF1(cat('f1'), cat('tp'), cat('fp'), cat('fn'), parts[0].valid, 'workgroup'), None
    if need_counts:
        raise ValueError(f'tp / fp / fn exist only on the workgroup route: it takes overlaps > 0 and up to {max_steps} steps, '
                         f'not overlaps {overlaps} on {yt.shape[1]} steps')
    if entity_minor:
        steps = yt.shape[1]
        yt, yp = yt.transpose(1, 2).reshape(-1, steps), yp.transpose(1, 2).reshape(-1, steps)
    n_seq = yt.shape[0]
    f1 = torch.empty(n_seq, len(overlaps), dtype=torch.float64, device=yt.device)
    valid = torch.zeros(n_seq, dtype=torch.int32, device=yt.device)
    for j, overlap in enumerate(overlaps):
        f1_j, valid_j = K.f1_at_k(yt, yp, num_classes, overlap, ignore_value)
        f1[:, j] = f1_j
        valid = valid_j.to(torch.int32)
    return SegmentF1(f1, None, None, None, valid, 'thread'), None


def f1_at_k_per_example(y_true, y_pred, num_classes: int, overlaps, ignore_value: float = None, *, need_counts: bool = False):
    """pyrutils/metrics.py:7-65 for every sequence of (n_seq, n_steps) label matrices and every overlap, in one launch:
    the values `dump_f1_scores_per_example` prints and `f1_at_k` averages. Returns a SegmentF1 of device tensors. Overlaps
    <= 0 and sequences longer than twog_segment_f1 holds are served by the per-thread kernel (f1 stored in fp32 there, no
    tp / fp / fn: `need_counts` makes that an error instead)."""
    yt, yp = _label_matrices(y_true, y_pred)
    return _segment_f1(get_kernels(), yt.reshape(-1, yt.shape[-1]), yp.reshape(-1, yp.shape[-1]), num_classes, overlaps,
                       ignore_value, False, need_counts)[0]


def _to_host(res, packed):
    """(f1 (n_seq, K) float64, valid (n_seq,)) as numpy arrays: one copy of the packed buffer on the workgroup route."""
    if packed is not None:
        f1, _, _, _, valid = unpack_segment_f1(packed.cpu(), *res.f1.shape)
        return f1.numpy(), valid.numpy()
    return res.f1.cpu().numpy(), res.valid.cpu().numpy()


def _entity_minor(target, output):
    """int64 (N, T, E) labels of one index on the output's device; (N, T) becomes (N, T, 1)."""
    target, output = _label_matrices(target, output)
    if target.ndim == 2:
        target, output = target.unsqueeze(-1), output.unsqueeze(-1)
    if target.ndim != 3 or target.shape != output.shape:
        raise ValueError(f'labels (N, T) or (N, T, E) of equal shape expected, not {tuple(target.shape)} and {tuple(output.shape)}')
    return target, output


def evaluate_f1_at_k_multi(targets: dict, outputs: dict, num_subactivities, num_affordances, overlaps=(0.10, 0.25, 0.50)):
    """The `evaluate_f1_at_k` calls of `predict_all` (predict.py:358-360, :425-426), one per overlap, from one launch and
    one copy per index: {index: labels (N, T) or (N, T, E)} -> {overlap: {index: F1@overlap}}. The labels are read in
    place (no transposition); the mean adds the per-sequence fp64 values in sequence order, like metrics.py:70-81."""
    K = get_kernels()
    results = {overlap: {} for overlap in overlaps}
    for index, target in sorted(targets.items()):
        target, output = _entity_minor(target, outputs[index])
        num_classes = num_affordances if 'affordance' in str(index) else num_subactivities
        f1, valid = _to_host(*_segment_f1(K, target, output, num_classes, overlaps, -1, True))
        n_valid = float(valid.sum())
        for j, overlap in enumerate(overlaps):
            total = 0.0
            for v in f1[valid != 0, j]:
                total += float(v)
            results[overlap][index] = total / n_valid if n_valid else float('nan')   # the reference divides by zero there
    return results


def f1_scores_per_example(outputs: dict, targets: dict, test_ids, num_subactivities, num_affordances, overlap: float,
                          file=None) -> str:
    """The text `dump_f1_scores_per_example` (predict.py:456-472) writes: per problem type, in the order of `outputs`, one
    line f'{problem_type}_{test_id}_{ent_id}: {f1:.4f}' for every entity of every clip that has a target step, then a blank
    line. {problem_type: labels (N, T, E)}; one launch and one copy per problem type. Returns the text and writes it to
    `file` (a path or an object with write) when one is given."""
    K = get_kernels()
    lines = []
    for problem_type in outputs:
        target, output = _entity_minor(targets[problem_type], outputs[problem_type])
        num_classes = num_subactivities if 'sub-activity' in str(problem_type) else num_affordances
        f1, valid = _to_host(*_segment_f1(K, target, output, num_classes, [overlap], -1, True))
        E = target.shape[2]
        for n, test_id in zip(range(target.shape[0]), test_ids):
            lines += [f'{problem_type}_{test_id}_{e}: {f1[n * E + e, 0]:.4f}\n' for e in range(E) if valid[n * E + e]]
        lines.append('\n')
    text = ''.join(lines)
    if file is not None:
        if hasattr(file, 'write'):
            file.write(text)
        else:
            with open(file, mode='w') as f:
                f.write(text)
    return text


# --------------------------------------------------------------------------------------------------------------------
# segmental edit score per example (twog_segment_edit)
SegmentEdit = namedtuple('SegmentEdit', 'score distance n_true n_pred valid')
SegmentEdit.__doc__ = """score float64 (n_seq,); distance, n_true, n_pred int32 (n_seq,): the Levenshtein distance between the
true and the predicted list of segment labels and their lengths; valid int32 (n_seq,), 0 for a sequence without a kept
step or with both lists empty (its other entries are zero)."""


def _sequential_mean(values, valid) -> float:
    """The values of the valid sequences added in sequence order in fp64, over their number; NaN when there is none."""
    total = 0.0
    for v in values[valid != 0]:
        total += float(v)
    n_valid = float(valid.sum())
    return total / n_valid if n_valid else float('nan')


def edit_score_per_example(y_true, y_pred, ignore_value: float = None, *, bg_label=None) -> SegmentEdit:
    """The segmental edit score of every sequence of (n_seq, n_steps) label matrices, in one launch, as a SegmentEdit of
    device tensors. Steps whose target is `ignore_value` are dropped from both sequences, both are run-length encoded
    into lists of segment labels, with `bg_label` the segments of that label are removed from both lists (the neighbours
    this brings together are NOT merged: A bg A is [A, A]), and score = 100 * (1 - Levenshtein distance / length of the
    longer list) with unit insertion, deletion and substitution costs. Raises RuntimeError above the kernel's step limit
    (`get_kernels().segment_edit_limits()`): there is no second route."""
    yt, yp = _label_matrices(y_true, y_pred)
    res = get_kernels().segment_edit(yt.reshape(-1, yt.shape[-1]), yp.reshape(-1, yp.shape[-1]), ignore_value, bg_label)
    return SegmentEdit(*res[:5])


def edit_score(y_true, y_pred, *, ignore_value: float = None, bg_label=None) -> float:
    """The mean of `edit_score_per_example` over the valid sequences, added on the host in sequence order in fp64 after
    one copy; NaN when no sequence is valid."""
    yt, yp = _label_matrices(y_true, y_pred)
    n_seq = yt.numel() // yt.shape[-1] if yt.shape[-1] else 0
    packed = get_kernels().segment_edit(yt.reshape(-1, yt.shape[-1]), yp.reshape(-1, yp.shape[-1]), ignore_value, bg_label)[5]
    score, _, _, _, valid = unpack_segment_edit(packed.cpu(), n_seq)
    return _sequential_mean(score.numpy(), valid.numpy())


def evaluate_edit_score(targets: dict, outputs: dict, bg_label=None) -> dict:
    """{index: labels (N, T) or (N, T, E)} -> {index: mean segmental edit score}, for the dictionaries
    `evaluate_f1_at_k_multi` takes: -1 targets ignored, the labels read in place (no transposition), one launch and one
    copy per index."""
    K = get_kernels()
    results = {}
    for index, target in sorted(targets.items()):
        target, output = _entity_minor(target, outputs[index])
        packed = K.segment_edit(target, output, -1, bg_label, entity_minor=True)[5]
        score, _, _, _, valid = unpack_segment_edit(packed.cpu(), target.shape[0] * target.shape[2])
        results[index] = _sequential_mean(score.numpy(), valid.numpy())
    return results


# --------------------------------------------------------------------------------------------------------------------
# metrics from confusion counts (host, fp64 numpy): counts[t, p] = positions of true class t predicted as class p
def _ratio(num, den):
    """num / den with scikit-learn's zero_division: a zero denominator gives 0."""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    return np.divide(num, den, out=np.zeros(np.broadcast(num, den).shape), where=den != 0)


def _class_sums(counts, labels=None):
    """(tp, predicted, true) per class; for `labels` beyond the matrix the three are 0."""
    counts = np.asarray(counts, dtype=np.int64)
    tp, pred, true = np.diag(counts), counts.sum(0), counts.sum(1)
    if labels is None:
        return tp, pred, true
    out = np.zeros((3, len(labels)), dtype=np.int64)
    inside = [i for i, c in enumerate(labels) if c < counts.shape[0]]
    for row, src in zip(out, (tp, pred, true)):
        row[inside] = src[[labels[i] for i in inside]]
    return out[0], out[1], out[2]


def _prf(tp, pred, true):
    return _ratio(tp, pred), _ratio(tp, true), _ratio(2 * tp, pred + true)  # F1 = 2 tp / (2 tp + fp + fn)


def precision_recall_f1(counts, average: str) -> dict:
    """scikit-learn's ``precision_recall_fscore_support(y_true, y_pred, average=average)`` (predict.py:224, labels=None)
    from a count matrix. 'micro' is over all counted positions; 'macro' is the plain mean over the classes PRESENT in
    the targets or the predictions, not over range(C). With nothing counted micro is 0.0 and macro is NaN: that is what
    scikit-learn 1.7.2 returns (the mean of no classes), other versions may differ; golden G15 pins it."""
    tp, pred, true = _class_sums(counts)
    if average == 'micro':
        p, r, f = _prf(tp.sum(), pred.sum(), true.sum())
    elif average == 'macro':
        present = (pred + true) > 0
        p, r, f = (v[present].mean() if present.any() else float('nan') for v in _prf(tp, pred, true))
    else:
        raise ValueError(f'average must be micro or macro, not {average!r}')
    return {'precision': float(p), 'recall': float(r), 'f1': float(f)}


def classification_report(counts, target_names, digits: int = 4, output_dict: bool = False):
    """scikit-learn's ``classification_report(y_true, y_pred, labels=range(len(target_names)), target_names=...)``
    (predict.py:220-222) from a count matrix, which may hold more classes than there are names. One row per name, then
    'accuracy' when the names cover every class present in the targets or predictions ('micro avg' otherwise), 'macro avg'
    (plain mean over the named classes) and 'weighted avg' (weights = support; plain mean when every support is 0)."""
    names = [str(n) for n in target_names]
    labels = list(range(len(names)))
    tp, pred, true = _class_sums(counts, labels)
    p, r, f = _prf(tp, pred, true)
    rows = {n: {'precision': float(p[i]), 'recall': float(r[i]), 'f1-score': float(f[i]), 'support': int(true[i])}
            for i, n in enumerate(names)}
    all_tp, all_pred, all_true = _class_sums(counts)
    covered = not ((all_pred + all_true)[len(labels):] > 0).any()
    support = int(true.sum())
    mp, mr, mf = _prf(tp.sum(), pred.sum(), true.sum())
    if covered:
        rows['accuracy'] = float(mf)
    else:
        rows['micro avg'] = {'precision': float(mp), 'recall': float(mr), 'f1-score': float(mf), 'support': support}
    mean = lambda v, w=None: float(np.average(v, weights=w)) if len(v) else float('nan')
    rows['macro avg'] = {'precision': mean(p), 'recall': mean(r), 'f1-score': mean(f), 'support': support}
    w = true if support > 0 else None
    rows['weighted avg'] = {'precision': mean(p, w), 'recall': mean(r, w), 'f1-score': mean(f, w), 'support': support}
    if output_dict:
        return rows
    width = max([len(n) for n in names] + [len('weighted avg')])
    head = ' ' * width + ''.join(f'{h:>{digits + 6}}' for h in ('precision', 'recall', 'f1-score', 'support'))
    lines = [head, '']
    fmt = lambda name, v: (f'{name:>{width}}' + ''.join(f'{v[k]:>{digits + 6}.{digits}f}' for k in ('precision', 'recall', 'f1-score'))
                           + f'{v["support"]:>{digits + 6}d}')
    lines += [fmt(n, rows[n]) for n in names] + ['']
    if covered:
        lines.append(f'{"accuracy":>{width}}' + ' ' * (2 * (digits + 6)) + f'{rows["accuracy"]:>{digits + 6}.{digits}f}'
                     + f'{support:>{digits + 6}d}')
    else:
        lines.append(fmt('micro avg', rows['micro avg']))
    lines += [fmt('macro avg', rows['macro avg']), fmt('weighted avg', rows['weighted avg']), '']
    return '\n'.join(lines)


def _check_flags(name, flags):
    bad_target, bad_step = int(flags[0]), int(flags[1])
    if bad_target:
        raise ValueError(f'output {name!r}: {bad_target} evaluated positions have a label outside [-1, num_classes)')
    if bad_step:
        raise ValueError(f'output {name!r}: {bad_step} evaluated positions have a step_index entry beyond the last target step')


def evaluate_predictions(targets: dict, outputs: dict, print_report: bool = True, subactivity_names=None,
                         affordance_names=None) -> dict:
    """predict.py:205-226: {index: labels (N, T) or (N, T, E)} (device tensors, as `process_output` returns them; -1
    targets ignored) -> {f'{index}-micro': {'precision', 'recall', 'f1'}, f'{index}-macro': ...}. The confusion counts
    come from twog_confusion_counts, the numbers from `precision_recall_f1`; with `print_report` the per-class table of
    `classification_report` is printed under the reference's headings."""
    K = get_kernels()
    results = {}
    for index, target in sorted(targets.items()):
        output = torch.as_tensor(outputs[index])
        target = torch.as_tensor(target).to(output.device)
        names = affordance_names if 'affordance' in str(index) else subactivity_names
        # the class count is the largest label seen (labels=None in predict.py:224), at least the number of names
        n_classes = max(int(max(target.max(), output.max())) + 1 if target.numel() else 1, len(names) if names else 1)
        state = K.zeros(n_classes * n_classes + 2, dtype=torch.int64, device=output.device)
        counts, flags = state[:-2].view(n_classes, n_classes), state[-2:]
        K.confusion_counts(target.reshape(-1), output.reshape(-1), n_classes, counts, flags)
        state = state.cpu().numpy()
        _check_flags(index, state[-2:])
        counts = state[:-2].reshape(n_classes, n_classes)
        if print_report:
            problem_type = 'Recognition' if 'recognition' in str(index) else 'Prediction'
            problem_class = 'Affordance' if 'affordance' in str(index) else 'Sub-activity'
            print(f'{problem_class} {problem_type}')
            print(classification_report(counts, names if names else range(n_classes), digits=4))
        for average in ('micro', 'macro'):
            results[f'{index}-{average}'] = precision_recall_f1(counts, average)
    return results


# --------------------------------------------------------------------------------------------------------------------
# which target steps are evaluated: step_index (N, S) int32, -1 = padding
def half_rate_step_index(T_tgt: int, is_15fps, device=None) -> torch.Tensor:
    """`downsample_bad_bimanual_videos` (predict.py:136-156) as a step index (N, T_tgt): clips flagged in `is_15fps`
    evaluate steps 1, 3, 5, ... (T_tgt // 2 of them) and pad the rest with -1; the other clips evaluate 0 .. T_tgt - 1."""
    flagged = np.asarray(is_15fps, dtype=bool).reshape(-1)
    index = np.tile(np.arange(T_tgt, dtype=np.int32), (flagged.size, 1))
    half = np.full(T_tgt, -1, dtype=np.int32)
    half[:T_tgt // 2] = np.arange(1, T_tgt, 2, dtype=np.int32)
    index[flagged] = half
    return torch.from_numpy(index).to(device) if device is not None else torch.from_numpy(index)


def segment_step_index(segment_starts, device=None) -> torch.Tensor:
    """`summarize_frames_into_segments` (predict.py:159-183) as a step index (N, longest list): clip v evaluates the
    first frame of each of its segments, `segment_starts[v]`, and pads with -1."""
    width = max((len(s) for s in segment_starts), default=0)
    index = np.full((len(segment_starts), width), -1, dtype=np.int32)
    for row, starts in zip(index, segment_starts):
        row[:len(starts)] = np.asarray(starts, dtype=np.int32)
    return torch.from_numpy(index).to(device) if device is not None else torch.from_numpy(index)


def _select_steps(labels: torch.Tensor, index: torch.Tensor, pad: int) -> torch.Tensor:
    """labels (N, T) or (N, T, E) -> labels[v, index[v, s]] with `pad` where index < 0."""
    index = index.to(labels.device).long()
    idx = index.clamp(min=0)
    keep = index >= 0
    if labels.ndim == 3:
        idx, keep = idx.unsqueeze(-1).expand(-1, -1, labels.shape[2]), keep.unsqueeze(-1)
    return torch.where(keep, torch.gather(labels, 1, idx), torch.full_like(labels[:1, :1], pad))


def downsample_bad_bimanual_videos(outputs: dict, targets: dict, is_15fps):
    """predict.py:136-156 on the LABELS of `process_output` ({index: (N, T) or (N, T, E)}): the clips flagged in
    `is_15fps` keep every second step from step 1; the freed tail is padded with prediction 0 (the argmax of the
    reference's -100 rows) and target -1. Returns (outputs, targets) as new dicts."""
    new_out, new_tgt = {}, {}
    for index, target in targets.items():
        step_index = half_rate_step_index(target.shape[1], is_15fps)
        new_out[index] = _select_steps(outputs[index], step_index, 0)
        new_tgt[index] = _select_steps(target, step_index, -1)
    return new_out, new_tgt


def summarize_frames_into_segments(labels: dict, segment_starts, is_ground_truth: bool) -> dict:
    """predict.py:159-183 on the LABELS of `process_output`: clip v keeps the first frame of each of its segments,
    padded to the longest list with -1 for targets and with 0 for predictions (the argmax of the reference's -1.0
    rows)."""
    step_index = segment_step_index(segment_starts)
    return {index: _select_steps(t, step_index, -1 if is_ground_truth else 0) for index, t in labels.items()}


class EvaluationAccumulator:
    """Running evaluation of a test set on the device: per output name the C x C confusion counts (row = true class,
    column = predicted class), the two error counters of twog_eval_update and, per overlap, the sums of the per-sequence
    F1@k and of the valid sequences. `update` issues kernels only -- no device-to-host copy, no synchronisation --
    `all_reduce` sums the state over the ranks of a sharded test set and `result` makes the one copy to the host.

    names: the evaluated outputs in model order (the last `len(names)` outputs and targets of a batch are used, like
    predict.py:61-63). num_classes: one int for all of them, or one per name. f1_route: 'thread' runs twog_f1_at_k once per
    overlap on transposed copies of the labels (fp32 per-sequence values); 'workgroup' runs twog_segment_f1 once for all
    overlaps on the labels as eval_update wrote them and twog_segment_f1_accumulate (fp64 throughout), and falls back to
    'thread' for a batch it cannot take (an overlap <= 0, more steps than its limit). `last_f1_route` names what the last
    update ran. edit: also keep, per name, the sum of the per-sequence segmental edit scores (twog_segment_edit on the same
    labels, `bg_label` as in `edit_score_per_example`) and of its valid sequences; `result()[name]['edit']` is their
    ratio. That metric has one route: a batch with more steps than `segment_edit_limits()` is a ValueError.
    decoder: a `ViterbiDecoder` or `SegmentalDecoder` for every name, or a list with one (or None) per name. A name with a
    decoder is evaluated on the decoded labels instead of the per-step argmax: its decode kernel (twog_viterbi_decode or
    twog_segdecode), `_select_steps`, twog_confusion_counts, and
    the F1 and edit kernels on those labels; `update(..., lengths=)` passes the valid model steps of the clips to it. A
    step_index entry beyond the last target step is counted in the second error counter and evaluated as padding, as
    twog_eval_update does. Without a decoder nothing changes."""

    def __init__(self, names, num_classes, downsampling: int = 1, overlaps=(0.1, 0.25, 0.5), f1_route: str = 'thread',
                 edit: bool = False, bg_label=None, decoder=None):
        if f1_route not in ('thread', 'workgroup'):
            raise ValueError(f"f1_route must be 'thread' or 'workgroup', not {f1_route!r}")
        self.f1_route = f1_route
        self.last_f1_route = None
        self.names = list(names)
        self.num_classes = [int(num_classes)] * len(self.names) if np.ndim(num_classes) == 0 else [int(c) for c in num_classes]
        if len(self.num_classes) != len(self.names):
            raise ValueError('num_classes must be one int or one per name')
        self.downsampling = max(1, int(downsampling))
        self.overlaps = tuple(float(o) for o in overlaps)
        self.edit = bool(edit)
        self.bg_label = bg_label
        self.decoders = list(decoder) if isinstance(decoder, (list, tuple)) else [decoder] * len(self.names)
        if len(self.decoders) != len(self.names):
            raise ValueError('decoder must be one decoder or one (or None) per name')
        for name, dec, c in zip(self.names, self.decoders, self.num_classes):
            if dec is not None and dec.num_classes != c:
                raise ValueError(f'output {name!r} has {c} classes, its transition model {dec.num_classes}')
        # 8-byte words: per name [C * C counts, 2 flags] as int64, then per name [f1 sums, valid sums] as fp64, then with
        # `edit` per name [edit sum, valid sum] as fp64
        self._state = None

    def _allocate(self, device):
        n_int = sum(c * c + 2 for c in self.num_classes)
        n_ov = len(self.overlaps)
        n_f1 = 2 * n_ov * len(self.names)
        n_edit = 2 * len(self.names) if self.edit else 0
        self._state = get_kernels().zeros(n_int + n_f1 + n_edit, dtype=torch.int64, device=device)
        self._ints = self._state[:n_int]
        self._floats = self._state[n_int:].view(torch.float64)
        self._counts, self._flags, self._f1, self._valid = [], [], [], []
        at = 0
        for i, c in enumerate(self.num_classes):
            self._counts.append(self._ints[at:at + c * c].view(c, c))
            self._flags.append(self._ints[at + c * c:at + c * c + 2])
            at += c * c + 2
            self._f1.append(self._floats[2 * n_ov * i:2 * n_ov * i + n_ov])
            self._valid.append(self._floats[2 * n_ov * i + n_ov:2 * n_ov * (i + 1)])
        if self.edit:
            self._edit = [self._floats[n_f1 + 2 * i:n_f1 + 2 * i + 1] for i in range(len(self.names))]
            self._edit_valid = [self._floats[n_f1 + 2 * i + 1:n_f1 + 2 * i + 2] for i in range(len(self.names))]

    def update(self, outputs, targets, step_index=None, lengths=None):
        """One batch: outputs / targets are the model's lists (the last len(names) are used), output (bs, C, T, E)
        log-probabilities, target (bs, T_tgt, E) labels on the same device; step_index (bs, S) from
        `half_rate_step_index` / `segment_step_index`, already on the device (a host tensor would be copied, which
        synchronises). lengths: int64 (bs,) on the device, the valid model steps of every clip, for the names that have
        a decoder (the argmax has no use for it)."""
        K = get_kernels()
        n = len(self.names)
        outputs, targets = list(outputs)[-n:], list(targets)[-n:]
        if len(outputs) != n or len(targets) != n:
            raise ValueError(f'{n} outputs and targets expected')
        if self.edit:   # before anything is added to the state
            max_steps = K.segment_edit_limits()
            for name, tgt in zip(self.names, targets):
                steps = step_index.shape[1] if step_index is not None else tgt.shape[1]
                if steps > max_steps:
                    raise ValueError(f'output {name!r}: the edit score takes up to {max_steps} steps per batch, not {steps}')
        for i, (out, tgt) in enumerate(zip(outputs, targets)):
            if out.ndim != 4:
                raise RuntimeError(f'Number of dimensions for output is {out.ndim}')  # predict.py:66-67
            if out.shape[1] != self.num_classes[i]:
                raise ValueError(f'output {self.names[i]!r} has {out.shape[1]} classes, not {self.num_classes[i]}')
            if self._state is None:
                self._allocate(out.device)
            if step_index is not None:
                step_index = step_index.to(device=out.device, dtype=torch.int32)
            if self.decoders[i] is None:
                labels, kept = K.eval_update(out, self.downsampling, tgt.to(torch.int64), step_index, self._counts[i],
                                             self._flags[i], want_labels=True)
            else:
                labels, kept = self._decoded(K, i, out, tgt.to(torch.int64), step_index, lengths)
            if self.edit:
                score, _, _, _, edit_valid, _ = K.segment_edit(kept, labels, -1, self.bg_label, entity_minor=True)
                K.segment_f1_accumulate(score.view(-1, 1), edit_valid, self._edit[i], self._edit_valid[i])
            if self.f1_route == 'workgroup' and self.overlaps and self._update_f1_workgroup(K, i, kept, labels):
                continue
            self.last_f1_route = 'thread'
            # f1_at_k wants sequence-major (n_seq, n_steps): the transposition of evaluate_f1_at_k
            steps = labels.shape[1]
            labels, kept = labels.transpose(1, 2).reshape(-1, steps), kept.transpose(1, 2).reshape(-1, steps)
            for j, overlap in enumerate(self.overlaps):
                f1, valid = K.f1_at_k(kept, labels, self.num_classes[i], overlap, -1)
                self._f1[i][j:j + 1].add_(f1.sum(dtype=torch.float64))
                self._valid[i][j:j + 1].add_(valid.sum(dtype=torch.float64))

    def _decoded(self, K, i, out, tgt, step_index, lengths):
        """What eval_update does for name i, on the decoder's labels: (labels, targets) int64 (bs, S or T_tgt, E) of the
        evaluated positions, their pairs added to the counts. Kernels and torch device operations only."""
        T_tgt = tgt.shape[1]
        labels = self.decoders[i].decode(out, self.downsampling, T_tgt, lengths)
        kept = tgt
        if step_index is not None:
            beyond = step_index >= T_tgt          # counted, then evaluated as padding: never read
            self._flags[i][1:2].add_(beyond.sum() * tgt.shape[2])
            index = step_index.masked_fill(beyond, -1)
            labels, kept = _select_steps(labels, index, 0), _select_steps(tgt, index, -1)
        labels, kept = labels.contiguous(), kept.contiguous()
        K.confusion_counts(kept.reshape(-1), labels.reshape(-1), self.num_classes[i], self._counts[i], self._flags[i])
        return labels, kept

    def _update_f1_workgroup(self, K, i, kept, labels) -> bool:
        """One twog_segment_f1 per max_overlaps overlaps on the entity-minor labels, one accumulate each; False (nothing
        issued) when the batch needs the per-thread kernel."""
        max_steps, max_overlaps = K.segment_f1_limits()
        if not _positive(self.overlaps) or labels.shape[1] > max_steps:
            return False
        for j in range(0, len(self.overlaps), max_overlaps):
            f1, _, _, _, valid, _ = K.segment_f1(kept, labels, self.num_classes[i], self.overlaps[j:j + max_overlaps], -1,
                                                 entity_minor=True)
            K.segment_f1_accumulate(f1, valid, self._f1[i][j:j + max_overlaps], self._valid[i][j:j + max_overlaps])
        self.last_f1_route = 'workgroup'
        return True

    def all_reduce(self, group=None):
        """Sum the state over the ranks of `group` (every rank evaluated its own shard of the clips). A process without
        an initialised process group is the only rank: nothing to do."""
        if self._state is None:
            raise RuntimeError('all_reduce before the first update: the state has no device yet')
        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(self._ints, op=dist.ReduceOp.SUM, group=group)
            dist.all_reduce(self._floats, op=dist.ReduceOp.SUM, group=group)

    def result(self) -> dict:
        """{name: {'micro': {...}, 'macro': {...}, 'report': {...}, 'f1@k': {overlap: value}, 'confusion': ndarray}}.
        Raises ValueError if a target was outside [-1, C) or a step_index entry pointed beyond the targets. F1@k is
        NaN when no sequence had a counted step (the reference divides by zero there). With `edit` every name has
        'edit' too: the mean segmental edit score, NaN when no sequence was valid."""
        if self._state is None:
            raise RuntimeError('result before the first update')
        host = self._state.cpu().numpy()   # the one device-to-host copy
        n_int = self._ints.numel()
        ints, floats = host[:n_int], host[n_int:].view(np.float64)
        n_ov = len(self.overlaps)
        res, at = {}, 0
        for i, (name, c) in enumerate(zip(self.names, self.num_classes)):
            counts = ints[at:at + c * c].reshape(c, c).copy()
            _check_flags(name, ints[at + c * c:at + c * c + 2])
            at += c * c + 2
            f1, valid = floats[2 * n_ov * i:2 * n_ov * i + n_ov], floats[2 * n_ov * i + n_ov:2 * n_ov * (i + 1)]
            res[name] = {'micro': precision_recall_f1(counts, 'micro'), 'macro': precision_recall_f1(counts, 'macro'),
                         'report': classification_report(counts, range(c), output_dict=True),
                         'f1@k': {ov: (float(f1[j] / valid[j]) if valid[j] > 0 else float('nan'))
                                  for j, ov in enumerate(self.overlaps)},
                         'confusion': counts}
            if self.edit:
                total, n_valid = floats[2 * n_ov * len(self.names) + 2 * i:2 * n_ov * len(self.names) + 2 * i + 2]
                res[name]['edit'] = float(total / n_valid) if n_valid > 0 else float('nan')
        return res
