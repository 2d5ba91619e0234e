"""Multi-task criterion of the 2G-GCN training step on the HIP library.

Mirror of the reference's loss interface -- `vhoi/losses.py:8-70` (`select_loss`) and `pyrutils/torch/losses.py:7-51`
(`multi_task_loss`, `binary_cross_entropy_loss`, `budget_loss`) -- with the same names, argument meaning and return
values (a list of weighted scalar losses, one per output of the model), so `train.py` keeps calling
`criterion(output, target)` / `sum(losses).backward()`. All terms run in ONE forward and ONE backward kernel launch
(`twog_multitask_loss_fwd/bwd`), with no host synchronisation (the reference calls `mask.sum().item()` per term).
Terms whose weight is 0 (stage-1: budget, BCE and the frame-level NLL terms) get no backward work at all.

Beyond the reference: the temporal smoothing loss (`temporal_smoothing_loss`, `multi_task_loss(..., smoothing=...)`,
`misc.smoothing_loss` of `select_loss`), MS-TCN's truncated MSE between the log-probabilities of adjacent steps -- the
training-side companion of the segmental metrics. Its terms follow the reference's in the same loss tensor, written by
ONE more launch per direction (`twog_smooth_loss_fwd/bwd`; definition in include/twog_gcn.h); off by default.

Against label imbalance: per-class weights on the NLL terms (`nll_loss(weight=)`, `multi_task_loss(class_weights=)`,
`misc.class_weights`) and the reference's `positive_class_weight` of the BCE terms (`multi_task_loss(positive_class_weights=)`,
`misc.segmentation_loss.positive_class_weight`). A call in which any term carries one runs ALL its terms through
`twog_weighted_loss_fwd/bwd` (twog_wloss_t in include/twog_gcn.h), still one launch per direction; a call without them makes
the launches it always made. `class_counts` (on the device) and `class_weights` ('balanced', 'effective') give the weights.

For sequence decoding: the linear-chain CRF loss (`LinearChainCRF`, `crf_loss`, `multi_task_loss(..., crf=...)`,
`misc.crf_loss` of `select_loss`), the sequence negative log-likelihood under learned transition scores, which trains the
emissions and the (C, C) scores jointly; the scores then go to `postprocess.ViterbiDecoder` (`module.decoder()`). Its terms
follow the smoothing terms in the same loss tensor, one launch pair per term and direction (`twog_crf_nll_fwd/bwd`;
definition in include/twog_gcn.h and at `crf_loss`); off by default. A `SemiMarkovCRF` module takes the place of a
`LinearChainCRF` wherever one is accepted: the loss over whole segments with learned duration scores (`semi_crf_loss`,
`twog_semicrf_nll_fwd/bwd`), whose three tables go to `postprocess.SegmentalDecoder` (`module.decoder()`).
"""
from collections import namedtuple
from functools import partial

import torch
import torch.nn.functional as F

from .kernels import get_kernels

_NLL, _BCE, _BUDGET = 0, 1, 2   # twog_loss_t::kind


def _misc(cfg):
    """cfg's `misc` section: an OmegaConf-style `.get('misc', default_value={})` or a plain dict."""
    try:
        return cfg.get('misc', default_value={})
    except TypeError:  # plain dict
        return cfg.get('misc', {})


def nll_loss(input, target, ignore_index=-1, reduction='mean', *, weight=None):
    """F.nll_loss(input, target, weight, ignore_index=ignore_index, reduction='mean') on the HIP path. weight: per-class
    weights, a [C] tensor or a sequence of floats: the weighted mean sum(w[y] * -x[y]) / sum(w[y]) over the kept targets."""
    return _run([input], [target], [_NLL], [1.0], ignore_index, reduction, class_weights=[weight])[0]


def binary_cross_entropy_loss(input, target, positive_class_weight=1, ignore_value=-1, reduction='mean'):
    """pyrutils/torch/losses.py:7-21. positive_class_weight p > 1 weighs the elements whose target is exactly 1.0 by p
    (the reference raises their input to the power p; here p * log x, see twog_wloss_t in include/twog_gcn.h); p <= 1
    changes nothing, as in the reference."""
    return _run([input], [target], [_BCE], [1.0], ignore_value, reduction,
                positive_class_weights=[positive_class_weight])[0]


def budget_loss(input, target, ignore_value=-1, reduction='mean'):
    """pyrutils/torch/losses.py:24-36."""
    return _run([input], [target], [_BUDGET], [1.0], ignore_value, 'mean')[0]


def temporal_smoothing_loss(input, target, tau=4.0, ignore_index=-1):
    """Truncated MSE between the log-probabilities of adjacent steps (T-MSE of MS-TCN): input (bs, C, T, E) log-probabilities,
    target (bs, T, E) labels; the mean over the pairs of adjacent kept steps and the classes of min((x_t - x_{t-1})^2, tau^2)
    with x_{t-1} held constant; 0 when no pair is kept. (The input rides on an NLL term of weight 0, whose value is dropped
    and which gets no backward work.)"""
    return _run([input], [target], [_NLL], [0.0], ignore_index, 'mean', [(0, 1.0, tau)])[1]


class LinearChainCRF(torch.nn.Module):
    """The parameters of a linear-chain CRF over `num_classes` labels: `transitions` A fp32 (C, C), row = from, column = to
    (the convention of `postprocess.viterbi_labels`), and `initial` pi fp32 (C,), both zero-initialised -- with zeros and
    normalised emissions the CRF loss is the per-sequence NLL. Trained beside the model: `DataParallel(model,
    extra_modules=[crf])` + `FusedAdam`, as `MultiTaskLossLearner` is. The state_dict is the two tensors."""

    def __init__(self, num_classes: int):
        super().__init__()
        self.num_classes = int(num_classes)
        if self.num_classes < 1:
            raise ValueError(f'num_classes must be positive, got {num_classes}')
        self.transitions = torch.nn.Parameter(torch.zeros(self.num_classes, self.num_classes, dtype=torch.float32))
        self.initial = torch.nn.Parameter(torch.zeros(self.num_classes, dtype=torch.float32))

    @classmethod
    def from_counts(cls, counts, smoothing: float = 1.0, initial_counts=None):
        """Start from label statistics: transitions = `postprocess.transition_log_probs(counts, smoothing)` of (C, C)
        transition counts (`postprocess.transition_counts`); initial = log((n + s) / (sum + C s)) of (C,) first-label counts,
        zeros without them. The smoothing must be positive: -inf scores are out of the loss's contract."""
        from .postprocess import transition_log_probs
        import numpy as np
        if not smoothing > 0:
            raise ValueError(f'smoothing must be positive (a -inf score is out of contract for training), got {smoothing}')
        A = transition_log_probs(counts, smoothing)
        crf = cls(A.shape[0])
        with torch.no_grad():
            crf.transitions.copy_(A)
            if initial_counts is not None:
                n = np.asarray(initial_counts.cpu() if torch.is_tensor(initial_counts) else initial_counts).astype(np.float64)
                if n.shape != (crf.num_classes,):
                    raise ValueError(f'initial counts must be ({crf.num_classes},), not {n.shape}')
                s = float(smoothing)
                crf.initial.copy_(torch.from_numpy(np.log((n + s) / (n.sum() + n.size * s)).astype(np.float32)))
        return crf

    def decoder(self):
        """A `postprocess.ViterbiDecoder` over detached copies of the current parameters (for `process_output(decoder=)` /
        `EvaluationAccumulator(decoder=)`); later training steps do not change it."""
        from .postprocess import ViterbiDecoder
        return ViterbiDecoder(self.transitions.detach().clone(), self.initial.detach().clone())

    def extra_repr(self):
        return f'num_classes={self.num_classes}'


def crf_loss(input, target, crf, ignore_index=-1):
    """The linear-chain CRF loss of (bs, C, T, E) fp32 log-probabilities `input` (the model's outputs at the model's rate, as
    the NLL terms get them) and int64 (bs, T, E) `target` under the LinearChainCRF `crf`: transitions A fp32 (C, C), row =
    from, column = to, and initial pi fp32 (C,). Finite A and pi are in contract; +-inf and NaN are not.

    A sequence is (clip b, entity e). Its kept steps t_0 < t_1 < ... < t_{K-1} are those with 0 <= target[b, t, e] < C and
    target != ignore_index (the NLL terms' rule); every other step is removed from the chain -- padding, an absent entity and a
    hole in the middle are the same case -- and transitions link consecutive kept steps. K = 0 contributes nothing. With
    x_k[c] = input[b, c, t_k, e] and y_k = target[b, t_k, e]:

        alpha_0[c] = pi[c] + x_0[c]
        alpha_k[c] = x_k[c] + logsumexp_{c'} (alpha_{k-1}[c'] + A[c', c])          k = 1 .. K-1
        logZ       = logsumexp_c alpha_{K-1}[c]
        gold       = pi[y_0] + x_0[y_0] + sum_{k>=1} (A[y_{k-1}, y_k] + x_k[y_k])
        nll_seq    = logZ - gold                                                    (>= 0)
        loss       = (sum over sequences of nll_seq) / (sum over sequences of K)

    The loss is 0 when no step is kept. The count of the term (what a data-parallel count reducer receives) is the total
    number of kept steps: the term is on the scale of the per-step NLL terms. Gradients, with g = dloss / count:

        beta_{K-1}[c] = 0
        beta_k[c']    = logsumexp_c (A[c', c] + x_{k+1}[c] + beta_{k+1}[c])
        gamma_k[c]    = exp(alpha_k[c] + beta_k[c] - logZ)
        xi_k[c', c]   = exp(alpha_{k-1}[c'] + A[c', c] + x_k[c] + beta_k[c] - logZ)
        d input[b, c, t_k, e] = g (gamma_k[c] - [c = y_k]), 0 at every removed step
        dA[c', c] = g sum_seq sum_{k>=1} (xi_k[c', c] - [y_{k-1} = c', y_k = c])       dpi[c] = g sum_seq (gamma_0[c] - [y_0 = c])

    The per-sequence recursions run in fp32, in the log domain with the maximum subtracted; the sums over sequences are carried
    in fp64 in index order and rounded once; no floating-point atomics, so two runs give the same bits. tests/crf_ref.py at
    fp64 is this definition in numpy. ValueError beyond `kernels.crf_limits()` (64 classes, 4096 steps), before any launch.
    (The input rides on an NLL term of weight 0, whose value is dropped and which gets no backward work.)"""
    return _run([input], [target], [_NLL], [0.0], ignore_index, 'mean', crf=[(0, 1.0, crf)])[1]


class SemiMarkovCRF(torch.nn.Module):
    """The parameters of a semi-Markov CRF over `num_classes` labels and segments of up to `max_duration` steps: `transitions`
    A fp32 (C, C) between consecutive segments, row = from, column = to (the diagonal is an entry like any other: a segment may
    be followed by one of its own class), `durations` dur fp32 (C, D) with dur[c, l-1] the score of a class-c segment of l
    steps, and `initial` pi fp32 (C,): the conventions of `postprocess.SegmentalDecoder`, to which `decoder()` hands them
    unchanged. All zero-initialised. Trained beside the model: `DataParallel(model, extra_modules=[scrf])` + `FusedAdam`, as
    `LinearChainCRF` is. The state_dict is the three tensors.

    -inf entries (a forbidden self-transition, an unseen duration) are in contract and get gradient exactly 0, so Adam leaves
    them where they are. Coupled (non-decoupled) weight decay does not: it adds decay * p to the gradient, and -inf then
    turns into NaN at the first step. Use AdamW (decoupled decay) or no decay for a module that holds -inf."""

    def __init__(self, num_classes: int, max_duration: int):
        super().__init__()
        self.num_classes, self.max_duration = int(num_classes), int(max_duration)
        if self.num_classes < 1 or self.max_duration < 1:
            raise ValueError(f'num_classes and max_duration must be positive, got {num_classes} and {max_duration}')
        C, D = self.num_classes, self.max_duration
        self.transitions = torch.nn.Parameter(torch.zeros(C, C, dtype=torch.float32))
        self.durations = torch.nn.Parameter(torch.zeros(C, D, dtype=torch.float32))
        self.initial = torch.nn.Parameter(torch.zeros(C, dtype=torch.float32))

    @classmethod
    def from_counts(cls, transition_counts, duration_counts, smoothing: float = 1.0, scheme: str = 'empirical',
                    self_transition=None, initial_counts=None):
        """Start from label statistics, exactly as a `SegmentalDecoder` is built from them: transitions =
        `postprocess.segment_transition_log_probs(transition_counts, smoothing, self_transition)` (self_transition None: a
        -inf diagonal, so max_duration must cover the longest labelled run), durations =
        `postprocess.duration_log_probs(duration_counts, smoothing, scheme)` (smoothing 0: -inf for unseen durations);
        initial = log((n + s) / (sum + C s)) of (C,) first-label counts, zeros without them."""
        from .postprocess import duration_log_probs, segment_transition_log_probs
        import numpy as np
        A = segment_transition_log_probs(transition_counts, smoothing, self_transition)
        dur = duration_log_probs(duration_counts, smoothing, scheme)
        if dur.shape[0] != A.shape[0]:
            raise ValueError(f'duration counts of {dur.shape[0]} classes for transition counts of {A.shape[0]}')
        scrf = cls(A.shape[0], dur.shape[1])
        with torch.no_grad():
            scrf.transitions.copy_(A)
            scrf.durations.copy_(dur)
            if initial_counts is not None:
                n = np.asarray(initial_counts.cpu() if torch.is_tensor(initial_counts) else initial_counts).astype(np.float64)
                if n.shape != (scrf.num_classes,):
                    raise ValueError(f'initial counts must be ({scrf.num_classes},), not {n.shape}')
                s = float(smoothing)
                with np.errstate(divide='ignore'):
                    scrf.initial.copy_(torch.from_numpy(np.log((n + s) / (n.sum() + n.size * s)).astype(np.float32)))
        return scrf

    def decoder(self):
        """A `postprocess.SegmentalDecoder` over detached copies of the current parameters (for `process_output(decoder=)` /
        `EvaluationAccumulator(decoder=)`); later training steps do not change it."""
        from .postprocess import SegmentalDecoder
        return SegmentalDecoder(self.transitions.detach().clone(), self.durations.detach().clone(),
                                self.initial.detach().clone())

    def extra_repr(self):
        return f'num_classes={self.num_classes}, max_duration={self.max_duration}'


def semi_crf_loss(input, target, scrf, ignore_index=-1):
    """The semi-Markov CRF loss of (bs, C, T, E) fp32 log-probabilities `input` and int64 (bs, T, E) `target` under the
    SemiMarkovCRF `scrf`: A fp32 (C, C), pi fp32 (C,), dur fp32 (C, D). It is the sum-product twin of the segmental decode.

    A sequence is (clip b, entity e); its kept steps t_0 < ... < t_{K-1} follow the NLL terms' rule exactly as for `crf_loss`:
    removed steps drop out of the chain, K = 0 contributes nothing. With x_k[c] = input[b, c, t_k, e], y_k = target[b, t_k, e]
    and S_c(s, l) = x_s[c] + ... + x_{s+l-1}[c]:

        e_0[c]   = pi[c]
        e_k[c]   = logsumexp_{c'} (d_{k-1}[c'] + A[c', c])                                   k >= 1
        d_k[c]   = logsumexp_{l = 1 .. min(D, k+1)} (e_{k-l+1}[c] + dur[c, l-1] + S_c(k-l+1, l))
        logZ     = logsumexp_c d_{K-1}[c]
        gold     = the score of the gold segmentation: the maximal runs of equal y over the kept steps; a run of n > D steps is
                   cut into pieces of D steps from its start with the remainder (1 .. D steps) last, consecutive pieces joined
                   by A[c, c]:  pi[c_1] + sum_j (dur[c_j, l_j - 1] + S_{c_j}(s_j, l_j)) + sum_{j >= 2} A[c_{j-1}, c_j]
        nll_seq  = logZ - gold                                                                (>= 0)
        loss     = (sum over sequences of nll_seq) / (sum over sequences of K)

    The loss is 0 when no step is kept, and the count of the term is the total number of kept steps, as for `crf_loss`.
    Gradients, with g = dloss / count:

        bd_{K-1}[c] = 0;   bd_k[c] = logsumexp_{c'} (A[c, c'] + be_{k+1}[c'])
        be_s[c]     = logsumexp_{l = 1 .. min(D, K-s)} (dur[c, l-1] + S_c(s, l) + bd_{s+l-1}[c])
        mu(s, l, c) = exp(e_s[c] + dur[c, l-1] + S_c(s, l) + bd_{s+l-1}[c] - logZ)           the segment marginal
        d input[b, c, t_k, e] = g (sum of mu over the segments of class c that cover k - [y_k = c]), 0 at every removed step
        ddur[c, l-1] = g sum_seq (sum_s mu(s, l, c) - #gold pieces of class c and length l)
        dA[c', c]    = g sum_seq (sum_{k>=1} exp(d_{k-1}[c'] + A[c', c] + be_k[c] - logZ) - #gold joins c' -> c)
        dpi[c]       = g sum_seq (exp(pi[c] + be_0[c] - logZ) - [c_1 = c])

    -inf is in contract in A, pi and dur: a logsumexp whose terms are all -inf is -inf, never NaN, and a -inf entry gets
    gradient exactly 0. Out of contract: +inf and NaN anywhere, and a sequence whose own gold score is -inf, such as a gold run
    longer than D under A[c, c] = -inf: choose D at least the longest labelled run, or keep the diagonal finite.

    The per-sequence recursions run in fp32, in the log domain with the maximum subtracted; the sums over sequences are carried
    in fp64 in index order and rounded once; no floating-point atomics, so two runs give the same bits. tests/semicrf_ref.py at
    fp64 is this definition in numpy. ValueError beyond `kernels.semicrf_limits()` (64 classes, 4096 steps, durations up to
    128), before any launch. (The input rides on an NLL term of weight 0, whose value is dropped and which gets no backward
    work.)"""
    return _run([input], [target], [_NLL], [0.0], ignore_index, 'mean', crf=[(0, 1.0, scrf)])[1]


_KIND = {nll_loss: _NLL, F.nll_loss: _NLL, binary_cross_entropy_loss: _BCE, budget_loss: _BUDGET}

# Data-parallel normalisation: every term is a sum over the valid (non-ignored) targets divided by their
# number (pyrutils/torch/losses.py:13-21, :30-36; F.nll_loss reduction='mean', :47). With ragged clips the ranks hold
# different numbers of valid targets, and the average of per-rank means is not the global mean. A registered reducer
# (distributed.DataParallel(count_weighted_loss=True)) maps this rank's per-term counts [terms] (fp64, on the device) to
# (global count) / W: the term becomes sum_rank / (count_global / W), whose average over the W ranks -- and so the
# averaged gradient -- is the global-batch value. No reducer: the reference's single-process arithmetic.
#
# The reducer is a COLLECTIVE, so it is never installed process-wide: it is active only inside
# `with dp.loss_scope():` (count_reducer_scope below), which the training step enters around its criterion call, and only
# while autograd is recording -- a validation pass on one rank, a second model's criterion or a no_grad evaluation issue
# no collective and cannot pair with another rank's all-reduce. Every rank must make the same number of criterion calls
# inside the scope.
_count_reducer = None


class count_reducer_scope:
    """Context manager: `fn` (or None) reduces the per-term counts of every criterion call made inside the scope."""

    def __init__(self, fn):
        self.fn, self.prev = fn, None

    def __enter__(self):
        global _count_reducer
        self.prev, _count_reducer = _count_reducer, self.fn
        return self

    def __exit__(self, *exc):
        global _count_reducer
        _count_reducer = self.prev
        return False


def get_count_reducer():
    return _count_reducer


# What _run hands to _MultiTaskLoss beside the tensors. smoothing: [(index, weight, tau)], crf and scrf: [(index, weight)] of
# the linear-chain and of the semi-Markov terms, options: None or ([class weight], [positive-class weight]) per term.
_Spec = namedtuple('_Spec', 'kinds targets weights ignore reducer smoothing options crf scrf')


class _Tail:
    """One family of terms that follow the zipped ones in the loss tensor (the smoothing terms, the CRF terms, the semi-Markov
    CRF terms). They take their inputs by index: index[j] is the zipped term whose input and gradient buffer term j shares.
    `name` gives the two launchers of the kernel layer, name_fwd and name_bwd; a term of the family owns n_params parameter
    tensors (CRF: A and pi; semi-Markov CRF: A, pi and dur)."""

    def __init__(self, name, index, terms, n_params=0):
        self.name, self.index, self.terms, self.n_params = name, index, terms, n_params

    def fwd(self, K, losses, stats):
        """Writes the family's part of the tail (views of the loss and stats tensors) in place."""
        getattr(K, self.name + '_fwd')(self.terms, losses, stats)

    def bwd(self, K, stats, dlosses, dins, accumulate, need_params):
        """Stores d(input) into dins[j] or adds to it; per term, the gradients of its parameter tensors or None."""
        launch = getattr(K, self.name + '_bwd')
        if self.n_params:
            return launch(self.terms, stats, dlosses, dins, accumulate, need_params)
        launch(self.terms, stats, dlosses, dins, accumulate)
        return [None] * len(self.terms)


class _MultiTaskLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, spec, *inputs):
        kinds, ignore = spec.kinds, spec.ignore
        # behind the n inputs: (transitions, initial) of every CRF term, then (transitions, initial, durations) of every
        # semi-Markov one, so that autograd hands their gradients to the modules
        inputs, crf_params = inputs[:len(kinds)], inputs[len(kinds):]
        scrf_params = crf_params[2 * len(spec.crf):]
        K = get_kernels()
        terms = []
        for x, y, k, w in zip(inputs, spec.targets, kinds, spec.weights):
            x = x.detach().contiguous()
            y = (y.to(torch.int64) if k == _NLL else y.to(torch.float32)).contiguous()
            terms.append(dict(kind=k, input=x, target=y, weight=w, ignore=ignore))
        # class weights / a positive-class weight on ANY term: all terms of the call go through twog_weighted_loss_*, still
        # one launch per direction; none: the plain entry points, exactly as before (same launches, same bits)
        ctx.weighted = spec.options is not None
        if ctx.weighted:
            for t, cw, p in zip(terms, *spec.options):
                t['class_weight'], t['positive_class_weight'] = cw, p
        fwd = K.weighted_loss_fwd if ctx.weighted else K.multitask_loss_fwd
        smooth = [dict(input=terms[i]['input'], target=terms[i]['target'], weight=w, tau=tau, ignore=ignore)
                  for i, w, tau in spec.smoothing]
        chains = [dict(input=terms[i]['input'], target=terms[i]['target'], weight=w, ignore=ignore,
                       transitions=crf_params[2 * j].detach().contiguous(), initial=crf_params[2 * j + 1].detach().contiguous())
                  for j, (i, w) in enumerate(spec.crf)]
        segs = [dict(input=terms[i]['input'], target=terms[i]['target'], weight=w, ignore=ignore,
                     transitions=scrf_params[3 * j].detach().contiguous(), initial=scrf_params[3 * j + 1].detach().contiguous(),
                     durations=scrf_params[3 * j + 2].detach().contiguous())
                for j, (i, w) in enumerate(spec.scrf)]
        # the smoothing terms, then the CRF terms, then the semi-Markov ones follow the n zipped ones in the same tensors: one
        # more launch (pair) each writes its part of the tail in place
        tails = []
        if smooth:
            tails.append(_Tail('smooth_loss', [i for i, _, _ in spec.smoothing], smooth))
        if chains:
            tails.append(_Tail('crf_nll', [i for i, _ in spec.crf], chains, n_params=2))
        if segs:
            tails.append(_Tail('semicrf_nll', [i for i, _ in spec.scrf], segs, n_params=3))
        tail_terms = smooth + chains + segs
        losses, stats = fwd(terms, room=len(tail_terms)) if tail_terms else fwd(terms)
        at = len(terms)
        for f in tails:
            f.fwd(K, losses[at:at + len(f.terms)], stats[at:at + len(f.terms)])
            at += len(f.terms)
        if spec.reducer is not None:
            # six to twelve scalars: sum_rank / (count_global / W) per term, 0 / 0 -> NaN for NLL like torch's mean over an
            # empty selection, 0 for the BCE / budget terms (pyrutils/torch/losses.py:15-16, :32-33). Same arithmetic as
            # loss_final_kernel (csrc/loss.hip): the fp64 quotient rounded to fp32, then the fp32 product with the weight
            # -- with a reducer that returns the counts unchanged (one rank) the losses are bit-identical to the plain path.
            # With class weights the column handed over is den, the sum of the kept weights: the global WEIGHTED mean.
            eff = spec.reducer(stats[:, 1].clone())
            val = stats[:, 0] / eff
            soft = torch.tensor([k != _NLL for k in kinds] + [True] * len(tail_terms), device=val.device)
            val = torch.where(soft & (eff <= 0), torch.zeros_like(val), val)
            w = torch.tensor([float(x) for x in spec.weights] + [t['weight'] for t in tail_terms], dtype=torch.float32,
                             device=val.device)
            losses = w * val.to(torch.float32)
            stats = torch.stack([stats[:, 0], eff], 1).contiguous()
        ctx.terms, ctx.stats, ctx.tails = terms, stats, tails
        return losses

    @staticmethod
    def backward(ctx, dlosses):
        wanted, n, K = ctx.needs_input_grad, len(ctx.terms), get_kernels()
        out = [None] * len(wanted)   # of spec, of the n inputs, then of the parameters of the tail terms in term order
        # weight 0 or nothing to differentiate: no backward work
        need = [wanted[i + 1] and t['weight'] != 0 for i, t in enumerate(ctx.terms)]
        dins = [None] * n
        if any(need):
            dins = list((K.weighted_loss_bwd if ctx.weighted else K.multitask_loss_bwd)(ctx.terms, ctx.stats, dlosses, need))
        at, p0 = n, 1 + n
        for f in ctx.tails:
            m = len(f.terms)
            slots = [range(p0 + f.n_params * j, p0 + f.n_params * (j + 1)) for j in range(m)]
            # a term asks for d(input) and for its parameters' gradients separately
            need_x = [wanted[i + 1] and t['weight'] != 0 for i, t in zip(f.index, f.terms)]
            need_p = [any(wanted[q] for q in s) and t['weight'] != 0 for s, t in zip(slots, f.terms)]
            if any(need_x) or any(need_p):
                # one gradient per input: the launch adds into the buffer an earlier launch (NLL, or a family before this one)
                # wrote on this stream, or stores into a buffer of its own where none of them had backward work for that input
                fdins, acc = [None] * m, [False] * m
                for j, (i, nd) in enumerate(zip(f.index, need_x)):
                    if nd:
                        acc[j] = dins[i] is not None
                        if not acc[j]:
                            dins[i] = torch.empty_like(ctx.terms[i]['input'])
                        fdins[j] = dins[i]
                grads = f.bwd(K, ctx.stats[at:at + m], dlosses.contiguous()[at:at + m], fdins, acc, need_p)
                for s, gr in zip(slots, grads):
                    for q, g in zip(s, gr or ()):
                        out[q] = g if wanted[q] else None
            at, p0 = at + m, p0 + f.n_params * m
        out[1:1 + n] = dins
        return tuple(out)


_uploaded_weights = {}   # (values, device) -> fp32 tensor: a host sequence of class weights is uploaded once per device


def _class_weight(cw, i, kind, x):
    """Entry i of class_weights -> a contiguous fp32 [C] tensor on x's device, or None. A host sequence is checked and
    uploaded once; a tensor is taken as it is and never read back (no host synchronisation)."""
    if cw is None:
        return None
    if kind != _NLL:
        raise ValueError(f'class weights on term {i}, which is not an NLL term')
    C = x.shape[1] if x.dim() >= 2 else -1
    if not torch.is_tensor(cw):
        values = tuple(float(v) for v in cw)
        if any(v < 0 or v != v or v in (float('inf'), float('-inf')) for v in values):
            raise ValueError(f'class weights of term {i}: negative or non-finite value in {values}')
        key = (values, x.device)
        if key not in _uploaded_weights:
            _uploaded_weights[key] = torch.tensor(values, dtype=torch.float32).to(x.device)
        cw = _uploaded_weights[key]
    if cw.dim() != 1 or cw.numel() != C:
        raise ValueError(f'class weights of term {i}: shape {tuple(cw.shape)} for an input of {C} classes')
    return cw.detach().to(device=x.device, dtype=torch.float32).contiguous()


def _positive_weight(p, i, kind):
    if p is None:
        return 1.0
    if kind != _BCE:
        raise ValueError(f'positive-class weight on term {i}, which is not a BCE term')
    p = float(p)
    if p < 0 or p != p or p == float('inf'):
        raise ValueError(f'positive-class weight of term {i}: {p} is negative or not finite')
    return p


def _options(inputs, kinds, class_weights, positive_class_weights):
    """None when no term carries an option (the plain launches), else ([class weight tensor or None], [p]) per term."""
    n = len(kinds)
    cws = list(class_weights) if class_weights is not None else [None] * n
    pws = list(positive_class_weights) if positive_class_weights is not None else [None] * n
    if len(cws) != n or len(pws) != n:
        raise ValueError(f'class_weights / positive_class_weights: {len(cws)} / {len(pws)} entries for {n} terms')
    cws = [_class_weight(cw, i, k, x) for i, (cw, k, x) in enumerate(zip(cws, kinds, inputs))]
    pws = [_positive_weight(p, i, k) for i, (p, k) in enumerate(zip(pws, kinds))]
    if all(cw is None for cw in cws) and all(p == 1.0 for p in pws):
        return None
    return cws, pws


def _crf_terms(crf, inputs, kinds):
    """The `crf` list of multi_task_loss checked against the call, before any launch: [(index, weight)], [module]."""
    terms, modules = [], []
    for entry in crf:
        i, w, module = entry
        i, w = int(i), float(w)
        if not 0 <= i < len(kinds) or kinds[i] != _NLL:
            raise ValueError(f'CRF term on input {i}: not one of the NLL terms of this call')
        x = inputs[i]
        if x.dim() != 4:
            raise ValueError(f'CRF term on input {i}: (bs, C, T, E) log-probabilities are expected, got {tuple(x.shape)}')
        if not isinstance(module, (LinearChainCRF, SemiMarkovCRF)):
            raise ValueError(f'CRF term on input {i}: a LinearChainCRF or SemiMarkovCRF module is expected, got '
                             f'{type(module).__name__}')
        if module.num_classes != x.shape[1]:
            raise ValueError(f'CRF term on input {i}: a module of {module.num_classes} classes for an input of {x.shape[1]}')
        if isinstance(module, SemiMarkovCRF):
            max_classes, max_steps, max_duration = get_kernels().semicrf_limits()
            if module.max_duration > max_duration:
                raise ValueError(f'CRF term on input {i}: durations up to {max_duration} are taken, not {module.max_duration}')
        else:
            max_classes, max_steps = get_kernels().crf_limits()
        if x.shape[1] > max_classes or x.shape[2] > max_steps:
            raise ValueError(f'CRF term on input {i}: up to {max_classes} classes and {max_steps} model steps are taken, '
                             f'not {x.shape[1]} and {x.shape[2]}')
        terms.append((i, w))
        modules.append(module)
    if len({i for i, _ in terms}) != len(terms):
        # (both would write the gradient buffer of that input)
        raise ValueError('more than one CRF term on the same input')
    return terms, modules


def _run(inputs, targets, kinds, weights, ignore_value, reduction, smoothing=(), class_weights=None,
         positive_class_weights=None, crf=()):
    if reduction != 'mean':
        raise NotImplementedError("only reduction='mean' (the reference's setting) is implemented")
    options = _options(inputs, kinds, class_weights, positive_class_weights)
    smoothing = [(int(i), float(w), float(tau)) for i, w, tau in smoothing]
    for i, _, tau in smoothing:
        if not 0 <= i < len(kinds) or kinds[i] != _NLL:
            raise ValueError(f'smoothing term on input {i}: not one of the NLL terms of this call')
        if not tau > 0:
            raise ValueError(f'smoothing term on input {i}: tau must be positive, got {tau}')
    if len({i for i, _, _ in smoothing}) != len(smoothing):
        # (both would write the gradient buffer of that input in the same launch)
        raise ValueError('more than one smoothing term on the same input')
    crf, modules = _crf_terms(crf, inputs, kinds)
    # the linear-chain terms, then the semi-Markov ones, each in list order
    semi = [isinstance(m, SemiMarkovCRF) for m in modules]
    scrf = [t for t, s in zip(crf, semi) if s]
    crf = [t for t, s in zip(crf, semi) if not s]
    crf_params = [p for m, s in zip(modules, semi) if not s for p in (m.transitions, m.initial)]
    crf_params += [p for m, s in zip(modules, semi) if s for p in (m.transitions, m.initial, m.durations)]
    # the scope's reducer, and only while autograd records (read here: grad mode is off inside Function.forward)
    reducer = _count_reducer if torch.is_grad_enabled() else None
    losses = _MultiTaskLoss.apply(_Spec(list(kinds), list(targets), [float(w) for w in weights], ignore_value, reducer,
                                        smoothing, options, crf, scrf), *inputs, *crf_params)
    return list(losses.unbind(0))


def multi_task_loss(input: list, target: list, loss_functions: list, weight: list = None, ignore_value=-1,
                    reduction: str = 'mean', smoothing: list = None, class_weights: list = None,
                    positive_class_weights: list = None, crf: list = None):
    """pyrutils/torch/losses.py:39-51: the list of weighted losses, one per (input, target, loss function).

    class_weights / positive_class_weights: lists aligned with the terms. class_weights[i] is None, a [C] tensor (taken as
    it is, never read back) or a sequence of floats (checked, uploaded once per device): F.nll_loss's weight= for NLL term i.
    positive_class_weights[i] is None or a number: the positive_class_weight of BCE term i. An entry on a term of another
    kind, a wrong length, or a negative / non-finite host value raises ValueError before any launch. When any term carries
    one, all terms of the call run through twog_weighted_loss_* (one launch per direction, as without).

    smoothing: a list of (index, weight, tau); term j is weight * temporal_smoothing_loss(input[index], target[index], tau),
    appended after the zipped terms in list order (input[index] must be an NLL term's (bs, C, T, E) log-probabilities). Each
    input still receives ONE gradient: the smoothing terms take the inputs by index.

    crf: a list of (index, weight, module), module a LinearChainCRF or a SemiMarkovCRF; a term is weight * crf_loss(
    input[index], target[index], module), or weight * semi_crf_loss(...) for a SemiMarkovCRF, appended after the zipped terms
    and after the smoothing terms: the linear-chain terms first, then the semi-Markov ones, each in list order. input[index]
    must be an NLL term's (bs, C, T, E) input. A class-count mismatch, a non-NLL index, two such terms on one input or a shape
    beyond kernels.crf_limits() / kernels.semicrf_limits() (max_duration included) raises ValueError before any launch. dA and
    dpi (and ddur) come back as the gradients of the module's parameters; a term of weight 0, or one whose parameters and
    input need no gradient, gets no backward work."""
    if weight is None:
        weight = [1.0] * len(input)
    n = min(len(input), len(target), len(loss_functions), len(weight))  # zip semantics
    kinds = []
    for fn in loss_functions[:n]:
        if fn not in _KIND:
            raise NotImplementedError(f'loss function {fn} is not part of the 2G-GCN criterion')
        kinds.append(_KIND[fn])
    return _run(list(input[:n]), list(target[:n]), kinds, list(weight[:n]), ignore_value, reduction, smoothing or (),
                None if class_weights is None else list(class_weights)[:n],
                None if positive_class_weights is None else list(positive_class_weights)[:n], crf or ())


_CRF_KEYS = ('SAR', 'SAP', 'OAR', 'OAP')


def _crf_keys(dataset_name, cfg, crf):
    """The keys of the CRF terms select_loss appends for this configuration (misc.crf_loss.add), in term order. crf: the dict
    of modules, or None where only the configuration is known (then: every final-level NLL term of the dataset)."""
    if not _misc(cfg).get('crf_loss', {}).get('add', False):
        return []
    allowed = _CRF_KEYS if dataset_name == 'cad120' else _CRF_KEYS[:2]
    if crf is None:
        return list(allowed)
    unknown = [k for k in crf if k not in allowed]
    if unknown:
        raise ValueError(f'CRF modules for {unknown}: the final-level NLL terms of {dataset_name} are {list(allowed)}')
    return [k for k in allowed if k in crf]


def _crf_term_names(keys, crf):
    """The names of the terms of these keys in the order multi_task_loss appends them: 'CRF_<key>' of the LinearChainCRF
    modules, then 'SCRF_<key>' of the SemiMarkovCRF ones. crf None: every module counts as a LinearChainCRF."""
    semi = [crf is not None and isinstance(crf[k], SemiMarkovCRF) for k in keys]
    return ['CRF_' + k for k, s in zip(keys, semi) if not s] + ['SCRF_' + k for k, s in zip(keys, semi) if s]


def select_loss(model_name: str, model_input_type: str, dataset_name: str, cfg, *, crf=None):
    """vhoi/losses.py:8-70 for model '2G-GCN': (criterion, loss_names). cfg needs `.get('misc', default_value={})`.
    crf: with misc.crf_loss = {add: true, weight: w}, a dict of LinearChainCRF or SemiMarkovCRF modules keyed by 'SAR', 'SAP',
    'OAR', 'OAP': one term per key present, on the final-level NLL term of that name, weighted w times that term's weight;
    named 'CRF_<key>' (linear-chain, first) and 'SCRF_<key>' (semi-Markov, after them)."""
    if model_name != '2G-GCN':
        raise NotImplementedError(f'{model_name}: only the 2G-GCN hot path is built (SURVEY section 8)')
    misc = _misc(cfg)
    hb_weight = ob_weight = 0.0
    if misc.get('budget_loss', {}).get('add', False):
        hb_weight = misc.get('budget_loss', {}).get('human_weight', 1.0)
        ob_weight = misc.get('budget_loss', {}).get('object_weight', 1.0)
    cad = dataset_name == 'cad120'
    weight = [hb_weight, ob_weight] if cad else [hb_weight]
    hs_weight = os_weight = 0.0
    seg = misc.get('segmentation_loss', {})
    s_weight, add_seg = seg.get('weight', 1.0), seg.get('add', False)
    if add_seg and not misc.get('input_human_segmentation', False):
        hs_weight = s_weight
    if add_seg and not misc.get('input_object_segmentation', False):
        os_weight = s_weight
    weight += [hs_weight, os_weight] if cad else [hs_weight]
    weight_val = 0.0 if (add_seg and seg.get('pretrain', False)) else 1.0
    ant_weight = misc.get('anticipation_loss_weight', 1.0)
    fl_weight = misc.get('first_level_loss_weight', 0.0)
    if cad:
        weight += [fl_weight] * 4 + [weight_val, ant_weight, weight_val, ant_weight]
        fns = (budget_loss, budget_loss, binary_cross_entropy_loss, binary_cross_entropy_loss) + (nll_loss,) * 8
        names = ['B_HS', 'B_OS', 'BCE_HS', 'BCE_OS', 'NLL_SAR_F', 'NLL_SAP_F', 'NLL_OAR_F', 'NLL_OAP_F',
                 'NLL_SAR', 'NLL_SAP', 'NLL_OAR', 'NLL_OAP']
    else:
        weight += [fl_weight] * 2 + [weight_val, ant_weight]
        fns = (budget_loss, binary_cross_entropy_loss) + (nll_loss,) * 4
        names = ['B_HS', 'BCE_HS', 'NLL_SAR_F', 'NLL_SAP_F', 'NLL_SAR', 'NLL_SAP']
    # Beyond the reference, against label imbalance. misc.class_weights = {add, subactivity: [...], affordance: [...]}: the
    # per-class weights of the human NLL terms (NLL_SAR(_F), NLL_SAP(_F)) and of the object ones (NLL_OA*); and
    # misc.segmentation_loss.positive_class_weight on the BCE terms. The keywords appear only with the keys.
    options = {}
    cw_cfg = misc.get('class_weights', {})
    if cw_cfg.get('add', False):
        by_prefix = {'NLL_SA': cw_cfg.get('subactivity', None), 'NLL_OA': cw_cfg.get('affordance', None)}
        cws = [by_prefix.get(name[:6]) for name in names]
        if any(cw is not None for cw in cws):
            options['class_weights'] = [None if cw is None else [float(v) for v in cw] for cw in cws]
    p = seg.get('positive_class_weight', 1)
    if p != 1:
        options['positive_class_weights'] = [float(p) if fn is binary_cross_entropy_loss else None for fn in fns]
    first = len(fns) - (4 if cad else 2)
    if misc.get('crf_loss', {}).get('add', False):
        # one CRF term per module, on the final-level NLL term of that name and weighted relative to it, as the smoothing
        # terms are; appended after them
        if not crf:
            raise ValueError('misc.crf_loss.add is set, but select_loss was given no CRF modules (crf={name: LinearChainCRF})')
        c_weight = misc.get('crf_loss', {}).get('weight', 1.0)
        index = {names[i][len('NLL_'):]: i for i in range(first, len(fns))}
        keys = _crf_keys(dataset_name, cfg, crf)
        options['crf'] = [(index[k], c_weight * weight[index[k]], crf[k]) for k in keys]
        crf_names = _crf_term_names(keys, crf)
    else:
        crf_names = []
    smooth = misc.get('smoothing_loss', {})
    if not smooth.get('add', False):
        return partial(multi_task_loss, loss_functions=fns, weight=weight, **options), names + crf_names
    # one smoothing term per final-level NLL term (the last 2 or 4 of the list; not the frame-level _F ones), weighted
    # relative to it: the stage-1 pretraining zeros and the anticipation weight carry over
    s_weight, tau = smooth.get('weight', 0.15), smooth.get('tau', 4.0)
    smoothing = [(i, s_weight * weight[i], tau) for i in range(first, len(fns))]
    names = names + ['TMSE_' + names[i][len('NLL_'):] for i in range(first, len(fns))] + crf_names
    return partial(multi_task_loss, loss_functions=fns, weight=weight, smoothing=smoothing, **options), names


def _n_smoothing_terms(dataset_name, cfg):
    """The smoothing terms select_loss appends for this configuration (misc.smoothing_loss.add)."""
    if not _misc(cfg).get('smoothing_loss', {}).get('add', False):
        return 0
    return 4 if dataset_name == 'cad120' else 2


def select_loss_types(model_name: str, dataset_name: str, cfg, *, crf=None):
    """vhoi/losses.py:72-80. crf: the dict of modules given to select_loss (None: one CRF term per final-level NLL term). A
    linear-chain term is 'crf', a semi-Markov one 'scrf'."""
    if model_name != '2G-GCN':
        raise ValueError(f'Multi-task learning option not implemented for {model_name}')
    types = ['budget'] * 2 + ['bce'] * 2 + ['softmax'] * 8 if dataset_name == 'cad120' else ['budget', 'bce'] + ['softmax'] * 4
    kinds = ['scrf' if n.startswith('SCRF_') else 'crf' for n in _crf_term_names(_crf_keys(dataset_name, cfg, crf), crf)]
    return types + ['mse'] * _n_smoothing_terms(dataset_name, cfg) + kinds


def select_loss_learning_mask(model_name: str, dataset_name: str, cfg, *, crf=None):
    """vhoi/losses.py:83-91. crf: as for select_loss_types."""
    if model_name != '2G-GCN':
        raise ValueError(f'Multi-task learning option not implemented for {model_name}')
    mask = [False] * 4 + [True] * 8 if dataset_name == 'cad120' else [False] * 2 + [True] * 4
    return mask + [False] * (_n_smoothing_terms(dataset_name, cfg) + len(_crf_keys(dataset_name, cfg, crf)))


def class_counts(targets, num_classes, ignore_index=-1, out=None):
    """Labels per class of a target tensor, on its device, under the NLL terms' rule (a label equal to ignore_index or outside
    [0, num_classes) is skipped): int64 [num_classes]. With `out` (such a tensor) the counts are ADDED to it and it is
    returned, so a pass over a loader's targets accumulates without a host synchronisation."""
    targets = targets.to(torch.int64).contiguous()
    if out is None:
        out = torch.zeros(int(num_classes), dtype=torch.int64, device=targets.device)
    return get_kernels().class_counts(targets, int(num_classes), int(ignore_index), out)


def class_weights(counts, scheme='balanced', beta=0.999):
    """Per-class weights from class counts, computed once on the host in fp64: fp32 [C] on the counts' device.
    'balanced': N / (K * n_c), N the number of labels and K the number of classes present (sklearn's
    compute_class_weight('balanced') over the classes present). 'effective': (1 - beta) / (1 - beta^n_c), the inverse
    effective number of samples (Cui et al., CVPR 2019), scaled to sum to K. A class without labels gets 0."""
    import numpy as np
    device = counts.device if torch.is_tensor(counts) else 'cpu'
    n = np.asarray(counts.cpu() if torch.is_tensor(counts) else counts).astype(np.float64)
    if n.ndim != 1 or (n < 0).any():
        raise ValueError('class counts: a 1-D array of non-negative numbers is expected')
    present = n > 0
    K = int(present.sum())
    w = np.zeros_like(n)
    if scheme == 'balanced':
        w[present] = n.sum() / (K * n[present])
    elif scheme == 'effective':
        if not 0 <= beta < 1:
            raise ValueError(f'beta must lie in [0, 1), got {beta}')
        w[present] = (1.0 - beta) / (1.0 - np.power(np.float64(beta), n[present]))
        w *= K / w.sum() if K else 0.0
    else:
        raise ValueError(f"scheme must be 'balanced' or 'effective', got {scheme!r}")
    return torch.from_numpy(w.astype(np.float32)).to(device)
