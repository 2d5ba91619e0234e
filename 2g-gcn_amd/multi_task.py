"""Multi-task loss learner of the reference's trainer (`misc.multi_task_loss_learner`, train.py:42-46) on the HIP library.

Mirror of `pyrutils/torch/multi_task.py:10-75` (Kendall et al.'s uncertainty weighting): same constructor, `forward(losses)
-> list`, `get_weights()` and state dict (one parameter, `log_sds`), so `losses = mtll_model(losses)` and the checkpoint's
`mtll_model_state_dict` keep working. The weighting of all terms runs in ONE forward and ONE backward launch
(`twog_mtl_weight_fwd/bwd`) that read the criterion's loss tensor in place; nothing syncs with the host.

Under `distributed.DataParallel(..., extra_modules=[learner])` the learner's `log_sds` live in the flat buffers after the
model's parameters: their gradient is all-reduced with the model's, `FusedAdam` steps them (the reference's
`optimizer.add_param_group`), and gradient clipping leaves them out (the reference clips `model.parameters()` only).
"""
from typing import List, Optional

import torch
import torch.nn as nn

from . import _lib as L
from .kernels import get_kernels

_KIND = {'softmax': L.MTL_SOFTMAX, 'mse': L.MTL_MSE, 'mean_squared_error': L.MTL_MSE, 'mae': L.MTL_MAE,
         'mean_absolute_error': L.MTL_MAE}


class _Weighting(torch.autograd.Function):
    @staticmethod
    def forward(ctx, spec, losses, log_sds):
        kinds, param = spec
        ctx.kinds, ctx.param = kinds, param
        ctx.losses, ctx.s = losses.detach(), log_sds.detach()
        return get_kernels().mtl_weight_fwd(kinds, ctx.losses, ctx.s)

    @staticmethod
    def backward(ctx, dout):
        K, prm = get_kernels(), ctx.param
        g = getattr(prm, 'grad', None)
        # the in-place gradient route of the flat buffers (ops.enable_grad_sinks): the kernel adds d(log_sds) into .grad
        sink = (ctx.needs_input_grad[2] and getattr(prm, '_twog_grad_sink', False) and g is not None and g.is_contiguous()
                and g.dtype == torch.float32 and g.device == prm.device and not getattr(prm, '_backward_hooks', None)
                and not getattr(prm, '_post_accumulate_grad_hooks', None))
        ds = g if sink else torch.empty_like(ctx.s)
        dlosses = K.mtl_weight_bwd(ctx.kinds, ctx.losses, ctx.s, dout, ds, accumulate=sink)
        return (None, dlosses if ctx.needs_input_grad[1] else None,
                None if sink or not ctx.needs_input_grad[2] else ds)


def _loss_tensor(losses):
    """The [n] tensor behind the loss list: the criterion's own output when the list is its unbind (losses._run), so the
    kernel reads it in place; otherwise one stack."""
    base = getattr(losses[0], '_base', None) if torch.is_tensor(losses[0]) else None
    if (base is not None and base.dim() == 1 and base.numel() == len(losses) and base.is_contiguous()
            and base.dtype == torch.float32
            and all(torch.is_tensor(x) and x._base is base and x.dim() == 0 and x.storage_offset() == base.storage_offset() + i
                    for i, x in enumerate(losses))):
        return base
    return torch.stack([torch.as_tensor(x, dtype=torch.float32) for x in losses])


class MultiTaskLossLearner(nn.Module):
    """Learns the weights of the losses of an external model (pyrutils/torch/multi_task.py:10-75).

    loss_types: one of 'softmax', 'mse' / 'mean_squared_error', 'mae' / 'mean_absolute_error' per learnable loss (other
    names are allowed for masked terms, e.g. 'budget', 'bce' of losses.select_loss_types). mask: which terms to learn
    (None: all); masked terms pass through unchanged."""

    def __init__(self, loss_types: List[str], mask: Optional[List[bool]] = None):
        super().__init__()
        self.loss_types = list(loss_types)
        self.mask = list(mask) if mask is not None else [True] * len(loss_types)
        self.log_sds = nn.Parameter(torch.zeros(len(loss_types), dtype=torch.float32))

    def _kinds(self):
        kinds = []
        for loss_type, learnable in zip(self.loss_types, self.mask):
            if not learnable:
                kinds.append(L.MTL_PASS)
            elif loss_type not in _KIND:
                raise ValueError('loss_type must be one of \'softmax\', \'mae\' or \'mse\'.')
            else:
                kinds.append(_KIND[loss_type])
        return kinds

    def forward(self, losses: List[torch.Tensor]) -> List[torch.Tensor]:
        assert len(self.loss_types) == len(losses), 'Specified loss types must match the number of input losses.'
        if len(self.mask) != len(self.loss_types):
            # (the reference zips the two and silently drops the terms past the shorter one)
            raise NotImplementedError('mask and loss_types of different lengths')
        out = _Weighting.apply((self._kinds(), self.log_sds), _loss_tensor(list(losses)), self.log_sds)
        return list(out.unbind(0))

    @staticmethod
    def _compute_loss_weight(loss_type: str, log_sd: torch.Tensor) -> torch.Tensor:
        """multi_task.py:62-71 (torch arithmetic: get_weights() is for logging, off the training step)."""
        if loss_type in {'mae', 'mean_absolute_error'}:
            return 2.0 ** 0.5 * torch.exp(-log_sd)
        if loss_type in {'mse', 'mean_squared_error'}:
            return 0.5 * torch.exp(-2 * log_sd)
        return torch.exp(-2 * log_sd)

    def get_weights(self) -> List[Optional[float]]:
        """The learned weights of the losses; None for the terms that are not learned."""
        with torch.no_grad():
            return [self._compute_loss_weight(t, s).item() if m else None
                    for t, s, m in zip(self.loss_types, self.log_sds, self.mask)]
