"""Helpers of the training-step option tests (gradient-norm clipping, multi-task loss learner): the G14 batches and the
kernel test double of the new entry points.

G14 (tools/make_golden_train_options.py) composes the reference's training step with `clip_gradient_at` and the
`MultiTaskLossLearner`: (a) is G12's MPHOI configuration (tests/helpers.py: g12_step_batch), (b) a CAD-120 layout with the
object heads (12 loss terms). Inputs, targets and initial weights are closed-form (oracle/detgen.py); the fixtures hold
what the reference produced.
"""
import json
import math
import os

import numpy as np
import torch

from oracle import detgen
from tests.fake_kernels import FakeKernels
from tests.helpers import GOLDEN, g12_step_batch, synth_inputs

G14_CASES = ('a', 'b')


def load_g14(case):
    z = np.load(os.path.join(GOLDEN, f'g14_{case}.npz'), allow_pickle=False)
    return z, json.loads(str(z['meta_json']))


def cad_targets(meta, step, mask):
    """CAD-120 targets of step `step`: segmentation gates and class labels of the human and the objects, a ragged tail on
    clip 1 and -1 for the virtual objects (objects_mask 0)."""
    bs, T, H, O, seed = meta['bs'], meta['T'], meta['H'], meta['O'], meta['seed']
    nh, no = meta['classes']
    pre = f"{meta['name']}.s{step}"
    hcls = [(detgen.uniform01(f'{pre}.hcls{i}', (bs, T, H), seed=seed) * nh).astype(np.int64) for i in range(2)]
    ocls = [(detgen.uniform01(f'{pre}.ocls{i}', (bs, T, O), seed=seed) * no).astype(np.int64) for i in range(2)]
    hseg = (detgen.uniform01(f'{pre}.hseg', (bs, T, H), seed=seed) > 0.55).astype(np.float32)
    oseg = (detgen.uniform01(f'{pre}.oseg', (bs, T, O), seed=seed) > 0.55).astype(np.float32)
    for a in hcls + [hseg]:
        a[1, T - 2:] = -1
    virtual = mask[:, None, :] == 0
    for a in ocls + [oseg]:
        a[1, T - 2:] = -1
        a[np.broadcast_to(virtual, a.shape)] = -1
    return hcls, ocls, hseg, oseg


def g14_step_batch(meta, step):
    """(model kwargs, criterion targets) of training step `step` of a G14 case."""
    if meta['layout'] == 'mphoi':
        return g12_step_batch(meta, step)
    xh, xo, mask = synth_inputs(f"{meta['name']}.s{step}", meta['H'], meta['O'], meta['N'], meta['bs'], meta['T'],
                                meta['seed'])
    hcls, ocls, hseg, oseg = cad_targets(meta, step, mask)
    kw = dict(x_human=torch.from_numpy(xh), x_objects=torch.from_numpy(xo), objects_mask=torch.from_numpy(mask),
              steps_per_example=torch.full((meta['bs'],), float(meta['T'])))
    t = torch.from_numpy
    target = [t(hseg), t(oseg), t(hseg), t(oseg)] + [t(hcls[0]), t(hcls[1]), t(ocls[0]), t(ocls[1])] * 2
    return kw, target


class TrainOptionKernels(FakeKernels):
    """FakeKernels plus torch implementations of twog_grad_norm, twog_adam_step_coef and twog_mtl_weight_fwd/bwd (the
    executable specification of csrc/train_opts.hip). Records the name of every optimizer / learner call in `calls`."""

    def grad_norm(self, buf, ranges, scale, max_norm, out=None):
        self.calls.append(('grad_norm', tuple((int(b), int(e)) for b, e in ranges)))
        s = torch.zeros((), dtype=torch.float64)
        for b, e in ranges:
            s = s + buf[b:e].double().square().sum()
        norm = (s.sqrt() * abs(float(scale))).float()
        coef = (norm + 1e-6).reciprocal() * float(max_norm)   # torch: max_norm / (total_norm + 1e-6)
        res = torch.stack([norm, coef])
        if out is None:
            return res
        out[:2].copy_(res)
        return out

    def adam_step_coef(self, param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step, grad_scale,
                       coef):
        self.calls.append(('adam_step_coef', param.numel()))
        c = coef.reshape(-1)[0]
        k = torch.where(c < 1, c, torch.ones_like(c))   # NaN: no clipping
        FakeKernels.adam_step(self, param, (grad * grad_scale) * k, exp_avg, exp_avg_sq, lr, beta1, beta2, eps,
                              weight_decay, step, 1.0)

    def adam_step(self, param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0):
        self.calls.append(('adam_step', param.numel()))
        super().adam_step(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step, grad_scale)

    @staticmethod
    def _weight(kind, s):
        """(w, dw/ds) of one term in torch's order of operations (pyrutils/torch/multi_task.py:62-71)."""
        if kind == 3:   # mae
            e = torch.exp(-s)
            return math.sqrt(2.0) * e, -(math.sqrt(2.0) * e)
        e = torch.exp(-2 * s)
        a = 0.5 if kind == 2 else 1.0
        return a * e, -2 * (a * e)

    def mtl_weight_fwd(self, kinds, losses, log_sds):
        self.calls.append(('mtl_weight_fwd', len(kinds)))
        out = losses.detach().clone()
        for i, k in enumerate(kinds):
            if k:
                w, _ = self._weight(k, log_sds[i])
                out[i] = w * losses[i] + log_sds[i]
        return out

    def mtl_weight_bwd(self, kinds, losses, log_sds, dout, dlog_sds, accumulate):
        self.calls.append(('mtl_weight_bwd', len(kinds)))
        dl = dout.detach().clone()
        ds = torch.zeros_like(log_sds)
        for i, k in enumerate(kinds):
            if k:
                w, dw = self._weight(k, log_sds[i])
                dl[i] = dout[i] * w
                ds[i] = dout[i] * losses[i] * dw + dout[i]
        if accumulate:
            dlog_sds += ds
        else:
            dlog_sds.copy_(ds)
        return dl


LOSS_REL, DELTA_REL, NORM_REL = 1e-4, 5e-4, 1e-4


def check_deltas(d, d_ref, meta, what):
    """G12's rule (tests/test_training_trajectory.py): within DELTA_REL of the largest reference delta, except a few
    elements inside 1e-2 of a full Adam step (gradients within fp32 summation noise of zero). Returns the number of those."""
    d, d_ref = np.asarray(d, np.float64), np.asarray(d_ref, np.float64)
    scale = np.abs(d_ref).max()
    assert scale > 0, what
    e = np.abs(d - d_ref)
    tight = e <= DELTA_REL * scale
    assert (~tight).sum() <= max(2, 0.002 * e.size), (what, int((~tight).sum()), e.size, float(e.max() / scale))
    assert e.max() <= 1e-2 * meta['lr'] * meta['steps'], (what, float(e.max()))
    return int((~tight).sum())


def product_g14_trajectory(case, device, dp_kwargs=None):
    """The product's training step with both options -- TGGCN + the fused criterion + MultiTaskLossLearner +
    DataParallel(extra_modules=[learner]) + FusedAdam(max_grad_norm) -- on the current kernel backend, checked against
    G14 `case`."""
    from twog_gcn_amd.distributed import DataParallel, FusedAdam
    from twog_gcn_amd.losses import select_loss, select_loss_types, select_loss_learning_mask
    from twog_gcn_amd.models import TGGCN
    from twog_gcn_amd.multi_task import MultiTaskLossLearner
    from tests.helpers import det_state_dict, sample_grad
    z, meta = load_g14(case)
    m = TGGCN(input_size=(2048 + 4 * meta['N'], 2048), num_classes=tuple(meta['classes']), **meta['cfg'])
    m.load_state_dict(det_state_dict(meta['state_dict_shapes'], seed=meta['seed'], gain=meta['gain']))
    m = m.to(device).train()
    init = {n: p.detach().cpu().clone() for n, p in m.named_parameters()}
    cfg = dict(misc=meta['misc'])
    mtll = MultiTaskLossLearner(select_loss_types('2G-GCN', meta['dataset'], cfg),
                                select_loss_learning_mask('2G-GCN', meta['dataset'], cfg)).to(device)
    assert mtll.loss_types == meta['loss_types'] and mtll.mask == meta['mask']
    assert list(mtll.state_dict()) == [str(k) for k in z['mtll_state_keys']]
    dp = DataParallel(m, extra_modules=[mtll], **(dp_kwargs or {}))
    opt = FusedAdam(dp.flat, lr=meta['lr'], max_grad_norm=meta['max_norm'])
    crit, names = select_loss('2G-GCN', 'multiple', meta['dataset'], cfg)
    assert names == [str(s) for s in z['loss_names']]
    raw_all, weighted_all, norms, clipped, log_sds = [], [], [], [], []
    for step in range(meta['steps']):
        kw, target = g14_step_batch(meta, step)
        m._gumbel_noise_override = torch.from_numpy(z[f'noise{step}'])
        dp.zero_grad()
        out = m(**{k: v.to(device) for k, v in kw.items()})
        with dp.loss_scope():
            losses = crit(out, [t.to(device) for t in target], reduction='mean')
        raw_all.append([float(v.detach()) for v in losses])
        losses = mtll(losses)
        sum(losses).backward()
        dp.all_reduce_gradients()
        norm = opt.step(dp.grad_scale)
        assert norm.dim() == 0 and norm.device == dp.flat.grad.device
        weighted_all.append([float(v.detach()) for v in losses])
        n32 = norm.detach().cpu().float()
        norms.append(float(n32))
        clipped.append(bool(meta['max_norm'] / (n32 + 1e-6) < 1))
        log_sds.append(mtll.log_sds.detach().cpu().numpy().copy())
        hard = out[0].detach().cpu().numpy()
        assert np.array_equal(hard, z['hard_gates'][step]), (case, step, 'hard gates')
    for key, got in (('losses_raw', raw_all), ('losses_weighted', weighted_all)):
        want = z[key]
        err = np.abs(np.array(got) - want) / np.maximum(np.abs(want), 1e-3)
        assert err.max() < LOSS_REL, (case, key, float(err.max()))
    nerr = np.abs(np.array(norms) - z['norms']) / z['norms']
    assert nerr.max() < NORM_REL, (case, 'norms', norms, z['norms'].tolist())
    assert clipped == z['clipped'].tolist(), (case, clipped, z['clipped'].tolist())
    for step in range(meta['steps']):   # log_sds start at zero: the value is the delta
        check_deltas(log_sds[step], z['log_sds'][step], meta, f'{case} log_sds step {step}')
    final = {n: p.detach().cpu() for n, p in m.named_parameters()}
    for n in meta['params']:
        check_deltas(sample_grad(final[n] - init[n]), z['delta_' + n], meta, f'{case} {n}')
    w = np.array([np.nan if v is None else v for v in mtll.get_weights()])
    assert np.allclose(w, z['weights_final'], rtol=1e-5, equal_nan=True)
    dp.close()
    return dict(norms=norms, clipped=clipped, log_sds=log_sds, final=final, dp=dp, mtll=mtll)
