"""Shared pieces of the baseline-model tests (test_baselines_cpu.py, test_baselines_gpu.py): the G13 fixtures
(tools/make_golden_baselines.py) and a test double of the kernel entry points the baselines add.

`BaselineFakeKernels` extends the torch double of the kernel interface (tests/fake_kernels.py) with the single-direction
recurrence and the entity pool / concat; each method is the executable specification of its HIP kernel
(include/twog_gcn.h: twog_gru_seq_*, twog_entity_pool_*)."""
import json
import os

import numpy as np
import torch

from oracle import detgen
from tests.fake_kernels import FakeKernels
from tests.helpers import GOLDEN, det_state_dict, rel_err, sample_grad

CASES = ['bim_default', 'bim_unidir', 'bim_nomp', 'bim_nobias', 'bim_h2', 'bim_h64_bs4', 'bim_h64_bs20', 'bim_h128_full',
         'cad_default', 'cad_unidir', 'cad_nomp', 'cad_h13']
OUT_REL, GRAD_REL = 1e-4, 5e-4   # the project's bars (tests/helpers.rel_err)
# G13 trajectory (tools/make_golden_baselines.py: the reference's Bimanual baseline + select_loss + Adam, three steps)
TRAJ = dict(kind='bimanual', bs=4, T=6, H=2, O=4, F=(40, 24), h=64, seed=1321, lr=1e-3, steps=3)


def make_inputs(name, c):
    """Closed-form inputs: one padded object in clip 0; every object of the last clip masked (a clip with no real
    object: the reference clamps the count to 1, the pool is 0)."""
    bs, T, H, O = c['bs'], c['T'], c['H'], c['O']
    x_h = np.maximum(detgen.normal(name + '.xh', (bs, T, H, c['F'][0]), seed=c['seed']), 0.0).astype(np.float32)
    x_o = np.maximum(detgen.normal(name + '.xo', (bs, T, O, c['F'][1]), seed=c['seed']), 0.0).astype(np.float32)
    mask = np.ones((bs, O), dtype=np.float32)
    mask[0, O - 1] = 0.0
    mask[bs - 1, :] = 0.0
    return x_h, x_o * mask[:, None, :, None], mask


def make_targets(name, c, classes):
    bs, T, H, O = c['bs'], c['T'], c['H'], c['O']
    y_h = (detgen.uniform01(name + '.yh', (bs, T, H), seed=c['seed']) * classes[0]).astype(np.int64)
    y_h[0, -1] = -1   # an ignored target
    ys = [y_h]
    if classes[1] is not None:
        ys.append((detgen.uniform01(name + '.yo', (bs, T, O), seed=c['seed']) * classes[1]).astype(np.int64))
    return ys


class BaselineFakeKernels(FakeKernels):
    name = 'fake-torch-baselines'

    def gru_seq_fwd(self, types, bs, T, h):
        outs = []
        for y in types:
            gi = y['gi']
            E = gi.shape[2]
            out = torch.zeros(bs, T, E, h, dtype=gi.dtype, device=gi.device)
            save = torch.zeros(bs, T, E, 4 * h, dtype=gi.dtype, device=gi.device)
            hp = torch.zeros(bs, E, h, dtype=gi.dtype, device=gi.device)
            b = y.get('b_hh')
            for t in range(T):
                gh = hp @ y['w_hh'].t() + (b if b is not None else 0.0)
                r, z, n, hn, g = self._gates(gi[:, t], gh, hp, h)
                out[:, t] = g
                save[:, t] = torch.cat([r, z, n, hn], -1)
                hp = g
            outs.append((out, save))
        return outs

    def gru_seq_bwd(self, types, bs, T, h):
        outs = []
        for y in types:
            d_out, save, out = y['d_out'], y['save'], y['out']
            E = d_out.shape[2]
            d_gi = torch.zeros(bs, T, E, 3 * h, dtype=d_out.dtype, device=d_out.device)
            d_gh = torch.zeros_like(d_gi)
            carry = torch.zeros(bs, E, h, dtype=d_out.dtype, device=d_out.device)
            for t in range(T - 1, -1, -1):
                hp = out[:, t - 1] if t > 0 else torch.zeros_like(carry)
                dgi, dgh, dprev, _ = self._gates_bwd(d_out[:, t] + carry, save[:, t], hp, h)
                d_gi[:, t], d_gh[:, t] = dgi, dgh
                carry = dprev + dgh @ y['w_hh']
            outs.append((d_gi, d_gh))
        return outs

    def entity_pool_fwd(self, hfr, ofr, mask, object_head):
        H, O = hfr.shape[2], ofr.shape[2]
        m = mask[:, None, :, None]
        pooled = (ofr * m).sum(2, keepdim=True) / mask.sum(1).clamp(min=1.0)[:, None, None, None]
        hin = torch.cat([hfr, pooled.expand(-1, -1, H, -1)], -1).contiguous()
        oin = None
        if object_head:
            oin = torch.cat([ofr, hfr.sum(2, keepdim=True).expand(-1, -1, O, -1)], -1).contiguous()
        return hin, oin

    def entity_pool_bwd(self, d_hin, d_oin, mask, O):
        W = d_hin.shape[-1] // 2
        d_hfr = d_hin[..., :W].clone()
        wgt = (mask / mask.sum(1, keepdim=True).clamp(min=1.0))[:, None, :, None]
        d_ofr = wgt * d_hin[..., W:].sum(2, keepdim=True)
        if d_oin is not None:
            d_hfr = d_hfr + d_oin[..., W:].sum(2, keepdim=True)
            d_ofr = d_ofr + d_oin[..., :W]
        return d_hfr.contiguous(), d_ofr.contiguous()


def load_case(name):
    z = np.load(os.path.join(GOLDEN, f'g13_baselines_model_{name}.npz'))
    return z, json.loads(str(z['meta_json']))


def build_case_model(meta, device='cpu'):
    from twog_gcn_amd.baselines import select_model
    cls = select_model('bimanual_baseline' if meta['kind'] == 'bimanual' else 'cad120_baseline')
    classes = tuple(meta['classes'])
    m = cls(input_size=tuple(meta['F']), num_classes=classes, hidden_size=meta['h'], **meta['kw'])
    vals = det_state_dict(meta['state_dict_shapes'], seed=meta['seed'], gain=1.0)
    m.load_state_dict(vals)
    return m.to(device)


def run_case(name, device='cpu'):
    """Forward + backward of one G13 case; returns (model, outputs, golden, meta)."""
    z, meta = load_case(name)
    m = build_case_model(meta, device)
    out = m(torch.from_numpy(z['x_human']).to(device), torch.from_numpy(z['x_objects']).to(device),
            torch.from_numpy(z['objects_mask']).to(device))
    loss = sum((o * torch.from_numpy(z[f'cot{i}']).to(device)).sum() for i, o in enumerate(out))
    loss.backward()
    return m, out, z, meta


def check_case(m, out, z, meta):
    """Outputs within OUT_REL, every parameter gradient within GRAD_REL of its scale; parameters the reference leaves
    without a gradient have none. Returns the worst (output, gradient) deviations."""
    n_out = 2 if meta['kind'] == 'cad120' else 1
    assert len(out) == n_out
    worst_o = worst_g = 0.0
    for i, o in enumerate(out):
        want = z[f'out{i}']
        assert tuple(o.shape) == want.shape, (i, tuple(o.shape), want.shape)
        e = rel_err(o.detach().cpu().numpy(), want)
        assert e < OUT_REL, (i, e)
        worst_o = max(worst_o, e)
    for n, p in m.named_parameters():
        if n in meta['no_grad']:
            assert p.grad is None, n
            continue
        assert p.grad is not None, n
        e = rel_err(sample_grad(p.grad), z['grad_' + n])
        assert e < GRAD_REL, (n, e)
        worst_g = max(worst_g, e)
    return worst_o, worst_g
