"""CPU: gradients with respect to the two feature inputs, x_human and x_objects.

  1. the oracle (oracle/cpu_ref.py, inputs as autograd leaves) against the reference's own input gradients (G16,
     tools/make_golden_input_grads.py), at the bar tests/test_oracle_golden.py uses for gradients;
  2. the product's host path (ops.tggcn_backward through TGGCNFunction) on the test double against the oracle's autograd,
     at the bar of tests/test_host_logic_cpu.py's parameter gradients / the project's GRAD_REL;
  3. - 6. what is and is not launched, the synchronised-BatchNorm guard, the other autograd routes.
"""
import json
import os

import numpy as np
import pytest
import torch

import twog_gcn_amd  # noqa: F401
from twog_gcn_amd import kernels as twog_kernels
from twog_gcn_amd import ops
from tests.helpers import GOLDEN, load_g4, sample_grad
from tests.input_grad_cases import G16_CASES, G16_LIMIT, G16_MODES, load_g16, oracle_run, product_forward, sample_stride
from tests.input_grad_fake import InputGradFakeKernels

CASE_MODES = [(c, m) for c in G16_CASES for m in G16_MODES]


class Recording(InputGradFakeKernels):
    """Counts gcn_input_bwd calls and keeps the GEMM launches (operand forms and shapes) in order."""

    def __init__(self):
        super().__init__()
        self.gemms, self.input_bwd_calls = [], 0

    def gemm(self, problems, a_kmajor=False, b_kmajor=False, **kw):
        if self._tape is None:
            self.gemms.append([int(a_kmajor), int(b_kmajor),
                               [[list(p['A'].shape), list(p['B'].shape), list(p['C'].shape), int(bool(p.get('accumulate'))),
                                 list(p.get('batch') or ())] for p in problems]])
        return super().gemm(problems, a_kmajor=a_kmajor, b_kmajor=b_kmajor, **kw)

    def gcn_input_bwd(self, *a, **kw):
        self.input_bwd_calls += 1
        return super().gcn_input_bwd(*a, **kw)


@pytest.fixture()
def fake():
    k = Recording()
    twog_kernels._set_backend_for_tests(k)
    yield k
    twog_kernels._set_backend_for_tests(None)


def _close(got, ref, rel, floor, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = max(float(np.abs(ref).max()), 1e-6)
    err = float(np.abs(got - ref).max())
    print(f'{what}: err {err:.3e} scale {scale:.3e} bound {rel * scale + floor:.3e}')
    assert err < rel * scale + floor, (what, err, scale)


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize('name,mode', CASE_MODES)
def test_oracle_input_gradients_match_the_reference(name, mode):
    z, meta = load_g16()
    assert meta['cases'] == G16_CASES and meta['limit'] == G16_LIMIT
    r = oracle_run(name, mode)
    k = f'{name}_{mode}_'
    vis = r['xh'][..., :2048].contiguous()
    assert int(z[k + 'xh_vis_stride']) == sample_stride(vis.numel()) and int(z[k + 'xo_stride']) == sample_stride(r['xo'].numel())
    _close(r['xh'][..., 2048:].numpy(), z[k + 'xh_geo'], 2e-4, 1e-6, k + 'xh_geo')
    _close(sample_grad(vis, G16_LIMIT), z[k + 'xh_vis'], 2e-4, 1e-6, k + 'xh_vis')
    _close(sample_grad(r['xo'], G16_LIMIT), z[k + 'xo'], 2e-4, 1e-6, k + 'xo')
    # only human 0's geometry is read: exact zeros for the others, in the reference and in the oracle
    assert not z[k + 'xh_geo'][:, :, 1:].any() and not r['xh'][:, :, 1:, 2048:].any()
    assert z[k + 'xh_geo'][:, :, 0].any() and z[k + 'xh_vis'].any() and z[k + 'xo'].any()


def test_masked_objects_follow_the_layout():
    """A masked object is multiplied out of every message it sends or receives, so on the layouts without object heads
    nothing downstream of its embedding reaches the loss: gradient exactly 0. The CAD-120 layout has the object heads
    (vhoi/models.py:905-926): the frame-level heads read every object's own BiGRU state, masked or not, so a masked
    object does receive a gradient there. Holds in the reference's own gradients."""
    z, _ = load_g16()
    for name in G16_CASES:
        z4, meta = load_g4(name)
        mask = z4['objects_mask']                                     # (bs, O)
        for mode in G16_MODES:
            g = oracle_run(name, mode)['xo']                          # (bs, T, O, F_o), pinned to G16 by the test above
            masked = g.permute(0, 2, 1, 3)[torch.from_numpy(mask) == 0]
            assert masked.numel() > 0
            if meta['layout'] == 'cad120':
                assert float(masked.abs().max()) > 0.0, (name, mode)
            else:
                assert float(masked.abs().max()) == 0.0, (name, mode)


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize('name,mode', CASE_MODES)
def test_product_host_path_against_oracle_autograd(name, mode, fake):
    """Fails without the feature: x_human.grad / x_objects.grad stay None."""
    ref = oracle_run(name, mode)
    m, kw, out, loss = product_forward(name, mode)
    loss.backward()
    gh, go = kw['x_human'].grad, kw['x_objects'].grad
    assert gh is not None and go is not None, 'the product path returned no input gradient'
    assert gh.shape == kw['x_human'].shape and go.shape == kw['x_objects'].shape
    assert fake.input_bwd_calls == 1
    _close(gh.numpy(), ref['xh'].numpy(), 5e-4, 5e-6, 'x_human.grad')
    _close(go.numpy(), ref['xo'].numpy(), 5e-4, 5e-6, 'x_objects.grad')
    # the geometry block at its own (smaller) scale, so that it cannot hide under the visual columns'
    _close(gh[:, :, 0, 2048:].numpy(), ref['xh'][:, :, 0, 2048:].numpy(), 5e-4, 5e-6, 'x_human.grad geometry')
    assert not gh[:, :, 1:, 2048:].any()
    z4, meta = load_g4(name)
    if meta['layout'] != 'cad120':
        masked = go.permute(0, 2, 1, 3)[torch.from_numpy(z4['objects_mask']) == 0]
        assert float(masked.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------- 3
def _param_grads(m):
    return {n: (None if p.grad is None else p.grad.clone()) for n, p in m.named_parameters()}


@pytest.mark.parametrize('name', ['c2_stage1', 'c1_stage2'])
def test_nothing_requested_nothing_changes(name, fake):
    """No input requires grad: no gcn_input_bwd call and the GEMM launches of the backward pass are, in order and shape, the
    ones the pass issued before input gradients existed (tests/golden/g16_parent_gemm_sequence.json: recorded with this
    file's Recording.gemm on the commit before the feature). Asking for both adds exactly one grouped launch and leaves
    every parameter gradient bit-identical."""
    parent = json.load(open(os.path.join(GOLDEN, 'g16_parent_gemm_sequence.json')))[name]
    m, kw, out, loss = product_forward(name, 'train', need=(False, False))
    fake.gemms.clear()
    loss.backward()
    assert fake.input_bwd_calls == 0
    assert kw['x_human'].grad is None and kw['x_objects'].grad is None
    none_seq = list(fake.gemms)
    assert none_seq == parent
    g_none = _param_grads(m)

    m2, kw2, out2, loss2 = product_forward(name, 'train', need=(True, True))
    fake.gemms.clear()
    loss2.backward()
    assert fake.input_bwd_calls == 1
    both_seq = list(fake.gemms)
    extra = [g for g in both_seq if g not in none_seq]
    assert len(both_seq) == len(none_seq) + 1 and len(extra) == 1 and len(extra[0][2]) == 2, extra
    assert [g for g in both_seq if g is not extra[0]] == none_seq
    g_both = _param_grads(m2)
    assert g_none.keys() == g_both.keys()
    for n, g in g_none.items():
        assert (g is None) == (g_both[n] is None), n
        if g is not None:
            assert torch.equal(g, g_both[n]), n
    for a, b in zip(out, out2):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize('mode', G16_MODES)
def test_only_x_objects_requires_grad(mode, fake):
    ref = oracle_run('c2_stage1', mode)
    m, kw, out, loss = product_forward('c2_stage1', mode, need=(False, True))
    fake.gemms.clear()
    loss.backward()
    assert kw['x_human'].grad is None
    assert fake.input_bwd_calls == 0
    _close(kw['x_objects'].grad.numpy(), ref['xo'].numpy(), 5e-4, 5e-6, 'x_objects.grad')
    parent = json.load(open(os.path.join(GOLDEN, 'g16_parent_gemm_sequence.json')))['c2_stage1']
    extra = [g for g in fake.gemms if g not in parent]
    assert len(fake.gemms) == len(parent) + 1 and len(extra) == 1 and len(extra[0][2]) == 1   # one problem in the group


def test_only_x_human_requires_grad(fake):
    ref = oracle_run('c1_stage2', 'train')
    m, kw, out, loss = product_forward('c1_stage2', 'train', need=(True, False))
    loss.backward()
    assert kw['x_objects'].grad is None and fake.input_bwd_calls == 1
    _close(kw['x_human'].grad.numpy(), ref['xh'].numpy(), 5e-4, 5e-6, 'x_human.grad')


# ---------------------------------------------------------------------------------------------------------------- 5
def test_sync_bn_guard(fake):
    z, meta = load_g4('c2_stage1')

    def model_with_hook():
        from tests.input_grad_cases import build_model
        m = build_model(meta)
        ops.set_model_extra(m, 'bn_stats_reduce', lambda sums, n_frames: (sums, n_frames))
        return m

    m, kw, out, loss = product_forward('c2_stage1', 'train', model=model_with_hook())
    with pytest.raises(NotImplementedError, match='x_human.*training.*synchronised BatchNorm'):
        loss.backward()
    assert fake.input_bwd_calls == 0 and kw['x_human'].grad is None and kw['x_objects'].grad is None
    # eval mode uses the running statistics: nothing is reduced over ranks, the gradient is the local one
    ref = oracle_run('c2_stage1', 'eval')
    m, kw, out, loss = product_forward('c2_stage1', 'eval', model=model_with_hook())
    loss.backward()
    _close(kw['x_human'].grad.numpy(), ref['xh'].numpy(), 5e-4, 5e-6, 'x_human.grad (eval, hook installed)')
    # x_objects does not pass through the BatchNorm: allowed in training mode as well
    m, kw, out, loss = product_forward('c2_stage1', 'train', need=(False, True), model=model_with_hook())
    loss.backward()
    assert kw['x_objects'].grad is not None and kw['x_human'].grad is None


# ---------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize('mode', G16_MODES)
def test_other_autograd_routes(mode, fake):
    m, kw, out, loss = product_forward('c5_stage1', mode)
    gh1, go1 = torch.autograd.grad(loss, [kw['x_human'], kw['x_objects']], retain_graph=True)
    assert kw['x_human'].grad is None
    loss.backward(retain_graph=True)
    gh2, go2 = kw['x_human'].grad.clone(), kw['x_objects'].grad.clone()
    assert torch.equal(gh1, gh2) and torch.equal(go1, go2)
    kw['x_human'].grad = kw['x_objects'].grad = None
    loss.backward()                                   # second backward over the retained graph
    assert torch.equal(kw['x_human'].grad, gh2) and torch.equal(kw['x_objects'].grad, go2)


def test_front_end_before_the_model_trains(fake):
    """A learned projection in front of the model receives a gradient through x_objects and x_human."""
    z, meta = load_g4('c2_stage1')
    adapter = torch.nn.Linear(2048, 2048, bias=False)
    with torch.no_grad():
        adapter.weight.copy_(torch.eye(2048))
    scale = torch.ones(4 * meta['N'], requires_grad=True)
    m, kw, out, loss = product_forward('c2_stage1', 'train', need=(False, False))
    xh = torch.cat([kw['x_human'][..., :2048], kw['x_human'][..., 2048:] * scale], -1)
    out = m(**dict(kw, x_human=xh, x_objects=adapter(kw['x_objects'])))
    sum((o * o).sum() for o in out if o.requires_grad).backward()
    assert adapter.weight.grad is not None and float(adapter.weight.grad.abs().max()) > 0
    assert scale.grad is not None and float(scale.grad.abs().max()) > 0
