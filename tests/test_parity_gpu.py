"""GPU: the shipped path (TGGCN on cuda through lib2ggcn_hip.so) against
  (1) the golden vectors captured from the real reference (small layouts C1/C2/C5, stage-1 and stage-2 semantics),
  (2) the CPU oracle on the synthetic N=34 layout (C3) at a reduced width, forward and backward,
  (3) the CPU oracle at the full BASELINE sizes (configs[2] T=120 N=34 h=512; configs[1] bs8; configs[4] shard), forward
      and backward,
  (4) size-independent properties at the full bench size: run-to-run bit determinism, batch independence in eval mode.
Tolerance: 1e-4 relative (north_star), stated per assertion."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import twog_gcn_amd  # noqa: F401
from twog_gcn_amd import kernels as twog_kernels
from twog_gcn_amd.models import TGGCN
from oracle import cpu_ref, detgen
from tests.helpers import G4_CASES, G4_CASES_R2_BUILT, load_g4, det_state_dict, g4_inputs, sample_grad

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
REL = 1e-4

STAGE1 = dict(attention_style='v3', discrete_optimization_strategy='gs', filter_discrete_updates=False,
              message_humans_to_human=True, message_human_to_objects=True, message_objects_to_human=True,
              message_objects_to_object=True, message_geometry_to_objects=True, message_geometry_to_human=False,
              message_segment=True, message_type='v2', message_granularity='v1', message_aggregation='att',
              object_segment_update_strategy='ind', update_segment_threshold=0.5)


@pytest.fixture(autouse=True)
def hip_backend():
    twog_kernels._set_backend_for_tests(None)
    assert twog_kernels.get_kernels().name == 'hip'
    yield


def _model_from_meta(meta):
    N = meta['N']
    m = TGGCN(input_size=(2048 + 4 * N, 2048), num_classes=tuple(meta['classes']), **meta['cfg'])
    m.load_state_dict(det_state_dict(meta['state_dict_shapes'], seed=meta['seed'], gain=meta['gain']))
    return m.to(DEV)


@pytest.mark.parametrize('name', G4_CASES + G4_CASES_R2_BUILT)
def test_golden_reference_vectors(name):
    z, meta = load_g4(name)
    m = _model_from_meta(meta)
    m.train()
    noise = torch.from_numpy(z['gumbel_noise'])
    m._gumbel_noise_override = noise if len(noise) else None
    kw = {k: v.to(DEV) for k, v in g4_inputs(z).items()}
    out = m(**kw)
    n_out = len([k for k in z.files if k.startswith('out')])
    assert len(out) == n_out
    for i, o in enumerate(out):
        ref = z[f'out{i}']
        got = o.detach().cpu().numpy()
        if ref.ndim == 3 and np.all((ref == 0) | (ref == 1)) and i < n_out - 4:
            assert np.array_equal(got, ref), f'{name} out{i} (hard gates must be exact)'
        else:
            assert np.abs(got - ref).max() < REL * max(1.0, np.abs(ref).max()), (name, i, float(np.abs(got - ref).max()))
    bn = m.geometry_embedding_gcn.joint_embed.cnn[0].bn
    assert np.allclose(bn.running_mean.cpu().numpy(), z['bn_running_mean'], rtol=1e-5, atol=1e-6)
    assert np.allclose(bn.running_var.cpu().numpy(), z['bn_running_var'], rtol=1e-5, atol=1e-6)
    if not bool(z['backward_ok']):
        return
    loss = 0
    for i, o in enumerate(out):
        if o.requires_grad:
            r = torch.from_numpy(detgen.normal(f'{name}.r{i}', tuple(o.shape), seed=meta['seed'])).to(DEV)
            loss = loss + (o * r).sum()
    assert abs(float(loss.detach()) - float(z['loss'])) < 1e-3 * max(1.0, abs(float(z['loss'])))
    loss.backward()
    none_ref = set(z['none_grads'].tolist())
    worst = 0.0
    for pname, p in m.named_parameters():
        if pname in none_ref:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, pname
            continue
        assert p.grad is not None, pname
        g_ref = z['grad_' + pname]
        g = sample_grad(p.grad)
        scale = max(np.abs(g_ref).max(), 1e-6)
        err = float(np.abs(g - g_ref).max())
        worst = max(worst, err / scale)
        assert err < 5e-4 * scale + 5e-6, (name, pname, err, float(scale))
    print(f'{name}: worst relative gradient error {worst:.2e}')


def _synthetic(bs, T, H, O, N, seed=0, virtual='clip1'):
    """virtual = 'clip1': the last two objects of clip 1 are virtual; 'half': the last two objects are virtual on every
    second clip (SURVEY 8d's input variant of the bench batch)."""
    g = torch.Generator().manual_seed(seed)
    vis = torch.relu(torch.randn(bs, T, H, 2048, generator=g))
    pos = torch.rand(bs, T, N, 2, generator=g)
    vel = torch.randn(bs, T, N, 2, generator=g) * 0.5
    geo = torch.cat([pos, vel], -1).reshape(bs, T, 1, 4 * N).expand(bs, T, H, 4 * N)
    x_human = torch.cat([vis, geo], -1).contiguous()
    x_objects = torch.relu(torch.randn(bs, T, O, 2048, generator=g))
    mask = torch.ones(bs, O)
    if virtual == 'half':
        mask[1::2, O - 2:] = 0.0
    elif bs > 1:
        mask[1, O - 2:] = 0.0
    x_objects = x_objects * mask[:, None, :, None]
    return x_human, x_objects, mask


GRAD_REL, GRAD_ABS = 5e-4, 5e-6      # the hard gate on every parameter gradient (of the tensor's scale, against the oracle)
MAX_YARDSTICK_TENSORS = 4            # tensors that may fall back on the fp64 yardstick (ill-conditioned, see below)
# conditioning bounds (tests/relu_boundary.py::condition_case): the ReLU activations (unit x row) found inside the rounding
# band of their own dot product -- what the bias nudges clear -- are at most 5e-5 of the activations the helper covers
# (measured: 1.1e-5 at configs[1] full size, 327 of 3.0e7), and the nudges touch at most a tenth of the distinct units
# (layer outputs; a unit is nudged when ANY of its 10^3 ... 10^5 rows sits in the band)
MAX_BOUNDARY_ACTIVATION_SHARE = 5e-5
MAX_NUDGED_UNIT_SHARE = 0.10
_RECORDS = []


def _record(**kw):
    """One line per full-path comparison in gpurun_out/parity_oracle_vs_hip.jsonl (what was nudged, what was measured)."""
    import json
    import os
    _RECORDS.append(kw)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    try:
        os.makedirs(os.path.join(root, 'gpurun_out'), exist_ok=True)
        with open(os.path.join(root, 'gpurun_out', 'parity_oracle_vs_hip.jsonl'), 'a') as f:
            f.write(json.dumps(kw) + '\n')
    except OSError:
        pass


def _grad_errors(m, osd):
    """Per parameter tensor (name, error / scale, scale, inside the 5e-4 gate) of the HIP gradients against the oracle's."""
    rows = []
    for pname, p in m.named_parameters():
        g_ref = osd[pname].grad
        if g_ref is None or p.grad is None:
            continue
        scale = max(g_ref.abs().max().item(), 1e-6)
        err = (p.grad.cpu() - g_ref).abs().max().item()
        rows.append((pname, err / scale, scale, err < GRAD_REL * scale + GRAD_ABS))
    return rows


def _raw_deviation(m, fwd, x_human, x_objects, mask, kw, noise, buffers, rs_of):
    """what the UN-conditioned case deviates by. The same comparison as the gate below, run once on the
    weights as drawn (before tests/relu_boundary.py moves any bias): per tensor the gradient error against the oracle; for
    every tensor beyond 5e-4 of its scale, whether the fp64 yardstick (HIP no further from the fp64 oracle than 3 x the
    fp32 oracle itself) explains it. Returns the record; the caller decides (a tensor beyond BOTH gates is only tolerated
    in a case where the conditioning then finds and confirms ReLU boundary units)."""
    f64 = torch.float64
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    osd = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and 'running' not in k else v.clone()) for k, v in sd.items()}
    ref = cpu_ref.tggcn_forward(osd, dict(m.cfg), x_human, x_objects, mask, training=True, gumbel_noise=noise, **kw)
    out = fwd()
    rs = rs_of(ref)
    sum((o * r).sum() for o, r in zip(ref, rs) if o.requires_grad).backward()
    m.zero_grad(set_to_none=True)
    sum((o * r.to(DEV)).sum() for o, r in zip(out, rs) if o.requires_grad).backward()
    rows = _grad_errors(m, osd)
    hard_equal = all(torch.equal(o.detach().cpu(), r.detach()) for o, r in list(zip(out, ref))[:1])
    beyond = [(n, e, sc) for n, e, sc, ok in rows if not ok]
    explained = {}
    if beyond:
        osd64 = {k: (v.detach().to(f64).requires_grad_(True) if v.is_floating_point() and 'running' not in k
                     else (v.detach().to(f64) if v.is_floating_point() else v.clone())) for k, v in sd.items()}
        ref64 = cpu_ref.tggcn_forward(osd64, dict(m.cfg), x_human.to(f64), x_objects.to(f64), mask.to(f64), training=True,
                                      gumbel_noise=None if noise is None else noise.to(f64),
                                      **{k: v.to(f64) for k, v in kw.items()})
        sum((o * r.to(f64)).sum() for o, r in zip(ref64, rs) if o.requires_grad).backward()
        P = dict(m.named_parameters())
        for n, e, sc in beyond:
            g64 = osd64[n].grad
            own = (osd[n].grad.to(f64) - g64).abs().max().item()
            err64 = (P[n].grad.cpu().to(f64) - g64).abs().max().item()
            explained[n] = bool(err64 <= 3.0 * own + 2e-5 * sc)
    m.zero_grad(set_to_none=True)
    m.load_state_dict(buffers, strict=False)   # the train-mode forward moved the BatchNorm running statistics
    return dict(raw_worst_grad_rel=max((e for _, e, _, _ in rows), default=0.0),
                raw_tensors_beyond_5e4=[(n, float(f'{e:.3e}'), explained[n]) for n, e, _ in beyond],
                raw_tensors_beyond_both_gates=[n for n, _, _ in beyond if not explained[n]],
                raw_hard_gates_equal=bool(hard_equal), raw_tensors_compared=len(rows))


def _oracle_vs_hip(bs, T, H, O, N, h, backward, seed=3, n_sub=13, n_aff=None, both_given=False, virtual='clip1',
                   max_nudged_share=0.04, max_rounds=8):
    """The full path on the HIP kernels against the CPU oracle on the same weights, inputs and noise: every output at
    1e-4, every parameter gradient at 5e-4 of its scale -- no escape clause.

    A ReLU unit whose pre-activation is below the rounding error of its own dot product would land on different sides of
    zero in the two implementations (different summation orders) and move its row of the gradient by percents. Such
    units exist in most full-size cases, so the CASE is moved off them first (tests/relu_boundary.py::condition_case
    nudges the bias of every such unit by a few band widths and re-checks; the nudged weights feed both sides). What
    remains beyond 5e-4 can only be conditioning (BatchNorm over few frames in front of the GCN parameters: both fp32
    implementations then sit ~1e-3 from the exact gradient): such a tensor must be no further from the oracle run in
    fp64 than three times the fp32 oracle itself is (+ 2e-5 of its scale), and at most MAX_YARDSTICK_TENSORS may need
    that."""
    from tests.relu_boundary import condition_case
    cfg = dict(STAGE1)
    if H == 1:
        cfg['message_humans_to_human'] = False
    torch.manual_seed(seed)
    m = TGGCN(input_size=(2048 + 4 * N, 2048), num_classes=(n_sub, n_aff), hidden_size=h, gcn_node=N, **cfg)
    buffers = {k: v.detach().clone() for k, v in m.state_dict().items() if 'running_' in k or 'num_batches' in k}
    x_human, x_objects, mask = _synthetic(bs, T, H, O, N, seed, virtual)
    g = torch.Generator().manual_seed(seed + 100)
    if both_given:   # CAD-120 semantics: both segmentations come from the annotation (vhoi/data_loading.py:1254-1256)
        kw = dict(human_segmentation=(torch.rand(bs, T, H, generator=g) < 0.3).float(),
                  objects_segmentation=(torch.rand(bs, T, O, generator=g) < 0.3).float())
        noise = None
    else:
        kw = dict(human_segmentation=torch.ones(bs, T, H))
        noise = torch.distributions.gumbel.Gumbel(0.0, 1.0).sample((T * O, bs, 2))
    m = m.to(DEV).train()
    m._gumbel_noise_override = noise
    dkw = {k: v.to(DEV) for k, v in kw.items()}
    xh_d, xo_d, mask_d = x_human.to(DEV), x_objects.to(DEV), mask.to(DEV)

    def fwd():
        return m(xh_d, xo_d, mask_d, **dkw)

    def rs_of(outs):
        return [torch.randn(o.shape, generator=torch.Generator().manual_seed(i)) for i, o in enumerate(outs)]

    raw = _raw_deviation(m, fwd, x_human, x_objects, mask, kw, noise, buffers, rs_of) if backward else None
    rounds, nudged = condition_case(m, fwd, max_rounds=max_rounds) if backward else (0, {})
    from tests import relu_boundary as _rb
    totals = dict(_rb.LAST_TOTALS)
    if backward and totals['units']:
        n_nudged = sum(nudged.values())
        assert n_nudged <= max(MAX_NUDGED_UNIT_SHARE, max_nudged_share) * totals['units'], ('too many ReLU units nudged', nudged, totals)
        # per shape class: 1 % at the configs[2] shapes, 4 % at configs[0] / [1], 10 % at configs[4]
        assert n_nudged <= max_nudged_share * totals['units'], ('nudged share above the bound of this shape class', n_nudged,
                                                                 totals['units'], max_nudged_share)
    if backward and raw['raw_tensors_beyond_both_gates']:
        # a raw tensor beyond BOTH gates is tolerated only where the conditioning found (and confirmed, by re-checking after the
        # nudge) ReLU units inside their rounding band: those are what moves a gradient row by percents between two summation
        # orders. Without a single such unit in the case there is nothing to blame but the kernels.
        assert sum(nudged.values()) > 0, ('un-conditioned gradients beyond 5e-4 AND beyond the fp64 yardstick, and no ReLU '
                                          'boundary unit in the case', raw)
        assert totals['boundary_activations'] <= max(8, MAX_BOUNDARY_ACTIVATION_SHARE * totals['activations']), (nudged, totals)
    m.load_state_dict(buffers, strict=False)   # the conditioning passes moved the BatchNorm running statistics
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    # oracle (CPU)
    osd = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and 'running' not in k else v.clone())
           for k, v in sd.items()}
    ref = cpu_ref.tggcn_forward(osd, dict(m.cfg), x_human, x_objects, mask, training=True, gumbel_noise=noise, **kw)
    # HIP
    out = fwd()
    assert len(out) == len(ref) == (12 if n_aff is not None else 6)
    worst_out = 0.0
    for i, (o, r) in enumerate(zip(out, ref)):
        got, want = o.detach().cpu(), r.detach()
        assert got.shape == want.shape
        err = (got - want).abs().max().item() / max(1.0, want.abs().max().item())
        worst_out = max(worst_out, err)
        assert err < REL, (i, err)
    if not backward:
        return
    rs = rs_of(ref)
    sum((o * r).sum() for o, r in zip(ref, rs) if o.requires_grad).backward()
    m.zero_grad(set_to_none=True)
    sum((o * r.to(DEV)).sum() for o, r in zip(out, rs) if o.requires_grad).backward()
    worst, worst_rel_only, off, abs_only = 0.0, 0.0, [], []
    for pname, p in m.named_parameters():
        g_ref = osd[pname].grad
        if g_ref is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, pname
            continue
        assert p.grad is not None, pname
        scale = max(g_ref.abs().max().item(), 1e-6)
        err = (p.grad.cpu() - g_ref).abs().max().item()
        if err < GRAD_REL * scale + GRAD_ABS:
            worst = max(worst, err / scale)
            if err >= GRAD_REL * scale:   # inside the gate only through its absolute floor: named in the record
                abs_only.append((pname, err / scale, scale))
            else:
                worst_rel_only = max(worst_rel_only, err / scale)
        else:
            off.append((pname, err / scale))
    yard = []
    if off:
        assert len(off) <= MAX_YARDSTICK_TENSORS, ('gradients beyond 5e-4 of their scale', sorted(off, key=lambda t: -t[1])[:8])
        f64 = torch.float64
        osd64 = {k: (v.detach().to(f64).requires_grad_(True) if v.is_floating_point() and 'running' not in k
                     else (v.detach().to(f64) if v.is_floating_point() else v.clone())) for k, v in sd.items()}
        ref64 = cpu_ref.tggcn_forward(osd64, dict(m.cfg), x_human.to(f64), x_objects.to(f64), mask.to(f64), training=True,
                                      gumbel_noise=None if noise is None else noise.to(f64),
                                      **{k: v.to(f64) for k, v in kw.items()})
        n_hard = 2 if n_aff is not None else 1
        assert all(torch.equal(ref64[i].float(), ref[i].detach()) for i in range(n_hard)), 'hard gates differ in fp64'
        sum((o * r.to(f64)).sum() for o, r in zip(ref64, rs) if o.requires_grad).backward()
        for pname, e in off:
            g64, g32 = osd64[pname].grad, osd[pname].grad
            scale = max(g32.abs().max().item(), 1e-6)
            own = (g32.to(f64) - g64).abs().max().item()
            err64 = (dict(m.named_parameters())[pname].grad.cpu().to(f64) - g64).abs().max().item()
            yard.append((pname, e, err64 / scale, own / scale))
            assert err64 <= 3.0 * own + 2e-5 * scale, ('beyond the fp64 yardstick', pname, e, err64 / scale, own / scale)
    print(f'worst output {worst_out:.2e}; worst gradient within 5e-4: {worst:.2e}; judged by the fp64 yardstick: '
          f'{[(n, f"{e:.1e}", f"hip-fp64 {a:.1e}", f"oracle32-fp64 {b:.1e}") for n, e, a, b in yard]}; '
          f'ReLU-boundary units nudged in {rounds} round(s): {nudged}; UN-conditioned case: worst gradient '
          f'{raw["raw_worst_grad_rel"]:.2e}, beyond 5e-4: {raw["raw_tensors_beyond_5e4"]}')
    _record(case=dict(bs=bs, T=T, H=H, O=O, N=N, h=h, seed=seed, n_aff=n_aff, both_given=both_given, virtual=virtual),
            worst_output_rel=worst_out, worst_grad_rel_within_tolerance=worst, tensors_on_fp64_yardstick=yard,
            tensors_within_the_gate_only_by_its_absolute_floor=[(n, float(f'{e:.3e}'), float(f'{sc:.3e}')) for n, e, sc in abs_only],
            worst_grad_rel_by_the_relative_term_alone=worst_rel_only,
            conditioning_rounds=rounds, relu_units_nudged=nudged, relu_units_covered=totals.get('units'),
            relu_activations_covered=totals.get('activations'),
            relu_activations_in_the_rounding_band=totals.get('boundary_activations'),
            relu_units_nudged_share=(sum(nudged.values()) / totals['units']) if totals.get('units') else 0.0,
            nudged_share_bound_of_the_shape_class=max_nudged_share, unconditioned=raw,
            gemm_x3=os.environ.get('TWOG_GEMM_X3', '1'))


def test_oracle_parity_c3_layout_reduced_width():
    """Synthetic layout of BASELINE configs[2] (H=2, O=8, N=34) at h=64, T=16: forward + backward vs the oracle."""
    _oracle_vs_hip(bs=3, T=16, H=2, O=8, N=34, h=64, backward=True, max_nudged_share=0.01)


def test_oracle_parity_c2_layout_hs128():
    _oracle_vs_hip(bs=2, T=10, H=2, O=4, N=26, h=128, backward=True, seed=5)


def test_oracle_parity_full_width_forward_backward():
    """BASELINE shape of the metric (configs[2]): T=120, N=34, h=512, forward AND backward -- a 120-step BPTT through the
    fused gate-epilogue chains and the split-K weight gradients, every parameter gradient against the oracle (one clip
    pair; the oracle needs a few minutes on the host cores)."""
    _oracle_vs_hip(bs=2, T=120, H=2, O=8, N=34, h=512, backward=True, seed=7, max_nudged_share=0.01)


@pytest.mark.parametrize('shape', [dict(bs=3, T=6, H=2, O=4, N=26, h=64), dict(bs=64, T=3, H=2, O=8, N=34, h=512),
                                   dict(bs=8, T=6, H=2, O=4, N=26, h=512)])
def test_deferred_gradient_launches_see_unchanged_operands(shape, monkeypatch):
    """ops._Grads defers the weight-gradient GEMMs, column sums, copies and additions of a backward stage until
    flush(); TWOG_VERIFY_DEFERRED=1 snapshots every deferred operand and compares it when the launch is issued. Runs the
    small-batch grouping (at most 8 192 rows), the held tall dW with its fused column sums (64 clips) and the persistent
    small-batch path on the device; the comparison against the oracle runs as usual."""
    monkeypatch.setenv('TWOG_VERIFY_DEFERRED', '1')
    _oracle_vs_hip(backward=True, seed=41, **shape)


def test_oracle_parity_bench_batch_short_clips():
    """The bench's batch (64 clips of the configs[2] layout, h = 512) at T = 3: every launch has the bench's tile counts, so
    the variants the tile-count policies pick only there -- the fused frame-level GRU step (22 row tiles x 8 unit tiles),
    the 128x128 class with split-K for the weight gradients, the grouped tile order -- run against the oracle, forward and
    backward."""
    _oracle_vs_hip(bs=64, T=3, H=2, O=8, N=34, h=512, backward=True, seed=11, max_nudged_share=0.01)


def test_oracle_parity_bench_batch_virtual_objects_on_half_the_clips():
    """SURVEY 8d's input variant at the bench batch: the last two objects are virtual on every second clip (masked
    senders and receivers inside every attention instance, masked gate rows), T = 3, forward and backward."""
    _oracle_vs_hip(bs=64, T=3, H=2, O=8, N=34, h=512, backward=True, seed=23, virtual='half', max_nudged_share=0.01)


def test_oracle_parity_c1_full_width():
    """BASELINE configs[0] (CAD-120) at full width on the GPU: one human, five objects, N = 19, h = 512, classes
    (10, 12) -> the 12-output order with the object heads, BOTH segmentations given (no gate is learned, no noise;
    vhoi/models.py:631-633, :909-926), T = 120, forward and backward."""
    _oracle_vs_hip(bs=2, T=120, H=1, O=5, N=19, h=512, backward=True, seed=21, n_sub=10, n_aff=12, both_given=True)


def test_oracle_parity_streaming_attention_kernels():
    """More than 1 024 (clip, frame) instances with ten entities each (9 clips x 120 frames, H=2, O=8): the frame-level
    attention runs its throughput-regime kernels -- column-parallel Gram forward, column-parallel dL/dw backward --
    inside the full path, forward and backward against the oracle (h=64 keeps the oracle at a minute)."""
    _oracle_vs_hip(bs=9, T=120, H=2, O=8, N=34, h=64, backward=True, seed=17)


def test_oracle_parity_streaming_attention_kernels_six_entities():
    """The same regime at the MPHOI layout (H=2, O=4): the 16-slot variant of the column-parallel Gram."""
    _oracle_vs_hip(bs=9, T=120, H=2, O=4, N=26, h=64, backward=True, seed=19)


def test_oracle_parity_c2_full_size():
    """BASELINE configs[1] at size: MPHOI layout (H=2, O=4, N=26), hs512, bs8, T=120, forward + backward."""
    _oracle_vs_hip(bs=8, T=120, H=2, O=4, N=26, h=512, backward=True, seed=9)


def test_oracle_parity_c5_full_size():
    """BASELINE configs[4] per-GPU shard at size: Bimanual layout (H=2, O=9, N=30), h=64, 16 clips, T=120."""
    _oracle_vs_hip(bs=16, T=120, H=2, O=9, N=30, h=64, backward=True, seed=13, n_sub=14, max_nudged_share=0.10)


def test_oracle_parity_c5_hs512():
    """The Bimanual layout at h = 512 ("also run h=512"; vhoi/data_loading.py:653-766 for
    the layout, conf/models/2G-GCN_stage1.yaml:15-17 for the width): 16 clips, H=2, O=9, N=30, T=120, forward + backward.
    Two human row tiles per chunk: the persistent segment launch does not serve it (csrc/seg_persist.hip::make_plan), so
    this is the launch-per-step segment recurrence at 144 object rows beside the persistent frame-level one."""
    from twog_gcn_amd import kernels
    # (21 120 entity rows through 512-unit layers: ~100 activations per layer lie within rounding of zero, and every nudge
    # upstream re-draws the sets downstream -- the conditioning needs more rounds here than at 8 clips, and moves a larger
    # share of the units; both are recorded in profiles/*_parity_oracle_vs_hip.jsonl)
    _oracle_vs_hip(bs=16, T=120, H=2, O=9, N=30, h=512, backward=True, seed=17, n_sub=14, max_nudged_share=0.20, max_rounds=24)
    K = kernels.get_kernels()
    assert not K.last_segrnn_persistent and not K.last_segrnn_bwd_persistent


def test_oracle_parity_at_bench_size():
    """The ONE shape the headline number is quoted on -- 64 clips x T = 120 x h = 512, N = 34 (BASELINE configs[2]) -- against
    the oracle. Eval mode: BatchNorm uses its running statistics, so clips are independent and the oracle can run clips
    {0, 31, 63} one at a time (a few seconds each) while the HIP path runs the whole batch with the bench's tile counts,
    split-K choices and time loops. Every output of those clips at 1e-4; hard gates exact. Gumbel noise is drawn in eval
    mode too (Appendix A7): the same pre-drawn tensor feeds both sides."""
    bs, T, H, O, N, h = 64, 120, 2, 8, 34, 512
    torch.manual_seed(31)
    m = TGGCN(input_size=(2048 + 4 * N, 2048), num_classes=(13, None), hidden_size=h, gcn_node=N, **STAGE1)
    bn = m.geometry_embedding_gcn.joint_embed.cnn[0].bn
    with torch.no_grad():   # non-trivial running statistics (a trained model's), fixed
        bn.running_mean.copy_(torch.rand(4 * N, generator=torch.Generator().manual_seed(1)) * 0.6)
        bn.running_var.copy_(0.05 + torch.rand(4 * N, generator=torch.Generator().manual_seed(2)))
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x_human, x_objects, mask = _synthetic(bs, T, H, O, N, seed=29, virtual='half')
    seg = torch.ones(bs, T, H)
    noise = torch.distributions.gumbel.Gumbel(0.0, 1.0).sample((T * O, bs, 2))
    m = m.to(DEV).eval()
    m._gumbel_noise_override = noise
    with torch.no_grad():
        out = m(x_human.to(DEV), x_objects.to(DEV), mask.to(DEV), human_segmentation=seg.to(DEV))
    out = [o.cpu() for o in out]
    worst = 0.0
    for c in (0, 31, 63):
        sl = slice(c, c + 1)
        with torch.no_grad():
            ref = cpu_ref.tggcn_forward(sd, dict(m.cfg), x_human[sl], x_objects[sl], mask[sl], training=False,
                                        gumbel_noise=noise[:, sl], human_segmentation=seg[sl])
        assert len(ref) == len(out) == 6
        assert torch.equal(out[0][sl], ref[0]), ('hard gates', c)
        for i, (o, r) in enumerate(zip(out, ref)):
            err = (o[sl] - r).abs().max().item() / max(1.0, r.abs().max().item())
            worst = max(worst, err)
            assert err < REL, (c, i, err)
    print(f'bench size (64 x 120 x 512), clips 0 / 31 / 63 against the oracle: worst output deviation {worst:.2e}')
    _record(case=dict(bs=bs, T=T, H=H, O=O, N=N, h=h, mode='eval, clips 0/31/63 against the oracle one at a time'),
            worst_output_rel=worst)


def test_seeded_default_generator_noise_reproduces_the_reference_without_an_override():
    """Appendix A7 end to end: with NO noise override the model draws its Gumbel noise from torch's CPU default generator
    in one (T n, bs, 2) call -- under torch.manual_seed(42), the seed the golden run used (tools/make_golden.py), that is
    bit for bit what the reference drew call by call, so the golden outputs must come out (stage-1: object gates learned;
    stage-2: human and object gates learned, local-maximum filter)."""
    for name in ('c2_stage1', 'c2_stage2', 'c5_stage1'):
        z, meta = load_g4(name)
        m = _model_from_meta(meta).train()
        assert m._gumbel_noise_override is None
        kw = {k: v.to(DEV) for k, v in g4_inputs(z).items()}
        torch.manual_seed(42)
        out = m(**kw)
        n_out = len([k for k in z.files if k.startswith('out')])
        for i, o in enumerate(out):
            ref = z[f'out{i}']
            got = o.detach().cpu().numpy()
            if ref.ndim == 3 and np.all((ref == 0) | (ref == 1)) and i < n_out - 4:
                assert np.array_equal(got, ref), (name, i)
            else:
                assert np.abs(got - ref).max() < REL * max(1.0, np.abs(ref).max()), (name, i)


def test_full_path_parity_on_the_native_fp32_mfma_kernels():
    """TWOG_GEMM_X3=0 -- the switch INTEGRATION.md offers for fp32 MFMA arithmetic throughout -- on the full path, not only
    at GEMM level: the reduced-width configs[2] layout and configs[1] at size against the oracle, forward and backward,
    in a child process (the switch is read once per process)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ids = ['tests/test_parity_gpu.py::test_oracle_parity_c3_layout_reduced_width',
           'tests/test_parity_gpu.py::test_oracle_parity_c2_full_size']
    r = subprocess.run([sys.executable, '-m', 'pytest', '-x', '-q', '-m', 'gpu', '-p', 'no:cacheprovider'] + ids, cwd=root,
                       env=dict(os.environ, TWOG_GEMM_X3='0'), capture_output=True, text=True, timeout=3000)
    assert r.returncode == 0 and '2 passed' in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_full_size_determinism_and_batch_independence():
    """bench-size properties (the bench's own 64 clips): two identical steps are bit-identical (split-K and all reductions
    are ordered); in eval mode a clip's outputs do not depend on the other clips of the batch."""
    bs, T, H, O, N, h = 64, 120, 2, 8, 34, 512
    torch.manual_seed(0)
    m = TGGCN(input_size=(2048 + 4 * N, 2048), num_classes=(13, None), hidden_size=h, gcn_node=N, **STAGE1).to(DEV)
    x_human, x_objects, mask = (t.to(DEV) for t in _synthetic(bs, T, H, O, N, 1))
    seg = torch.ones(bs, T, H, device=DEV)
    noise = torch.distributions.gumbel.Gumbel(0.0, 1.0).sample((T * O, bs, 2))
    m._gumbel_noise_override = noise
    m.train()
    runs = []
    for _ in range(2):
        m.zero_grad(set_to_none=True)
        bn = m.geometry_embedding_gcn.joint_embed.cnn[0].bn
        bn.running_mean.zero_(); bn.running_var.fill_(1.0)
        out = m(x_human, x_objects, mask, human_segmentation=seg)
        (out[4].sum() + out[5].sum() + out[1].sum()).backward()
        runs.append(([o.detach().clone() for o in out], {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a, b)
    for n in runs[0][1]:
        assert torch.equal(runs[0][1][n], runs[1][1][n]), n
    assert all(torch.isfinite(g).all() for g in runs[0][1].values())
    m.eval()
    with torch.no_grad():
        full = m(x_human, x_objects, mask, human_segmentation=seg)
        m._gumbel_noise_override = noise[:, 3:5]
        part = m(x_human[3:5], x_objects[3:5], mask[3:5], human_segmentation=seg[3:5])
    for a, b in zip(full[1:], part[1:]):
        err = (a[3:5] - b).abs().max().item()
        assert err < REL * max(1.0, b.abs().max().item()), err


def test_graph_replay_path_matches_direct_launches(monkeypatch):
    """The opt-in hipGraph path of the four time loops (TWOG_GRAPHS=1: first sighting direct, then capture, then replays)
    gives bit for bit what the default direct launches give, forward and backward, step after step. (The launch-per-step
    loops are what is captured: the persistent launches that would serve this small batch are switched off.)"""
    monkeypatch.setenv('TWOG_BIGRU_PERSIST', '0')
    monkeypatch.setenv('TWOG_SEG_PERSIST', '0')
    bs, T, H, O, N, h = 4, 12, 2, 4, 26, 64
    torch.manual_seed(2)
    m = TGGCN(input_size=(2048 + 4 * N, 2048), num_classes=(13, None), hidden_size=h, gcn_node=N, **STAGE1).to(DEV).train()
    x_human, x_objects, mask = (t.to(DEV) for t in _synthetic(bs, T, H, O, N, 4))
    seg = torch.ones(bs, T, H, device=DEV)
    m._gumbel_noise_override = torch.distributions.gumbel.Gumbel(0.0, 1.0).sample((T * O, bs, 2))
    bn = m.geometry_embedding_gcn.joint_embed.cnn[0].bn
    stats0 = twog_kernels.get_kernels().graph_cache_stats()[0]

    def step(check=None):
        m.zero_grad(set_to_none=True)
        bn.running_mean.zero_(); bn.running_var.fill_(1.0)
        out = m(x_human, x_objects, mask, human_segmentation=seg)
        (out[4].sum() + out[5].sum() + out[1].sum()).backward()
        if check is None:
            return [o.detach().clone() for o in out], {n_: p.grad.clone() for n_, p in m.named_parameters() if p.grad is not None}
        # compared in place: no allocation that outlives the step, so every step sees the same buffer addresses -- the
        # steady state of a training loop, and what the capture-on-second-sighting rule keys on
        for a, b in zip(out, check[0]):
            assert torch.equal(a.detach(), b)
        for n_, g in check[1].items():
            assert torch.equal(dict(m.named_parameters())[n_].grad, g), n_
        return None

    direct = step()
    assert twog_kernels.get_kernels().graph_cache_stats()[0] == stats0
    monkeypatch.setenv('TWOG_GRAPHS', '1')
    for _ in range(5):
        step(direct)
    assert twog_kernels.get_kernels().graph_cache_stats()[0] > stats0, 'no loop was captured'


# ------------------------------------------------------------------------------------------------- edge cases
@pytest.mark.parametrize('bs,T,H,O,N,h,mask_mode', [
    (1, 1, 2, 4, 26, 32, 'all'),        # single clip, single frame (chain start == chain end, forced last gate)
    (2, 3, 1, 5, 19, 32, 'none_real'),  # CAD-120 layout (H=1, no human-human relation), every object virtual
    (2, 4, 2, 12, 34, 16, 'ragged'),    # maximum supported object count, ragged object sets
])
def test_edge_cases_vs_oracle(bs, T, H, O, N, h, mask_mode):
    cfg = dict(STAGE1)
    if H == 1:
        cfg['message_humans_to_human'] = False
    torch.manual_seed(11)
    n_aff = 12 if H == 1 else None
    m = TGGCN(input_size=(2048 + 4 * N, 2048), num_classes=(10 if H == 1 else 13, n_aff), hidden_size=h, gcn_node=N, **cfg)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(5)
    x_human = torch.rand(bs, T, H, 2048 + 4 * N, generator=g)
    x_objects = torch.rand(bs, T, O, 2048, generator=g)
    mask = torch.ones(bs, O)
    if mask_mode == 'none_real':
        mask.zero_()
    elif mask_mode == 'ragged':
        mask[0, 3:] = 0
        mask[1, 7:] = 0
    x_objects = x_objects * mask[:, None, :, None]
    n_gated = H + O
    noise = torch.distributions.gumbel.Gumbel(0.0, 1.0).sample((T * n_gated, bs, 2))
    ref = cpu_ref.tggcn_forward(sd, dict(m.cfg), x_human, x_objects, mask, training=True, gumbel_noise=noise)
    m = m.to(DEV).train()
    m._gumbel_noise_override = noise
    out = m(x_human.to(DEV), x_objects.to(DEV), mask.to(DEV))
    assert len(out) == len(ref) == (12 if n_aff else 6)
    for i, (o, r) in enumerate(zip(out, ref)):
        got, want = o.detach().cpu(), r.detach()
        assert got.shape == want.shape
        assert not torch.isnan(got).any(), i
        assert (got - want).abs().max().item() < REL * max(1.0, want.abs().max().item()), i
    sum(o.sum() for o in out if o.requires_grad).backward()
    assert all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)


@pytest.mark.parametrize('H,O,N', [(2, 14, 40), (5, 3, 34), (3, 16, 50)])
def test_more_entities_than_the_tuned_attention_kernel_holds(H, O, N):
    """Round 6: the tuned four-relations kernel keeps at most 4 humans and 12 objects in registers
    (csrc/attn.hip:22; the reference has no such limit, its datasets at most 2 and 9). Larger clips are routed to the general
    single-relation kernels (up to 16 receivers / senders per relation, both levels) instead of raising: forward + backward
    against the oracle."""
    _oracle_vs_hip(bs=2, T=5, H=H, O=O, N=N, h=32, backward=True, seed=19, max_nudged_share=0.10)


def _watch_the_message_kernels(monkeypatch):
    """Counts the calls that reach the general single-relation kernels and collects the code path of every host-issued
    attention backward launch (HipKernels.attn_last_path)."""
    from twog_gcn_amd.kernels import HipKernels
    seen = dict(general=0, attn_bwd_paths=[])
    for name in ('relation_fwd', 'relation_fwd_many', 'relation_bwd', 'relation_bwd_many'):
        def counting(self, *a, _f=getattr(HipKernels, name), **kw):
            seen['general'] += 1
            return _f(self, *a, **kw)
        monkeypatch.setattr(HipKernels, name, counting)

    def attn_bwd(self, descs, _f=HipKernels.attn_bwd):
        _f(self, descs)
        seen['attn_bwd_paths'].append(self.attn_last_path())
    monkeypatch.setattr(HipKernels, 'attn_bwd', attn_bwd)
    return seen


@pytest.mark.parametrize('H,O,N,h', [(3, 10, 40, 32), (4, 12, 50, 32), (4, 2, 34, 64)])
def test_as_many_entities_as_the_tuned_attention_kernel_holds(H, O, N, h, monkeypatch):
    """The complement of the test above: 3 and 4 humans, up to 12 objects -- the clips the host routes to the TUNED kernels
    (attn.hip, ssp.hip, segrnn.hip; at h = 64 the persistent segment launch) -- forward + backward against the oracle, at
    the tolerances and the nudged-unit share of the test above; no call may reach the general single-relation kernels."""
    seen = _watch_the_message_kernels(monkeypatch)
    _oracle_vs_hip(bs=2, T=5, H=H, O=O, N=N, h=h, backward=True, seed=19, max_nudged_share=0.10)
    assert seen['general'] == 0, 'a clip within the tuned range ran on the general single-relation kernels'
    assert seen['attn_bwd_paths'], 'the tuned attention backward kernel did not run'


def test_4_humans_and_12_objects_at_full_width_take_the_unstaged_attention_backward(monkeypatch):
    """(4, 12) at h = 512: the rows the frame-level attention backward would stage (82 rows of 516 floats) exceed the 160 KB
    of LDS, so the launch falls back to the unstaged 256-thread form at 3 instances -- reached through the model here."""
    from twog_gcn_amd.kernels import HipKernels as HK
    seen = _watch_the_message_kernels(monkeypatch)
    _oracle_vs_hip(bs=1, T=3, H=4, O=12, N=50, h=512, backward=True, seed=19, max_nudged_share=0.10)
    assert seen['general'] == 0
    want = HK.ATTN_BACKWARD | 256 << HK.ATTN_THREADS_SHIFT
    assert want in seen['attn_bwd_paths'], [hex(p) for p in seen['attn_bwd_paths']]


def test_limits_fail_loudly():
    """More entities than ANY kernel of the path supports must raise, not silently fall back."""
    N, h, O = 26, 16, 17
    m = TGGCN(input_size=(2048 + 4 * N, 2048), num_classes=(13, None), hidden_size=h, gcn_node=N, **STAGE1).to(DEV)
    with pytest.raises(RuntimeError):
        m(torch.rand(1, 2, 2, 2048 + 4 * N, device=DEV), torch.rand(1, 2, O, 2048, device=DEV), torch.ones(1, O, device=DEV),
          human_segmentation=torch.ones(1, 2, 2, device=DEV))
    with pytest.raises(ValueError):  # feature width inconsistent with gcn_node
        m(torch.rand(1, 2, 2, 2048 + 4 * 19, device=DEV), torch.rand(1, 2, 4, 2048, device=DEV), torch.ones(1, 4, device=DEV))


def test_randomised_layouts_vs_oracle():
    """Random layouts (clips, frames, humans, objects, nodes, width, masks), gate semantics (given / learned
    segmentation, local-maximum filter), message switches, train / eval: HIP vs oracle, outputs 1e-4, gradients 5e-4."""
    import random
    from tools.parity_fuzz import one_case
    rng = random.Random(0)
    worst_o = worst_g = 0.0
    for i in range(30):
        d = one_case(rng, i, dev=DEV)
        worst_o, worst_g = max(worst_o, d['worst_output_rel']), max(worst_g, d['worst_grad_rel'])
        # a gradient deviation is accepted only with a ReLU unit CONFIRMED on the rounding boundary by the fp64 recompute
        # of tests/relu_boundary.py (one_case raises otherwise), and always against the fp64 oracle run
        assert d.get('relu_boundary_confirmed', True) and d.get('grad_ref', 'fp64|fp32') in ('fp64|fp32', 'none', 'not judged'), d
    print(f'30 random cases: worst output {worst_o:.2e}, worst gradient {worst_g:.2e}')


GENERAL_FORMS = {
    'relational': dict(message_type='v1'),
    'specific': dict(message_granularity='v2'),
    'concat': dict(attention_style='v1'),
    'bilinear': dict(attention_style='v4'),
    'specific_concat': dict(message_granularity='v2', attention_style='v1'),
    'specific_mean_pool': dict(message_granularity='v2', message_aggregation='mp'),
    'distance': dict(),
    'constructor_defaults': None,
}


@pytest.mark.parametrize('form', sorted(GENERAL_FORMS))
def test_general_segment_loop_replayed_by_the_library_equals_the_composed_loop_and_the_oracle(form, monkeypatch):
    """The general segment-level loop (relational / receiver-specific messages, concat / bilinear / distance attention)
    composes its first steps on the host and lets the library replay the rest (twog_tape_run: every descriptor word
    affine in the step index). At T = 12: (a) the replayed loop's outputs and parameter gradients are BIT-IDENTICAL to
    the loop composed step by step (TWOG_GENERAL_TAPE=0) -- the same launches with the same arguments; (b) both agree
    with the oracle (outputs 1e-4, gradients 5e-4 of their scale + 5e-6)."""
    bs, T, H, O, N, h = 3, 12, 2, 3, 26, 32
    over = GENERAL_FORMS[form]
    cfg = dict(message_segment=True) if over is None else dict(STAGE1, **over)
    torch.manual_seed(77)
    m = TGGCN(input_size=(2048 + 4 * N, 2048), num_classes=(13, None), hidden_size=h, gcn_node=N, **cfg)
    assert m_plan_is_general(m, bs, T, H, O, N, form == 'distance')
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x_human, x_objects, mask = _synthetic(bs, T, H, O, N, seed=5)
    g = torch.Generator().manual_seed(9)
    kw = dict(human_segmentation=(torch.rand(bs, T, H, generator=g) < 0.6).float())
    if form == 'distance':
        def dd(*shape):
            d = torch.rand(*shape, generator=g) * 2 + 0.05
            d[torch.rand(*shape, generator=g) < 0.15] = 0.0
            return d
        kw.update(human_human_distances=dd(bs, T, H, H), human_object_distances=dd(bs, T, H, O),
                  object_object_distances=dd(bs, T, O, O))
    noise = torch.distributions.gumbel.Gumbel(0.0, 1.0).sample((T * O, bs, 2))
    osd = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and 'running' not in k else v.clone())
           for k, v in sd.items()}
    ref = cpu_ref.tggcn_forward(osd, dict(m.cfg), x_human, x_objects, mask, training=True, gumbel_noise=noise, **kw)
    rs = [torch.randn(o.shape, generator=torch.Generator().manual_seed(i)) for i, o in enumerate(ref)]
    sum((o * r).sum() for o, r in zip(ref, rs) if o.requires_grad).backward()
    m = m.to(DEV).train()
    m._gumbel_noise_override = noise
    dkw = {k: v.to(DEV) for k, v in kw.items()}
    K = twog_kernels.get_kernels()
    runs = {}
    for mode in ('1', '0'):
        monkeypatch.setenv('TWOG_GENERAL_TAPE', mode)
        m.load_state_dict(sd)
        m.zero_grad(set_to_none=True)
        replays = []
        if mode == '1':
            real = K.tape_run
            monkeypatch.setattr(K, 'tape_run', lambda *a, **k: (replays.append(a[2:4]), real(*a, **k))[1])
        out = m(x_human.to(DEV), x_objects.to(DEV), mask.to(DEV), **dkw)
        sum((o * r.to(DEV)).sum() for o, r in zip(out, rs) if o.requires_grad).backward()
        if mode == '1':
            monkeypatch.undo()
            assert replays == [(0, T - 1), (0, T - 2)], replays   # forward steps 1 ... T-1, backward steps T-2 ... 1
        runs[mode] = ([o.detach().cpu() for o in out],
                      {n: (None if p.grad is None else p.grad.detach().cpu().clone()) for n, p in m.named_parameters()})
    for a, b in zip(runs['1'][0], runs['0'][0]):
        assert torch.equal(a, b)
    for n, ga in runs['1'][1].items():
        gb = runs['0'][1][n]
        assert (ga is None) == (gb is None) and (ga is None or torch.equal(ga, gb)), n
    for i, (o, r) in enumerate(zip(runs['1'][0], ref)):
        err = (o - r.detach()).abs().max().item() / max(1.0, r.detach().abs().max().item())
        assert err < REL, (form, i, err)
    for n, ga in runs['1'][1].items():
        g_ref = osd[n].grad
        if g_ref is None:
            assert ga is None or float(ga.abs().max()) == 0.0, n
            continue
        scale = max(g_ref.abs().max().item(), 1e-6)
        err = (ga - g_ref).abs().max().item()
        assert err < GRAD_REL * scale + GRAD_ABS, (form, n, err / scale)


def m_plan_is_general(m, bs, T, H, O, N, dists):
    from twog_gcn_amd import ops
    p = ops.Plan(m.cfg, bs, T, H, O, N, 2048, 13, None, True, False)
    if dists:
        p.dists = {'hh': 1}
    return p.general_segment()


def test_inspect_model_attention_scores_vs_oracle():
    """predict.py --inspect_model on the HIP path: the three (bs, H, T, O) objects->human attention tensors."""
    z, meta = load_g4('c2_stage1')
    m = _model_from_meta(meta).eval()
    noise = torch.from_numpy(z['gumbel_noise'])
    m._gumbel_noise_override = noise
    kw = g4_inputs(z)
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        out, att = m(**{k: v.to(DEV) for k, v in kw.items()}, inspect_model=True)
        ref_out, ref_att = cpu_ref.tggcn_forward(sd, dict(m.cfg), kw['x_human'], kw['x_objects'], kw['objects_mask'],
                                                 human_segmentation=kw.get('human_segmentation'),
                                                 objects_segmentation=kw.get('objects_segmentation'), training=False,
                                                 gumbel_noise=noise, inspect_model=True)
    assert len(att) == 3 and len(out) == len(ref_out)
    for a, r in zip(att, ref_att):
        assert tuple(a.shape) == tuple(r.shape)
        assert (a.cpu() - r).abs().max().item() < 1e-5
    for o, r in zip(out, ref_out):
        assert (o.cpu() - r).abs().max().item() < REL * max(1.0, r.abs().max().item())
