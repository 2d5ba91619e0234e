"""GPU: the baseline models on the HIP kernels -- the entity pool / concat kernel and the single-direction recurrence
against fp64 restatements, every G13 case of the reference (tools/make_golden_baselines.py) forward and backward, the
reference's three-step training trajectory through loader, fetcher, feeder, criterion and Adam, and bit-reproducibility."""
import json

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

import twog_gcn_amd  # noqa: F401
from twog_gcn_amd import baselines
from twog_gcn_amd.kernels import get_kernels
from tests.baseline_helpers import (CASES, GRAD_REL, OUT_REL, TRAJ, BaselineFakeKernels, check_case, make_inputs,
                                    make_targets, run_case)
from tests.helpers import GOLDEN, det_state_dict, rel_err, sample_grad

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _pool_inputs(bs, T, H, O, W, seed):
    g = torch.Generator().manual_seed(seed)
    hfr = torch.randn(bs, T, H, W, generator=g)
    ofr = torch.randn(bs, T, O, W, generator=g)
    mask = torch.ones(bs, O)
    mask[1, O // 2:] = 0.0      # some real objects (clip 1)
    mask[2, :] = 0.0            # none (clip 2); clip 0: all real
    d_hin = torch.randn(bs, T, H, 2 * W, generator=g)
    d_oin = torch.randn(bs, T, O, 2 * W, generator=g)
    return hfr, ofr, mask, d_hin, d_oin


def test_entity_pool_against_fp64():
    K, F = get_kernels(), BaselineFakeKernels()
    for W in (2, 3, 128, 1024):
        for H in (1, 2, 5):
            for O in (1, 4, 16):
                hfr, ofr, mask, d_hin, d_oin = _pool_inputs(3, 4, H, O, W, seed=W * 100 + H * 10 + O)
                for object_head in (False, True):
                    hin, oin = K.entity_pool_fwd(hfr.to(DEV), ofr.to(DEV), mask.to(DEV), object_head)
                    rh, ro = F.entity_pool_fwd(hfr.double(), ofr.double(), mask.double(), object_head)
                    assert rel_err(hin.cpu().numpy(), rh.numpy()) < 1e-6, (W, H, O)
                    if object_head:
                        assert rel_err(oin.cpu().numpy(), ro.numpy()) < 1e-6, (W, H, O)
                    else:
                        assert oin is None
                    doi = d_oin if object_head else None
                    dh, do = K.entity_pool_bwd(d_hin.to(DEV), None if doi is None else doi.to(DEV), mask.to(DEV), O)
                    rdh, rdo = F.entity_pool_bwd(d_hin.double(), None if doi is None else doi.double(), mask.double(), O)
                    assert rel_err(dh.cpu().numpy(), rdh.numpy()) < 1e-6, (W, H, O, object_head)
                    assert rel_err(do.cpu().numpy(), rdo.numpy()) < 1e-6, (W, H, O, object_head)
                    # the clip without a real object: the pooled half is exactly 0 and so is its object gradient from the pool
                    assert float(hin[2, :, :, W:].abs().max()) == 0.0
                    if not object_head:
                        assert float(do[2].abs().max()) == 0.0
                    # fixed-order reductions: a second run is bit-identical
                    hin2, oin2 = K.entity_pool_fwd(hfr.to(DEV), ofr.to(DEV), mask.to(DEV), object_head)
                    dh2, do2 = K.entity_pool_bwd(d_hin.to(DEV), None if doi is None else doi.to(DEV), mask.to(DEV), O)
                    assert torch.equal(hin, hin2) and torch.equal(dh, dh2) and torch.equal(do, do2)
                    if object_head:
                        assert torch.equal(oin, oin2)


@pytest.mark.parametrize('h,T', [(2, 120), (64, 120), (512, 40)])
def test_single_direction_recurrence_against_torch_gru_fp64(h, T):
    K, F = get_kernels(), BaselineFakeKernels()
    bs, E = 3, 2
    g = torch.Generator().manual_seed(h * 1000 + T)
    gru = torch.nn.GRU(h, h, batch_first=True).double()
    with torch.no_grad():
        for p in gru.parameters():
            p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) / h ** 0.5)
    x = torch.randn(bs, T, E, h, generator=g, dtype=torch.float64)
    w_ih, w_hh, b_ih, b_hh = gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0
    gi = (x @ w_ih.t() + b_ih).detach()
    ref, _ = gru(x.permute(0, 2, 1, 3).reshape(bs * E, T, h))
    ref = ref.reshape(bs, E, T, h).permute(0, 2, 1, 3).detach()
    (out, save), = K.gru_seq_fwd([dict(gi=gi.float().contiguous().to(DEV), w_hh=w_hh.detach().float().to(DEV),
                                        b_hh=b_hh.detach().float().to(DEV))], bs, T, h)
    assert rel_err(out.cpu().numpy(), ref.numpy()) < OUT_REL, rel_err(out.cpu().numpy(), ref.numpy())
    d_out = torch.randn(bs, T, E, h, generator=g, dtype=torch.float64)
    (d_gi, d_gh), = K.gru_seq_bwd([dict(d_out=d_out.float().to(DEV), save=save, out=out,
                                         w_hh=w_hh.detach().float().to(DEV))], bs, T, h)
    # fp64 backward through time (torch.autograd on nn.GRU): d gi is the gradient wrt the input projection
    gi_leaf = gi.clone().requires_grad_(True)
    (fo, fs), = F.gru_seq_fwd([dict(gi=gi_leaf, w_hh=w_hh.detach(), b_hh=b_hh.detach())], bs, T, h)
    assert rel_err(fo.detach().numpy(), ref.numpy()) < 1e-10   # the double itself is nn.GRU
    (fo * d_out).sum().backward()
    assert rel_err(d_gi.cpu().numpy(), gi_leaf.grad.numpy()) < GRAD_REL
    (rgi, rgh), = F.gru_seq_bwd([dict(d_out=d_out, save=fs.detach(), out=fo.detach(), w_hh=w_hh.detach())], bs, T, h)
    assert rel_err(d_gh.cpu().numpy(), rgh.numpy()) < GRAD_REL


@pytest.mark.parametrize('name', CASES)
def test_model_matches_the_reference(name):
    m, out, z, meta = run_case(name, DEV)
    torch.cuda.synchronize()
    wo, wg = check_case(m, out, z, meta)
    if name == 'bim_h64_bs4':   # a small batch: the frame recurrence ran as the persistent launch
        assert get_kernels().last_bigru_persistent
    print(f'{name}: outputs {wo:.2e}, gradients {wg:.2e}')


@pytest.mark.parametrize('name', ['bim_h64_bs4', 'bim_h64_bs20'])
def test_model_matches_the_reference_on_the_launch_per_step_recurrence(name, monkeypatch):
    """The same cases with the persistent launches switched off: both forms of the recurrence against the reference."""
    monkeypatch.setenv('TWOG_BIGRU_PERSIST', '0')
    m, out, z, meta = run_case(name, DEV)
    torch.cuda.synchronize()
    assert not get_kernels().last_bigru_persistent
    check_case(m, out, z, meta)


def test_forward_backward_is_bit_reproducible():
    for name in ('bim_default', 'cad_unidir'):
        runs = []
        for _ in range(2):
            m, out, _, _ = run_case(name, DEV)
            runs.append(([o.detach().clone() for o in out], [p.grad.clone() for p in m.parameters() if p.grad is not None]))
        (o1, g1), (o2, g2) = runs
        assert all(torch.equal(a, b) for a, b in zip(o1, o2)), name
        assert all(torch.equal(a, b) for a, b in zip(g1, g2)), name


def test_training_trajectory_end_to_end():
    """loader -> fetcher -> feeder -> select_loss -> backward -> Adam reproduces the reference's three steps. Tolerances of
    tests/test_training_trajectory.py: losses 1e-4 relative, parameter deltas 5e-4 of the largest delta (plus its
    Adam-noise allowance for elements whose gradient is within rounding of zero)."""
    z = np.load(f'{GOLDEN}/g13_baselines_trajectory.npz')
    meta = json.loads(str(z['meta_json']))
    c = TRAJ
    model = baselines.BimanualBaseline(input_size=c['F'], num_classes=(14, None), hidden_size=c['h'])
    model.load_state_dict(det_state_dict({k: list(v.shape) for k, v in model.state_dict().items()}, seed=c['seed'], gain=1.0))
    model = model.to(DEV)
    init = {n: p.detach().clone() for n, p in model.named_parameters()}
    crit, names = baselines.select_loss('bimanual_baseline', 'multiple', 'bimanual', {})
    assert names == z['loss_names'].tolist()
    fetch = baselines.select_model_data_fetcher('bimanual_baseline', 'multiple')
    feed = baselines.select_model_data_feeder('bimanual_baseline', 'multiple')
    opt = torch.optim.Adam(model.parameters(), lr=c['lr'])
    got = []
    for step in range(c['steps']):
        x_h, x_o, mask = make_inputs(f'g13traj.s{step}', c)
        ys = make_targets(f'g13traj.s{step}', c, (14, None))
        loader = DataLoader(TensorDataset(*[torch.from_numpy(a) for a in (x_h, x_o, mask, *ys)]), batch_size=c['bs'])
        data, targets = fetch(next(iter(loader)), DEV)
        opt.zero_grad()
        out = feed(model, data)
        ls = crit(out, targets)
        sum(ls).backward()
        opt.step()
        got.append([float(v) for v in ls])
    want = z['losses']
    err = np.abs(np.array(got) - want) / np.maximum(np.abs(want), 1e-3)
    assert err.max() < 1e-4, (got, want.tolist())
    P = dict(model.named_parameters())
    for n in meta['params']:
        d_ref = z['delta_' + n].astype(np.float64)
        d = sample_grad(P[n].detach() - init[n]).astype(np.float64)
        scale = np.abs(d_ref).max()
        e = np.abs(d - d_ref)
        tight = e <= 5e-4 * scale
        assert (~tight).sum() <= max(2, 0.002 * e.size), (n, int((~tight).sum()), float(e.max() / scale))
        assert e.max() <= 1e-2 * c['lr'] * c['steps'], (n, float(e.max()))
