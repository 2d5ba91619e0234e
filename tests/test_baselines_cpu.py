"""CPU: the baseline models (twog_gcn_amd.baselines) against the reference's G13 fixtures (tools/make_golden_baselines.py)
-- registries, constructor / state_dict layout, seeded initialisation, loaders, fetchers, feeders and losses -- and the
host composition (BaselineFunction) on the torch double of the kernel interface (tests/baseline_helpers.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import twog_gcn_amd  # noqa: F401
from twog_gcn_amd import baselines, data_loading, losses, models
from twog_gcn_amd import kernels as twog_kernels
from twog_gcn_amd import _lib
from tests.baseline_helpers import CASES, BaselineFakeKernels, check_case, load_case, run_case
from tests.helpers import GOLDEN, ROOT, sample_grad
from tests.test_batching_cpu import raw_videos   # the generator of tools/make_golden.py::_raw_videos (G6, G13)

G13 = lambda part: np.load(os.path.join(GOLDEN, f'g13_baselines_{part}.npz'))


@pytest.fixture()
def fake():
    fk = BaselineFakeKernels()
    twog_kernels._set_backend_for_tests(fk)
    yield fk
    twog_kernels._set_backend_for_tests(None)


def test_registry_has_the_three_reference_models():
    assert baselines.select_model('bimanual_baseline') is baselines.BimanualBaseline
    assert baselines.select_model('cad120_baseline') is baselines.CAD120Baseline
    assert baselines.select_model('2G-GCN') is models.TGGCN
    with pytest.raises(KeyError):
        baselines.select_model('lstm_baseline')
    # the existing registries keep refusing the baseline names
    with pytest.raises(KeyError):
        models.select_model('bimanual_baseline')


@pytest.mark.parametrize('name', ['bim_default', 'bim_unidir', 'bim_nomp', 'bim_nobias', 'bim_h2', 'cad_default',
                                  'cad_unidir', 'cad_nomp', 'cad_h13'])
def test_state_dict_layout_matches_the_reference(name):
    _, meta = load_case(name)
    cls = baselines.select_model('bimanual_baseline' if meta['kind'] == 'bimanual' else 'cad120_baseline')
    m = cls(input_size=tuple(meta['F']), num_classes=tuple(meta['classes']), hidden_size=meta['h'], **meta['kw'])
    got = {k: list(v.shape) for k, v in m.state_dict().items()}
    assert got == meta['state_dict_shapes']
    assert list(got) == list(meta['state_dict_shapes'])   # registration order too


@pytest.mark.parametrize('kind', ['bimanual', 'cad120'])
@pytest.mark.parametrize('h', [2, 128])
def test_seeded_init_matches_the_reference_bit_for_bit(kind, h):
    z = G13('init')
    cls = baselines.BimanualBaseline if kind == 'bimanual' else baselines.CAD120Baseline
    torch.manual_seed(0)
    m = cls(input_size=(40, 24), num_classes=(14, None) if kind == 'bimanual' else (10, 12), hidden_size=h)
    for k, v in m.state_dict().items():
        want = z[f'{kind}_h{h}_{k}']
        assert list(v.shape) == z[f'{kind}_h{h}_{k}__shape'].tolist(), k
        got = v.numpy() if h == 2 else sample_grad(v)
        assert np.array_equal(got, want), k


def test_gradients_go_to_parameters_only_and_no_grad_keeps_no_state(fake):
    z, meta = load_case('cad_default')
    from tests.baseline_helpers import build_case_model
    m = build_case_model(meta)
    xh, xo, mask = (torch.from_numpy(z[k]).requires_grad_(True) for k in ('x_human', 'x_objects', 'objects_mask'))
    out = m(xh, xo, mask)
    sum(o.sum() for o in out).backward()
    assert xh.grad is None and xo.grad is None and mask.grad is None
    assert all(p.grad is not None for p in m.parameters())
    with torch.no_grad():
        out = m(xh, xo, mask)
    assert all(o.grad_fn is None for o in out)
    m.eval()
    out_eval = m(xh, xo, mask)
    m.train()
    out_train = m(xh, xo, mask)
    assert all(torch.equal(a, b) for a, b in zip(out_eval, out_train))


@pytest.mark.parametrize('name', CASES)
def test_host_composition_matches_the_reference(fake, name):
    m, out, z, meta = run_case(name)
    check_case(m, out, z, meta)


def test_baseline_path_runs_no_torch_math():
    src = open(os.path.join(ROOT, '2g-gcn_amd', 'baselines.py')).read()
    for pat in ('matmul', 'F.linear', 'torch.softmax', 'log_softmax', 'torch.cat', '@ '):
        assert pat not in src, pat


@pytest.mark.parametrize('kind,model_name', [('bimanual', 'bimanual_baseline'), ('cad120', 'cad120_baseline')])
def test_loaders_fetchers_and_feeders_match_g13(kind, model_name):
    z = G13('loaders')
    vids_fn = raw_videos
    for sigma, test_data in ((0.0, False), (2.0, False), (0.0, True)):
        loader, _, _ = baselines.create_data_loader(vids_fn(kind, seed=60), model_name, 'multiple', kind, batch_size=2,
                                                    shuffle=False, sigma=sigma, downsampling=3, test_data=test_data)
        tensors = loader.dataset.tensors
        keys = sorted((k for k in z.files if k.startswith(f'{kind}_s{sigma}_t{int(test_data)}_')),
                      key=lambda k: int(k.rsplit('_', 1)[1]))
        assert len(tensors) == len(keys)
        for t, k in zip(tensors, keys):
            want = z[k]
            assert t.numpy().dtype == want.dtype and t.shape == want.shape, k
            if want.dtype.kind in 'iub':
                assert np.array_equal(t.numpy(), want), k
            else:
                assert np.allclose(t.numpy(), want, rtol=1e-6, atol=1e-6), k
    loader, _, _ = baselines.create_data_loader(vids_fn(kind, seed=60), model_name, 'multiple', kind, batch_size=2,
                                                shuffle=False, downsampling=3)
    batch = next(iter(loader))
    data, targets = baselines.select_model_data_fetcher(model_name, 'multiple')(batch, 'cpu')
    assert len(data) == int(z[f'{kind}_fetch_n_data']) and len(targets) == int(z[f'{kind}_fetch_n_targets'])
    seen = {}

    def rec(*args, **kw):
        seen['args'], seen['kw'] = args, kw
        return 'out'

    assert baselines.select_model_data_feeder(model_name, 'multiple')(rec, data) == 'out'
    assert len(seen['args']) == int(z[f'{kind}_feed_n_args']) and len(seen['kw']) == int(z[f'{kind}_feed_n_kw'])
    for i, a in enumerate(seen['args']):
        assert np.allclose(a.numpy(), z[f'{kind}_feed_arg{i}'], rtol=1e-6, atol=1e-6)
    assert baselines.input_size_from_data_loader(loader, model_name, 'multiple') == (tensors[0].shape[-1], tensors[1].shape[-1])


def test_loader_refusals():
    vids = raw_videos
    with pytest.raises(ValueError, match='length_bucketing'):
        baselines.create_data_loader(vids('bimanual', 60), 'bimanual_baseline', 'multiple', 'bimanual', 2, False,
                                     length_bucketing=True)
    with pytest.raises(ValueError):
        baselines.create_data_loader(vids('mphoi', 60), 'bimanual_baseline', 'multiple', 'mphoi', 2, False)
    with pytest.raises(ValueError):
        baselines.create_data_loader(vids('cad120', 60), 'bimanual_baseline', 'multiple', 'cad120', 2, False)
    # the existing functions keep refusing the baseline names
    with pytest.raises(KeyError):
        data_loading.select_model_data_fetcher('cad120_baseline', 'multiple')
    assert baselines.determine_num_classes('bimanual_baseline', 'multiple', 'bimanual') == (14, None)
    assert baselines.determine_num_classes('cad120_baseline', 'multiple', 'cad120') == (10, 12)


def test_select_loss_names_weights_and_values(fake):
    z = G13('losses')
    for kind, model_name, n in (('bimanual', 'bimanual_baseline', 1), ('cad120', 'cad120_baseline', 2)):
        crit, names = baselines.select_loss(model_name, 'multiple', kind, {})
        assert names == z[f'{kind}_names'].tolist()
        assert crit.keywords['loss_functions'] == (losses.nll_loss,) * n
        assert 'weight' not in crit.keywords   # (multi_task_loss's default: 1.0 each)
        case = 'bim_default' if kind == 'bimanual' else 'cad_default'
        zc, _ = load_case(case)
        outs = [torch.from_numpy(zc[f'out{i}']) for i in range(n)]
        ys = [torch.from_numpy(z[f'{kind}_target{i}']) for i in range(n)]
        got = np.array([float(v) for v in crit(outs, ys)])
        assert np.allclose(got, z[f'{kind}_losses'], rtol=1e-5), (got, z[f'{kind}_losses'])
        with pytest.raises(ValueError):
            baselines.select_loss_types(model_name, kind, {})
        with pytest.raises(ValueError):
            baselines.select_loss_learning_mask(model_name, kind, {})
        assert baselines.decide_num_main_losses(model_name, kind, {}) is None
    assert baselines.decide_num_main_losses('2G-GCN', 'cad120', {}) == 4
    with pytest.raises(NotImplementedError):
        losses.select_loss('cad120_baseline', 'multiple', 'cad120', {})


def test_new_abi_structs_match_the_c_compiler(tmp_path):
    header = os.path.join(ROOT, 'include', 'twog_gcn.h')
    structs = {'twog_entity_pool_t': _lib.EntityPool, 'twog_entity_pool_bwd_t': _lib.EntityPoolBwd}
    src = tmp_path / 'sz.c'
    body = ''.join(f'printf("{n} %zu\\n", sizeof({n}));' for n in structs)
    src.write_text(f'#include <stdio.h>\n#include "{header}"\nint main(void){{{body}return 0;}}\n')
    exe = tmp_path / 'sz'
    subprocess.run(['gcc', str(src), '-o', str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    for line in out.strip().splitlines():
        name, size = line.split()
        assert ctypes.sizeof(structs[name]) == int(size), (name, ctypes.sizeof(structs[name]), size)
    for sym in ('twog_gru_seq_fwd', 'twog_gru_seq_bwd', 'twog_entity_pool_fwd', 'twog_entity_pool_bwd'):
        assert sym in _lib.exported_symbols()
