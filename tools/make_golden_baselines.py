#!/usr/bin/env python3
"""Generate tests/golden/g13_baselines_*.npz by running the REAL reference's baseline models (BimanualBaseline,
CAD120Baseline, vhoi/models.py:15-175), its select_loss / data loader branches for the baseline names and a three-step
Adam trajectory.

Runs only in the build container (the reference never travels to the GPU box). Weights come from oracle/detgen.py, so the
fixtures hold inputs, outputs, (sampled) gradients and targets. Usage:  python tools/make_golden_baselines.py
"""
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('TWOG_REFERENCE', '/root/reference')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, REF)

from oracle import detgen  # noqa: E402
from make_golden import load_det, sample_grad, _raw_videos  # noqa: E402
from vhoi.models import BimanualBaseline, CAD120Baseline  # noqa: E402
from tests.baseline_helpers import TRAJ, make_inputs, make_targets  # noqa: E402  (closed-form: the tests regenerate them)
from vhoi.losses import select_loss  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')

# name -> model kind, constructor keywords, layout. F_h / F_o narrow except one case at the real widths.
CASES = {
    'bim_default': dict(kind='bimanual', kw=dict(), bs=3, T=7, H=2, O=4, F=(40, 24), h=16, seed=1301),
    'bim_unidir': dict(kind='bimanual', kw=dict(bidirectional=False), bs=3, T=7, H=2, O=4, F=(40, 24), h=16, seed=1302),
    'bim_nomp': dict(kind='bimanual', kw=dict(with_message_passing=False), bs=3, T=7, H=2, O=4, F=(40, 24), h=16, seed=1303),
    'bim_nobias': dict(kind='bimanual', kw=dict(bias=False), bs=3, T=7, H=2, O=4, F=(40, 24), h=16, seed=1304),
    'bim_h2': dict(kind='bimanual', kw=dict(), bs=3, T=8, H=2, O=4, F=(40, 24), h=2, seed=1305),
    'bim_h64_bs4': dict(kind='bimanual', kw=dict(), bs=4, T=6, H=2, O=4, F=(40, 24), h=64, seed=1306),
    'bim_h64_bs20': dict(kind='bimanual', kw=dict(), bs=20, T=4, H=2, O=4, F=(40, 24), h=64, seed=1307),
    'bim_h128_full': dict(kind='bimanual', kw=dict(), bs=2, T=5, H=2, O=4, F=(2168, 2048), h=128, seed=1308),
    'cad_default': dict(kind='cad120', kw=dict(), bs=3, T=7, H=1, O=5, F=(40, 24), h=16, seed=1311),
    'cad_unidir': dict(kind='cad120', kw=dict(bidirectional=False), bs=3, T=7, H=1, O=5, F=(40, 24), h=16, seed=1312),
    'cad_nomp': dict(kind='cad120', kw=dict(with_message_passing=False), bs=3, T=7, H=1, O=5, F=(40, 24), h=16, seed=1313),
    'cad_h13': dict(kind='cad120', kw=dict(), bs=3, T=6, H=1, O=5, F=(40, 24), h=13, seed=1314),
}
CLASSES = {'bimanual': (14, None), 'cad120': (10, 12)}
TRAJ_PARAMS = ['human_embedding_mlp.0.weight', 'human_bd_rnn.weight_hh_l0', 'object_bd_rnn.weight_ih_l0_reverse',
               'human_recognition_mlp.0.weight', 'human_recognition_mlp.0.bias']


def model_class(kind):
    return BimanualBaseline if kind == 'bimanual' else CAD120Baseline


def model_case(name, c):
    classes = CLASSES[c['kind']]
    model = model_class(c['kind'])(input_size=c['F'], num_classes=classes, hidden_size=c['h'], **c['kw'])
    load_det(model, seed=c['seed'], gain=1.0)
    x_h, x_o, mask = make_inputs(name, c)
    out = model(torch.from_numpy(x_h), torch.from_numpy(x_o), torch.from_numpy(mask))
    cots = [detgen.normal(f'{name}.cot{i}', tuple(o.shape), seed=c['seed']).astype(np.float32) for i, o in enumerate(out)]
    loss = sum((o * torch.from_numpy(w)).sum() for o, w in zip(out, cots))
    loss.backward()
    save = dict(x_human=x_h, x_objects=x_o, objects_mask=mask)
    for i, (o, w) in enumerate(zip(out, cots)):
        save[f'out{i}'], save[f'cot{i}'] = o.detach().numpy(), w
    for n, p in model.named_parameters():
        if p.grad is not None:
            save['grad_' + n] = sample_grad(p.grad)
    meta = dict(kind=c['kind'], kw=c['kw'], bs=c['bs'], T=c['T'], H=c['H'], O=c['O'], F=list(c['F']), h=c['h'],
                seed=c['seed'], classes=list(classes),
                state_dict_shapes={k: list(v.shape) for k, v in model.state_dict().items()},
                no_grad=[n for n, p in model.named_parameters() if p.grad is None])
    save['meta_json'] = np.array(json.dumps(meta))
    return save


def seeded_init():
    save = {}
    for kind in ('bimanual', 'cad120'):
        for h in (2, 128):
            torch.manual_seed(0)
            m = model_class(kind)(input_size=(40, 24), num_classes=CLASSES[kind], hidden_size=h)
            for k, v in m.state_dict().items():   # (h = 128: every 16th element, under 4096 per tensor)
                save[f'{kind}_h{h}_{k}'] = v.numpy().copy() if h == 2 else sample_grad(v)
                save[f'{kind}_h{h}_{k}__shape'] = np.array(v.shape)
    return save


def loaders():
    sys.modules.setdefault('zarr', types.ModuleType('zarr'))
    tb = types.ModuleType('torch.utils.tensorboard')
    tb.SummaryWriter = object
    sys.modules.setdefault('torch.utils.tensorboard', tb)
    import vhoi.data_loading as ref_dl
    out = {}
    for kind, model_name in (('bimanual', 'bimanual_baseline'), ('cad120', 'cad120_baseline')):
        for sigma, test_data in ((0.0, False), (2.0, False), (0.0, True)):
            loader, _, _ = ref_dl.create_data_loader(_raw_videos(kind, seed=60), model_name, 'multiple', kind,
                                                     batch_size=2, shuffle=False, sigma=sigma, downsampling=3,
                                                     test_data=test_data)
            for i, t in enumerate(loader.dataset.tensors):
                out[f'{kind}_s{sigma}_t{int(test_data)}_{i}'] = t.numpy()
        loader, _, _ = ref_dl.create_data_loader(_raw_videos(kind, seed=60), model_name, 'multiple', kind, batch_size=2,
                                                 shuffle=False, downsampling=3)
        batch = next(iter(loader))
        data, targets = ref_dl.select_model_data_fetcher(model_name, 'multiple')(batch, 'cpu')
        out[f'{kind}_fetch_n_data'], out[f'{kind}_fetch_n_targets'] = np.array(len(data)), np.array(len(targets))

        class Rec:
            def __call__(self, *args, **kw):
                self.args, self.kw = args, kw
                return 'out'

        rec = Rec()
        ref_dl.select_model_data_feeder(model_name, 'multiple')(rec, data)
        out[f'{kind}_feed_n_args'], out[f'{kind}_feed_n_kw'] = np.array(len(rec.args)), np.array(len(rec.kw))
        for i, a in enumerate(rec.args):
            out[f'{kind}_feed_arg{i}'] = a.numpy()
    return out


def loss_values(model_saves):
    out = {}
    for case, kind, model_name in (('bim_default', 'bimanual', 'bimanual_baseline'),
                                   ('cad_default', 'cad120', 'cad120_baseline')):
        c = CASES[case]
        s = model_saves[case]
        crit, names = select_loss(model_name, 'multiple', kind, {})
        outs = [torch.from_numpy(s[f'out{i}']) for i in range(2 if kind == 'cad120' else 1)]
        ys = [torch.from_numpy(y) for y in make_targets(case, c, CLASSES[kind])]
        vals = crit(outs, ys)
        out[f'{kind}_names'] = np.array(names)
        out[f'{kind}_losses'] = np.array([float(v) for v in vals], dtype=np.float64)
        for i, y in enumerate(ys):
            out[f'{kind}_target{i}'] = y.numpy()
    return out


def trajectory():
    c = TRAJ
    model = BimanualBaseline(input_size=c['F'], num_classes=CLASSES['bimanual'], hidden_size=c['h'])
    load_det(model, seed=c['seed'], gain=1.0)
    init = {n: p.detach().clone() for n, p in model.named_parameters()}
    crit, names = select_loss('bimanual_baseline', 'multiple', 'bimanual', {})
    opt = torch.optim.Adam(model.parameters(), lr=c['lr'])
    losses = []
    for step in range(c['steps']):
        x_h, x_o, mask = make_inputs(f'g13traj.s{step}', c)
        ys = make_targets(f'g13traj.s{step}', c, CLASSES['bimanual'])
        opt.zero_grad()
        out = model(torch.from_numpy(x_h), torch.from_numpy(x_o), torch.from_numpy(mask))
        ls = crit(out, [torch.from_numpy(y) for y in ys])
        sum(ls).backward()
        opt.step()
        losses.append([float(v) for v in ls])
    save = dict(losses=np.array(losses, dtype=np.float64), loss_names=np.array(names))
    P = dict(model.named_parameters())
    for n in TRAJ_PARAMS:
        save['final_' + n] = sample_grad(P[n])
        save['delta_' + n] = sample_grad(P[n].detach() - init[n])
    save['meta_json'] = np.array(json.dumps(dict(c, F=list(c['F']), params=TRAJ_PARAMS)))
    return save


def main():
    torch.set_num_threads(8)
    os.makedirs(OUT, exist_ok=True)
    saves = {}
    for name, c in CASES.items():
        saves[name] = model_case(name, c)
        np.savez_compressed(os.path.join(OUT, f'g13_baselines_model_{name}.npz'), **saves[name])
    np.savez_compressed(os.path.join(OUT, 'g13_baselines_init.npz'), **seeded_init())
    np.savez_compressed(os.path.join(OUT, 'g13_baselines_loaders.npz'), **loaders())
    np.savez_compressed(os.path.join(OUT, 'g13_baselines_losses.npz'), **loss_values(saves))
    np.savez_compressed(os.path.join(OUT, 'g13_baselines_trajectory.npz'), **trajectory())
    print('g13:', len(CASES), 'model cases')


if __name__ == '__main__':
    main()
