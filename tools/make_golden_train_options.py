#!/usr/bin/env python3
"""Generate the G14 golden vectors (tests/golden/g14_*.npz): the reference's TRAINING STEP with its two training options,
`optimization.clip_gradient_at` and `misc.multi_task_loss_learner`, run by the REAL reference (build container only; the
reference never travels to the GPU box).

Order of pyrutils/torch/train_utils.py:143-154 with train.py:38-46's optimizer: zero_grad, forward, criterion
(reduction='mean'), mtll_model(losses), sum, backward, clip_grad_norm_(model.parameters(), max_norm), step, where the
optimizer is torch.optim.Adam(model.parameters(), lr) with add_param_group({'params': mtll_model.parameters()}).
  (a) G12's configuration (MPHOI layout, 6 terms, 4 learnable), 5 steps; max_norm between the steps' norms, so some
      steps clip and some do not;
  (b) a CAD-120 layout with the object heads (12 terms, 8 learnable), 4 steps; a max_norm that clips every step.
Stored per step: raw and weighted losses, the pre-clip norm, whether it clipped, log_sds after the step, the hard gates and
the Gumbel noise; after the last step the deltas of a sample of parameters (as G12). Usage:
    python tools/make_golden_train_options.py
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from make_golden import STAGE1, G12, G12_MISC, G12_PARAMS, GumbelRecorder, OUT  # noqa: E402  (puts the reference on sys.path)
from vhoi.models import TGGCN  # noqa: E402
from vhoi.losses import select_loss, select_loss_types, select_loss_learning_mask  # noqa: E402
from pyrutils.torch.multi_task import MultiTaskLossLearner  # noqa: E402

from tests.helpers import det_state_dict, sample_grad  # noqa: E402
from tests.train_options_helpers import g14_step_batch  # noqa: E402

CAD_PARAMS = G12_PARAMS + ['object_recognition_mlp.0.weight', 'object_frame_prediction_mlp.0.weight']
CASES = {
    'a': dict(G12, name='g12', layout='mphoi', dataset='mphoi', cfg_over={}, max_norm=2.5, params=G12_PARAMS),
    'b': dict(name='g14b', layout='cad120', dataset='cad120', H=1, O=4, N=19, hid=16, bs=3, T=8, classes=(10, 12), seed=61,
              gain=1.6, steps=4, lr=1e-4, cfg_over=dict(message_humans_to_human=False), max_norm=0.05, params=CAD_PARAMS),
}
MARGIN = 1e-3   # no norm within this relative distance of max_norm: the clip decision cannot flip on rounding


class Cfg(dict):
    def get(self, k, default_value=None, **kw):
        return dict.get(self, k, default_value if default_value is not None else kw.get('default'))


def run(case):
    c = CASES[case]
    cfg = dict(STAGE1)
    cfg.update(c['cfg_over'])
    cfg.update(hidden_size=c['hid'], gcn_node=c['N'])
    model = TGGCN(input_size=(2048 + 4 * c['N'], 2048), num_classes=c['classes'], **cfg)
    shapes = {k: list(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(det_state_dict(shapes, seed=c['seed'], gain=c['gain']))
    model.train()
    rcfg = Cfg(misc=G12_MISC)
    crit, names = select_loss('2G-GCN', 'multiple', c['dataset'], rcfg)
    loss_types = select_loss_types('2G-GCN', c['dataset'], rcfg)
    mask = select_loss_learning_mask('2G-GCN', c['dataset'], rcfg)
    mtll = MultiTaskLossLearner(loss_types=loss_types, mask=mask)
    mtll.train()
    opt = torch.optim.Adam(model.parameters(), lr=c['lr'])
    opt.add_param_group({'params': mtll.parameters()})
    init = {n: p.detach().clone() for n, p in model.named_parameters()}
    meta = {k: (list(v) if isinstance(v, tuple) else v) for k, v in c.items() if k != 'cfg_over'}
    meta.update(cfg=cfg, misc=G12_MISC, loss_types=loss_types, mask=mask, state_dict_shapes=shapes)
    torch.manual_seed(42)
    save, rec_ = {}, dict(raw=[], weighted=[], norm=[], clipped=[], log_sds=[], hard=[])
    for step in range(c['steps']):
        kw, target = g14_step_batch(meta, step)
        with GumbelRecorder() as rec:
            opt.zero_grad()
            out = model(**kw)
            losses = crit(out, target, reduction='mean')
            raw = [float(v.detach()) for v in losses]
            losses = mtll(losses)
            loss = sum(losses)
            loss.backward()
            norm = torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=c['max_norm'])
            opt.step()
        save[f'noise{step}'] = torch.stack(rec.drawn, 0).numpy()
        coef = c['max_norm'] / (norm.detach().float() + 1e-6)   # torch's own coefficient (fp32)
        rec_['raw'].append(raw)
        rec_['weighted'].append([float(v.detach()) for v in losses])
        rec_['norm'].append(float(norm))
        rec_['clipped'].append(bool(coef < 1))
        rec_['log_sds'].append(mtll.log_sds.detach().numpy().copy())
        rec_['hard'].append(out[0].detach().numpy().copy())
        assert abs(float(norm) - c['max_norm']) > MARGIN * c['max_norm'], (case, step, float(norm), c['max_norm'])
        print(f'g14 {case} step {step}: loss {float(loss.detach()):.6f} norm {float(norm):.6f} clipped {bool(coef < 1)} '
              f'min|soft-0.5| {float((out[2 if c["layout"] == "cad120" else 1].detach() - 0.5).abs().min()):.4f}')
    if case == 'a':
        assert any(rec_['clipped']) and not all(rec_['clipped']), rec_['norm']
    else:
        assert all(rec_['clipped']), rec_['norm']
    save['losses_raw'] = np.array(rec_['raw'], dtype=np.float64)
    save['losses_weighted'] = np.array(rec_['weighted'], dtype=np.float64)
    save['norms'] = np.array(rec_['norm'], dtype=np.float64)
    save['clipped'] = np.array(rec_['clipped'])
    save['log_sds'] = np.stack(rec_['log_sds'], 0)
    save['hard_gates'] = np.stack(rec_['hard'], 0)
    save['loss_names'] = np.array(names)
    P = dict(model.named_parameters())
    for n in c['params']:
        save['delta_' + n] = sample_grad(P[n].detach() - init[n])
    save['mtll_state_keys'] = np.array(list(mtll.state_dict().keys()))
    save['weights_final'] = np.array([np.nan if w is None else w for w in mtll.get_weights()], dtype=np.float64)
    save['meta_json'] = np.array(json.dumps(meta))
    np.savez_compressed(os.path.join(OUT, f'g14_{case}.npz'), **save)
    print(f'g14 {case}:', len(save), 'arrays; norms', [round(v, 5) for v in rec_['norm']], 'max_norm', c['max_norm'])


if __name__ == '__main__':
    torch.set_num_threads(8)
    for case in (sys.argv[1:] or CASES):
        run(case)
