"""The reference's two baseline models on the gfx950 path, with the data, loss and registry companions that run them.

Counterpart of ``BimanualBaseline`` / ``CAD120Baseline`` (vhoi/models.py:15-175) and of the baseline branches of
``select_model`` (:1589-1595), ``select_loss`` (vhoi/losses.py:62-67), ``select_model_data_fetcher/feeder``
(vhoi/data_loading.py:1215-1230) and ``assemble_tensors`` / ``assemble_bimanual_tensors`` (:436-501).

A module of its own: ``models.select_model``, ``losses.select_loss`` and ``data_loading.select_model_data_fetcher``
keep refusing the baseline names (their contract, tested as such). The registries here are the reference's full
three-name registries, and ``'2G-GCN'`` delegates to the existing functions unchanged, so one import covers all three
models::

    from twog_gcn_amd.baselines import (select_model, select_loss, select_model_data_fetcher, select_model_data_feeder,
                                        create_data_loader, input_size_from_data_loader, determine_num_classes)

The computation is ``BaselineFunction``: one autograd node whose every FLOP is a call of ``kernels.get_kernels()`` --
embedding GEMMs with fused ReLU, the input projections, the frame recurrence (``bigru_fwd`` or, for
``bidirectional=False``, ``gru_seq_fwd``), the entity pool / concatenation kernel and the label heads with their fused
log-softmax. torch.nn modules are parameter containers only, built in the reference's order so that a given
``torch.manual_seed`` yields the reference's initial weights.
"""
from functools import partial
from typing import Optional

import numpy as np
import torch
import torch.nn as nn
from torch.utils.data import DataLoader, TensorDataset

from . import data_loading, losses, models, ops
from .kernels import get_kernels

BASELINES = ('bimanual_baseline', 'cad120_baseline')


# ---------------------------------------------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------------------------------------------
class _Plan:
    """Static shape / configuration of one forward call."""

    def __init__(self, bs, T, H, O, F_h, F_o, h, bidirectional, message_passing, n_classes):
        self.bs, self.T, self.H, self.O, self.F_h, self.F_o, self.h = bs, T, H, O, F_h, F_o, h
        self.D = 2 if bidirectional else 1
        self.mp = message_passing
        self.n_classes = n_classes   # (human,) or (human, object)
        self.object_head = len(n_classes) == 2
        # the object branch feeds nothing in a Bimanual model without message passing (its parameters get no gradient,
        # as in the reference, whose object recurrence output is discarded there)
        self.object_branch = self.object_head or message_passing

    def sfx(self):
        return ('', '_reverse')[:self.D]

    def entities(self):
        return ('human', 'object') if self.object_branch else ('human',)


def used_parameter_names(plan, named):
    out = []
    for ent in plan.entities():
        out += [f'{ent}_embedding_mlp.0.weight', f'{ent}_embedding_mlp.0.bias']
        for s in plan.sfx():
            out += [f'{ent}_bd_rnn.{k}_l0{s}' for k in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')]
    out += ['human_recognition_mlp.0.weight', 'human_recognition_mlp.0.bias']
    if plan.object_head:
        out += ['object_recognition_mlp.0.weight', 'object_recognition_mlp.0.bias']
    return [n for n in out if n in named]   # (no biases under bias=False)


def baseline_forward(K, p, P, x_human, x_objects, objects_mask, backward_follows=False):
    """Returns (outputs list, saved dict). P: dict name -> parameter tensor."""
    bs, T, H, O, h, D = p.bs, p.T, p.H, p.O, p.h, p.D
    dev = x_human.device
    if hasattr(K, 'verify_persistent'):
        K.verify_persistent(dev)

    def empty(*shape):
        return torch.empty(*shape, dtype=torch.float32, device=dev)

    X = {'human': (x_human, H), 'object': (x_objects, O)}
    ents = p.entities()
    # embeddings: ReLU(Linear), one grouped launch
    EMB = {e: empty(bs, T, X[e][1], h) for e in ents}
    K.gemm([dict(A=X[e][0].view(-1, X[e][0].shape[-1]), B=P[f'{e}_embedding_mlp.0.weight'], C=EMB[e].view(-1, h),
                 bias=P.get(f'{e}_embedding_mlp.0.bias'), act=1) for e in ents])
    # input projections W_ih x + b_ih of every time step, both directions, both entity types: one grouped launch
    GI = {e: empty(bs, T, X[e][1], D * 3 * h) for e in ents}
    probs = []
    for e in ents:
        giv = GI[e].view(-1, D * 3 * h)
        for d, s in enumerate(p.sfx()):
            probs.append(dict(A=EMB[e].view(-1, h), B=P[f'{e}_bd_rnn.weight_ih_l0{s}'], C=giv[:, d * 3 * h:(d + 1) * 3 * h],
                              bias=P.get(f'{e}_bd_rnn.bias_ih_l0{s}')))
    K.gemm(probs)
    # frame-level recurrence, weights shared across the entities of a type (the entities are rows)
    if D == 2:
        res = K.bigru_fwd([dict(gi=GI[e], w_hh_f=P[f'{e}_bd_rnn.weight_hh_l0'], b_hh_f=P.get(f'{e}_bd_rnn.bias_hh_l0'),
                                w_hh_r=P[f'{e}_bd_rnn.weight_hh_l0_reverse'],
                                b_hh_r=P.get(f'{e}_bd_rnn.bias_hh_l0_reverse')) for e in ents], bs, T, h)
    else:
        res = K.gru_seq_fwd([dict(gi=GI[e], w_hh=P[f'{e}_bd_rnn.weight_hh_l0'], b_hh=P.get(f'{e}_bd_rnn.bias_hh_l0'))
                             for e in ents], bs, T, h)
    FR = {e: r[0] for e, r in zip(ents, res)}
    saves = {e: r[1] for e, r in zip(ents, res)}
    # head inputs: [hfr | pooled objects] (and [ofr | summed humans]) or the recurrence outputs themselves
    if p.mp:
        hin, oin = K.entity_pool_fwd(FR['human'], FR['object'], objects_mask, p.object_head)
    else:
        hin, oin = FR['human'], (FR['object'] if p.object_head else None)
    heads = [('human_recognition_mlp', hin, H, p.n_classes[0])]
    if p.object_head:
        heads.append(('object_recognition_mlp', oin, O, p.n_classes[1]))
    logits = [empty(bs * T * E, C) for _, _, E, C in heads]
    K.gemm([dict(A=xin.view(-1, xin.shape[-1]), B=P[f'{n}.0.weight'], C=lg, bias=P.get(f'{n}.0.bias'))
            for (n, xin, _, _), lg in zip(heads, logits)])
    outputs = [K.logsoftmax_permute_fwd(lg, bs, T, E, C) for (_, _, E, C), lg in zip(heads, logits)]
    S = dict(EMB=EMB, FR=FR, saves=saves, hin=hin, oin=oin, outputs=[o.detach() for o in outputs])
    if hasattr(K, 'verify_persistent'):
        # as ops.tggcn_forward: a persistent recurrence launch whose error word was left for later is guarded (outputs ->
        # NaN) when a backward pass follows and verified there; a forward-only call waits here
        if not (backward_follows and hasattr(K, 'guard_persistent') and K.guard_persistent(dev, S['outputs'])):
            K.verify_persistent(dev)
    return outputs, S


def baseline_backward(K, p, P, S, x_human, x_objects, objects_mask, d_outputs):
    """Hand-derived backward pass. Returns dict name -> gradient of every parameter the forward used."""
    bs, T, H, O, h, D = p.bs, p.T, p.H, p.O, p.h, p.D
    dev = x_human.device
    G = ops._Grads(K, None, known=P)

    def empty(*shape):
        return torch.empty(*shape, dtype=torch.float32, device=dev)

    def zeros(*shape):
        return K.zeros(*shape, device=dev) if hasattr(K, 'fill_zero') else torch.zeros(*shape, dtype=torch.float32, device=dev)

    X = {'human': (x_human, H), 'object': (x_objects, O)}
    ents = p.entities()
    # heads: log-softmax backward, dW / db, d(head input)
    heads = [('human_recognition_mlp', S['hin'], S['outputs'][0], d_outputs[0])]
    if p.object_head:
        heads.append(('object_recognition_mlp', S['oin'], S['outputs'][1], d_outputs[1]))
    d_in = []
    for n, xin, y, dy in heads:
        if dy is None:
            d_in.append(zeros(*xin.shape))
            continue
        dlog = K.logsoftmax_permute_bwd(y, dy.contiguous())
        ops._lin_w_grads(K, G, f'{n}.0.weight', f'{n}.0.bias', dlog, xin.view(-1, xin.shape[-1]))
        dx = empty(*xin.shape)
        K.gemm([dict(A=dlog, B=P[f'{n}.0.weight'], C=dx.view(-1, xin.shape[-1]))], b_kmajor=True)
        d_in.append(dx)
    d_hin = d_in[0]
    d_oin = d_in[1] if p.object_head else None
    if p.mp:
        dFR = dict(zip(('human', 'object'), K.entity_pool_bwd(d_hin, d_oin, objects_mask, O)))
    else:
        dFR = {'human': d_hin, 'object': d_oin}
    FR, saves, EMB = S['FR'], S['saves'], S['EMB']
    if D == 2:
        res = K.bigru_bwd([dict(d_out=dFR[e], save=saves[e], out=FR[e], w_hh_f=P[f'{e}_bd_rnn.weight_hh_l0'],
                                w_hh_r=P[f'{e}_bd_rnn.weight_hh_l0_reverse']) for e in ents], bs, T, h)
    else:
        res = K.gru_seq_bwd([dict(d_out=dFR[e], save=saves[e], out=FR[e], w_hh=P[f'{e}_bd_rnn.weight_hh_l0'])
                             for e in ents], bs, T, h)
    for e, (dgi, dgh) in zip(ents, res):
        E = X[e][1]
        dgiv, dghv = dgi.view(-1, D * 3 * h), dgh.view(-1, D * 3 * h)
        embv = EMB[e].view(-1, h)
        dEMB = empty(bs * T * E, h)
        for d, s in enumerate(p.sfx()):
            c0, c1 = d * 3 * h, (d + 1) * 3 * h
            ops._lin_w_grads(K, G, f'{e}_bd_rnn.weight_ih_l0{s}', None, dgiv[:, c0:c1], embv)
            ops._gru_bias_grads(K, G, f'{e}_bd_rnn.bias_ih_l0{s}', f'{e}_bd_rnn.bias_hh_l0{s}', dgiv[:, c0:c1],
                                dghv[:, c0:c1], h)
            # dW_hh = sum_t d_gh(t) h_prev(t)^T: h_prev is the previous frame's output in this direction's order
            if T > 1:
                dW_hh = empty(3 * h, h)
                if d == 0:
                    A = dgh[:, 1:, :, c0:c1].reshape(bs, (T - 1) * E, 3 * h)
                    B = FR[e][:, :T - 1, :, 0:h].reshape(bs, (T - 1) * E, h)
                else:
                    A = dgh[:, :T - 1, :, c0:c1].reshape(bs, (T - 1) * E, 3 * h)
                    B = FR[e][:, 1:, :, h:2 * h].reshape(bs, (T - 1) * E, h)
                G.dw_gemm(dict(A=A, B=B, C=dW_hh))
            else:
                dW_hh = zeros(3 * h, h)
            G.add(f'{e}_bd_rnn.weight_hh_l0{s}', dW_hh)
            K.gemm([dict(A=dgiv[:, c0:c1], B=P[f'{e}_bd_rnn.weight_ih_l0{s}'], C=dEMB, accumulate=d > 0)], b_kmajor=True)
        dpre = K.relu_bwd(dEMB, embv, dEMB)
        x = X[e][0]
        ops._lin_w_grads(K, G, f'{e}_embedding_mlp.0.weight', f'{e}_embedding_mlp.0.bias', dpre, x.view(-1, x.shape[-1]))
    G.flush()
    if hasattr(K, 'verify_persistent'):
        K.verify_persistent(dev)
    return G.g


class BaselineFunction(torch.autograd.Function):
    """One autograd node for a whole baseline forward pass. Inputs after the fixed ones are the parameters in the order of
    ``used_parameter_names``."""

    @staticmethod
    def forward(ctx, plan, names, x_human, x_objects, objects_mask, *params):
        K = get_kernels()
        P = dict(zip(names, params))
        outputs, S = baseline_forward(K, plan, P, x_human, x_objects, objects_mask,
                                      backward_follows=any(ctx.needs_input_grad))
        ctx.plan, ctx.names, ctx.P = plan, names, P
        ctx.inputs = (x_human, x_objects, objects_mask)
        tensors = []
        ctx.state_skeleton = ops._pack_state(S, tensors)
        ctx.save_for_backward(*tensors)
        ctx.set_materialize_grads(False)
        return tuple(outputs)

    @staticmethod
    def backward(ctx, *d_outputs):
        K = get_kernels()
        S = ops._unpack_state(ctx.state_skeleton, ctx.saved_tensors)
        x_human, x_objects, objects_mask = ctx.inputs
        grads = baseline_backward(K, ctx.plan, ctx.P, S, x_human, x_objects, objects_mask, list(d_outputs))
        out = [None] * 5
        for n in ctx.names:
            g = grads.get(n)
            out.append(None if g is None else g.reshape(ctx.P[n].shape))
        return tuple(out)


class _Baseline(nn.Module):
    _object_head = False

    def __init__(self, input_size: tuple, num_classes: tuple, hidden_size: int = 128, bidirectional: bool = True,
                 with_message_passing: bool = True, bias: bool = True):
        super().__init__()
        human_input_size, object_input_size = input_size
        num_subactivities, num_affordances = num_classes
        self.with_message_passing = with_message_passing
        self.hidden_size, self.bidirectional = hidden_size, bidirectional
        self.num_classes = (num_subactivities, num_affordances) if self._object_head else (num_subactivities,)
        # construction order of vhoi/models.py:23-34 / :98-111 (same RNG draws under a given seed)
        self.human_embedding_mlp = models.build_mlp([human_input_size, hidden_size], ['relu'], bias=bias)
        self.object_embedding_mlp = models.build_mlp([object_input_size, hidden_size], ['relu'], bias=bias)
        self.human_bd_rnn = nn.GRU(hidden_size, hidden_size, num_layers=1, bias=bias, batch_first=True,
                                   bidirectional=bidirectional)
        self.object_bd_rnn = nn.GRU(hidden_size, hidden_size, num_layers=1, bias=bias, batch_first=True,
                                    bidirectional=bidirectional)
        recognition_input_size = hidden_size
        if with_message_passing:
            recognition_input_size *= 2
        if bidirectional:
            recognition_input_size *= 2
        lsm = [{'name': 'logsoftmax', 'dim': -1}]
        self.human_recognition_mlp = models.build_mlp([recognition_input_size, num_subactivities], lsm, bias=bias)
        if self._object_head:
            self.object_recognition_mlp = models.build_mlp([recognition_input_size, num_affordances], lsm, bias=bias)

    def forward(self, x_human, x_objects, objects_mask):
        """Same contract as the reference forward: x_human (bs, T, H, F_h), x_objects (bs, T, O, F_o), objects_mask
        (bs, O) -> [y_human] (Bimanual) or [y_human, y_object] (CAD-120), each (bs, classes, T, entities) log-probabilities.
        Gradients flow to the parameters only."""
        bs, T, H, F_h = x_human.shape
        O, F_o = x_objects.shape[2], x_objects.shape[3]
        if x_objects.shape[:2] != (bs, T) or tuple(objects_mask.shape) != (bs, O):
            raise ValueError(f'inconsistent shapes: x_human {tuple(x_human.shape)}, x_objects {tuple(x_objects.shape)}, '
                             f'objects_mask {tuple(objects_mask.shape)}')
        if H < 1 or O < 1:
            raise ValueError('the baselines need at least one human and one object per clip')
        x_human = x_human.contiguous().float()
        x_objects = x_objects.contiguous().float()
        objects_mask = objects_mask.contiguous().float()
        plan = _Plan(bs, T, H, O, F_h, F_o, self.hidden_size, self.bidirectional, self.with_message_passing,
                     self.num_classes)
        sd = dict(self.named_parameters())
        names = used_parameter_names(plan, sd)
        out = BaselineFunction.apply(plan, names, x_human, x_objects, objects_mask, *[sd[n] for n in names])
        return list(out)


class BimanualBaseline(_Baseline):
    """vhoi/models.py:15-87."""
    _object_head = False


class CAD120Baseline(_Baseline):
    """vhoi/models.py:90-175."""
    _object_head = True


def select_model(model_name: str):
    """vhoi/models.py:1589-1595 (all three names)."""
    return {'bimanual_baseline': BimanualBaseline, 'cad120_baseline': CAD120Baseline, '2G-GCN': models.TGGCN}[model_name]


# ---------------------------------------------------------------------------------------------------------------
# losses (vhoi/losses.py:62-67, :72-91)
# ---------------------------------------------------------------------------------------------------------------
def select_loss(model_name: str, model_input_type: str, dataset_name: str, cfg):
    if model_name == 'bimanual_baseline':
        return partial(losses.multi_task_loss, loss_functions=(losses.nll_loss,)), ['NLL_SAR']
    if model_name == 'cad120_baseline':
        return partial(losses.multi_task_loss, loss_functions=(losses.nll_loss, losses.nll_loss)), ['NLL_SAR', 'NLL_OAR']
    if model_name == '2G-GCN':
        return losses.select_loss(model_name, model_input_type, dataset_name, cfg)
    raise ValueError(f'Unknown model {model_name}')


def select_loss_types(model_name: str, dataset_name: str, cfg):
    return losses.select_loss_types(model_name, dataset_name, cfg)   # (raises ValueError for the baselines, as the reference)


def select_loss_learning_mask(model_name: str, dataset_name: str, cfg):
    return losses.select_loss_learning_mask(model_name, dataset_name, cfg)


def decide_num_main_losses(model_name: str, dataset_name: str, misc_dict: dict):
    """vhoi/losses.py:103-112: None (every loss is a main loss) except for 2G-GCN."""
    if model_name != '2G-GCN':
        return None
    seg = misc_dict.get('segmentation_loss', {})
    if seg.get('add', False) and seg.get('pretrain', False):
        return 10 if dataset_name == 'cad120' else 5
    return 4 if dataset_name == 'cad120' else 2


# ---------------------------------------------------------------------------------------------------------------
# data (vhoi/data_loading.py:362-379, :436-501, :1215-1230, :1318-1340)
# ---------------------------------------------------------------------------------------------------------------
def assemble_tensors(data, model_name, model_input_type='multiple', sigma=0.0, downsampling=1, test_data=False):
    """CAD-120, :436-471. The baseline's arrays are slots of the 2G-GCN assembly: x_human (with the fake human
    dimension), x_objects, objects_mask; targets human then object recognition."""
    if model_name != 'cad120_baseline':
        return data_loading.assemble_tensors(data, model_name, model_input_type, sigma, downsampling, test_data)
    xs, ys = data_loading.assemble_tensors(data, '2G-GCN', model_input_type, sigma, downsampling, test_data)
    return xs[:3], [ys[4], ys[6]]


def assemble_bimanual_tensors(data, model_name, sigma=0.0, downsampling=1, test_data=False):
    """Bimanual, :480-501: x_human, x_objects, objects_mask; target human recognition."""
    if model_name != 'bimanual_baseline':
        return data_loading.assemble_bimanual_tensors(data, model_name, sigma, downsampling, test_data)
    xs, ys = data_loading.assemble_bimanual_tensors(data, '2G-GCN', sigma, downsampling, test_data)
    return xs[:3], [ys[2]]


def create_data_loader(data, model_name: str, model_input_type: str, dataset_name: str, batch_size: int, shuffle: bool,
                       scaling_strategy: Optional[str] = None, scalers: Optional[dict] = None, sigma: float = 0.0,
                       downsampling: int = 1, test_data: bool = False, pin_memory: bool = False,
                       length_bucketing: bool = False):
    """data_loading.create_data_loader, with the baseline names."""
    if model_name not in BASELINES:
        return data_loading.create_data_loader(data, model_name, model_input_type, dataset_name, batch_size, shuffle,
                                               scaling_strategy, scalers, sigma, downsampling, test_data, pin_memory,
                                               length_bucketing)
    if length_bucketing:
        raise ValueError('length_bucketing keys on the steps slot of the 2G-GCN tuple; the baselines have none')
    name = dataset_name.lower()
    if name == 'cad120':
        if model_name != 'cad120_baseline':
            raise ValueError(f'{model_name} is not an option for model name.')
        x, y = assemble_tensors(data, model_name, model_input_type, sigma, downsampling, test_data)
    elif name == 'mphoi':
        raise ValueError(f'MPHOI code not implemented for {model_name} yet.')
    else:
        if model_name != 'bimanual_baseline':
            raise ValueError(f'Bimanual code not implemented for {model_name} yet.')
        x, y = assemble_bimanual_tensors(data, model_name, sigma, downsampling, test_data)
    x, scalers = data_loading.maybe_scale_input_tensors(x, model_name, scaling_strategy=scaling_strategy, scalers=scalers)
    x = [np.nan_to_num(ix, copy=False, nan=0.0) for ix in x]
    tensors = [torch.from_numpy(np.ascontiguousarray(a)) for a in x + y]
    if pin_memory and torch.cuda.is_available():
        tensors = [t.pin_memory() for t in tensors]
    loader = DataLoader(TensorDataset(*tensors), batch_size=batch_size, shuffle=shuffle, num_workers=0, pin_memory=False,
                        drop_last=False)
    segmentations = data_loading.assemble_cad120_segmentations_from_frame_level_features(data) if name == 'cad120' else None
    return loader, scalers, segmentations


def baseline_fetcher(dataset, device, non_blocking: bool = False, n: int = 3):
    """pyrutils fetchers.multiple_input_multiple_output: the first n tensors are inputs, the rest targets."""
    to = lambda t: t.to(device, non_blocking=non_blocking)
    return [to(t) for t in dataset[:n]], [to(t) for t in dataset[n:]]


def baseline_feeder(model, data, **kwargs):
    """pyrutils forwarders.multiple_input_forward: model(*data)."""
    return model(*data)


def select_model_data_fetcher(model_name: str, model_input_type: str, **kwargs):
    if model_name in BASELINES:
        return partial(baseline_fetcher, n=3)
    return data_loading.select_model_data_fetcher(model_name, model_input_type, **kwargs)


def select_model_data_feeder(model_name: str, model_input_type: str, **kwargs):
    if model_name in BASELINES:
        return baseline_feeder
    return data_loading.select_model_data_feeder(model_name, model_input_type, **kwargs)


def determine_num_classes(model_name: str, model_input_type: str, dataset_name: str):
    return data_loading.determine_num_classes(model_name, model_input_type, dataset_name)


def input_size_from_data_loader(data_loader: DataLoader, model_name: str, model_input_type: str):
    if model_name in BASELINES:
        return data_loader.dataset[0][0].size(-1), data_loader.dataset[0][1].size(-1)
    return data_loading.input_size_from_data_loader(data_loader, model_name, model_input_type)


def load_bimanual_training_data(data_path, data_path_zarr, data_path_bbs_zarr, data_path_hps_zarr, model_name: str,
                                model_input_type: str, test_subject_id: int, video_id_to_video_fps: dict,
                                batch_size: int = 8, val_fraction: float = 0.2, seed: int = 42, debug: bool = False,
                                scaling_strategy=None, sigma: float = 0.0, downsampling: int = 1):
    """data_loading.load_bimanual_training_data (vhoi/data_loading.py:63-115), with the baseline names."""
    if model_name not in BASELINES:
        return data_loading.load_bimanual_training_data(
            data_path, data_path_zarr, data_path_bbs_zarr, data_path_hps_zarr, model_name, model_input_type,
            test_subject_id, video_id_to_video_fps, batch_size, val_fraction, seed, debug, scaling_strategy, sigma,
            downsampling)
    stores = {'feat': data_path_zarr, 'bbs': data_path_bbs_zarr, 'hps': data_path_hps_zarr}
    records, _ = data_loading._read_videos('bimanual', data_path, stores,
                                           lambda v: data_loading._bimanual_subject(v) != test_subject_id,
                                           video_id_to_video_fps)
    training_data, val_data = data_loading.split_train_test(records, test_fraction=val_fraction, seed=seed)
    if debug:
        training_data, val_data = training_data[:4], val_data[:1]
    train_loader, scalers, _ = create_data_loader(training_data, model_name, model_input_type, 'bimanual',
                                                  batch_size=batch_size, shuffle=True, scaling_strategy=scaling_strategy,
                                                  sigma=sigma, downsampling=downsampling, test_data=False)
    val_loader, _, _ = create_data_loader(val_data, model_name, model_input_type, 'bimanual', batch_size=len(val_data),
                                          shuffle=False, scalers=scalers, sigma=sigma, downsampling=downsampling,
                                          test_data=False)
    data_info = {'input_size': input_size_from_data_loader(train_loader, model_name, model_input_type)}
    return train_loader, val_loader, data_info, scalers


def load_bimanual_testing_data(data_path, data_path_zarr, data_path_bbs_zarr, data_path_hps_zarr, model_name: str,
                               model_input_type: str, test_subject_id: int, video_id_to_video_fps: dict,
                               batch_size: int, scalers: Optional[dict] = None, downsampling: int = 1):
    """data_loading.load_bimanual_testing_data (vhoi/data_loading.py:234-282), with the baseline names."""
    if model_name not in BASELINES:
        return data_loading.load_bimanual_testing_data(data_path, data_path_zarr, data_path_bbs_zarr, data_path_hps_zarr,
                                                       model_name, model_input_type, test_subject_id,
                                                       video_id_to_video_fps, batch_size, scalers, downsampling)
    stores = {'feat': data_path_zarr, 'bbs': data_path_bbs_zarr, 'hps': data_path_hps_zarr}
    records, ids = data_loading._read_videos('bimanual', data_path, stores,
                                             lambda v: data_loading._bimanual_subject(v) == test_subject_id,
                                             video_id_to_video_fps)
    test_loader, _, segmentations = create_data_loader(records, model_name, model_input_type, 'bimanual',
                                                       batch_size=batch_size, shuffle=False, scalers=scalers,
                                                       downsampling=downsampling, test_data=True)
    data_info = {'input_size': input_size_from_data_loader(test_loader, model_name, model_input_type)}
    return test_loader, data_info, segmentations, ids
