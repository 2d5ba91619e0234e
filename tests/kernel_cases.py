"""Seeded case builders shared by the kernel-level tests (tests/test_kernels_gpu.py, tests/test_entity_envelope_*.py) and by
the tools that reuse them: inputs of the entity attention and of the segment-level recurrence in the layouts the product
path uses (operands that are column blocks of wider rows, masked and all-virtual clips)."""
import math

import torch


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).float()


def _attn_case(dev, H, O, D, h, n_inst, ipc, geo, recv_mask, seed=0):
    t = lambda *s, sd=0: rnd(*s, seed=seed + sd).to(dev)
    W = 3 * h
    d = dict(feat_h=t(n_inst * H, D + 8, sd=1)[:, :D], feat_o=t(n_inst * O, D, sd=2),
             msg_hh=t(n_inst * H, 2 * h, sd=3)[:, :h], msg_ho=t(n_inst * H, 2 * h, sd=4)[:, h:],
             msg_oh=t(n_inst * O, h, sd=5), msg_oo=t(n_inst * O, h, sd=6),
             out_hh=torch.zeros(n_inst * H, W, device=dev)[:, :h], out_oh=torch.zeros(n_inst * H, W, device=dev)[:, h:2 * h],
             out_ho=torch.zeros(n_inst * O, W, device=dev)[:, :h], out_oo=torch.zeros(n_inst * O, W, device=dev)[:, 2 * h:],
             att=torch.zeros(n_inst, H * H + 2 * H * O + O * O, device=dev), n_inst=n_inst, inst_per_clip=ipc, H=H, O=O,
             D=D, hidden=h, scale=1.0 / math.sqrt(D), recv_mask_ho=recv_mask)
    mask = (rnd(n_inst // ipc, O, seed=seed + 7) > -0.3).float()
    mask[0] = 0.0  # a clip with only virtual objects (NaN -> 0 path)
    d['obj_mask'] = mask.to(dev)
    if geo:
        d.update(msg_so=t(n_inst, h, sd=8), msg_sh=t(n_inst, h, sd=9),
                 out_so=torch.zeros(n_inst * O, h, device=dev), out_sh=torch.zeros(n_inst * H, h, device=dev))
    return d


def _seg_params(dev, bs, T, H, O, h, rels, msg_segment=True, seed=0, b_hh=True, b_smsg=True, obj_mask='two_clips', gates='random'):
    """b_hh / b_smsg False: the descriptor carries no such bias (None). obj_mask: 'two_clips' (the last object of clip 0 and every
    object of clip 1 virtual), None (no mask: every object valid), 'all' (every object of every clip virtual), 'one_valid' (object
    b % O of clip b is the only valid one). gates: 'random' 0 / 1, 'closed' (u = 0: no state ever changes), 'open' (u = 1)."""
    w_sc = 0.3 if h <= 64 else 0.3 * math.sqrt(64.0 / h)   # keep pre-activations O(1) at full width
    if T > 32:
        w_sc = 0.4 / math.sqrt(h)   # long chains: contractive dynamics, so rounding differences do not amplify over T
    t = lambda *s, sd=0, sc=None: rnd(*s, seed=seed + sd, scale=w_sc if sc is None else sc).to(dev)
    rel_hh, rel_ho, rel_oh, rel_oo = rels
    nmh, nmo = int(rel_hh) + int(rel_oh), int(rel_ho) + int(rel_oo)
    nsh, nso = int(rel_hh) + int(rel_ho), int(rel_oh) + int(rel_oo)
    fw_h, fw_o = 3 * h, 4 * h
    wih_h = [t(3 * h, fw_h + nmh * h, sd=1 + d) for d in range(2)]
    wih_o = [t(3 * h, fw_o + nmo * h, sd=3 + d) for d in range(2)]
    if obj_mask == 'two_clips':
        mask = torch.ones(bs, O)
        mask[0, O - 1] = 0
        if bs > 1:
            mask[1] = 0
    elif obj_mask == 'all':
        mask = torch.zeros(bs, O)
    elif obj_mask == 'one_valid':
        mask = torch.zeros(bs, O)
        mask[torch.arange(bs), torch.arange(bs) % O] = 1
    else:
        assert obj_mask is None, obj_mask
        mask = None
    gate = {'random': lambda g: g, 'closed': torch.zeros_like, 'open': torch.ones_like}[gates]
    bias = lambda on, *s, sd: [t(*s, sd=sd + d) if on else None for d in range(2)]
    p = dict(bs=bs, T=T, H=H, O=O, hidden=h, msg_segment=msg_segment, rel_hh=rel_hh, rel_ho=rel_ho, rel_oh=rel_oh,
             rel_oo=rel_oo, att_scale=1 / math.sqrt(h), gi_h=t(bs, T, H, 6 * h, sd=5, sc=1.0), gi_o=t(bs, T, O, 6 * h, sd=6, sc=1.0),
             u_h=gate((rnd(bs, T, H, seed=seed + 7) > 0).float()).to(dev), u_o=gate((rnd(bs, T, O, seed=seed + 8) > 0).float()).to(dev),
             obj_mask=None if mask is None else mask.to(dev),
             w_hh_h=[t(3 * h, h, sd=9 + d) for d in range(2)], b_hh_h=bias(b_hh, 3 * h, sd=11),
             w_hh_o=[t(3 * h, h, sd=13 + d) for d in range(2)], b_hh_o=bias(b_hh, 3 * h, sd=15),
             w_ihm_h=[w[:, fw_h:] for w in wih_h], w_ihm_o=[w[:, fw_o:] for w in wih_o],
             ld_ih_h=fw_h + nmh * h, ld_ih_o=fw_o + nmo * h,
             w_smsg_h=t(max(nsh, 1) * h, h, sd=17)[:nsh * h], b_smsg_h=t(max(nsh, 1) * h, sd=18)[:nsh * h] if b_smsg else None,
             w_smsg_o=t(max(nso, 1) * h, h, sd=19)[:nso * h], b_smsg_o=t(max(nso, 1) * h, sd=20)[:nso * h] if b_smsg else None)
    p['_keep'] = (wih_h, wih_o)
    return p


def attn_bwd_case(dev, d, D=None, seed=100, dw_extra=False):
    """Backward descriptor on top of the forward case d: gradients accumulate into non-zero feature-gradient buffers,
    ReLU mask on the message gradients, one incoming gradient per relation that is on."""
    n_inst, H, O, h = d['n_inst'], d['H'], d['O'], d['hidden']
    D = d['D'] if D is None else D
    t = lambda *s, sd=0: rnd(*s, seed=seed + sd).to(dev)
    natt = H * H + 2 * H * O + O * O
    b = dict(f=d, dfeat_accumulate=1, relu_mask_dmsg=1, dfeat_h=t(n_inst * H, D, sd=1), dfeat_o=t(n_inst * O, D, sd=2),
             dw_extra=t(n_inst, natt, sd=3) if dw_extra else None)
    for i, (rel, R) in enumerate((('hh', H), ('oh', H), ('ho', O), ('oo', O), ('so', O), ('sh', H))):
        if d.get('msg_' + rel) is None:
            continue
        b['dout_' + rel] = t(n_inst * R, h, sd=10 + i)
        S_ = {'hh': H, 'ho': H, 'oh': O, 'oo': O, 'so': 0, 'sh': 0}[rel]
        b['dmsg_' + rel] = torch.zeros(n_inst * S_ if S_ else n_inst, h, device=dev)
    return b
