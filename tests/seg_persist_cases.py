"""The segment-level recurrence as ONE persistent launch, forward and backward (csrc/seg_persist.hip): case lists over the whole
range of make_plan(), the host function that deals the clips to chunks, picks the instance seg_persist_fwd_kernel<1, mo> /
seg_persist_bwd_kernel<1, mo, x3q1> and the pair mask of the Gram tiles. Shared by tests/test_seg_persist_cpu.py (the library's
launch-free report, twog_segrnn_persistent_plan at 256 compute units, against what every case claims; the specification in fp32
against fp64; the judgement against planted faults) and tests/test_seg_persist_gpu.py (the launches against both).

A case is the inputs of tests.kernel_cases._seg_params -- shape (bs, T, H, O, h) and the switchable optional inputs b_hh, b_smsg,
obj_mask, gates -- with the claims the report must confirm ON THE DEVICE THAT RUNS IT:
    inst       (mh, mo): 16-row tiles of a chunk's human / object rows, the template arguments of both kernels,
    x3q1       the third template argument of the backward kernel,
    cpc, n_chunks, last   clips per chunk, chunks per direction, clips of the last chunk (last < cpc: ragged),
    pair_mask  which Gram tiles hold two rows of one clip.
The claims are stated for 256 compute units. If make_plan() changes, the claim stays and the SHAPE is changed until it holds again:
the `why` says which branch the case is there for.

LAUNCHED: run by tests/test_seg_persist_gpu.py.  PINNED: the shapes the older persistent tests run (SEG_PERSIST_SHAPES of
tests/test_kernels_gpu.py, SEG_PERSISTENT of tests/entity_envelope.py): claims only, so that what those tests reach is on record and
counts towards coverage.  REFUSED: the report says "not served"; the wrapper runs the launch-per-step path."""
import functools

import torch

from tests import entity_envelope as EE
from tests.kernel_cases import rnd, _seg_params

N_CUS = 256   # the compute units the claims are stated for (MI355X)
M1, M2, M2X = 0x203, 0x40207, 0x40607   # the masks make_plan() can produce: one object tile; two; two with a clip across both
ALL_RELS = (True, True, True, True)


def _sc(id, why, shape, mo, cpc, n_chunks, last, pair_mask, zero=(), exact=(), **inputs):
    """zero: the judged tensors that are exactly 0 in this case (all of it; partial zeros are named by exact_zeros). exact: the judged
    tensors the specification reproduces exactly in both precisions -- relu(b_smsg) of a zero state, weights that are 0 or 1 and the
    messages they copy: e_ref = 0 by construction, not by accident, and the floor of the rule (4 x 2^-24) is the whole allowance."""
    bs, T, H, O, h = shape
    assert set(inputs) <= {'b_hh', 'b_smsg', 'obj_mask', 'gates'}, inputs
    return dict(id=id, why=why, shape=shape, bs=bs, T=T, H=H, O=O, h=h, inst=(1, mo), x3q1=h >= 256, cpc=cpc, n_chunks=n_chunks,
                last=last, pair_mask=pair_mask, zero=frozenset(zero), exact=frozenset(exact), inputs=inputs, rels=ALL_RELS, msg=True)


INSTANCES = [
    _sc('h128_mo2_straddle', 'the <1, 2> instances at h = 128 (nkb 4 / 8 / 12), never run before; a clip across the two object tiles',
        (8, 3, 2, 9, 128), 2, 2, 4, 2, M2X),
    _sc('h128_mo2_exact', '<1, 2> at h = 128 with 16 + 32 rows exactly and no clip across the object tiles', (32, 2, 2, 4, 128), 2, 8, 4, 8, M2),
    _sc('h64_mo2_cpc8', 'cpc = 8 at h = 64 (the older shapes stop at 2 there); mask without the (1, 2) tile below h = 512',
        (64, 2, 2, 4, 64), 2, 8, 8, 8, M2),
    _sc('h64_cpc16', 'cpc = 16, the largest the plan serves: every human row of the tile a clip of its own', (128, 2, 1, 2, 64), 2, 16, 8, 16, M2),
    _sc('h512_cpc16', 'cpc = 16 at h = 512: one chunk, every compute unit', (16, 3, 1, 2, 512), 2, 16, 1, 16, M2),
    _sc('h64_cpc3_30rows', 'cpc = 3 with 30 object rows: the second object tile partly filled, clip 1 across both', (24, 2, 2, 10, 64), 2, 3, 8, 3, M2X),
    _sc('h64_corner_cpc2', 'the entity corner (4 humans, 12 objects) with two clips per chunk: dw_pad 384', (16, 2, 4, 12, 64), 2, 2, 8, 2, M2X),
    _sc('h256_mo2_ragged', 'ragged last chunk with two object tiles (chunks of 3 and 2 clips: 18 and 12 object rows), x3q1',
        (5, 3, 3, 6, 256), 2, 3, 2, 2, M2X),
    _sc('h64_mo1_ragged', 'ragged last chunk with one object tile (chunks of 3, .., 2 clips)', (17, 3, 2, 4, 64), 1, 3, 6, 2, M1),
    _sc('h128_cpc9', 'cpc = 9: one row of each kind per clip, last chunk of 6', (33, 2, 1, 1, 128), 1, 9, 4, 6, M1, exact=('att',)),
    _sc('h256_mo_boundary', 'exactly 16 object rows: the last shape of mo = 1', (8, 3, 2, 4, 256), 1, 4, 2, 4, M1),
    _sc('h128_corner', 'the entity corner, one clip per chunk, h = 128', (2, 2, 4, 12, 128), 1, 1, 2, 1, M1),
    _sc('h256_corner', 'the entity corner, one clip per chunk, h = 256', (2, 3, 4, 12, 256), 1, 1, 2, 1, M1),
]
# one human and one object: no hh / oo sender, every other weight is 1 (att exact, mg a copy of msrc). Gates open and no object mask:
# with the default inputs the one human never moves and the one object is virtual. T = 1: every state read is 0, msrc = relu(b_smsg)
_ONE = dict(gates='open', obj_mask=None)
SEQUENCE = [
    _sc('one_row_T1', 'one row of each kind, grid 32; T = 1: first and last step coincide, no hand-off is waited for', (1, 1, 1, 1, 64), 1, 1, 1, 1, M1,
        exact=('att', 'msrc_h', 'msrc_o', 'mg_h', 'mg_o'), **_ONE),
    _sc('one_row_T2', 'T = 2: the only hand-offs are the first and the last', (1, 2, 1, 1, 512), 1, 1, 1, 1, M1, exact=('att',), **_ONE),
    _sc('one_row_T3', 'T = 3: one middle step', (1, 3, 1, 1, 256), 1, 1, 1, 1, M1, exact=('att',), **_ONE),
    _sc('mo2_T1', 'T = 1 with two object tiles', (8, 1, 2, 4, 512), 2, 8, 1, 8, M2, exact=('msrc_h', 'msrc_o')),
    _sc('mo2_T2', 'T = 2 with two object tiles', (8, 2, 2, 4, 512), 2, 8, 1, 8, M2),
    _sc('h64_T33', 'T = 33: a chain long enough for a stale hand-off or a wrong step index to compound (contractive weights)',
        (2, 33, 2, 3, 64), 1, 1, 2, 1, M1),
]
_OPT = ((4, 3, 2, 8, 128), 1, 1, 4, 1, M1)
OPTIONAL = [
    _sc('no_b_hh', 'b_hh_* = NULL: the `b ? .. : 0.f` arm; hn of the first step of each direction is exactly 0 in save', *_OPT, b_hh=False),
    _sc('no_b_smsg', 'b_smsg_* = NULL: msrc of the first step of each direction is exactly 0', *_OPT, b_smsg=False),
    _sc('no_obj_mask', 'obj_mask = NULL: the `P.mask ? .. : 1.f` arm, every object a valid sender', *_OPT, obj_mask=None),
]
_G1, _G2 = ((3, 4, 2, 5, 256), 1, 2, 2, 1, M1), ((8, 3, 2, 9, 128), 2, 2, 4, 2, M2X)
_CLOSED = ('hs_h', 'hs_o', 'd_gi_h', 'd_gi_o', 'd_gh_h', 'd_gh_o', 'd_pre_h', 'd_pre_o')
GATES = [_sc(f'{what}_{tag}', why, *shp, zero=zero, exact=exact, **inp) for tag, shp in (('mo1', _G1), ('mo2', _G2))
         for what, why, zero, exact, inp in (
    ('gates_closed', 'u = 0: no state ever leaves 0 -- the Gram tiles are zero, attention is uniform over the valid senders, nothing '
     'flows back through the gates; msrc = relu(b_smsg)', _CLOSED, ('msrc_h', 'msrc_o'), dict(gates='closed')),
    ('gates_open', 'u = 1: every step replaces the state', (), (), dict(gates='open')),
    ('all_masked', 'every object of every clip virtual: no valid object sender, the oh / oo weights and messages are exactly 0 and '
     'nothing flows back into the objects\' sender MLPs', ('d_pre_o',), (), dict(obj_mask='all')),
    ('one_valid', 'one valid object per clip: it has no valid object sender itself (its oo weights and message are exactly 0), every '
     'other receiver has exactly one (weight exactly 1)', (), (), dict(obj_mask='one_valid')))]
LAUNCHED = INSTANCES + SEQUENCE + OPTIONAL + GATES

PINNED = [_sc('pinned_' + 'x'.join(map(str, s)), 'a shape of the older persistent tests', s, *claim) for s, claim in (
    ((8, 120, 2, 4, 512), (2, 8, 1, 8, M2)), ((16, 120, 2, 9, 64), (2, 2, 8, 2, M2X)), ((1, 20, 1, 5, 512), (1, 1, 1, 1, M1)),
    ((8, 7, 2, 4, 512), (2, 8, 1, 8, M2)), ((5, 9, 2, 3, 128), (1, 2, 3, 1, M1)), ((3, 6, 1, 5, 256), (1, 2, 2, 1, M1)),
    ((13, 5, 2, 9, 64), (2, 2, 7, 1, M2X)), ((4, 6, 2, 8, 64), (1, 1, 4, 1, M1)), ((2, 1, 2, 4, 128), (1, 1, 2, 1, M1)),
    ((8, 6, 4, 12, 64), (1, 1, 8, 1, M1)), ((2, 7, 4, 12, 512), (2, 2, 1, 2, M2X)), ((4, 5, 4, 8, 512), (2, 4, 1, 4, M2)),
    ((3, 6, 3, 10, 256), (2, 2, 2, 1, M2X)))]


def _rf(id, why, shape, n_cus=N_CUS, rels=ALL_RELS, msg=True, step=True):
    """step False: the launch-per-step path rejects the shape too (its attention kernels take up to 4 humans and 12 objects) or the
    case is a statement about another device -- asserted from the report only."""
    c = _sc('refused_' + id, why, shape, 0, 0, 0, 0, 0)
    c.update(inst=None, n_cus=n_cus, rels=rels, msg=msg, step=step)
    return c


REFUSED = [
    _rf('mh2', '18 human rows in the one chunk h = 512 leaves room for: mh = 2', (9, 3, 2, 4, 512)),
    _rf('mo3_h512', '36 object rows in one chunk: mo = 3', (3, 3, 4, 12, 512)),
    _rf('mo3_h128', 'chunks of 3 clips x 12 objects = 36 object rows at h = 128', (9, 2, 1, 12, 128)),
    _rf('h96', 'hidden not 64 / 128 / 256 / 512', (3, 3, 2, 4, 96)),
    _rf('H5', 'more than 4 humans', (2, 3, 5, 4, 64), step=False),
    _rf('O13', 'more than 12 objects', (2, 3, 2, 13, 64), step=False),
    _rf('no_hh', 'relation human -> human off', _OPT[0], rels=(False, True, True, True)),
    _rf('no_ho', 'relation human -> object off', _OPT[0], rels=(True, False, True, True)),
    _rf('no_oh', 'relation object -> human off', _OPT[0], rels=(True, True, False, True)),
    _rf('no_oo', 'relation object -> object off', _OPT[0], rels=(True, True, True, False)),
    _rf('no_msg', 'message_segment off', _OPT[0], msg=False),
    _rf('h512_128cus', 'h = 512 needs 8 x 32 = 256 workgroups for one chunk: not on 128 compute units', (1, 3, 1, 1, 512), n_cus=128, step=False),
]
BY_ID = {c['id']: c for c in LAUNCHED + PINNED + REFUSED}
CLAIM_KEYS = ('inst', 'x3q1', 'cpc', 'n_chunks', 'last', 'pair_mask')


def claimed(plan):
    """What a report (kernels.segrnn_persistent_plan / _lib.segrnn_persistent_plan) says in the terms of a case's claims."""
    return dict(inst=(plan['mh'], plan['mo']), x3q1=plan['x3q1'], cpc=plan['cpc'], n_chunks=plan['n_chunks'], last=plan['last'],
                pair_mask=plan['pair_mask'])


def claims(c):
    return {k: c[k] for k in CLAIM_KEYS}


def plan_args(c):
    """Arguments of segrnn_persistent_plan after n_cus."""
    return dict(msg_segment=c['msg'], rels=c['rels'])


def pair_mask_of(cpc, H, O):
    """The pair mask from its definition: bit (8 i + j), i <= j, for every pair of 16-row tiles (humans: tile 0, since cpc x H <= 16;
    objects: from tile 1) that hold two rows -- or the same row twice -- of one clip."""
    mask = 0
    for b in range(cpc):
        tiles = {(b * H + e) // 16 for e in range(H)} | {1 + (b * O + e) // 16 for e in range(O)}
        for i in tiles:
            for j in tiles:
                if i <= j:
                    mask |= 1 << (8 * i + j)
    return mask


# ------------------------------------------------------------------------------------------------------- inputs and specification
def params(c, dev):
    bs, T, H, O, h = c['shape']
    return _seg_params(dev, bs, T, H, O, h, c['rels'], c['msg'], **c['inputs'])


def fwd_keys(c):
    return EE.SEG_FWD_KEYS if c['msg'] else ['hs_h', 'hs_o', 'save_h', 'save_o']   # without messages msrc / mg / att are never written


def bwd_keys(c, o):
    return [k for k in sorted(o) if c['msg'] or not k.startswith('d_pre')]


def judged_rows(c, k, t):
    """The tensor as entity_envelope.judge takes it: rows are the vectors of the last dimension -- except d_u_* [bs][T][E], whose rows
    are the CHUNKS of the plan, [n_chunks][cpc x T x E] (a ragged last chunk padded with zeros, which add no error and no scale; a
    refused shape has no chunks: its rows are the clips).

    Why. An element of d_u is ONE scalar, a sum of 2h signed products that largely cancel, and E can be 1. The row-wise rule divides
    the largest kernel error of a row by the largest specification error of the same row. Over a row of one element that is the
    ratio of two independent errors of one number each, which exceeds a factor f with probability about 2 / (pi f) whatever the
    kernel does; over a row of n elements the specification's largest error falls below 1 / f of the kernel's with probability about
    (1.5 / f)^n. A perfect kernel passes f = 8 on some hundred rows only from n = 6 or so: rows of E = 1 .. 4 scalars cannot be
    judged one by one. What the row-wise rule is for -- an error confined to a small part, hidden by the tensor-wide maximum -- has
    for d_u the form "one chunk, or one clip of it, is wrong" (a clip index, the last clip of a ragged chunk, a lost slice of a
    group's partial sums). Every element of d_u has the same scale (2h products of O(1) terms), so such a fault is O(1) of its
    row's largest value, five orders of magnitude above the rule, in a row of one chunk as in a row of one clip."""
    if not k.startswith('d_u'):
        return t
    cpc = c['cpc'] or 1
    t = t.reshape(c['bs'], -1)
    if c['bs'] % cpc:
        t = torch.cat([t, t.new_zeros(cpc - c['bs'] % cpc, t.shape[1])])
    return t.reshape(-1, cpc * t.shape[1])


@functools.lru_cache(maxsize=2)
def _spec(id):
    c = BY_ID[id]
    bs, T, H, O, h = c['shape']
    p32 = params(c, 'cpu')
    p64 = EE.to64(p32)
    wih_h, wih_o = p64['_keep']   # the message blocks of W_ih are views of the whole matrices: rebuilt from the fp64 copies
    p64['w_ihm_h'], p64['w_ihm_o'] = [w[:, 3 * h:] for w in wih_h], [w[:, 4 * h:] for w in wih_o]
    b32, b64 = EE.F.segrnn_fwd(p32), EE.F.segrnn_fwd(p64)
    dh_h, dh_o = rnd(bs, T, H, 2 * h, seed=31), rnd(bs, T, O, 2 * h, seed=32)
    o32 = EE.F.segrnn_bwd(p32, b32, dh_h, dh_o)
    o64 = EE.F.segrnn_bwd(p64, EE.to64(b32), dh_h.double(), dh_o.double())
    return b32, b64, (dh_h, dh_o), o32, o64


def spec(c):
    """As entity_envelope.seg_spec with the case's inputs: (forward buffers fp32 / fp64, incoming gradients, backward outputs fp32 /
    fp64); both backward runs read the fp32 forward buffers, as the kernel under test does. Cached: do not write into the result."""
    return _spec(c['id'])


def first_steps(c):
    """(direction, t) of the first step of each direction: the step whose previous state is 0."""
    return ((0, 0), (1, c['T'] - 1))


def exact_zeros(c, b):
    """{name: view of the forward buffers b} that the case's inputs make exactly 0 (beside whole tensors, c['zero'])."""
    bs, T, H, O, h = c['shape']
    i, z = c['inputs'], {}
    for d, t in first_steps(c):
        for k in ('h', 'o'):
            if i.get('b_hh') is False:
                z[f'save_{k}[{d}, :, {t}] hn'] = b['save_' + k][d, :, t, :, 3 * h:]
            if i.get('b_smsg') is False:
                z[f'msrc_{k}[{d}, :, {t}]'] = b['msrc_' + k][d, :, t]
    att_oo = b['att'][..., H * H + 2 * H * O:].reshape(2, T, bs, O, O)
    if i.get('obj_mask') == 'all':
        z['att oh'], z['att oo'] = b['att'][..., H * H:H * H + H * O], att_oo
        z['mg_h oh'], z['mg_o oo'] = b['mg_h'][..., h:], b['mg_o'][..., h:]
    if i.get('obj_mask') == 'one_valid':
        clip, valid = torch.arange(bs), torch.arange(bs) % O
        z['att oo of the valid object'] = att_oo[:, :, clip, valid]
        z['mg_o oo of the valid object'] = b['mg_o'][:, clip, :, valid][..., h:]
    return z


def uniform_attention_failures(c, att):
    """Gates closed: every score is 0, so every receiver's weights are 1 / (its valid senders) on them and 0 elsewhere, to 2 ulp."""
    bs, T, H, O, h = c['shape']
    p = params(c, 'cpu')
    m = (p['obj_mask'] if p['obj_mask'] is not None else torch.ones(bs, O)) != 0
    eyeH, eyeO = torch.eye(H, dtype=torch.bool), torch.eye(O, dtype=torch.bool)
    ok = {'att_hh': (~eyeH).expand(bs, H, H), 'att_oh': m.unsqueeze(1).expand(bs, H, O), 'att_ho': torch.ones(bs, O, H, dtype=torch.bool),
          'att_oo': (~eyeO).unsqueeze(0) & m.unsqueeze(1)}
    fails = []
    att = att.detach().cpu().double().reshape(2 * T, bs, -1)
    for dt in range(2 * T):
        for k, w in EE.split_att(att[dt], bs, H, O).items():
            v = ok[k].reshape(w.shape).double()
            want = v / v.sum(-1, keepdim=True).clamp_min(1.0)
            if float((w - want).abs().max()) > 2 * EE.EPS:
                fails.append(f'{k} of (direction, step) {divmod(dt, T)}: not uniform over the valid senders')
    return fails


# ------------------------------------------------------------------------------------------------------- planted faults
def chunk_of_clips(c):
    """[(first clip, clips)] of every chunk."""
    return [(b0, min(c['cpc'], c['bs'] - b0)) for b0 in range(0, c['bs'], c['cpc'])]


def plant_stale_hand_off(c, b):
    """Forward direction: the states of step t - 1 in place of step t (what a consumer reads when it does not wait)."""
    h, out = c['h'], {k: v.clone() for k, v in b.items()}
    for k in ('hs_h', 'hs_o'):
        out[k][:, 1:, :, :h] = b[k][:, :-1, :, :h]
    return out, ('hs_h', 'hs_o')


def plant_ragged_clip_lost(c, b):
    """The rows of the last clip of the ragged last chunk are zero (a chunk always worked as if it were full, or never past `last`)."""
    assert c['last'] < c['cpc']
    out = {k: v.clone() for k, v in b.items()}
    for k in ('hs_h', 'hs_o'):
        out[k][c['bs'] - 1] = 0
    return out, ('hs_h', 'hs_o')


def plant_object_tiles_swapped(c, b):
    """The clip whose objects lie across the two object tiles: its rows of the second tile and as many of the first change places."""
    O, out = c['O'], {k: v.clone() for k, v in b.items()}
    bl = next(bl for bl in range(c['cpc']) if bl * O < 16 < (bl + 1) * O)   # first clip of chunk 0 across the boundary
    n2 = (bl + 1) * O - 16
    out['hs_o'][bl, :, :n2], out['hs_o'][bl, :, O - n2:] = b['hs_o'][bl, :, O - n2:], b['hs_o'][bl, :, :n2]
    return out, ('hs_o',)


# (case id, fault): each needs a case that has the structure the fault is about
PLANTED = [('h64_T33', plant_stale_hand_off), ('h128_mo2_straddle', plant_stale_hand_off), ('h256_mo2_ragged', plant_ragged_clip_lost),
           ('h64_mo1_ragged', plant_ragged_clip_lost), ('h128_mo2_straddle', plant_object_tiles_swapped),
           ('h64_cpc3_30rows', plant_object_tiles_swapped)]
