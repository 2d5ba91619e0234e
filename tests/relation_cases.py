"""The general single-relation kernels (csrc/relation.hip) at their limits: the case list, seeded inputs, and runners that execute
a case on the executable specification (tests/fake_kernels.py, fp32 or fp64 on the CPU) or on the HIP kernels. Shared by
tests/test_relation_kernels_cpu.py (the list and the specification themselves) and tests/test_relation_kernels_gpu.py (the
kernels against both specification runs, judged by tests.entity_envelope.judge).

run(Kx, c, dev, dtype) builds the inputs of case c as seeded fp32 tensors on the CPU, casts them to dtype on dev (all three runs
see identical values), calls relation_fwd and relation_bwd of Kx and returns {name: (tensor, how)}:
  JUDGE  a floating-point result: out, att, dmsg, dp_r, dp_s, dq, dk, da_r, dc_s, dscore_sum (one value per instance);
  EXACT  must be bit-equal to the fp32 specification: `<name>_outside`, the whole backing buffer of a written operand with the
         written view zeroed (every buffer is pre-filled with seeded values: what the call leaves outside the view must be those),
         and dq / dk of the modes without scores (zeros when overwritten, the pre-filled values when accumulated into).

What the shapes are for (read off relation.hip): wdot, the weight-gradient loop and the two ReLU-pair loops advance by 64 lanes,
so D and hidden around 64 and far beyond it make them turn with and without a ragged tail; R = S = 16 fills the five 256-float LDS
arrays, gives each of the four waves 64 trips over the pairs and fills the `threadIdx.x < R` / `64 <= threadIdx.x < 64 + S`
branches. The `why` of a case names what it is there for; the CPU test asserts from the list that every claim is met.

Sign decisions. a + c > 0 (pair ReLU), a_r + c_s > 0 (additive score), msg > 0, mask == 0 and dist == 0 are decided alike in fp32
and fp64 on the same fp32 inputs (a sum of two floats rounds to zero only when it is zero). The sign of scale <q, k> + bias under
relu_scores can depend on the summation order: relu_margin() measures how far every pair of such a case is from the band
16 x 2^-24 x (scale <|q|, |k|> + |bias|), and the CPU test asserts that no pair lies inside (a condition on the seeds)."""
import math

import torch

from tests.fake_kernels import FakeKernels
from tests.kernel_cases import rnd
from tests.entity_envelope import EPS

F = FakeKernels()
EXACT, JUDGE = 'exact', 'judge'
SUM, DOT, ADDITIVE, DISTANCE, MEAN = F.REL_SUM, F.REL_DOT, F.REL_ADDITIVE, F.REL_DISTANCE, F.REL_MEAN
SENDER, PAIR = F.REL_MSG_SENDER, F.REL_MSG_PAIR
SCORED = (DOT, ADDITIVE)
MAXE, MAXREL_F, MAXREL_B = 16, 8, 6   # entity limit, descriptors per forward / backward launch (relation.hip)
GUARD = 8                              # pre-filled floats on either side of a flat output
RELU_BAND = 16 * EPS
# The raw dot scores are about N(0, 1) (scale = 1 / sqrt(D)): a bias of that size can push nearly every pair of a case below the
# ReLU, which leaves receivers with one surviving pair or none -- rows that test nothing (all zero) or a single cancellation
# w (dw - t). A quarter of it keeps both branches of the ReLU well populated; the CPU test asserts the share of positive pairs.
BIAS_SCALE = 0.25
HIDDEN_WIDTHS, D_WIDTHS = (1, 63, 64, 65, 300, 512), (1, 63, 64, 65, 200)
ROW_OPERANDS = ('q', 'k', 'msg', 'p_r', 'p_s', 'out', 'dout', 'dmsg', 'dp_r', 'dp_s', 'dq', 'dk')
f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))   # a scalar as the value the C ABI (float) receives


def _c(id, score, msg, R, S, why, D=0, h=40, n_inst=6, ipc=2, excl=0, smask=0, rmask=0, relu=0, views='dense', grads=None,
       self_rel=0, zero_dist_recv=0, relu_mask_dmsg=1, row_factors=None):
    """grads = (dq_accumulate, dk_accumulate): dq and dk are given (None: they are not). views: how every row operand of the case
    arrives ('dense', 'cols': a 2-D column block of a wider buffer at an offset that is no multiple of 4, '3d': a (n_inst, n, w)
    view of a padded buffer). row_factors: {tensor: factor of the row-wise rule}, stated with its reason where one is needed."""
    assert grads is not None or score != DOT
    return dict(id=id, score=score, msg=msg, R=R, S=S, D=D, hidden=h, n_inst=n_inst, ipc=ipc, excl=excl, smask=smask, rmask=rmask,
                relu=relu, views=views, grads=grads, self_rel=self_rel, zero_dist_recv=zero_dist_recv,
                relu_mask_dmsg=relu_mask_dmsg, row_factors=row_factors or {}, why=why, desc_R=R)


CASES = [
    # ---- the entity limit, every score mode x message mode the host composes (ops._relation_fwd)
    _c('lim_sum_pair', SUM, PAIR, 16, 16, 'relational objects -> object at the limit; dq zeroed, dk left alone', D=65, h=65, excl=1,
       smask=1, grads=(0, 1)),
    _c('lim_mean_pair', MEAN, PAIR, 16, 16, 'mean pooling of pair messages at the limit; dq left alone, dk zeroed', D=63, h=63,
       excl=1, smask=1, grads=(1, 0)),
    _c('lim_dot_sender', DOT, SENDER, 16, 16, 'dot attention at the limit, D = 200 (4 trips of wdot, ragged), hidden = 300; both '
       'feature gradients accumulate', D=200, h=300, excl=1, rmask=1, grads=(1, 1)),
    _c('lim_dot_pair', DOT, PAIR, 16, 16, 'receiver-specific + dot at the limit, D = hidden = 64: exactly one trip; neither '
       'feature gradient accumulates', D=64, h=64, excl=1, smask=1, grads=(0, 0)),
    _c('lim_dot_relu_sender', DOT, SENDER, 16, 16, 'bilinear form (relu + bias) at the limit, hidden = 512: 8 full trips; '
       'dscore_sum per instance', D=200, h=512, relu=1, excl=1, smask=1, rmask=1, grads=(1, 0)),
    _c('lim_dot_relu_pair', DOT, PAIR, 16, 16, 'bilinear + receiver-specific at the limit, D = 63, hidden = 65', D=63, h=65, relu=1,
       excl=1, grads=(0, 1)),
    _c('lim_add_sender', ADDITIVE, SENDER, 16, 16, 'concat attention at the limit: the R and the 64 + S thread branches full',
       h=300, excl=1, smask=1, rmask=1),
    _c('lim_add_pair', ADDITIVE, PAIR, 16, 16, 'concat + receiver-specific at the limit, hidden = 300', h=300, excl=1, smask=1),
    _c('lim_dist_sender', DISTANCE, SENDER, 16, 16, 'distance attention at the limit; one receiver with all distances 0; dq zeroed, '
       'dk left alone', D=5, h=64, excl=1, smask=1, rmask=1, zero_dist_recv=1, grads=(0, 1)),
    _c('lim_dist_pair', DISTANCE, PAIR, 16, 16, 'distance attention over pair messages at the limit', h=63, excl=1),
    _c('lim_mean_sender', MEAN, SENDER, 16, 16, 'mean pooling at the limit; dq and dk both zeroed', D=3, h=65, excl=1, smask=1,
       rmask=1, grads=(0, 0)),
    # ---- rectangular relations
    _c('rect_16x1_sum_sender', SUM, SENDER, 16, 1, 'geometry -> objects: one sender, receiver mask; dq left alone, dk zeroed', D=4,
       h=64, rmask=1, grads=(1, 0)),
    _c('rect_1x16_dot_sender', DOT, SENDER, 1, 16, 'one receiver; D = 1 and hidden = 1: 63 idle lanes', D=1, h=1, smask=1,
       grads=(1, 0)),
    _c('rect_13x16_add_pair', ADDITIVE, PAIR, 13, 16, 'R < S = 16: r * S + s differs from r * 16 + s only in rows; hidden = 63',
       h=63, smask=1),
    _c('rect_5x3_dot_relu_pair', DOT, PAIR, 5, 3, 'R > S, both odd; D = 65, hidden = 300', D=65, h=300, relu=1, grads=(1, 0)),
    _c('rect_1x1_excl_dot_sender', DOT, SENDER, 1, 1, 'no valid sender at all: weights, outputs and gradients exactly 0, no NaN', D=8,
       h=8, excl=1, grads=(0, 0)),
    _c('rect_1x1_excl_mean_pair', MEAN, PAIR, 1, 1, 'no valid sender, mean pooling: count clamps to 1', D=8, h=8, excl=1,
       grads=(0, 1)),
    # ---- widths around the 64-lane stride at few entities
    _c('w_dot_pair_D1_h1', DOT, PAIR, 3, 5, 'D = 1, hidden = 1 with pair messages', D=1, h=1, grads=(0, 0)),
    _c('w_dot_sender_D63_h63', DOT, SENDER, 4, 3, 'one trip, the last lane idle', D=63, h=63, grads=(1, 1)),
    _c('w_dot_sender_D64_h64', DOT, SENDER, 3, 4, 'one full trip; dmsg without the folded ReLU mask', D=64, h=64, grads=(0, 1),
       relu_mask_dmsg=0),
    _c('w_dot_relu_sender_D65_h65', DOT, SENDER, 3, 5, 'a second trip of one lane; relu + bias', D=65, h=65, relu=1, grads=(1, 0)),
    _c('w_dot_pair_D200_h512', DOT, PAIR, 3, 4, 'D = 200, hidden = 512 with pair messages', D=200, h=512, grads=(1, 0)),
    _c('w_add_sender_h1', ADDITIVE, SENDER, 4, 6, 'hidden = 1 under additive scores', h=1, smask=1),
    _c('w_add_pair_h512', ADDITIVE, PAIR, 4, 3, 'hidden = 512 under additive scores, pair messages', h=512),
    # ---- instances
    _c('inst_n1', DOT, PAIR, 3, 4, 'one instance, one instance per clip', D=24, h=40, n_inst=1, ipc=1, grads=(1, 1)),
    _c('inst_n8_ipc4', ADDITIVE, SENDER, 7, 9, 'n_inst = 8 with four instances per clip: the second clip fully masked', h=40,
       n_inst=8, ipc=4, smask=1, rmask=1),
    _c('inst_n3_ipc1', SUM, PAIR, 2, 4, 'three clips of one instance', h=24, n_inst=3, ipc=1, smask=1),
    # ---- views: every row operand as a column block and as a 3-D view (dist is a transposed view in every distance case)
    _c('view_cols_dot_sender', DOT, SENDER, 5, 7, 'q, k, msg, out, dout, dmsg, dq, dk as column blocks at odd offsets', D=24, h=40,
       rmask=1, views='cols', grads=(1, 0)),
    _c('view_3d_dot_sender', DOT, SENDER, 5, 7, 'q, k, msg, out, dout, dmsg, dq, dk as 3-D views of padded buffers', D=24, h=40,
       smask=1, views='3d', grads=(0, 1)),
    _c('view_cols_dot_pair', DOT, PAIR, 7, 5, 'p_r, p_s, dp_r, dp_s (and the rest) as column blocks at odd offsets', D=65, h=63,
       views='cols', grads=(0, 1)),
    _c('view_3d_dot_pair', DOT, PAIR, 7, 5, 'p_r, p_s, dp_r, dp_s (and the rest) as 3-D views of padded buffers', D=65, h=63,
       views='3d', grads=(1, 0)),
    _c('view_3d_4x1_sum_sender', SUM, SENDER, 4, 1, '3-D views with one row per instance on the sender side (inner == 1)', D=6, h=24,
       views='3d', grads=(0, 0)),
    # ---- feature gradients
    _c('self_dot_sender_16', DOT, SENDER, 16, 16, 'the self relation: q and k the same rows, dq and dk the same buffer, both '
       'accumulating; D = 65', D=65, h=40, excl=1, self_rel=1, grads=(1, 1)),
    _c('fg_dist_sender', DISTANCE, SENDER, 3, 6, 'distance attention: dq left alone, dk zeroed', D=24, h=40, smask=1, grads=(1, 0)),
]
for _k, _case in enumerate(CASES):
    _case['seed'] = 1000 * (_k + 1)
BY_ID = {c['id']: c for c in CASES}


def case(id, **override):
    """A case of the list, or a variant of one (desc_R = 0: the descriptor announces no receivers over the same buffers)."""
    return dict(BY_ID[id], **override) if override else BY_ID[id]


# The descriptors of the multi-descriptor calls: more than one chunk (8 forward / 6 backward descriptors per launch), different
# n_inst within a chunk with the largest never first, one R = 0 descriptor in the middle of the first chunk. The first
# MANY_*_SHORT of each list end in a chunk of a single descriptor.
R0 = dict(desc_R=0)
MANY_FWD = [('w_dot_pair_D1_h1', {}), ('inst_n1', {}), ('inst_n8_ipc4', {}), ('rect_5x3_dot_relu_pair', R0), ('view_cols_dot_sender', {}),
            ('inst_n3_ipc1', {}), ('lim_dot_relu_sender', {}), ('view_3d_dot_pair', {}),
            ('inst_n3_ipc1', {}), ('lim_add_pair', {}), ('rect_16x1_sum_sender', {})]
MANY_BWD = [('view_cols_dot_pair', {}), ('inst_n1', {}), ('inst_n8_ipc4', R0), ('inst_n8_ipc4', {}), ('lim_sum_pair', {}),
            ('inst_n3_ipc1', {}),
            ('inst_n1', {}), ('self_dot_sender_16', {})]
MANY_FWD_SHORT, MANY_BWD_SHORT = MAXREL_F + 1, MAXREL_B + 1


def chunks(entries, per_launch):
    return [entries[i:i + per_launch] for i in range(0, len(entries), per_launch)]


# ------------------------------------------------------------------------------------------------------------- inputs
def cv(t, dev, dtype):
    return t.to(dev, dtype, copy=True)


def _row_operand(c, n, w, seed, dev, dtype):
    """-> (backing buffer, the view the call receives) of n rows of w columns per instance."""
    nI = c['n_inst']
    if c['views'] == 'cols':
        off = (1, 2, 3, 5, 6, 7)[seed % 6]
        b = cv(rnd(nI * n, w + 9, seed=seed), dev, dtype)
        return b, b[:, off:off + w]
    if c['views'] == '3d':
        b = cv(rnd(nI, n + 2, w + 3, seed=seed), dev, dtype)
        return b, b[:, 1:1 + n, 2:2 + w]
    b = cv(rnd(nI * n, w, seed=seed), dev, dtype)
    return b, b


def send_mask_of(c):
    """Clips in turn: random, all senders masked, exactly one valid sender."""
    n_clip, S = c['n_inst'] // c['ipc'], c['S']
    m = (rnd(n_clip, S, seed=c['seed'] + 40) > -0.4).float()
    for clip in range(n_clip):
        if clip % 3 == 1:
            m[clip] = 0.0
        elif clip % 3 == 2:
            m[clip] = 0.0
            m[clip, (5 * clip + 2) % S] = 1.0
    return m


def recv_mask_of(c):
    n_clip, R = c['n_inst'] // c['ipc'], c['R']
    m = (rnd(n_clip, R, seed=c['seed'] + 41) > -0.4).float()
    m[0, 0], m[0, -1] = 0.0, 1.0 if R > 1 else 0.0
    return m


def dist_of(c):
    """(n_inst, S, R), to be passed transposed: at or above 0.05, or exactly 0 ("no such sender")."""
    nI, R, S = c['n_inst'], c['R'], c['S']
    dist = rnd(nI, S, R, seed=c['seed'] + 42).abs() + 0.05
    dist[rnd(nI, S, R, seed=c['seed'] + 43) > 1.0] = 0.0
    if c['zero_dist_recv']:
        dist[:, :, R // 2] = 0.0
    return dist


def build(c, dev, dtype):
    """-> (forward descriptor d, backward descriptor b with b['f'] = d, written = {name: (backing buffer, written view)}).
    Every buffer, written ones included, holds seeded values."""
    nI, ipc, R, S, D, h, sd = c['n_inst'], c['ipc'], c['R'], c['S'], c['D'], c['hidden'], c['seed']
    written = {}

    def rows(name, n, w, k, out=False):
        backing, view = _row_operand(c, n, w, sd + k, dev, dtype)
        if out:
            written[name] = (backing, view)
        return view

    def flat(name, shape, k):
        n = math.prod(shape)
        backing = cv(rnd(n + 2 * GUARD, seed=sd + k), dev, dtype)
        written[name] = (backing, backing[GUARD:GUARD + n].view(shape))
        return written[name][1]

    d = dict(score_mode=c['score'], msg_mode=c['msg'], n_inst=nI, inst_per_clip=ipc, R=c['desc_R'], S=S, D=D, hidden=h,
             exclude_self=c['excl'], relu_scores=c['relu'], scale=f32(1.0 / math.sqrt(max(D, 1))),
             out=rows('out', R, h, 1, True), att=flat('att', (nI, R, S), 2))
    if c['smask']:
        d['send_mask'] = cv(send_mask_of(c), dev, dtype)
    if c['rmask']:
        d['recv_mask'] = cv(recv_mask_of(c), dev, dtype)
    if c['score'] == DOT:
        d['q'] = rows('q', R, D, 3)
        d['k'] = d['q'] if c['self_rel'] else rows('k', S, D, 4)
        if c['relu']:
            d['score_bias'] = cv(rnd(1, seed=sd + 5, scale=BIAS_SCALE), dev, dtype)
    elif c['score'] == ADDITIVE:
        d.update(a_r=cv(rnd(nI * R, seed=sd + 6), dev, dtype), c_s=cv(rnd(nI * S, seed=sd + 7), dev, dtype))
    elif c['score'] == DISTANCE:
        d['dist'] = cv(dist_of(c), dev, dtype).transpose(1, 2)
    if c['msg'] == SENDER:
        d['msg'] = rows('msg', S, h, 10)
    else:
        d.update(p_r=rows('p_r', R, h, 11), p_s=rows('p_s', S, h, 12))

    b = dict(f=d, dout=rows('dout', R, h, 20), relu_mask_dmsg=c['relu_mask_dmsg'])
    if c['msg'] == SENDER:
        b['dmsg'] = rows('dmsg', S, h, 21, True)
    else:
        b.update(dp_r=rows('dp_r', R, h, 22, True), dp_s=rows('dp_s', S, h, 23, True))
    if c['grads'] is not None:
        b.update(dq=rows('dq', R, D, 24, True), dq_accumulate=c['grads'][0], dk_accumulate=c['grads'][1])
        b['dk'] = b['dq'] if c['self_rel'] else rows('dk', S, D, 25, True)
    if c['score'] == ADDITIVE:
        b.update(da_r=flat('da_r', (nI, R), 26), dc_s=flat('dc_s', (nI, S), 27))
    if c['score'] == DOT and c['relu']:
        b['dscore_sum'] = flat('dscore_sum', (nI,), 28)
    return d, b, written


def outside(backing, view):
    """The backing buffer with the written view zeroed: what a call must leave as it was."""
    o = backing.detach().clone()
    torch.as_strided(o, view.shape, view.stride(), view.storage_offset() - backing.storage_offset()).zero_()
    return o


def per_instance_dscore(d, b):
    """d loss / d score_bias of every instance: autograd on the specification's forward with the bias expanded to one leaf per
    instance (FakeKernels.relation_bwd keeps its contract: the total in element 0)."""
    nI = d['n_inst']
    sb = d['score_bias'].detach().reshape(1, 1, 1).expand(nI, 1, 1).clone().requires_grad_(True)
    with torch.enable_grad():
        out, _ = F._rel_forward(d, {'score_bias': sb})
        out.backward(F._rel_rows(b['dout'], nI, d['R']).reshape(out.shape).detach())
    return sb.grad.reshape(nI)


def collect(c, written):
    res = {}
    for name, (backing, view) in written.items():
        unscored_grad = name in ('dq', 'dk') and c['score'] not in SCORED
        res[name] = (view, EXACT if unscored_grad else JUDGE)
        res[name + '_outside'] = (outside(backing, view), EXACT)
    return res


def run(Kx, c, dev, dtype):
    """Forward and backward of case c on Kx -> {name: (tensor, how)}."""
    d, b, written = build(c, dev, dtype)
    Kx.relation_fwd(d)
    Kx.relation_bwd(b)
    if isinstance(Kx, FakeKernels) and 'dscore_sum' in written and d['R'] > 0:
        written['dscore_sum'][1].copy_(per_instance_dscore(d, b))
    return collect(c, written)


# ----------------------------------------------------------------------------------------------- properties of the inputs
def valid_pairs(c):
    """(n_inst, R, S) bool: the sender may carry weight (send mask, exclude_self, distance 0)."""
    nI, ipc, R, S = c['n_inst'], c['ipc'], c['R'], c['S']
    v = torch.ones(nI, R, S, dtype=torch.bool)
    if c['smask']:
        v &= (send_mask_of(c) != 0).repeat_interleave(ipc, 0).view(nI, 1, S)
    if c['excl']:
        v &= ~torch.eye(R, S, dtype=torch.bool).view(1, R, S)
    if c['score'] == DISTANCE:
        v &= dist_of(c).transpose(1, 2) != 0
    return v


def att_structure_failures(att, c):
    """The weights of a forward call: finite; invalid senders exactly 0 (so receivers without a sender are all 0); SUM: valid
    senders exactly 1 (the mask value); every other mode: receivers with a valid sender sum to 1 within 4 x 2^-24 x S."""
    S = c['S']
    att = att.detach().cpu().double().reshape(c['n_inst'], c['R'], S)
    v = valid_pairs(c)
    fails = []
    if not torch.isfinite(att).all():
        fails.append('non-finite weights')
        att = torch.nan_to_num(att, nan=1e30, posinf=1e30, neginf=-1e30)
    if (~v).any() and float(att[~v].abs().max()) != 0.0:
        fails.append('an excluded or masked sender has a non-zero weight')
    if c['score'] == SUM:
        if v.any() and not bool((att[v] == 1.0).all()):
            fails.append('a valid sender of the masked sum has a weight other than 1')
        return fails
    off = (att.sum(-1) - 1.0).abs()[v.any(-1)]
    if off.numel() and float(off.max()) > 4 * EPS * S:
        fails.append(f'a row of weights sums to 1 {float(off.max()):.2e} off (> 4 x 2^-24 x {S})')
    return fails


def relu_margin(c):
    """DOT with relu_scores: the smallest |raw| / mag over ALL pairs of the case, raw = scale <q, k> + bias and
    mag = scale <|q|, |k|> + |bias| in fp64. Must exceed RELU_BAND for the ReLU decisions to be independent of summation order."""
    d, _, _ = build(c, 'cpu', torch.float64)
    nI, R, S = c['n_inst'], c['R'], c['S']
    q, k = F._rel_rows(d['q'], nI, R), F._rel_rows(d['k'], nI, S)
    bias = d['score_bias'].reshape(())
    raw = torch.einsum('nrd,nsd->nrs', q, k) * d['scale'] + bias
    mag = torch.einsum('nrd,nsd->nrs', q.abs(), k.abs()) * d['scale'] + bias.abs()
    return float((raw.abs() / mag).min())


def relu_positive_share(c):
    """DOT with relu_scores: the share of the valid pairs whose raw score is positive (fp64)."""
    d, _, _ = build(c, 'cpu', torch.float64)
    q, k = F._rel_rows(d['q'], c['n_inst'], c['R']), F._rel_rows(d['k'], c['n_inst'], c['S'])
    raw = torch.einsum('nrd,nsd->nrs', q, k) * d['scale'] + d['score_bias'].reshape(())
    v = valid_pairs(c)
    return float((raw[v] > 0).double().mean())
