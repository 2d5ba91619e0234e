"""The geometric-level GCN kernels (csrc/geo_fused.hip, geo_attn_mfma.hip, geo_gcn.hip) at batch-sized frame counts: the
case list, the inputs, the executable specification (tests/fake_kernels.py) run in fp32 and in fp64, and the row-wise rule.
Shared by tests/test_gcn_frames_cpu.py (the specification and the inputs themselves) and tests/test_gcn_frames_gpu.py (the
HIP kernels against both).

Every one of these kernels is launched with a capped grid and walks the frames; the cases are chosen so that the loops make
a second trip (the GPU test file proves it per case from HipKernels.gcn_launch_plan, not from arithmetic copied here).

How a result is judged. Tensor-wide: the rule of tests/entity_envelope.py unchanged (e_hip <= 8 e_ref + 4 x 2^-24, both
against the fp64 specification, the yardstick is the fp32 specification's own error). Row-wise, with
er(row) = max|x - s64| / max|s64| over the row, the own-row rule of entity_envelope.judge cannot be used as it stands on
30 000 ... 260 000 short rows (the ratio of two independent rounding errors has a heavy tail), so:
  R1  every row: er_hip(row) <= 8 x max over rows of er_ref + floor; rows that are zero in the specification are exactly zero;
  R2  spread regime, tensors of at least R2_MIN_ROWS rows: the own-row rule er_hip(row) <= 8 er_ref(row) + floor may be missed
      by at most R2_CAP = 0.2 % of the rows. The cap lies above the 0.056 % that two fp32 evaluations of the specification
      show against each other and below the share a defect bound to one (frame slot of a group, node) position produces,
      1 / (FG x N) >= 0.33 % for every N of the list. It is a condition, not a measurement.
In the sharp regime (scores up to +-500, near-one-hot rows) R1 holds for X, the adjacency and Z only: rows whose gradient
vanishes have a relative error of 2 ... 7 in the specification itself."""
import functools

import torch

from tests.entity_envelope import EPS, FACTOR, F, judge

R2_CAP = 0.002
R2_MIN_ROWS = 10000
FLOOR = 4 * EPS

# (md scale of M, of d) through the projections the production call folds: M = Wk^T Wq is a sum of 128 products, so weights
# of scale s give M the scale 128^0.5 s^2, and d = Wk^T bq the scale 128^0.5 s s_b
REGIMES = {'spread': (0.003, 0.03), 'sharp': (0.05, 0.3)}
SPREAD_SIGMA = 0.8   # see inputs()


def _c(N, bs, T, H, regime='spread', why='', reduced=False):
    # fold: whose ab / mean / invstd the forward and backward kernels of the case are given. Up to one group of frames the batch
    # variance is (near) zero, invstd reaches 316 and x^ = a x + b cancels: the fp32 specification itself is then 2e-5 from
    # fp64, so those cases take the inference-mode fold (running statistics); both folds are judged in every case.
    return dict(N=N, bs=bs, T=T, H=H, regime=regime, why=why, reduced=reduced, frames=bs * T,
                fold='eval_' if bs * T <= 8 else 'train_', id=f'N{N}_{bs}x{T}_H{H}_{regime}')


# 2 093 frames = 7 clips x 299: more groups than the fused kernel's grid at every FG (8 / 6 / 4 frames per group), a ragged last
# group on a workgroup that ran a full one, > 256 and not a multiple of it (attn2 backward), > 512 (attn2 forward), > 2 048
# (the two-projection attention), 2 093 // 8 = 261 > 240 stats blocks wanted -> 240 blocks of 9 frames of which the last 7 are
# empty, 2 093 % 4 = 1, and T = 299 is a multiple of no FG (groups straddle clips).
BIG = [
    _c(1, 7, 299, 1, why='NT = 1, a single node: every row tile is padding but one row', reduced=True),
    _c(16, 7, 299, 3, why='NT = 1, no padding column; 33 488 rows: embed1 forward makes a second trip, embed1 backward below its cap'),
    _c(19, 7, 299, 2, why='NT = 2, 13 padding columns', reduced=True),
    _c(34, 7, 299, 2, why='NT = 3, the production node count; 71 162 rows: embed1 backward at its grid cap', reduced=True),
    _c(50, 7, 299, 1, why='NT = 4, FG = 6, attn2 backward without the M copy'),
    _c(64, 7, 299, 3, why='NT = 4, FG = 4, no padding, attn2 backward without the M copy', reduced=True),
]
SHARP = [_c(N, 3, 347, H, 'sharp', why='near-one-hot rows, scores up to +-500: the max-subtraction')
         for N, H in ((1, 2), (16, 1), (19, 3), (34, 2), (50, 2), (64, 1))]
BENCH = [_c(34, 64, 120, 2, why='the bench shape: 960 groups on 256 workgroups')]
SMALL = [
    _c(1, 1, 1, 1, why='one frame, one node'),
    _c(34, 1, 1, 2, why='one frame'),
    _c(34, 1, 5, 3, why='fewer frames than a group'),
    _c(34, 1, 8, 2, why='exactly one group (FG = 8)'),
    _c(64, 1, 3, 2, why='fewer frames than a group (FG = 4)'),
    _c(64, 2, 2, 1, why='exactly one group (FG = 4)'),
    _c(50, 1, 6, 2, why='exactly one group (FG = 6)'),
    _c(34, 2, 128, 2, why='256 frames: attn2 backward makes exactly one trip per workgroup', reduced=True),
    _c(34, 1, 257, 2, why='257 frames: one attn2 backward workgroup makes two trips', reduced=True),
    _c(64, 1, 257, 1, why='257 frames without the M copy'),
]
CASES = BIG + SHARP + BENCH + SMALL
REDUCED = [c for c in CASES if c['reduced']]   # also run through gcn_attn2_fwd and the two-projection attention kernels


def _rnd(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def inputs(c, seed=0):
    """The fp32 inputs of case c. Every human's geometry is random (a wrong frame / human stride reads other numbers), the eight
    appearance features in front of the geometry are a constant 7 (an offset that is one float4 short reads them)."""
    N, bs, T, H = c['N'], c['bs'], c['T'], c['H']
    g = torch.Generator().manual_seed(1000 * N + 10 * H + seed + c['frames'])
    xh = torch.zeros(bs, T, H, 2048 + 4 * N)
    xh[..., 2040:2048] = 7.0
    xh[..., 2048:] = _rnd(g, bs, T, H, 4 * N)
    sm, sd = REGIMES[c['regime']]
    s = (sm / 128 ** 0.5) ** 0.5
    p = dict(xh=xh, gamma=_rnd(g, 4 * N).abs() + 0.5, beta=_rnd(g, 4 * N), rm=_rnd(g, 4 * N, scale=0.1), rv=_rnd(g, 4 * N).abs() + 0.5,
             w1=_rnd(g, 64, 4), b1=_rnd(g, 64), w2=_rnd(g, 64, 64, scale=0.2), b2=_rnd(g, 64, scale=0.2),
             wq=_rnd(g, 128, 64, scale=s), wk=_rnd(g, 128, 64, scale=s), bq=_rnd(g, 128, scale=sd / (128 ** 0.5 * s)),
             dz=_rnd(g, bs * T * N, 64), de1=_rnd(g, bs * T * N, 64), qk=None)
    if c['reduced']:
        p['qk'] = _rnd(g, bs * T * N, 256, scale=0.3 if c['regime'] == 'sharp' else 0.1)
    if c['regime'] == 'spread' and N > 1:
        # X = relu(..) has a large common component, so how sharp x_i^T M x_j is depends on the draw of M (2 to 30 effective
        # senders of 34 at one nominal scale). The spread regime is a condition on the inputs: wq and bq (M and d are linear in
        # them) are scaled so that a receiver's scores have a standard deviation of SPREAD_SIGMA over its senders, measured on
        # the first frames with the running statistics; Gaussian scores of that spread give N exp(-sigma^2) effective senders.
        nf = min(bs * T, 64)
        a = p['gamma'] / torch.sqrt(p['rv'] + 1e-5)
        X, _, _ = F.gcn_fused_fwd(xh.reshape(1, bs * T, H, -1)[:, :nf].double(), N, torch.stack([a, p['beta'] - p['rm'] * a]).double(),
                                  p['w1'].double(), p['b1'].double(), p['w2'].double(), p['b2'].double(), torch.zeros(65, 64, dtype=torch.float64))
        X = X.view(nf, N, 64)
        sc = (X @ (p['wk'].t() @ p['wq']).double().t() + (p['wk'].t() @ p['bq']).double()) @ X.transpose(1, 2)
        t = SPREAD_SIGMA / float(sc.std(-1).median())
        p['wq'], p['bq'] = p['wq'] * t, p['bq'] * t
    return p


def geo64(xh):
    """An fp64 x_human that holds human 0 only (all the specification reads)."""
    return xh[:, :, :1].double()


def bn_state(p, dt=torch.float32, dev='cpu'):
    return p['rm'].to(dt).to(dev).clone(), p['rv'].to(dt).to(dev).clone(), torch.tensor(5, dtype=torch.int64, device=dev)


def run_bn(Kx, c, p, xh, training, dt=torch.float32, dev='cpu'):
    """bn_fold as the production call uses it (with the fold) -> dict ab, mi, md, rm, rv, nbt."""
    cv = lambda t: t.to(dt).to(dev)
    rm, rv, nbt = bn_state(p, dt, dev)
    ab, mi, md = Kx.bn_fold(xh, c['N'], cv(p['gamma']), cv(p['beta']), rm, rv, nbt, training,
                            fold=(cv(p['wq']), cv(p['wk']), cv(p['bq'])))
    return dict(ab=ab, mi=mi, md=md, rm=rm, rv=rv, nbt=nbt)


def _forward(Kx, c, xh, ab, md, p, cv):
    X, adj, Z = Kx.gcn_fused_fwd(xh, c['N'], ab, cv(p['w1']), cv(p['b1']), cv(p['w2']), cv(p['b2']), md)
    return dict(X=X, adj=adj, Z=Z, e1=Kx.gcn_embed1_fwd(xh, c['N'], ab, cv(p['w1']), cv(p['b1'])))


@functools.lru_cache(maxsize=2)
def _spec_cached(cid):
    return _spec(next(c for c in CASES if c['id'] == cid))


def spec(c):
    """(p, s32, s64): the inputs and every output of the specification in fp32 and in fp64. Each kernel's fp64 specification
    runs on fp64 copies of the fp32 values that kernel is given: the forward pass takes ab and md of the fp32 fold, the
    backward passes read the fp32 run's saved X, adjacency, ab, mean / invstd and the ReLU mask (inside de1), as the kernels do,
    so no hard decision can flip between the two runs. (Cached: callers must not write into the result.)"""
    return _spec_cached(c['id'])


def _spec(c):
    p = inputs(c)
    N, nF = c['N'], c['frames']
    x64 = geo64(p['xh'])
    s32, s64 = {}, {}
    for training in (True, False):
        tag = 'train_' if training else 'eval_'
        for s, xh, dt in ((s32, p['xh'], torch.float32), (s64, x64, torch.float64)):
            s.update({tag + k: v for k, v in run_bn(F, c, p, xh, training, dt).items()})
    ab, mi, md = (s32[c['fold'] + k] for k in ('ab', 'mi', 'md'))
    s32.update(_forward(F, c, p['xh'], ab, md, p, lambda t: t))
    s64.update(_forward(F, c, x64, ab.double(), md.double(), p, lambda t: t.double()))
    p['de1m'] = p['de1'] * (s32['e1'] > 0)     # dL/d(pre-activation): the ReLU mask of the fp32 run
    X, adj = s32['X'], s32['adj']
    s32['dX'], s32['dmd'] = F.gcn_attn2_bwd(X, md, adj, p['dz'], nF, N)
    s64['dX'], s64['dmd'] = F.gcn_attn2_bwd(X.double(), md.double(), adj.double(), p['dz'].double(), nF, N)
    for s, xh, cv in ((s32, p['xh'], lambda t: t), (s64, x64, lambda t: t.double())):
        s['dw1'], s['db1'], s['dgamma'], s['dbeta'] = F.gcn_embed1_bwd(xh, N, cv(ab), cv(mi), cv(p['w1']), cv(p['de1m']))
    if c['reduced']:
        s32['adj2'], s32['Z2'] = F.gcn_attn2_fwd(X, md, nF, N)
        s64['adj2'], s64['Z2'] = F.gcn_attn2_fwd(X.double(), md.double(), nF, N)
        qk = p['qk']
        s32['adjq'], s32['Zq'] = F.gcn_attn_fwd(qk, X, nF, N)
        s64['adjq'], s64['Zq'] = F.gcn_attn_fwd(qk.double(), X.double(), nF, N)
        s32['dXq'], s32['dqk'] = F.gcn_attn_bwd(qk, X, s32['adjq'], p['dz'], nF, N)
        s64['dXq'], s64['dqk'] = F.gcn_attn_bwd(qk.double(), X.double(), s32['adjq'].double(), p['dz'].double(), nF, N)
    return p, s32, s64


def permuted(c, p, s32, seed=5):
    """A second, equally legitimate fp32 evaluation of the specification: the 64 hidden features, the 64 output features and
    the frames permuted, so every sum runs in another order. Same keys as s32 (the tensors that involve arithmetic)."""
    N, nF = c['N'], c['frames']
    g = torch.Generator().manual_seed(seed)
    ph, po = torch.randperm(64, generator=g), torch.randperm(64, generator=g)
    inv = torch.argsort(po)
    out = {}
    ab, mi, md = (s32[c['fold'] + k] for k in ('ab', 'mi', 'md'))
    # forward: hidden layer permuted by ph, X features by po
    mdp = torch.cat([md[:64][po][:, po], md[64:, po]], 0)
    f = _forward(F, c, p['xh'], ab, mdp, dict(w1=p['w1'][ph], b1=p['b1'][ph], w2=p['w2'][po][:, ph], b2=p['b2'][po]), lambda t: t)
    out.update(X=f['X'][:, inv], adj=f['adj'], Z=f['Z'][:, inv], e1=f['e1'][:, torch.argsort(ph)])
    Xp = s32['X'][:, po].contiguous()
    dX, dmd = F.gcn_attn2_bwd(Xp, mdp, s32['adj'], p['dz'][:, po].contiguous(), nF, N)
    out.update(dX=dX[:, inv], dmd=torch.cat([dmd[:64][inv][:, inv], dmd[64:, inv]], 0))
    ihp = torch.argsort(ph)
    r = F.gcn_embed1_bwd(p['xh'], N, ab, mi, p['w1'][ph], p['de1m'][:, ph].contiguous())
    out.update(dw1=r[0][ihp], db1=r[1][ihp], dgamma=r[2], dbeta=r[3])
    # the fold with the 128 projection outputs permuted; the statistics over the clips in reverse order
    pp = torch.randperm(128, generator=g)
    q = dict(p, wq=p['wq'][pp], wk=p['wk'][pp], bq=p['bq'][pp])
    for training in (True, False):
        tag = 'train_' if training else 'eval_'
        out.update({tag + k: v for k, v in run_bn(F, c, q, p['xh'].flip(0), training).items()})
    return out


# ---------------------------------------------------------------------------------------------------------- the judgement
def rows_of(name, t, N):
    """The row structure by which tensor `name` is judged: one (frame, node) for X, Z, dX, e1 and the adjacency (N weights), one
    channel block of N for ab, mean / invstd, dgamma, dbeta and the running statistics, one row of the 65 x 64 md gradient."""
    if name.split('_')[-1] in ('ab', 'mi', 'rm', 'rv', 'dgamma', 'dbeta'):
        return t.reshape(-1, N)
    return t.reshape(-1, t.shape[-1])


def judge_rows(hip, s32, s64, regime='spread', r1=True, factor=FACTOR):
    """hip, s32, s64 as 2-D (rows, width) -> (record, failures): the tensor-wide rule of entity_envelope.judge, R1 and R2 of the
    module docstring. record: e_hip, e_ref, ratio (tensor-wide factor needed), r1_ratio = worst er_hip(row) over the
    specification's worst row, r2_share = share of rows beyond their own-row rule, rows."""
    assert hip.dim() == 2 and hip.shape == s32.shape == s64.shape, (hip.shape, s32.shape, s64.shape)
    hip, s32, s64 = (t.detach().cpu().double() for t in (hip, s32, s64))
    rec, fails = judge(hip.reshape(-1), s32.reshape(-1), s64.reshape(-1), factor)   # one row = the tensor-wide rule alone
    rec = dict(e_hip=rec['e_hip'], e_ref=rec['e_ref'], ratio=rec['ratio'], r1_ratio=0.0, r2_share=0.0, rows=hip.shape[0])
    if not hip.numel() or not torch.isfinite(hip).all():
        return rec, fails
    rs = s64.abs().amax(1)
    live = rs > 0
    if (~live).any() and float(hip[~live].abs().max()) != 0.0:
        fails.append('a row that is zero in the specification is not exactly zero')
    if not live.any():
        return rec, fails
    rsafe = rs.clamp_min(1e-300)
    er_hip = torch.where(live, (hip - s64).abs().amax(1) / rsafe, torch.zeros_like(rs))
    er_ref = torch.where(live, (s32 - s64).abs().amax(1) / rsafe, torch.zeros_like(rs))
    worst_ref = float(er_ref.max())
    worst = float(er_hip.max())
    rec['r1_ratio'] = 0.0 if worst <= FLOOR else ((worst - FLOOR) / worst_ref if worst_ref > 0 else float('inf'))
    if r1 and worst > factor * worst_ref + FLOOR:
        br = int(torch.argmax(er_hip))
        fails.append(f'R1: row {br} of {hip.shape[0]}: er_hip {worst:.3e} > {factor:g} x the worst row of the specification '
                     f'{worst_ref:.3e} + 4 x 2^-24 (needs {rec["r1_ratio"]:.1f}; '
                     f'{int((er_hip > factor * worst_ref + FLOOR).sum())} rows beyond)')
    beyond = int((er_hip > factor * er_ref + FLOOR).sum())
    rec['r2_share'] = beyond / hip.shape[0]
    if regime == 'spread' and hip.shape[0] >= R2_MIN_ROWS and rec['r2_share'] > R2_CAP:
        fails.append(f'R2: {beyond} of {hip.shape[0]} rows ({100 * rec["r2_share"]:.3f} %) miss their own-row rule, cap {100 * R2_CAP:g} %')
    return rec, fails


# tensors of the sharp regime that R1 holds: see the module docstring
SHARP_R1 = ('X', 'adj', 'Z', 'e1', 'adj2', 'Z2', 'adjq', 'Zq')


def judge_named(c, name, hip, s32, s64):
    N = c['N']
    r1 = c['regime'] == 'spread' or name in SHARP_R1 or name.split('_')[0] in ('train', 'eval')
    return judge_rows(rows_of(name, hip, N), rows_of(name, s32, N), rows_of(name, s64, N), c['regime'], r1)


def adjacency_stats(adj):
    """(median effective number of senders 1 / sum w^2, median largest weight) over the rows of an adjacency."""
    w = adj.reshape(-1, adj.shape[-1]).double()
    return float((1.0 / (w * w).sum(1)).median()), float(w.amax(1).median())
