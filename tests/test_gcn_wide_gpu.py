"""GPU: the wide family of the geometric-level GCN kernels (csrc/geo_wide.hip and the 256-node instances of csrc/geo_gcn.hip),
65 ... 256 nodes, through the six HipKernels methods that route to it.

Kernel level: every output of every case of tests/gcn_wide.py against the specification run in fp64, the fp32 specification's
own error as the yardstick (e_hip <= 8 e_ref + 4 x 2^-24 tensor-wide, for the worst row, exact zeros; R2 with the cap
1 / (2 FG N) of tests/gcn_wide.py); canaries behind every output; two runs bit-equal; adjacency rows sum to 1; frames do not leak
into each other; bad node counts are refused before any launch. Model level: TGGCN(gcn_node = 72, 77, 176) against the CPU
oracle under the gates of tests/test_parity_gpu.py and tests/test_input_grads_gpu.py; the wide entry points run for 72 nodes and
none of them for 34; gcn_node = 257 raises NotImplementedError."""
import pytest
import torch

import twog_gcn_amd  # noqa: F401
from twog_gcn_amd import kernels as twog_kernels
from twog_gcn_amd.models import TGGCN
from oracle import cpu_ref
from tests import gcn_frames as GF
from tests import gcn_wide as GW
from tests.entity_envelope import EPS, FACTOR, judge

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CANARY = -12345.0
WIDE_ENTRY_POINTS = ('twog_gcn_wide_bn_stats', 'twog_gcn_wide_bn_finalize', 'twog_gcn_wide_embed1_fwd', 'twog_gcn_wide_fwd',
                     'twog_gcn_wide_bwd', 'twog_gcn_wide_embed1_bwd', 'twog_gcn_wide_input_bwd')


@pytest.fixture()
def K():
    twog_kernels._set_backend_for_tests(None)
    k = twog_kernels.get_kernels()
    assert k.name == 'hip' and k._force_wide is False
    yield k
    k._force_wide = False


# --------------------------------------------------------------------------------------------- the case list against the plan
def test_limits_and_the_case_list_against_the_plan(K):
    assert K.lib.twog_gcn_wide_max_nodes() == GW.WIDE_MAX and K.lib.twog_gcn_max_nodes() == GW.TUNED_MAX
    for c in GW.CASES:
        for kernel in (K.WIDE_PLAN_FWD, K.WIDE_PLAN_BWD):
            grid, fg, lds, _ = K.gcn_wide_launch_plan(kernel, c['frames'], c['N'])
            assert fg == GW.FG and lds <= 160 * 1024 and grid == min(c['frames'], GW.MAX_GRID)
    for c in GW.SECOND_TRIP:   # a second, ragged trip: grid + 1 frames, taken from the plan
        assert c['frames'] == K.gcn_wide_launch_plan(K.WIDE_PLAN_FWD, c['frames'], c['N'])[0] + 1
        assert c['frames'] == K.gcn_wide_launch_plan(K.WIDE_PLAN_BWD, c['frames'], c['N'])[0] + 1
        assert c['frames'] * c['N'] >= GF.R2_MIN_ROWS
    assert {K.gcn_wide_launch_plan(K.WIDE_PLAN_FWD, 1, c['N'])[3] for c in GW.CASES} == {4, 8, 12, 16}   # every instance
    assert {c['H'] for c in GW.THREE} == {2, 3} and all(c['frames'] == 3 for c in GW.THREE)
    assert all(not K._gcn_wide(c['N']) for c in GW.FORCED) and all(K._gcn_wide(c['N']) for c in GW.CASES if not c['forced'])


def test_node_counts_out_of_range_are_refused_before_any_launch(K):
    lib, st = K.lib, K._stream()
    out = (twog_kernels.C.c_int * 4)()
    for n in (lib.twog_gcn_wide_max_nodes() + 1, 0):
        assert lib.twog_gcn_wide_fwd(None, 0, 8, n, None, None, None, None, None, None, None, None, None, st) < 0
        assert lib.twog_gcn_wide_bwd(None, None, None, None, 8, n, None, None, 8, st) < 0
        assert lib.twog_gcn_wide_embed1_fwd(None, 0, 8, n, None, None, None, None, st) < 0
        assert lib.twog_gcn_wide_embed1_bwd(None, 0, 8, n, None, None, None, None, None, 1, None, None, None, None, st) < 0
        assert lib.twog_gcn_wide_input_bwd(None, 0, 8, n, 1, 0, None, None, None, None, None, None, 1, None, 1, st) < 0
        assert lib.twog_gcn_wide_bn_stats(None, 0, 8, n, None, 1, st) < 0
        assert lib.twog_gcn_wide_bn_finalize(None, 1, 8, n, None, None, None, None, None, 1, None, None, None, None, None, None, st) < 0
        for kernel in range(3):
            assert lib.twog_gcn_wide_launch_plan(kernel, 8, n, out) == -1
    assert lib.twog_gcn_wide_launch_plan(99, 8, 72, out) == -2
    # the tuned entry points keep their limit
    assert lib.twog_gcn_fused_fwd(None, 0, 8, 65, None, None, None, None, None, None, None, None, None, st) < 0
    torch.cuda.synchronize()
    assert float((torch.ones(4, device=DEV) + 1).sum()) == 8.0   # the device computes afterwards


# ------------------------------------------------------------------------------------------------------------ the judgement
class Verdict:
    """Collects the judgement of every tensor of one case: all of them are measured before the case fails."""

    def __init__(self, c, fg):
        self.c, self.fg, self.fails, self.worst, self.worst_row, self.share = c, fg, [], (0.0, ''), (0.0, ''), (0.0, '')

    def add(self, name, hip, s32, s64):
        rec, fails = GW.judge_named(self.c, name, hip, s32[name], s64[name], self.fg)
        self.fails += [f'{name}: {f}' for f in fails]
        self.worst, self.worst_row = max(self.worst, (rec['ratio'], name)), max(self.worst_row, (rec['r1_ratio'], name))
        if rec['rows'] >= GF.R2_MIN_ROWS:
            self.share = max(self.share, (rec['r2_share'], name))

    def same(self, name, a, b):
        if not torch.equal(a, b):
            self.fails.append(f'{name}: two runs of the same call differ')

    def canary(self, name, buf, n):
        if not bool((buf.reshape(-1)[n:] == CANARY).all()):
            self.fails.append(f'{name}: written behind the last frame')

    def check(self):
        print(f"{self.c['id']}: worst e_hip / e_ref {self.worst[0]:.2f} ({self.worst[1]}), worst row / the specification's worst row "
              f'{self.worst_row[0]:.2f} ({self.worst_row[1]}), largest R2 share {100 * self.share[0]:.4f} % ({self.share[1]}) of the cap '
              f'{100 * GW.r2_cap(self.c, self.fg):.3f} %')
        assert not self.fails, f"{self.c['id']}:\n  " + '\n  '.join(self.fails)


def _buf(n, extra):
    return torch.full((n + extra,), CANARY, dtype=torch.float32, device=DEV)


def _adjacency_structure(V, name, adj, N):
    a = adj.detach().cpu().double().reshape(-1, N)
    if not torch.isfinite(a).all():
        V.fails.append(f'{name}: non-finite weights')
    elif float((a.sum(1) - 1.0).abs().max()) > 4 * EPS * N:
        V.fails.append(f'{name}: a row sums to 1 {float((a.sum(1) - 1.0).abs().max()):.2e} off (> 4 ulp x {N})')


@pytest.mark.parametrize('c', GW.CASES, ids=lambda c: c['id'])
def test_wide_kernels_against_the_fp64_specification(K, c):
    """bn_fold (both modes, with the fold), gcn_fused_fwd (with and without save_x), gcn_embed1_fwd, gcn_attn2_bwd, gcn_embed1_bwd and
    gcn_input_bwd through HipKernels, which picks the wide entry points (by n_nodes, or by the private switch for N <= 64); the
    forward and the attention backward once more through the raw entry points into buffers with canaries behind them."""
    p, s32, s64 = GW.spec(c)
    N, nF = c['N'], c['frames']
    rows = nF * N
    K._force_wide = c['forced']
    assert K._gcn_wide(N)
    fg = K.gcn_wide_launch_plan(K.WIDE_PLAN_FWD, nF, N)[1]
    V = Verdict(c, fg)
    g = lambda t: t.to(DEV)
    xh = g(p['xh'])
    for training in (True, False):
        tag = 'train_' if training else 'eval_'
        r, r2 = GF.run_bn(K, c, p, xh, training, dev=DEV), GF.run_bn(K, c, p, xh, training, dev=DEV)
        for k in r:
            if k == 'nbt':
                assert int(r[k]) == int(s32[tag + k]) == int(r2[k])
                continue
            V.add(tag + k, r[k], s32, s64)
            V.same(tag + k, r[k], r2[k])
    ab, mi, md = (g(s32[c['fold'] + k]) for k in ('ab', 'mi', 'md'))
    w1, b1, w2, b2 = (g(p[k]) for k in ('w1', 'b1', 'w2', 'b2'))
    ptr, fstride, nf_ = K._geo(xh)
    assert nf_ == nF
    # ---- forward: raw entry point into buffers with two frames of canary rows behind the last frame, then HipKernels twice
    Xb, adjb, Zb = _buf(rows * 64, 2 * N * 64), _buf(rows * N, 2 * N * N), _buf(rows * 64, 2 * N * 64)
    K._check(K.lib.twog_gcn_wide_fwd(ptr, fstride, nF, N, ab.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(),
                                     md.data_ptr(), Xb.data_ptr(), adjb.data_ptr(), Zb.data_ptr(), K._stream()), 'twog_gcn_wide_fwd')
    X, adj, Z = K.gcn_fused_fwd(xh, N, ab, w1, b1, w2, b2, md)
    Xn, adjn, Zn = K.gcn_fused_fwd(xh, N, ab, w1, b1, w2, b2, md, save_x=False)
    assert Xn is None
    for name, t, buf, tn in (('X', X, Xb, X), ('adj', adj, adjb, adjn), ('Z', Z, Zb, Zn)):
        V.add(name, t, s32, s64)
        V.canary(name, buf, t.numel())
        V.same(name, t.reshape(-1), buf[:t.numel()])
        V.same(name + ' (save_x=False)', t, tn)
    _adjacency_structure(V, 'adj', adj, N)
    # ---- embed1 forward; the e1 the backward pass recomputes is what the forward kernel multiplied
    e1b = _buf(rows * 64, 2 * N * 64)
    K._check(K.lib.twog_gcn_wide_embed1_fwd(ptr, fstride, nF, N, ab.data_ptr(), w1.data_ptr(), b1.data_ptr(), e1b.data_ptr(),
                                            K._stream()), 'twog_gcn_wide_embed1_fwd')
    e1 = K.gcn_embed1_fwd(xh, N, ab, w1, b1)
    V.add('e1', e1, s32, s64)
    V.canary('e1', e1b, rows * 64)
    V.same('e1', e1.reshape(-1), e1b[:rows * 64])
    want = torch.relu(e1.double() @ w2.double().t() + b2.double())
    err, tol = float((X.double() - want).abs().max()), 1e-5 + 2e-5 * float(want.abs().max())
    if err > tol:
        V.fails.append(f'forward X vs embed1 + fp64 GEMM: {err:.3e} > {tol:.3e}')
    # ---- attention backward on the specification's saved X and adjacency
    Xs, adjs, dz = g(s32['X']), g(s32['adj']), g(p['dz'])
    nblk = K.gcn_wide_launch_plan(K.WIDE_PLAN_BWD, nF, N)[0]
    dxb, part = _buf(rows * 64, 2 * N * 64), _buf(nblk * 65 * 64, 65 * 64)
    K._check(K.lib.twog_gcn_wide_bwd(Xs.data_ptr(), md.data_ptr(), adjs.data_ptr(), dz.data_ptr(), nF, N, dxb.data_ptr(),
                                     part.data_ptr(), nblk, K._stream()), 'twog_gcn_wide_bwd')
    dX, dmd = K.gcn_attn2_bwd(Xs, md, adjs, dz, nF, N)
    V.add('dX', dX, s32, s64)
    V.add('dmd', dmd, s32, s64)
    V.canary('dX', dxb, rows * 64)
    V.canary('attention backward partials', part, nblk * 65 * 64)
    V.same('dX', dX.reshape(-1), dxb[:rows * 64])
    V.same('dmd', dmd, K.colsum(part[:nblk * 65 * 64].view(nblk, 65 * 64)).view(65, 64))
    # ---- embedding backward and the gradient of the geometry input
    de1 = g(p['de1m'])
    r, r2 = (K.gcn_embed1_bwd(xh, N, ab, mi, w1, de1) for _ in range(2))
    for k, a, b in zip(('dw1', 'db1', 'dgamma', 'dbeta'), r, r2):
        V.add(k, a, s32, s64)
        V.same(k, a, b)
    for name in ('dxg_eval', 'dxg_train'):
        if name not in s32:
            continue
        training = name == 'dxg_train'
        outs = []
        for _ in range(2):
            grad = torch.full(xh.shape, CANARY, device=DEV)
            K.gcn_input_bwd(xh, N, ab, mi, w1, de1, g(s32['dgamma']) if training else None, g(s32['dbeta']) if training else None,
                            training, grad)
            outs.append(grad)
        V.same(name, outs[0], outs[1])
        if not bool((outs[0][..., :2048] == CANARY).all()):
            V.fails.append(f'{name}: written outside the geometry columns')
        if bool(outs[0][:, :, 1:, 2048:].any()):
            V.fails.append(f'{name}: the humans >= 1 did not get exact zeros')
        V.add(name, outs[0][:, :, 0, 2048:].reshape(-1, 4), s32, s64)
    # ---- below the threshold the tuned kernels answer the same question: adjacency and Z of the two families side by side
    if c['forced']:
        K._force_wide = False
        assert not K._gcn_wide(N)
        _, adj_t, Z_t = K.gcn_fused_fwd(xh, N, ab, w1, b1, w2, b2, md)
        for name, wide, tuned in (('adj', adj, adj_t), ('Z', Z, Z_t)):
            e_ref = judge(s32[name].reshape(-1).double(), s32[name].reshape(-1).double(), s64[name].reshape(-1))[0]['e_ref']
            scale = float(s64[name].abs().max())
            e = float((wide.double() - tuned.double()).abs().max()) / scale
            print(f"{c['id']} {name}: wide vs tuned {e:.2e}, the fp32 specification's own error {e_ref:.2e}")
            if e > FACTOR * e_ref + 4 * EPS:
                V.fails.append(f'{name}: the wide family is {e:.3e} from the tuned kernels, > 8 x {e_ref:.3e} + 4 x 2^-24')
    torch.cuda.synchronize()
    V.check()


# ----------------------------------------------------------------------------------------------------- frame independence
def _fwd(K, c, p, s32, xh, fold):
    g = lambda t: t.to(DEV)
    return K.gcn_fused_fwd(g(xh), c['N'], g(s32[fold + 'ab']), g(p['w1']), g(p['b1']), g(p['w2']), g(p['b2']), g(s32[fold + 'md']))


def _frames_that_differ(a, b, nF):
    return torch.nonzero((a.reshape(nF, -1) != b.reshape(nF, -1)).any(1) | (torch.isnan(a.reshape(nF, -1)).any(1))).flatten().tolist()


def test_a_frame_changes_only_its_own_rows(K):
    """With ab fixed, another geometry in one frame -- one of the first trip, the frame of the second trip -- leaves every row of X,
    adjacency and Z of every other frame bit-identical."""
    c = GW.SECOND_TRIP[0]
    p, s32, _ = GW.spec(c)
    nF = c['frames']
    clean = _fwd(K, c, p, s32, p['xh'], c['fold'])
    for f in (5, nF - 1):
        xh = p['xh'].clone()
        xh.view(nF, c['H'], -1)[f, 0, 2048:] += 0.5
        got = _fwd(K, c, p, s32, xh, c['fold'])
        for name, a, b in zip(('X', 'adjacency', 'Z'), got, clean):
            assert _frames_that_differ(a, b, nF) == [f], f'{name}: the geometry of frame {f} changed other frames'


def test_a_non_finite_frame_stays_inside_itself(K):
    """tests/test_gcn_frames_gpu.py::test_a_non_finite_frame_stays_inside_its_clip at N = 72: inference mode, one +inf coordinate
    that reaches X of its node; every other frame is bit-identical to the clean run (the wide kernels take one frame per trip, so
    the frame -- not only the clip -- is the boundary). Frames on both sides of it and the second trip's frame are covered."""
    c = GW.SECOND_TRIP[0]
    p, s32, _ = GW.spec(c)
    nF, N = c['frames'], c['N']
    p = dict(p, w1=torch.cat([p['w1'][:, :1], p['w1'][:, 1:2].abs() + 0.1, p['w1'][:, 2:]], 1), w2=p['w2'].abs())
    clean = _fwd(K, c, p, s32, p['xh'], 'eval_')
    assert all(torch.isfinite(t).all() for t in clean)
    for f in (0, 100):   # frame 0 shares its workgroup with the second trip's frame
        xh = p['xh'].clone()
        xh.view(nF, c['H'], -1)[f, 0, 2048 + 4 * 5 + 1] = float('inf')
        got = _fwd(K, c, p, s32, xh, 'eval_')
        assert not torch.isfinite(got[0].view(nF, -1)[f]).all(), 'the +inf coordinate did not reach X: the test perturbs nothing'
        for name, a, b in zip(('X', 'adjacency', 'Z'), got, clean):
            bad = [i for i in _frames_that_differ(a, b, nF) if i != f]
            assert not bad, f'{name}: the non-finite frame {f} changed the frames {bad[:8]}'


# ------------------------------------------------------------------------------------------------------------- model level
def _count_wide_calls(K, monkeypatch):
    """Counts the calls of every wide entry point the HipKernels methods make (the library object is wrapped, not the kernels)."""
    calls = {n: 0 for n in WIDE_ENTRY_POINTS}

    class Counting:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            fn = getattr(self._lib, name)
            if name not in calls:
                return fn

            def counted(*a):
                calls[name] += 1
                return fn(*a)
            return counted

    monkeypatch.setattr(K, 'lib', Counting(K.lib))
    return calls


@pytest.mark.parametrize('H,O,N', [(2, 4, 72), (5, 16, 77), (16, 16, 176)])
def test_model_beyond_64_nodes_against_the_oracle(K, monkeypatch, H, O, N):
    """The full path, forward + backward, under the gates of tests/test_parity_gpu.py::_oracle_vs_hip (imported, not copied):
    outputs 1e-4, every parameter gradient 5e-4 of its scale + 5e-6, at most 10 % of the ReLU units nudged as in the entity
    tests. The wide entry points are what ran."""
    from tests.test_parity_gpu import _oracle_vs_hip
    calls = _count_wide_calls(K, monkeypatch)
    _oracle_vs_hip(bs=2, T=5, H=H, O=O, N=N, h=32, backward=True, seed=19, max_nudged_share=0.10)
    assert all(calls[n] > 0 for n in WIDE_ENTRY_POINTS if n != 'twog_gcn_wide_input_bwd'), calls
    assert calls['twog_gcn_wide_input_bwd'] == 0    # no input gradient was asked for


def test_model_at_34_nodes_runs_no_wide_entry_point(K, monkeypatch):
    from tests.test_parity_gpu import _oracle_vs_hip
    calls = _count_wide_calls(K, monkeypatch)
    _oracle_vs_hip(bs=2, T=5, H=2, O=4, N=34, h=32, backward=True, seed=19, max_nudged_share=0.10)
    assert not any(calls.values()), calls


def test_model_at_72_nodes_eval_mode_against_the_oracle(K):
    """Inference mode (running statistics, no saved X): every output at 1e-4 of tests/test_parity_gpu.py."""
    from tests import test_parity_gpu as P
    H, O, N, bs, T, seed = 2, 4, 72, 2, 5, 19
    torch.manual_seed(seed)
    m = TGGCN(input_size=(2048 + 4 * N, 2048), num_classes=(13, None), hidden_size=32, gcn_node=N, **dict(P.STAGE1))
    x_human, x_objects, mask = P._synthetic(bs, T, H, O, N, seed, 'clip1')
    kw = dict(human_segmentation=torch.ones(bs, T, H))
    noise = torch.distributions.gumbel.Gumbel(0.0, 1.0).sample((T * O, bs, 2))
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    m = m.to(DEV).eval()
    m._gumbel_noise_override = noise
    with torch.no_grad():
        out = m(x_human.to(DEV), x_objects.to(DEV), mask.to(DEV), **{k: v.to(DEV) for k, v in kw.items()})
        ref = cpu_ref.tggcn_forward(sd, dict(m.cfg), x_human, x_objects, mask, training=False, gumbel_noise=noise, **kw)
    assert len(out) == len(ref)
    for i, (o, r) in enumerate(zip(out, ref)):
        err = (o.cpu() - r).abs().max().item() / max(1.0, r.abs().max().item())
        assert err < P.REL, (i, err)


def test_model_at_72_nodes_input_gradients_against_the_oracle(K, monkeypatch):
    """x_human.requires_grad: the geometry gradient against the oracle's under the rule of tests/test_input_grads_gpu.py
    (_input_grads_vs_oracle, imported); the wide input-gradient entry point is what ran."""
    from tests.test_input_grads_gpu import _input_grads_vs_oracle
    calls = _count_wide_calls(K, monkeypatch)
    _input_grads_vs_oracle(bs=2, T=5, H=2, O=4, N=72, h=32, seed=19, max_nudged_share=0.10)
    assert calls['twog_gcn_wide_input_bwd'] > 0, calls


def test_a_model_beyond_the_wide_limit_names_the_limit(K):
    N = K.lib.twog_gcn_wide_max_nodes() + 1
    from tests import test_parity_gpu as P
    m = TGGCN(input_size=(2048 + 4 * N, 2048), num_classes=(13, None), hidden_size=32, gcn_node=N, **dict(P.STAGE1)).to(DEV)
    x_human, x_objects, mask = P._synthetic(1, 2, 2, 4, N, 3, 'clip1')
    with pytest.raises(NotImplementedError, match=f'gcn_node = {N} > {N - 1}'):
        m(x_human.to(DEV), x_objects.to(DEV), mask.to(DEV), human_segmentation=torch.ones(1, 2, 2, device=DEV))
