"""GPU: Adam with its step state on the device (twog_optim_prepare / twog_optim_apply, csrc/train_opts.hip) against the numpy
specification (tests/optim_state_ref.py), bit for bit: synthetic gradients go straight into the buffers, no model runs.

  * prepare over the sequence apply, skip (NaN norm), skip (inf norm), apply, apply, with 0 / 1 / 2 norms, the learning rate by
    value and by pointer, clip coefficients below 1, above 1, NaN and absent; the fp64 powers compared as raw bits;
  * apply over sizes 1, 3, 4, 7, 1029, sub-ranges 0..3 elements into an aligned buffer, one size beyond the capped grid (the
    library's own plan), every combination of decay / clip / EMA, guard elements around every written range, and a skipped
    step that writes nothing;
  * the neutral step judged by the fp64 rule of test_stream_kernels_gpu.test_adam_against_fp64_adam (same cases);
  * FusedAdam end to end, every option on, a poisoned gradient in the middle and a checkpoint through the CPU: the HIP backend
    and the test double agree in every bit.
"""
import io
import itertools

import numpy as np
import pytest
import torch

import twog_gcn_amd  # noqa: F401
from twog_gcn_amd import kernels as twog_kernels
from twog_gcn_amd.distributed import FlatParameters, FusedAdam
from tests import optim_state_ref as R
from tests import stream_cases as SC
from tests.optim_state_fake import OptimStateKernels, state_fields

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
HYPER = dict(beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, grad_scale=0.5, ema_decay=0.99)
GUARD = 8   # elements in front of and behind every range (a multiple of 4: the range begins `off` elements behind a boundary)


@pytest.fixture(scope='module')
def K():
    twog_kernels._set_backend_for_tests(None)
    k = twog_kernels.get_kernels()
    assert k.name == 'hip'
    return k


def _dev(x):
    return torch.tensor([x], dtype=torch.float32, device=DEV)


# ---------------------------------------------------------------------------------------------------------------- prepare
NAN, INF = float('nan'), float('inf')
#            what          norm0, norm1 (the bad one moves between the two)      clip coefficient
SEQUENCE = [('apply', (3.0, 0.25), 0.5),
            ('skip_nan', (NAN, 1.0), 0.25),
            ('skip_inf', (2.0, INF), 2.0),
            ('apply', (1e30, 7.0), NAN),
            ('apply', (0.0, 0.0), None)]


@pytest.mark.parametrize('skip', [True, False], ids=['skip', 'noskip'])
@pytest.mark.parametrize('lr_by', ['value', 'pointer'])
@pytest.mark.parametrize('n_norms', [0, 1, 2])
def test_prepare_is_the_specification_bit_for_bit(K, n_norms, lr_by, skip):
    hyper = dict(HYPER, weight_decay=0.01)
    flags = K.OPTIM_SKIP_NONFINITE if skip else 0
    state = K.new_optim_state(0, 0, hyper['beta1'], hyper['beta2'], DEV)
    ref = R.unpack(state.cpu().numpy())
    assert (ref['step'], ref['beta1_pow'], ref['beta2_pow']) == (0, 1.0, 1.0)
    lr_t = _dev(0.0)
    kinds = []
    for i, (what, norms, coef) in enumerate(SEQUENCE):
        lr = 1e-3 * (i + 1)
        if n_norms == 1:   # the one norm carries the bad value of this step
            norms = (next((x for x in norms if not np.isfinite(x)), norms[0]),)
        norms = norms[:n_norms]
        if lr_by == 'pointer':
            lr_t.fill_(lr)
        K.optim_prepare(state, hyper, lr_t if lr_by == 'pointer' else lr, norms=[_dev(x) for x in norms],
                        coef=None if coef is None else _dev(coef), flags=flags)
        R.prepare(ref, hyper, lr, norms=norms, coef=coef, flags=flags)
        got = state_fields(state)
        want = {k: (np.asarray(v).tobytes().hex() if isinstance(v, np.floating) else int(v)) for k, v in ref.items()}
        assert got == want, (i, what, got, want)
        kinds.append(int(ref['apply']))
    skipped = skip and n_norms > 0
    assert kinds == ([1, 0, 0, 1, 1] if skipped else [1] * 5)
    s = twog_kernels.read_optim_state(state)
    assert (s['step'], s['skipped']) == ((3, 2) if skipped else (5, 0))
    assert s['clip_k'] == 1.0 and s['lr'] == float(F32(5e-3))   # the last step: no coefficient


# ------------------------------------------------------------------------------------------------------------------ apply
OPTIONS = [dict(decay=d, clip=c, ema=e) for d, c, e in itertools.product(('none', 'l2', 'decoupled'), (False, True), (False, True))]
SIZES, OFFSETS = (1, 3, 4, 7, 1029), (0, 1, 2, 3)


def _opt_id(o):
    return f"{o['decay']}{'_clip' if o['clip'] else ''}{'_ema' if o['ema'] else ''}"


def _prepared(K, o, apply=True):
    """A state block three steps in, prepared for a fourth with the options of `o` (or for a skipped one), the hyper-parameters
    and the flags; the specification gets the scalars READ BACK from the block."""
    hyper = dict(HYPER, weight_decay=0.0 if o['decay'] == 'none' else 0.1)
    flags = (K.OPTIM_DECOUPLED if o['decay'] == 'decoupled' else 0) | (K.OPTIM_CLIP if o['clip'] else 0)
    state = K.new_optim_state(3, 0, hyper['beta1'], hyper['beta2'], DEV)
    if apply:
        K.optim_prepare(state, hyper, 1e-2, coef=_dev(0.3) if o['clip'] else None, flags=flags)
    else:
        K.optim_prepare(state, hyper, 1e-2, norms=[_dev(NAN)], flags=flags | K.OPTIM_SKIP_NONFINITE)
    s = R.unpack(state.cpu().numpy())
    assert s['apply'] == int(apply) and s['step'] == (4 if apply else 3)
    if apply:
        assert float(s['clip_k']) == float(F32(0.3) if o['clip'] else 1.0)
    return state, s, hyper, flags


@torch.no_grad()
def _buffers(n, off, seed):
    """Five aligned base buffers of GUARD + off + n + GUARD elements (CPU, fp32): p, g, m, v, ema."""
    gen = torch.Generator().manual_seed(seed)
    total = GUARD + off + n + GUARD
    p, g, m, ema = (torch.randn(total, generator=gen) * s for s in (1.0, 3.0, 0.1, 1.0))
    v = torch.randn(total, generator=gen) ** 2 * 0.01
    return [p, g, m, v, ema]


def _run_case(K, state, s, hyper, flags, ema_on, n, off, seed):
    base = _buffers(n, off, seed)
    dev = [t.to(DEV, copy=True) for t in base]
    assert all(t.data_ptr() % 16 == 0 for t in dev)
    lo, hi = GUARD + off, GUARD + off + n
    views = [t[lo:hi] for t in dev]
    K.optim_apply(views[0], views[1], views[2], views[3], views[4] if ema_on else None, hyper, flags, state)
    want = [t.clone().numpy() for t in base]
    wv = [a[lo:hi] for a in want]
    R.apply(wv[0], wv[1], wv[2], wv[3], wv[4] if ema_on else None, hyper, flags, s)
    torch.cuda.synchronize()
    for name, d, w, b in zip('pgmve', dev, want, base):
        got = d.cpu().numpy()
        assert got.view(np.int32).tobytes() == w.view(np.int32).tobytes(), \
            (name, n, off, int((got.view(np.int32) != w.view(np.int32)).sum()), np.nonzero(got.view(np.int32) != w.view(np.int32))[0][:4].tolist())
        changed = name in 'pmv' or (name == 'e' and ema_on)
        if s['apply'] and changed:
            assert not np.array_equal(got[lo:hi], b.numpy()[lo:hi]), (name, 'the range was not written')
        assert np.array_equal(got[:lo], b.numpy()[:lo]) and np.array_equal(got[hi:], b.numpy()[hi:]), (name, 'guard elements')


@pytest.mark.parametrize('o', OPTIONS, ids=_opt_id)
def test_apply_is_the_specification_bit_for_bit(K, o):
    """Every size and every sub-range offset: a head of (4 - off) % 4 single elements, the 16-byte body, a tail of up to 3; the
    guard elements on both sides of every buffer come back as they were (the whole base buffers are compared)."""
    state, s, hyper, flags = _prepared(K, o)
    for k, (n, off) in enumerate(itertools.product(SIZES, OFFSETS)):
        _run_case(K, state, s, hyper, flags, o['ema'], n, off, seed=1000 + k)
    assert twog_kernels.read_optim_state(state)['step'] == 4   # apply never writes the block


@pytest.mark.parametrize('o', [OPTIONS[0], OPTIONS[-1]], ids=_opt_id)
@pytest.mark.parametrize('off', [0, 3])
def test_apply_strides_beyond_the_capped_grid(K, o, off):
    """One size just above what one trip of the capped grid covers, from the library's own plan (twog_stream_grid): some thread
    is sure to make a second trip of the stride loop, with a ragged end."""
    cap = K.stream_grid(K.STREAM_OPTIM, 2 ** 40)
    n = cap * K.STREAM_THREADS * 4 + 6 + 1029
    grid = K.stream_grid(K.STREAM_OPTIM, n)
    assert grid == cap and grid * K.STREAM_THREADS * 4 < n - 6 and (n - (4 - off) % 4) % 4 != 0   # second trip; a tail behind the body
    state, s, hyper, flags = _prepared(K, o)
    _run_case(K, state, s, hyper, flags, o['ema'], n, off, seed=77)


@pytest.mark.parametrize('o', [OPTIONS[-1], OPTIONS[4]], ids=_opt_id)
def test_a_skipped_step_writes_nothing(K, o):
    state, s, hyper, flags = _prepared(K, o, apply=False)
    for n, off in ((1029, 1), (5, 0)):
        _run_case(K, state, s, hyper, flags, True, n, off, seed=5)   # _run_case compares all five whole buffers


# ------------------------------------------------------------------------------------------ neutral options against fp64
class _AsAdamStep:
    """adam_step of the streaming-kernel cases (tests/stream_cases.adam_run) on the new entry points with neutral options: a
    state block at step - 1, one prepare, one apply."""

    def __init__(self, K):
        self.K = K

    def adam_step(self, param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0):
        h = dict(beta1=beta1, beta2=beta2, eps=eps, weight_decay=weight_decay, grad_scale=grad_scale, ema_decay=None)
        st = self.K.new_optim_state(step - 1, 0, beta1, beta2, param.device)
        self.K.optim_prepare(st, h, lr)
        self.K.optim_apply(param, grad, exp_avg, exp_avg_sq, None, h, 0, st)


@pytest.mark.parametrize('c', SC.ADAM_CASES, ids=lambda c: c['id'])
def test_neutral_step_against_fp64_adam(K, c):
    """The rule test_adam_against_fp64_adam applies to twog_adam_step (tests.entity_envelope.judge: e_hip <= 8 e_ref + 4 x 2^-24
    against the specification of twog_adam_step in fp64, the fp32 run's own error as the yardstick), on the same cases."""
    from tests.test_stream_kernels_gpu import Verdict
    s32, s64 = SC.adam_run(SC.F, c, 'cpu', torch.float32), SC.adam_run(SC.F, c, 'cpu', torch.float64)
    hip = SC.adam_run(_AsAdamStep(K), c, DEV, torch.float32)
    torch.cuda.synchronize()
    V = Verdict('optim_neutral_' + c['id'])
    V.all(hip, s32, s64)
    V.check()


# ------------------------------------------------------------------------------------------------------------- end to end
class _Extra(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.log_sds = torch.nn.Parameter(torch.zeros(6))


def _small(seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(5, 3), torch.nn.Tanh(), torch.nn.Linear(3, 7)), _Extra()   # 15, 3, 21, 7; 6


def _end_to_end(dev):
    """5 steps, the third with a NaN in the model's gradient, every option on, the learning rate a device tensor that a
    schedule changes; after the fourth step the optimizer goes through a checkpoint on the CPU into a new one."""
    kw = dict(max_grad_norm=0.5, skip_nonfinite=True, decoupled_weight_decay=True, weight_decay=0.05, ema_decay=0.9)

    def make():
        model, extra = _small()
        model, extra = model.to(dev), extra.to(dev)
        flat = FlatParameters(model, stage_of=lambda name: 0 if name.endswith('bias') else 1, extra_modules=[extra])
        return model, extra, flat

    model, extra, flat = make()
    lr = torch.tensor([1e-2], dtype=torch.float32, device=dev)
    opt = FusedAdam(flat, lr=lr, **kw)
    norms = []
    for k in range(5):
        g = torch.randn(flat.numel, generator=torch.Generator().manual_seed(300 + k)) * (2.0 if k % 2 else 0.05)
        full = torch.zeros(flat.numel)
        for p in flat.params:
            o = p.data.storage_offset()
            full[o:o + p.numel()] = g[o:o + p.numel()]
        if k == 2:
            full[flat.params[1].data.storage_offset() + 1] = NAN
        opt.flat.grad.copy_(full)
        lr.fill_(1e-2 / (k + 1))
        norms.append(opt.step(0.5).cpu())
        if k == 3:
            f = io.BytesIO()
            torch.save(dict(model=model.state_dict(), extra=extra.state_dict(), opt=opt.state_dict()), f)
            ck = torch.load(io.BytesIO(f.getvalue()), map_location='cpu', weights_only=False)
            model, extra, flat = make()
            model.load_state_dict(ck['model'])
            extra.load_state_dict(ck['extra'])
            opt = FusedAdam(flat, lr=lr, **kw)
            opt.load_state_dict(ck['opt'])
    with opt.swap_ema():
        swapped = opt.flat.flat.cpu().clone()
    out = dict(p=opt.flat.flat, m=opt.exp_avg, v=opt.exp_avg_sq, ema=opt.ema, norms=torch.stack(norms))
    out = {k: t.detach().cpu().clone() for k, t in out.items()}
    assert torch.equal(swapped, out['ema'])
    return out, state_fields(opt.state), (opt.step_number(), opt.skipped_steps())


def test_end_to_end_hip_and_the_test_double_agree_in_every_bit(K):
    twog_kernels._set_backend_for_tests(OptimStateKernels())
    try:
        want, want_state, want_counts = _end_to_end('cpu')
    finally:
        twog_kernels._set_backend_for_tests(None)
    got, got_state, got_counts = _end_to_end(DEV)
    assert want_counts == got_counts == (4, 1)
    assert not bool(torch.isfinite(want['norms'][2])) and bool(torch.isfinite(want['norms'][[0, 1, 3, 4]]).all())
    for k in want:
        assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), k
    assert got_state == want_state
    assert bool(torch.isfinite(got['p']).all()) and not torch.equal(got['p'], got['ema'])
