"""CPU: Adam with its step state on the device (FusedAdam's device path: checkpoints, NaN skip, AdamW, EMA) on the kernel test
double (tests/optim_state_fake.OptimStateKernels), and the numpy specification behind it (tests/optim_state_ref.py).

  * the specification in fp64 against torch.optim.Adam in fp64 (plain, L2, decoupled, clipped), and its hand-computed cases;
  * FusedAdam: resume from state_dict() bit for bit, interchange with torch.optim.Adam in both directions, a NaN / inf gradient
    skipped without a trace (and not skipped without the option), swap_ema(), the calls each option issues, the device path
    with neutral options against the path without device state;
  * the layout of twog_optim_state_t against the C compiler, and the argument checks of the two entry points (no device).
"""
import ctypes
import io
import os
import subprocess

import numpy as np
import pytest
import torch

import twog_gcn_amd  # noqa: F401
from twog_gcn_amd import _lib
from twog_gcn_amd import kernels as twog_kernels
from twog_gcn_amd.distributed import DataParallel, FlatParameters, FusedAdam
from tests import optim_state_ref as R
from tests.optim_state_fake import OptimStateKernels, state_fields
from tests.helpers import ROOT
from tests.train_options_helpers import check_deltas

F32, F64 = np.float32, np.float64
HEADER = os.path.join(ROOT, 'include', 'twog_gcn.h')


@pytest.fixture
def double():
    K = OptimStateKernels()
    twog_kernels._set_backend_for_tests(K)
    yield K
    twog_kernels._set_backend_for_tests(None)


# ------------------------------------------------------------------------------------------------------ the specification
@pytest.mark.parametrize('case', ['plain', 'l2', 'decoupled', 'clipped'])
def test_specification_in_fp64_is_torch_adam_in_fp64(case):
    """5 steps on random tensors. 1e-12 relative (of the tensor's largest magnitude) is the project's fp64 bound: both sides
    round every operation to fp64 (2^-53), torch in another order (lerp, addcdiv)."""
    g = torch.Generator().manual_seed(5)
    shapes, steps, lr, betas, eps, max_norm = [(7, 5), (33,), (3, 4, 2)], 5, 1e-2, (0.9, 0.999), 1e-8, 0.7
    wd = 0.0 if case in ('plain', 'clipped') else 0.1
    ps = [torch.nn.Parameter(torch.randn(*s, generator=g, dtype=torch.float64)) for s in shapes]
    opt = torch.optim.Adam(ps, lr=lr, betas=betas, eps=eps, weight_decay=wd, decoupled_weight_decay=case == 'decoupled',
                           foreach=False)
    sizes = [p.numel() for p in ps]
    p = np.concatenate([t.detach().numpy().reshape(-1) for t in ps]).copy()
    m, v = np.zeros_like(p), np.zeros_like(p)
    hyper = dict(beta1=betas[0], beta2=betas[1], eps=eps, weight_decay=wd, grad_scale=1.0, ema_decay=None)
    state = R.new_state(0, 0, *betas)
    state['beta1_pow'], state['beta2_pow'] = F64(1), F64(1)
    flags = (R.DECOUPLED if case == 'decoupled' else 0) | (R.CLIP if case == 'clipped' else 0)
    for k in range(steps):
        grads = [torch.randn(*s, generator=g, dtype=torch.float64) * (3.0 if k % 2 else 0.05) for s in shapes]
        gflat = np.concatenate([t.numpy().reshape(-1) for t in grads])
        coef = None
        if case == 'clipped':
            coef = max_norm / (np.sqrt((gflat * gflat).sum()) + 1e-6)
        for t, gr in zip(ps, grads):
            t.grad = gr.clone()
        if case == 'clipped':
            torch.nn.utils.clip_grad_norm_(ps, max_norm)
        opt.step()
        R.prepare(state, hyper, lr, coef=coef, flags=flags, dtype=F64)
        R.apply(p, gflat, m, v, None, hyper, flags, state, dtype=F64)
    if case == 'clipped':
        assert state['clip_k'] == 1.0   # the last (small) gradient is below the bound, the one before was clipped
    off = 0
    for t, n in zip(ps, sizes):
        st = opt.state[t]
        for name, ours, theirs in (('p', p, t.detach()), ('m', m, st['exp_avg']), ('v', v, st['exp_avg_sq'])):
            want = theirs.numpy().reshape(-1)
            err = np.abs(ours[off:off + n] - want).max() / np.abs(want).max()
            assert err <= 1e-12, (case, name, err)
        assert int(st['step']) == state['step'] == steps
        off += n


@pytest.mark.parametrize('dtype', [F32, F64], ids=['fp32', 'fp64'])
@pytest.mark.parametrize('case', R.HAND_CASES, ids=lambda c: c[0])
def test_specification_reproduces_the_hand_computed_steps(case, dtype):
    name, flags, wd, coef, grad, gscale, want = case
    H = R.HAND_HYPER
    hyper = dict(beta1=H['beta1'], beta2=H['beta2'], eps=H['eps'], weight_decay=wd, grad_scale=gscale, ema_decay=H['ema_decay'])
    state = R.new_state(0, 0, H['beta1'], H['beta2'])
    R.prepare(state, hyper, H['lr'], coef=coef, flags=flags, dtype=dtype)
    assert (state['step'], state['beta1_pow'], state['beta2_pow'], state['step_size'], state['bc2s']) == (1, 0.5, 0.75, 0.5, 0.5)
    assert state['clip_k'] == want.get('clip_k', 1.0) and state['decay_mul'] == 1.0 - H['lr'] * wd   # written by every applied prepare
    p, g, m, v, ema = (np.full(3, x, dtype=dtype) for x in (1.0, grad, 0.0, 0.0, 1.0))
    R.apply(p, g, m, v, ema, hyper, flags, state, dtype=dtype)
    for k, a in (('p', p), ('m', m), ('v', v), ('ema', ema)):
        assert a.dtype == dtype and (a == want[k]).all(), (name, k, a, want[k])


def test_specification_skips_and_counts():
    hyper = dict(beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, grad_scale=1.0, ema_decay=None)
    s = R.new_state(3, 1, 0.9, 0.999)
    before = dict(s)
    R.prepare(s, hyper, 1e-3, norms=[1.0, float('inf')], flags=R.SKIP_NONFINITE)
    assert s == dict(before, skipped=2, apply=0)
    R.prepare(s, hyper, 1e-3, norms=[float('nan')], flags=0)   # not asked to skip: the step is applied
    assert s['step'] == 4 and s['apply'] == 1 and s['skipped'] == 2
    assert R.unpack(R.pack(s)) == s and R.pack(s).nbytes == 64


# --------------------------------------------------------------------------------------------- FusedAdam on the test double
class _Extra(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.log_sds = torch.nn.Parameter(torch.zeros(6))


def _small(seed=0):
    """A model whose parameter sizes (15, 3, 21, 7) are no multiples of 4, and an extra module (6)."""
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(5, 3), torch.nn.Tanh(), torch.nn.Linear(3, 7)), _Extra()


def _flat(model, extra):
    # biases first in the flat layout: the layout's order is NOT the order of model.parameters()
    return FlatParameters(model, stage_of=lambda name: 0 if name.endswith('bias') else 1, extra_modules=[extra])


def _grad(flat, k, seed=100):
    """A seeded gradient in every parameter's view; the padding between the views stays zero, as in a training step."""
    g = torch.randn(flat.numel, generator=torch.Generator().manual_seed(seed + k)) * (2.0 if k % 2 else 0.1)
    flat.grad.zero_()
    for p in flat.params:
        off = p.data.storage_offset()
        flat.grad[off:off + p.numel()] = g[off:off + p.numel()]


MODES = {
    'legacy': dict(weight_decay=0.01),
    'legacy_clip': dict(max_grad_norm=0.5),
    'device': dict(device_state=True, weight_decay=0.01),
    'device_ema': dict(ema_decay=0.9),
    'device_all': dict(ema_decay=0.9, skip_nonfinite=True, decoupled_weight_decay=True, weight_decay=0.01, max_grad_norm=0.5),
}


def _buffers(opt):
    b = dict(p=opt.flat.flat, m=opt.exp_avg, v=opt.exp_avg_sq)
    if opt.ema is not None:
        b['ema'] = opt.ema
    return {k: t.detach().clone() for k, t in b.items()}


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k   # bit for bit (NaN included)


def _scalars(opt):
    return state_fields(opt.state) if opt.on_device else dict(step=opt.step_count)


@pytest.mark.parametrize('mode', MODES)
def test_resume_from_state_dict_is_bit_identical(double, mode):
    model, extra = _small()
    opt = FusedAdam(_flat(model, extra), lr=1e-2, **MODES[mode])
    for k in range(4):
        _grad(opt.flat, k)
        opt.step(0.5)
    want, want_scalars = _buffers(opt), _scalars(opt)

    model, extra = _small()
    opt = FusedAdam(_flat(model, extra), lr=1e-2, **MODES[mode])
    for k in range(2):
        _grad(opt.flat, k)
        opt.step(0.5)
    f = io.BytesIO()
    torch.save(dict(model=model.state_dict(), extra=extra.state_dict(), opt=opt.state_dict()), f)
    ck = torch.load(io.BytesIO(f.getvalue()), weights_only=False)

    model, extra = _small(seed=9)   # a fresh process: other initial weights, a new optimizer with ANOTHER learning rate
    opt = FusedAdam(_flat(model, extra), lr=3e-4, **MODES[mode])
    model.load_state_dict(ck['model'])
    extra.load_state_dict(ck['extra'])
    opt.load_state_dict(ck['opt'])
    assert opt.step_number() == 2 and opt.skipped_steps() == 0 and opt.lr == 1e-2
    for k in range(2, 4):
        _grad(opt.flat, k)
        opt.step(0.5)
    _same(_buffers(opt), want)
    assert _scalars(opt) == want_scalars
    assert opt.step_number() == 4


def _torch_adam(model, extra, lr, **kw):
    """The reference's construction (train.py:39-46)."""
    o = torch.optim.Adam(model.parameters(), lr=lr, **kw)
    o.add_param_group({'params': extra.parameters()})
    return o


@pytest.mark.parametrize('mode', ['legacy', 'device'])
def test_state_moves_to_torch_adam_and_back(double, mode):
    kw = dict(device_state=True) if mode == 'device' else {}
    # ours -> torch
    model, extra = _small()
    opt = FusedAdam(_flat(model, extra), lr=1e-2, **kw)
    for k in range(2):
        _grad(opt.flat, k)
        opt.step()
    sd = opt.state_dict()
    assert [len(g['params']) for g in sd['param_groups']] == [4, 1]
    tmodel, textra = _small()
    topt = _torch_adam(tmodel, textra, lr=5e-1)
    topt.load_state_dict(sd)
    for (name, p), tp in zip(list(model.named_parameters()) + list(extra.named_parameters()),
                             list(tmodel.parameters()) + list(textra.parameters())):
        st = topt.state[tp]
        assert int(st['step']) == 2
        for key, buf in (('exp_avg', opt.exp_avg), ('exp_avg_sq', opt.exp_avg_sq)):
            assert st[key].shape == p.shape and torch.equal(st[key], opt._view(buf, p)), (name, key)
            off = p.data.storage_offset()
            assert torch.equal(st[key].reshape(-1), buf[off:off + p.numel()])   # the flat slice itself
    assert topt.param_groups[0]['lr'] == 1e-2 and topt.param_groups[1]['lr'] == 1e-2
    for tp in list(tmodel.parameters()) + list(textra.parameters()):
        tp.grad = torch.ones_like(tp)
    topt.step()   # the layout is complete: torch continues on it
    assert int(topt.state[next(iter(tmodel.parameters()))]['step']) == 3

    # torch -> ours
    tmodel, textra = _small()
    topt = _torch_adam(tmodel, textra, lr=2e-3, weight_decay=0.01)
    gen = torch.Generator().manual_seed(3)
    for _ in range(3):
        for tp in list(tmodel.parameters()) + list(textra.parameters()):
            tp.grad = torch.randn(tp.shape, generator=gen)
        topt.step()
    model, extra = _small(seed=4)
    opt = FusedAdam(_flat(model, extra), lr=1.0, **kw)
    opt.load_state_dict(topt.state_dict())
    assert opt.step_number() == 3 and opt.skipped_steps() == 0 and (opt.lr, opt.wd) == (2e-3, 0.01)
    for (name, p), tp in zip(list(model.named_parameters()) + list(extra.named_parameters()),
                             list(tmodel.parameters()) + list(textra.parameters())):
        for key, buf in (('exp_avg', opt.exp_avg), ('exp_avg_sq', opt.exp_avg_sq)):
            off = p.data.storage_offset()
            assert torch.equal(buf[off:off + p.numel()], topt.state[tp][key].reshape(-1)), (name, key)
    if mode == 'device':   # the powers are rebuilt by 3 fp64 multiplications by the fp32 betas
        want = R.new_state(3, 0, 0.9, 0.999)
        got = R.unpack(opt.state.numpy())
        assert got['beta1_pow'].tobytes() == want['beta1_pow'].tobytes() and got['beta2_pow'].tobytes() == want['beta2_pow'].tobytes()
    with pytest.raises(ValueError):   # a checkpoint of other parameters
        FusedAdam(FlatParameters(_small()[0]), **kw).load_state_dict(topt.state_dict())


BAD = [('nan_model', float('nan'), 'model'), ('inf_model', float('inf'), 'model'), ('nan_extra', float('nan'), 'extra'),
       ('neg_inf_extra', float('-inf'), 'extra')]


def _poison(flat, value, where):
    b, e = flat.module_ranges[0 if where == 'model' else 1]
    flat.grad[b + (e - b) // 2] = value


@pytest.mark.parametrize('bad', BAD, ids=lambda b: b[0])
def test_a_nonfinite_gradient_is_skipped_without_a_trace(double, bad):
    _, value, where = bad
    kw = dict(lr=1e-2, skip_nonfinite=True, ema_decay=0.9, max_grad_norm=0.5, weight_decay=0.01)
    opt = FusedAdam(_flat(*_small()), **kw)
    _grad(opt.flat, 0)
    opt.step()
    before, scalars = _buffers(opt), _scalars(opt)
    _grad(opt.flat, 7)
    _poison(opt.flat, value, where)
    norm = opt.step()
    assert torch.isfinite(norm) == (where == 'extra')   # the returned norm is the model's
    _same(_buffers(opt), before)
    assert _scalars(opt) == dict(scalars, skipped=1, apply=0)   # step, both powers and the step's scalars: unchanged bits
    assert opt.skipped_steps() == 1 and opt.step_number() == 1
    _grad(opt.flat, 1)
    opt.step()

    clean = FusedAdam(_flat(*_small()), **kw)   # a run that never saw the bad gradient
    for k in range(2):
        _grad(clean.flat, k)
        clean.step()
    _same(_buffers(opt), _buffers(clean))
    assert _scalars(opt) == dict(_scalars(clean), skipped=1)


@pytest.mark.parametrize('bad', BAD[:2], ids=lambda b: b[0])
def test_without_skip_nonfinite_the_bad_gradient_reaches_the_parameters(double, bad):
    _, value, where = bad
    opt = FusedAdam(_flat(*_small()), lr=1e-2, ema_decay=0.9)
    _grad(opt.flat, 7)
    _poison(opt.flat, value, where)
    opt.step()
    b, e = opt.flat.module_ranges[0]
    for buf in (opt.flat.flat, opt.ema):
        assert not bool(torch.isfinite(buf[b + (e - b) // 2]))
    assert opt.skipped_steps() == 0 and opt.step_number() == 1


def test_swap_ema_exchanges_and_restores(double):
    model, extra = _small()
    opt = FusedAdam(_flat(model, extra), lr=1e-2, ema_decay=0.5)
    assert torch.equal(opt.ema, opt.flat.flat)   # starts as a copy of the parameters
    for k in range(2):
        _grad(opt.flat, k)
        opt.step()
    before = _buffers(opt)
    assert not torch.equal(before['p'], before['ema'])
    with opt.swap_ema():
        assert torch.equal(opt.flat.flat, before['ema']) and torch.equal(opt.ema, before['p'])
        assert torch.equal(model[0].weight.detach(), opt._view(before['ema'], model[0].weight))   # the model runs on the average
        with pytest.raises(RuntimeError, match='swap_ema'):
            opt.step()
    _same(_buffers(opt), before)
    ema = opt.ema_state_dict()
    assert list(ema) == [n for n, _ in model.named_parameters()]
    assert torch.equal(ema['2.bias'], opt._view(opt.ema, model[2].bias))
    other, _ = _small(seed=3)
    assert not other.load_state_dict(ema, strict=False).unexpected_keys
    with pytest.raises(RuntimeError, match='ema_decay'):
        FusedAdam(_flat(*_small())).ema_state_dict()


def test_lr_as_a_device_tensor_is_the_same_step(double):
    a = FusedAdam(_flat(*_small()), lr=1e-2, device_state=True)
    lr = torch.tensor([1e-2], dtype=torch.float32)
    b = FusedAdam(_flat(*_small()), lr=lr)
    assert b.on_device
    for k in range(2):
        for o in (a, b):
            _grad(o.flat, k)
            o.step()
    _same(_buffers(a), _buffers(b))
    lr.fill_(0.0)   # a schedule writes the tensor: the next step reads it
    before = b.flat.flat.clone()
    _grad(b.flat, 2)
    b.step()
    assert torch.equal(b.flat.flat, before) and b.step_number() == 3


def test_the_calls_each_option_issues(double):
    flat = _flat(*_small())
    (b, e), n = flat.module_ranges[0], flat.numel
    K = double

    def calls(**kw):
        opt = FusedAdam(flat, **kw)
        before = len(K.calls)
        out = opt.step(0.5)
        return [c for c in K.calls[before:]], out

    # today's arguments: today's calls, no state block
    got, out = calls()
    assert got == [('adam_step', n)] and out is None
    got, out = calls(max_grad_norm=1.0)
    assert got == [('grad_norm', ((b, e),)), ('adam_step_coef', e - b), ('adam_step', n - e)] and out.dim() == 0
    assert not [c for c in K.calls if c[0].startswith('optim_') or c[0] == 'new_optim_state']
    # the device path, in the order norm(s), prepare, apply (model), apply (extra modules)
    got, out = calls(device_state=True)
    assert got == [('optim_prepare', 0, False, 0), ('optim_apply', e - b, False, 0), ('optim_apply', n - e, False, 0)] and out is None
    got, out = calls(ema_decay=0.99, decoupled_weight_decay=True)
    assert got == [('optim_prepare', 0, False, K.OPTIM_DECOUPLED), ('optim_apply', e - b, True, K.OPTIM_DECOUPLED),
                   ('optim_apply', n - e, True, K.OPTIM_DECOUPLED)]
    got, out = calls(device_state=True, max_grad_norm=1.0)
    assert got == [('grad_norm', ((b, e),)), ('optim_prepare', 1, True, 0), ('optim_apply', e - b, False, K.OPTIM_CLIP),
                   ('optim_apply', n - e, False, 0)] and out.dim() == 0
    S = K.OPTIM_SKIP_NONFINITE
    got, out = calls(skip_nonfinite=True)
    assert got == [('grad_norm', ((b, e),)), ('grad_norm', ((e, n),)), ('optim_prepare', 2, False, S), ('optim_apply', e - b, False, S),
                   ('optim_apply', n - e, False, S)] and out.dim() == 0
    got, out = calls(skip_nonfinite=True, max_grad_norm=1.0)
    assert got == [('grad_norm', ((b, e),)), ('grad_norm', ((e, n),)), ('optim_prepare', 2, True, S),
                   ('optim_apply', e - b, False, S | K.OPTIM_CLIP), ('optim_apply', n - e, False, S)]
    # no extra module: one norm, one apply
    flat1 = FlatParameters(_small()[0])
    opt = FusedAdam(flat1, skip_nonfinite=True)
    before = len(K.calls)
    opt.step()
    assert K.calls[before:] == [('grad_norm', ((0, flat1.numel),)), ('optim_prepare', 1, False, S), ('optim_apply', flat1.numel, False, S)]
    for bad in (0.0, 1.0, -0.5):
        with pytest.raises(ValueError, match='ema_decay'):
            FusedAdam(flat1, ema_decay=bad)


def test_defaults_issue_only_the_calls_of_the_step_without_device_state(double):
    """The step of a model under DataParallel with today's arguments: one fused Adam launch, nothing of the new entry points."""
    from tests.test_train_options_cpu import _batch, _tiny_model
    xh, xo, mask, cls, seg = _batch()
    model = _tiny_model().train()
    dp = DataParallel(model)
    opt = FusedAdam(dp.flat, lr=1e-3)
    dp.zero_grad()
    torch.nn.functional.nll_loss(model(xh, xo, mask)[4], cls, ignore_index=-1).backward()
    dp.all_reduce_gradients()
    before = len(double.calls)
    assert opt.step(dp.grad_scale) is None
    assert double.calls[before:] == [('adam_step', dp.flat.numel)]
    assert not [c for c in double.calls if c[0] in ('grad_norm', 'new_optim_state', 'optim_prepare', 'optim_apply')]
    assert opt.state is None and opt.ema is None and opt.step_number() == 1 and opt.skipped_steps() == 0
    dp.close()


def test_neutral_device_path_stays_within_the_trajectory_bound_of_the_path_without_device_state(double):
    """3 steps of the tiny model: the two paths differ by contraction and the form of the bias corrections only, so the
    parameter deltas agree by the rule of the training-trajectory tests (train_options_helpers.check_deltas)."""
    from tests.test_train_options_cpu import _batch, _tiny_model
    xh, xo, mask, cls, seg = _batch()
    lr, steps, deltas = 1e-3, 3, []
    for kw in ({}, dict(device_state=True)):
        model = _tiny_model().train()
        torch.manual_seed(21)   # the Gumbel noise of the forward passes
        dp = DataParallel(model)
        opt = FusedAdam(dp.flat, lr=lr, **kw)
        init = dp.flat.flat.clone()
        for _ in range(steps):
            dp.zero_grad()
            torch.nn.functional.nll_loss(model(xh, xo, mask)[4], cls, ignore_index=-1).backward()
            dp.all_reduce_gradients()
            opt.step(dp.grad_scale)
        deltas.append((dp.flat.flat - init).numpy())
        assert opt.step_number() == steps
        dp.close()
    assert np.abs(deltas[0]).max() > 0.5 * lr
    check_deltas(deltas[1], deltas[0], dict(lr=lr, steps=steps), 'device path against the path without device state')


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_state_block_layout_matches_the_c_compiler(tmp_path):
    """sizeof and every field offset of twog_optim_state_t / twog_optim_hyper_t: the C compiler, ctypes and the numpy record."""
    structs = {'twog_optim_state_t': _lib.OptimState, 'twog_optim_hyper_t': _lib.OptimHyper}
    body = ''
    for name, cls in structs.items():
        body += f'printf("{name} size %zu\\n", sizeof({name}));'
        body += ''.join(f'printf("{name} {f} %zu\\n", offsetof({name}, {f}));' for f, _ in cls._fields_)
    src = tmp_path / 'layout.c'
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\nint main(void){{{body}return 0;}}\n')
    subprocess.run(['gcc', str(src), '-o', str(tmp_path / 'layout')], check=True)
    out = subprocess.run([str(tmp_path / 'layout')], capture_output=True, text=True, check=True).stdout
    seen = 0
    for line in out.strip().splitlines():
        name, field, value = line.split()
        cls = structs[name]
        assert (ctypes.sizeof(cls) if field == 'size' else getattr(cls, field).offset) == int(value), line
        if name == 'twog_optim_state_t':
            assert (R.STATE_DTYPE.itemsize if field == 'size' else R.STATE_DTYPE.fields[field][1]) == int(value), line
        seen += 1
    assert seen == 2 + len(_lib.OptimState._fields_) + len(_lib.OptimHyper._fields_)
    assert ctypes.sizeof(_lib.OptimState) == 64
    blk = twog_kernels.optim_state_block(3, 2, 0.9, 0.999)
    assert blk.dtype == torch.uint8 and blk.numel() == 64
    got, want = R.unpack(blk.numpy()), R.new_state(3, 2, 0.9, 0.999)
    assert all(np.asarray(got[k]).tobytes() == np.asarray(want[k], dtype=np.asarray(got[k]).dtype).tobytes()
               for k in ('step', 'skipped', 'beta1_pow', 'beta2_pow', 'clip_k', 'decay_mul', 'apply'))
    assert twog_kernels.read_optim_state(blk)['beta2_pow'] == float(want['beta2_pow'])


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """-2 without a device: NULL pointers, n_norms outside 0..2, an ema_decay outside (0, 1) with an EMA buffer, pointers that
    are not congruent modulo 16 bytes. (The pointers are never dereferenced on the host.)"""
    lib = _lib.load()
    h = _lib.OptimHyper(0.9, 0.999, 1e-8, 0.0, 1.0, 0.5)
    hp = ctypes.byref(h)
    st, a = 4096, 8192   # stand-ins for device addresses
    two = (ctypes.c_void_p * 2)(a, a + 4)
    assert lib.twog_optim_prepare(None, hp, 1e-3, None, None, 0, None, 0, None) == -2
    assert lib.twog_optim_prepare(st, None, 1e-3, None, None, 0, None, 0, None) == -2
    for n in (-1, 3):
        assert lib.twog_optim_prepare(st, hp, 1e-3, None, two, n, None, 0, None) == -2
    assert lib.twog_optim_prepare(st, hp, 1e-3, None, None, 1, None, 0, None) == -2
    assert lib.twog_optim_prepare(st, hp, 1e-3, None, (ctypes.c_void_p * 2)(a, None), 2, None, 0, None) == -2
    ok = [a, a + 1024, a + 2048, a + 3072, a + 4096]
    for i in range(4):
        args = list(ok)
        args[i] = None
        assert lib.twog_optim_apply(*args, 8, hp, 0, st, None) == -2
    assert lib.twog_optim_apply(*ok, 8, None, 0, st, None) == -2 and lib.twog_optim_apply(*ok, 8, hp, 0, None, None) == -2
    assert lib.twog_optim_apply(*ok, -1, hp, 0, st, None) == -2
    for d in (0.0, 1.0, -0.1, 1.5, float('nan')):
        bad = _lib.OptimHyper(0.9, 0.999, 1e-8, 0.0, 1.0, d)
        assert lib.twog_optim_apply(*ok, 8, ctypes.byref(bad), 0, st, None) == -2
    for i in (1, 2, 3, 4):   # one buffer 4 bytes off the others; a pointer that is not 4-byte aligned
        args = list(ok)
        args[i] += 4
        assert lib.twog_optim_apply(*args, 8, hp, 0, st, None) == -2
    assert lib.twog_optim_apply(*[x + 2 for x in ok], 8, hp, 0, st, None) == -2
    assert lib.twog_optim_apply(*ok, 0, hp, 0, st, None) == 0   # nothing to do: no launch


def test_launch_free_grid_of_the_update():
    """twog_stream_grid(TWOG_STREAM_OPTIM): groups of four elements, 256 threads, a cap that is reached; the ids before it stay."""
    lib = _lib.load()
    K = OptimStateKernels()
    cap = lib.twog_stream_grid(K.STREAM_OPTIM, 2 ** 40, 0)
    assert cap == lib.twog_stream_grid(K.STREAM_OPTIM, 2 ** 41, 0) == K.stream_grid(K.STREAM_OPTIM, 2 ** 40)
    works = [0, 1, 3, 4, 1023, 1024, 1025, 1029, 4 * 256 * 7 + 5, cap * 1024 - 1, cap * 1024, cap * 1024 + 1]
    grids = [lib.twog_stream_grid(K.STREAM_OPTIM, w, 0) for w in works]
    assert grids[0] == 1 and grids == sorted(grids) and grids[-1] == cap
    for w, g in zip(works, grids):
        assert g == cap or g * 256 * 4 >= w - 3, (w, g)
    assert lib.twog_stream_grid(K.STREAM_OPTIM, -1, 0) == -2 and lib.twog_stream_grid(14, 1, 0) == -2
    assert twog_kernels.HipKernels.STREAM_OPTIM == K.STREAM_OPTIM
