"""The numpy specification of Adam with its step state on the device: twog_optim_prepare and twog_optim_apply of
include/twog_gcn.h ("Adam with its step state on the device"), csrc/train_opts.hip.

dtype=np.float32 is the contract of the kernels: every fp32 operation below is one numpy operation on fp32 operands, so it is
rounded once and nothing is fused; the step's powers of the betas are fp64 running products (no pow), the two bias
corrections one fp64 subtraction (and square root) rounded to fp32. The HIP kernels must reproduce it bit for bit
(tests/test_optim_state_gpu.py). dtype=np.float64 runs the same statements in fp64 (every fl() is then an fp64 rounding): the
form that is compared with torch.optim.Adam in fp64 (tests/test_optim_state_cpu.py).

The state is a dict with the fields of twog_optim_state_t; pack() / unpack() move it to and from the 64 bytes of the block.
"""
import numpy as np

CLIP, DECOUPLED, SKIP_NONFINITE = 1, 2, 4   # TWOG_OPTIM_*
STATE_DTYPE = np.dtype([('step', '<i8'), ('skipped', '<i8'), ('beta1_pow', '<f8'), ('beta2_pow', '<f8'), ('lr', '<f4'),
                        ('step_size', '<f4'), ('bc2s', '<f4'), ('clip_k', '<f4'), ('decay_mul', '<f4'), ('apply', '<i4'),
                        ('reserved_', '<i8')])
assert STATE_DTYPE.itemsize == 64
FIELDS = [n for n in STATE_DTYPE.names if n != 'reserved_']


def new_state(step=0, skipped=0, beta1=0.9, beta2=0.999):
    """The block at `step`: the powers by `step` fp64 multiplications by the fp32 betas, a neutral current step."""
    b1, b2, p1, p2 = np.float64(np.float32(beta1)), np.float64(np.float32(beta2)), np.float64(1.0), np.float64(1.0)
    for _ in range(step):
        p1, p2 = p1 * b1, p2 * b2
    return dict(step=step, skipped=skipped, beta1_pow=p1, beta2_pow=p2, lr=np.float32(0), step_size=np.float32(0),
                bc2s=np.float32(0), clip_k=np.float32(1), decay_mul=np.float32(1), apply=1)


def unpack(block):
    """64 bytes (any array of them) -> state dict."""
    rec = np.frombuffer(np.ascontiguousarray(block).tobytes(), dtype=STATE_DTYPE)[0]
    return {n: rec[n] for n in FIELDS}


def pack(state):
    rec = np.zeros(1, dtype=STATE_DTYPE)
    for n in FIELDS:
        rec[n][0] = state[n]
    return np.frombuffer(rec.tobytes(), dtype=np.uint8).copy()


def prepare(state, hyper, lr, norms=(), coef=None, flags=0, dtype=np.float32):
    """twog_optim_prepare on the state dict, in place. lr: the learning rate the launch sees (by value or read through lr_ptr:
    the same statement); norms: up to two fp32 norms; coef: the clip coefficient or None."""
    f = dtype
    assert len(norms) <= 2
    with np.errstate(all='ignore'):
        finite = all(bool(np.isfinite(np.float32(x))) for x in norms)
        if (flags & SKIP_NONFINITE) and not finite:
            state['skipped'] = state['skipped'] + 1
            state['apply'] = 0
            return state
        b1p = np.float64(state['beta1_pow']) * np.float64(f(hyper['beta1']))
        b2p = np.float64(state['beta2_pow']) * np.float64(f(hyper['beta2']))
        lr = f(lr)
        bc1 = f(np.float64(1.0) - b1p)
        k = f(1)
        if coef is not None and f(coef) < f(1):   # a NaN coefficient compares false: no clipping
            k = f(coef)
        state.update(step=state['step'] + 1, beta1_pow=b1p, beta2_pow=b2p, lr=lr, step_size=f(lr / bc1),
                     bc2s=f(np.sqrt(np.float64(1.0) - b2p)), clip_k=k, decay_mul=f(f(1) - f(lr * f(hyper['weight_decay']))),
                     apply=1)
    return state


def apply(p, g, m, v, ema, hyper, flags, state, dtype=np.float32):
    """twog_optim_apply on numpy arrays of `dtype`, in place (g is read only; ema may be None)."""
    if not state['apply']:
        return
    f = dtype
    for a in (p, g, m, v) + (() if ema is None else (ema,)):
        assert a.dtype == f, a.dtype
    one = f(1)
    b1, b2, eps, wd, gs = (f(hyper[k]) for k in ('beta1', 'beta2', 'eps', 'weight_decay', 'grad_scale'))
    step_size, bc2s, clip_k, decay_mul = (f(state[k]) for k in ('step_size', 'bc2s', 'clip_k', 'decay_mul'))
    with np.errstate(all='ignore'):
        g = g * gs
        if flags & CLIP:
            g = g * clip_k
        p0 = p
        if flags & DECOUPLED:
            p0 = p * decay_mul
        elif wd != 0:
            g = g + wd * p
        m[...] = b1 * m + (one - b1) * g
        v[...] = b2 * v + (one - b2) * (g * g)
        p[...] = p0 - (step_size * m) / (np.sqrt(v) / bc2s + eps)
        if ema is not None:
            d = f(hyper['ema_decay'])
            ema[...] = d * ema + (one - d) * p
    for a in (p, m, v):
        assert a.dtype == f


# Hand-computed steps (every number is a dyadic rational: exact in fp32 and fp64). Step 1 from zero moments with
# beta1 = 0.5, beta2 = 0.75, lr = 0.25, eps = 0, p = 1, ema = 1, d = 0.5:  beta1_pow = 0.5 -> step_size = 0.25 / 0.5 = 0.5;
# beta2_pow = 0.75 -> bc2s = sqrt(0.25) = 0.5;  m' = 0.5 g, v' = 0.25 g^2, sqrt(v') = 0.5 |g|,
# p' = p0 - (0.5 * 0.5 g) / (0.5 |g| / 0.5) = p0 - 0.25 sign(g)    (Adam's first step is lr sign(g))
HAND_HYPER = dict(beta1=0.5, beta2=0.75, eps=0.0, lr=0.25, ema_decay=0.5)
HAND_CASES = [
    # (name, flags, weight_decay, coef, grad, grad_scale) -> expected (g as it enters the moments, m', v', p', ema')
    ('plain', 0, 0.0, None, 2.0, 1.0, dict(m=1.0, v=1.0, p=0.75, ema=0.875)),
    ('grad_scale', 0, 0.0, None, 4.0, 0.5, dict(m=1.0, v=1.0, p=0.75, ema=0.875)),
    # L2: g = 2 + 0.5 * 1 = 2.5, m' = 1.25, v' = 0.25 * 6.25 = 1.5625, sqrt = 1.25, p' = 1 - 0.625 / 2.5
    ('l2', 0, 0.5, None, 2.0, 1.0, dict(m=1.25, v=1.5625, p=0.75, ema=0.875)),
    # decoupled: decay_mul = 1 - 0.25 * 0.5 = 0.875, p0 = 0.875, p' = 0.625, ema' = 0.5 + 0.3125
    ('decoupled', DECOUPLED, 0.5, None, 2.0, 1.0, dict(m=1.0, v=1.0, p=0.625, ema=0.8125, decay_mul=0.875)),
    # clip: k = 0.5, g = 1, m' = 0.5, v' = 0.25
    ('clip', CLIP, 0.0, 0.5, 2.0, 1.0, dict(m=0.5, v=0.25, p=0.75, ema=0.875, clip_k=0.5)),
    ('clip_coef_above_one', CLIP, 0.0, 3.0, 2.0, 1.0, dict(m=1.0, v=1.0, p=0.75, ema=0.875, clip_k=1.0)),
    ('clip_coef_nan', CLIP, 0.0, float('nan'), -2.0, 1.0, dict(m=-1.0, v=1.0, p=1.25, ema=1.125, clip_k=1.0)),
]
