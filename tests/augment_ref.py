"""The numpy specification of twog_augment_inputs (include/twog_gcn.h), operation by operation in float32 arrays: every line
below is one fp32 operation rounded once, as in the kernel (no contraction, correctly rounded division, no transcendentals),
so the GPU tests compare bit for bit. Written from the contract in the header, not from the kernel; the generator is the
Philox4x32-10 of tests/gumbel_noise_ref.py under other keys. The test double (tests/augment_fake.py) is built on it.

`opts` everywhere: the dict augment.InputAugmentation.kernel_options makes (tan_half_max, scale_max, shift_max, cx, cy, amp,
keep_scale, drop_threshold, gcn_node); its floats are fp32 values.

geometry64 / transform64 restate the geometry in float64 for the properties that rounding would blur (c^2 + s^2 = 1, the
velocity relation, the exact quarter turn)."""
import numpy as np

from tests.gumbel_noise_ref import MASK32, philox4x32_10, uniform_of_words

TAG_GEOMETRY, TAG_HUMAN, TAG_OBJECT = 0x47454F4D, 0x48554D4E, 0x4F424A53   # TWOG_AUGMENT_TAG_* of the header
F32 = np.float32


def words(seed, epoch, clip, index, tag):
    """Four uint32 arrays: Philox4x32-10 at counter (epoch low, epoch high, clip, index) under key (seed low, seed high ^ tag).
    seed and epoch are taken modulo 2^64, clip modulo 2^32; clip and index broadcast."""
    seed, epoch = int(seed) % 2 ** 64, int(epoch) % 2 ** 64
    return philox4x32_10((epoch & MASK32, epoch >> 32, np.asarray(clip, dtype=np.uint64) & MASK32, index),
                         (seed & MASK32, (seed >> 32) ^ tag))


def signed_unit(w):
    """r = 2u - 1 of the 23-bit uniform u of a word: exact in fp32 (an odd numerator below 2^23 over 2^23)."""
    u = uniform_of_words(w)
    r = (u + u) - F32(1.0)
    assert r.dtype == np.float32
    return r


def params_of_units(r0, r1, r2, r3, opts):
    """(a, b, tx, ty) float32 from the four signed units of a clip."""
    r0, r1, r2, r3 = (np.asarray(r, dtype=F32) for r in (r0, r1, r2, r3))
    t = F32(opts['tan_half_max']) * r0
    q = t * t
    d = F32(1.0) + q
    c = (F32(1.0) - q) / d
    s = (t + t) / d
    g = F32(1.0) + F32(opts['scale_max']) * r1
    out = np.stack([g * c, g * s, F32(opts['shift_max']) * r2, F32(opts['shift_max']) * r3], axis=-1)
    assert out.dtype == np.float32
    return out


def clip_params(seed, epoch, clip_ids, opts):
    """float32 [bs][4] = (a, b, tx, ty): generator call 0 under the geometry key."""
    w = words(seed, epoch, np.asarray(clip_ids), 0, TAG_GEOMETRY)
    return params_of_units(*(signed_unit(x) for x in w), opts)


def _frames_on(T, steps_b):
    return np.arange(T, dtype=F32) < F32(steps_b) if steps_b is not None else np.ones(T, dtype=bool)


def geometry(x_human, params, opts, steps=None):
    """In place on x_human float32 (bs, T, H, F_h): the nodes of the last 4 * gcn_node channels."""
    N = int(opts['gcn_node'])
    bs, T, H, F_h = x_human.shape
    cx, cy = F32(opts['cx']), F32(opts['cy'])
    for b in range(bs):
        a, bb, tx, ty = (F32(v) for v in params[b])
        nodes = x_human[b, :, :, F_h - 4 * N:].reshape(T, H, N, 4)   # a view: the writes below land in x_human
        assert np.shares_memory(nodes, x_human) or nodes.size == 0
        x, y, vx, vy = (nodes[..., i].copy() for i in range(4))
        on = ((x != 0) | (y != 0)) & _frames_on(T, None if steps is None else steps[b])[:, None, None]
        dx, dy = x - cx, y - cy
        nx = ((a * dx - bb * dy) + cx) + tx
        ny = ((bb * dx + a * dy) + cy) + ty
        nvx = a * vx - bb * vy
        nvy = bb * vx + a * vy
        for i, new in enumerate((nx, ny, nvx, nvy)):
            assert new.dtype == np.float32
            nodes[..., i][on] = new[on]
    return x_human


def feature_words(seed, epoch, clip, e, tag):
    """(dropout word, jitter word) of elements e (uint64 array) of one clip: call e >> 1, words 2 (e & 1) and 2 (e & 1) + 1."""
    e = np.asarray(e, dtype=np.uint64)
    w = words(seed, epoch, clip, e >> np.uint64(1), tag)
    odd = (e & np.uint64(1)).astype(bool)
    return np.where(odd, w[2], w[0]), np.where(odd, w[3], w[1])


def features_block(x, seed, epoch, clip, tag, width, opts, steps_b=None, present=None):
    """In place on one clip's block x float32 (T, E, F): channels < width of the frames t < steps_b and the entities with
    present > 0. Element numbers run over the whole block."""
    T, E, F = x.shape
    on = np.zeros((T, E, F), dtype=bool)
    on[:, :, :width] = True
    on &= _frames_on(T, steps_b)[:, None, None]
    if present is not None:
        on &= (np.asarray(present) > 0)[None, :, None]
    e = np.arange(T * E * F, dtype=np.uint64).reshape(T, E, F)[on]
    w_drop, w_jitter = feature_words(seed, epoch, clip, e, tag)
    keep = (w_drop >> np.uint32(8)) >= np.uint32(opts['drop_threshold'])
    v = (x[on] + F32(opts['amp']) * signed_unit(w_jitter)) * F32(opts['keep_scale'])
    assert v.dtype == np.float32
    x[on] = np.where(keep, v, F32(0.0))
    return x


def geometry_on(opts):
    return opts['tan_half_max'] != 0 or opts['scale_max'] != 0 or opts['shift_max'] != 0


def features_on(opts):
    return opts['amp'] != 0 or opts['drop_threshold'] != 0


def augment(x_human, x_objects, clip_ids, seed, epoch, opts, steps=None, objects_mask=None):
    """The whole entry point, in place on float32 numpy arrays (x_objects may be None). Returns the parameters [bs][4]."""
    assert x_human.dtype == np.float32 and (x_objects is None or x_objects.dtype == np.float32)
    bs, T, H, F_h = x_human.shape
    geo_offset = F_h - 4 * int(opts['gcn_node'])
    assert geo_offset >= 0
    clip_ids = np.asarray(clip_ids)
    params = clip_params(seed, epoch, clip_ids, opts)
    if geometry_on(opts):
        geometry(x_human, params, opts, steps)
    if features_on(opts):
        for b in range(bs):
            sb = None if steps is None else steps[b]
            features_block(x_human[b], seed, epoch, clip_ids[b], TAG_HUMAN, geo_offset, opts, sb)
            if x_objects is not None:
                features_block(x_objects[b], seed, epoch, clip_ids[b], TAG_OBJECT, x_objects.shape[-1], opts, sb,
                               None if objects_mask is None else objects_mask[b])
    return params


# ---------------------------------------------------------------------------------------------------------------- fp64
def geometry64(r0, r1, r2, r3, tan_half_max, scale_max, shift_max):
    """(c, s, a, b, tx, ty) in float64 from the signed units."""
    t = np.float64(tan_half_max) * np.float64(r0)
    q = t * t
    c, s = (1.0 - q) / (1.0 + q), (t + t) / (1.0 + q)
    g = 1.0 + np.float64(scale_max) * np.float64(r1)
    return c, s, g * c, g * s, np.float64(shift_max) * np.float64(r2), np.float64(shift_max) * np.float64(r3)


def transform64(nodes, a, b, tx, ty, cx=0.0, cy=0.0):
    """float64 (..., 4) nodes (x, y, vx, vy) -> transformed copy (no zero-node rule: the caller's track has none)."""
    x, y, vx, vy = (np.asarray(nodes, dtype=np.float64)[..., i] for i in range(4))
    dx, dy = x - cx, y - cy
    return np.stack([((a * dx - b * dy) + cx) + tx, ((b * dx + a * dy) + cy) + ty, a * vx - b * vy, b * vx + a * vy], axis=-1)
