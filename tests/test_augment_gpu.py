"""GPU: twog_augment_inputs against its numpy specification (tests/augment_ref.py), BIT FOR BIT, and through the host layer.

Shapes: the smallest at which each path can go wrong.
  aligned     bs 3, T 5, H 2, N 3, geo_offset 8, O 2, F_o 8: every row starts on 16 bytes, the 16-byte form of the feature pass;
  scalar      the same with geo_offset 6 and F_o 7: the scalar form; element pairs straddle rows and entities (odd row lengths);
  shifted     the aligned shape on buffers that start 4 bytes off a 16-byte boundary: the scalar form chosen by the pointer;
  no_objects  O = 0, x_objects None;   one_human  H = 1;   zero_clip  a clip whose nodes are all zero;
  two_trips   3 * 343 * (1 + 1) = 2 058 rows on a grid capped at 2 048 workgroups (twog_augment_grid): the feature pass's second
              trip, in both forms; geometry_trips: 2 048 * 256 + 5 nodes, the geometry pass's second trip.
Every case runs with steps of T, 1 and 0, ids at the top of the 32-bit range, an epoch above 2^32 and a negative seed, inside
guard bands, with the per-clip parameters read back through the test hook."""
import ctypes as C
from functools import partial

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

import twog_gcn_amd  # noqa: F401
from twog_gcn_amd import _lib as L
from twog_gcn_amd import kernels as twog_kernels
from twog_gcn_amd.augment import InputAugmentation
from twog_gcn_amd.data_loading import DevicePrefetcher, gcn_fetcher
from tests import augment_ref as R
from tests.augment_cases import OPTION_SETS, bits, kernel_options, make_batch, same_bits, tensor_dataset
from tests.helpers import g4_inputs, load_g4
from tests.input_grad_cases import build_model, g4_loss

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SEED, EPOCH = -12345, 2 ** 32 + 3
GUARD, GUARD_VALUE = 64, 777.0          # 64 floats = 256 bytes: the guarded view keeps the allocation's alignment
ALL = OPTION_SETS['all']

ALIGNED = dict(bs=3, T=5, H=2, N=3, geo_offset=8, O=2, F_o=8)
SHAPES = {'aligned': ALIGNED, 'scalar': dict(ALIGNED, geo_offset=6, F_o=7), 'shifted': ALIGNED, 'no_objects': dict(ALIGNED, O=0),
          'one_human': dict(ALIGNED, H=1), 'zero_clip': ALIGNED,
          'two_trips': dict(bs=3, T=343, H=1, N=1, geo_offset=4, O=1, F_o=4),
          'two_trips_scalar': dict(bs=3, T=343, H=1, N=1, geo_offset=3, O=1, F_o=5)}


@pytest.fixture(autouse=True)
def hip_backend():
    twog_kernels._set_backend_for_tests(None)
    assert twog_kernels.get_kernels().name == 'hip'
    yield


def _batch(case):
    s = SHAPES[case]
    xh, xo, mask, steps = make_batch(**s, seed=len(case), steps=[s['T'], 1, 0])
    if case == 'zero_clip':
        xh[0, :, :, s['geo_offset']:] = 0.0
    return xh, xo, mask, steps


def _ids(bs):
    return np.array([2 ** 32 - 1, 2 ** 32 - 2, 5, 2 ** 31, 0, 77][:bs], dtype=np.int64)


def _guarded(a, shift=0):
    buf = torch.full((GUARD + shift + a.size + GUARD,), GUARD_VALUE, device=DEV)
    view = buf[GUARD + shift:GUARD + shift + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 4 * (shift % 4)
    return buf, view


def _guards_intact(buf, view):
    lo = (view.data_ptr() - buf.data_ptr()) // 4
    return bool((buf[:lo] == GUARD_VALUE).all()) and bool((buf[lo + view.numel():] == GUARD_VALUE).all())


def _run(K, batch, ids, opts, seed=SEED, epoch=EPOCH, shift=0):
    """The kernel on guarded device copies of `batch` -> (x_human, x_objects, params) as numpy."""
    xh, xo, mask, steps = batch
    bh, vh = _guarded(xh, shift)
    bo, vo = _guarded(xo, shift) if xo is not None else (None, None)
    params = torch.full((len(ids), 4), GUARD_VALUE, device=DEV)
    dev = lambda a: None if a is None else torch.from_numpy(a).to(DEV)
    K.augment_inputs(vh, vo, dev(ids), K.new_noise_state(seed, epoch, device=DEV), opts, steps=dev(steps), objects_mask=dev(mask),
                     params_out=params)
    assert _guards_intact(bh, vh) and (bo is None or _guards_intact(bo, vo))
    return vh.cpu().numpy(), None if vo is None else vo.cpu().numpy(), params.cpu().numpy()


def _spec(batch, ids, opts, seed=SEED, epoch=EPOCH):
    xh, xo, mask, steps = (None if a is None else a.copy() for a in batch)
    params = R.augment(xh, xo, ids, seed, epoch, opts, steps, mask)
    return xh, xo, params


def _assert_same(got, want, what=''):
    for k, name in enumerate(('x_human', 'x_objects', 'params')):
        if want[k] is None:
            assert got[k] is None
            continue
        bad = bits(got[k]) != bits(want[k])
        assert not bad.any(), (what, name, int(bad.sum()), np.argwhere(bad)[:4].tolist())


# ---------------------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize('case', list(SHAPES))
def test_all_options_bit_for_bit(case):
    K = twog_kernels.get_kernels()
    s = SHAPES[case]
    batch, ids, opts = _batch(case), _ids(s['bs']), kernel_options(s['N'], **ALL)
    if case.startswith('two_trips'):
        rows = s['bs'] * s['T'] * (s['H'] + s['O'])
        assert K.augment_grid(rows) == 2048 < rows, 'no workgroup of the feature pass makes a second trip'
    got = _run(K, batch, ids, opts, shift=1 if case == 'shifted' else 0)
    want = _spec(batch, ids, opts)
    _assert_same(got, want, case)
    assert not same_bits(got[0], batch[0])
    _assert_same(_run(K, batch, ids, opts, shift=1 if case == 'shifted' else 0), got, case + ': second run')


@pytest.mark.parametrize('shape', ['aligned', 'scalar'])
@pytest.mark.parametrize('name', [n for n in OPTION_SETS if n != 'all'])
def test_each_option_alone_bit_for_bit(name, shape):
    K = twog_kernels.get_kernels()
    s = SHAPES[shape]
    batch, ids, opts = _batch(shape), _ids(s['bs']), kernel_options(s['N'], **OPTION_SETS[name])
    got, want = _run(K, batch, ids, opts), _spec(batch, ids, opts)
    _assert_same(got, want, name)
    assert not same_bits(got[0], batch[0])
    geometry = R.geometry_on(opts)
    go = s['geo_offset']
    assert same_bits(got[0][..., :go], batch[0][..., :go]) == geometry         # each part leaves the other's channels alone
    assert same_bits(got[0][..., go:], batch[0][..., go:]) == (not geometry)


def test_geometry_pass_second_trip():
    K = twog_kernels.get_kernels()
    N = 2048 * 256 + 5
    assert K.augment_grid((N + 255) // 256) == 2048 < (N + 255) // 256
    batch = make_batch(1, 1, 1, N, 0, 0, 0, seed=3)
    opts = kernel_options(N, **ALL)
    _assert_same(_run(K, batch, _ids(1), opts), _spec(batch, _ids(1), opts))


def test_grid_plan():
    K = twog_kernels.get_kernels()
    assert [K.augment_grid(w) for w in (0, 1, 2047, 2048, 2049, 2 ** 40)] == [1, 1, 2047, 2048, 2048, 2048]
    assert K.lib.twog_augment_grid(-1) == -2


def test_neutral_options_launch_nothing_and_keep_the_bits():
    K = twog_kernels.get_kernels()
    batch = _batch('aligned')
    got = _run(K, batch, _ids(3), kernel_options(3))
    assert same_bits(got[0], batch[0]) and same_bits(got[1], batch[1])
    assert np.array_equal(got[2], np.tile(np.float32([1, 0, 0, 0]), (3, 1)))  # the hook alone: the identity


def test_draw_depends_on_seed_epoch_and_id_only():
    K = twog_kernels.get_kernels()
    s = dict(ALIGNED, bs=6)
    batch = make_batch(**s, seed=9, steps=[5, 4, 3, 5, 1, 2])
    ids, opts = _ids(6), kernel_options(3, **ALL)
    full = _run(K, batch, ids, opts)
    for sl in (slice(0, 2), slice(2, 3), slice(3, 6)):
        part = _run(K, tuple(a[sl].copy() for a in batch), ids[sl], opts)
        _assert_same(part, tuple(a[sl] for a in full), str(sl))
    for seed, epoch in ((SEED + 1, EPOCH), (SEED, EPOCH + 1), (SEED, EPOCH - 2 ** 32), (SEED + 2 ** 32, EPOCH)):
        other = _run(K, batch, ids, opts, seed=seed, epoch=epoch)
        _assert_same(other, _spec(batch, ids, opts, seed=seed, epoch=epoch), (seed, epoch))
        assert not same_bits(other[0][0], full[0][0]) and not same_bits(other[2], full[2])


def test_rejected_arguments():
    K = twog_kernels.get_kernels()
    lib, s = K.lib, ALIGNED
    batch = _batch('aligned')
    xh, xo = torch.from_numpy(batch[0]).to(DEV), torch.from_numpy(batch[1]).to(DEV)
    ids, state = torch.from_numpy(_ids(3)).to(DEV), K.new_noise_state(1, 0, device=DEV)
    opts = kernel_options(3, **ALL)

    def call(**over):
        a = L.Augment()
        a.x_human, a.x_objects, a.clip_ids, a.state = xh.data_ptr(), xo.data_ptr(), ids.data_ptr(), state.data_ptr()
        a.bs, a.T, a.H, a.O, a.F_h, a.F_o, a.N, a.geo_offset = 3, 5, 2, 2, 20, 8, 3, 8
        for k in ('tan_half_max', 'scale_max', 'shift_max', 'cx', 'cy', 'amp', 'keep_scale', 'drop_threshold'):
            setattr(a, k, opts[k])
        for k, v in over.items():
            setattr(a, k, v)
        return lib.twog_augment_inputs(C.byref(a), K._stream())

    assert lib.twog_augment_inputs(None, K._stream()) == -1
    assert call(N=-1, geo_offset=24) == -1                                     # N < 0
    assert call(geo_offset=-4, N=6) == -1                                      # geo_offset < 0
    assert call(geo_offset=4) == -1 and call(N=4) == -1                        # impossible: geo_offset + 4 N != F_h
    assert call(T=-1) == -1 and call(bs=-3) == -1 and call(O=-1) == -1
    assert call(drop_threshold=2 ** 24) == -1
    assert call(x_human=xh.data_ptr() + 2) == -1 and call(x_objects=xo.data_ptr() + 1) == -1       # misaligned pointers
    assert call(clip_ids=ids.data_ptr() + 4) == -1 and call(state=state.data_ptr() + 4) == -1
    assert call(clip_ids=None) == -1 and call(state=None) == -1 and call(x_human=None) == -1
    # a clip's row block beyond 2^33 elements: e >> 1 no longer fits the counter word (2^33 itself is the last that does)
    assert call(T=2 ** 20, H=2 ** 4, F_h=2 ** 10, N=0, geo_offset=2 ** 10) == -2
    assert call(T=2 ** 20, O=2 ** 4, F_o=2 ** 10) == -2
    assert call(bs=0, T=2 ** 20, H=2 ** 3, F_h=2 ** 10 + 1, N=0, geo_offset=2 ** 10 + 1) == -2
    assert call(bs=0, T=2 ** 20, H=2 ** 3, F_h=2 ** 10, N=0, geo_offset=2 ** 10) == 0              # (no clip: nothing launched)
    with pytest.raises(RuntimeError, match='twog_augment_inputs failed with code -1'):
        K.augment_inputs(xh, xo, ids, state, dict(opts, gcn_node=6))
    with pytest.raises(ValueError, match='contiguous'):
        K.augment_inputs(xh[..., :16], xo, ids, state, dict(opts, gcn_node=2))
    torch.cuda.synchronize()
    assert same_bits(xh.cpu().numpy(), batch[0]) and same_bits(xo.cpu().numpy(), batch[1])      # a rejected call writes nothing
    assert call() == 0


# ---------------------------------------------------------------------------------------------------------------- host layer
FETCH = partial(gcn_fetcher, dataset_name='mphoi')


def _prefetcher(*args, **kw):
    """A DevicePrefetcher as shipped -- copies on a side stream, the augmentation on the consumer's -- whose side stream is the
    library's CU-masked one (kernels.side_stream: a hardware queue of its own, cached for the process) instead of one more of
    torch's pool streams. Pool streams are never given back, and they share the process's few hardware queues: with the
    prefetchers of this file on pool streams, the side stream that a later test of the suite takes from the pool
    (tests/test_kernels_gpu.py: a persistent launch beside a tenant that holds compute units) no longer got its tenant to
    run beside the launch on the caller's stream -- no persistent launch gave up, so that test failed in the whole suite,
    while it passes alone, right behind this file, and in the suite with the prefetcher tests of this file left out."""
    K = twog_kernels.get_kernels()
    side = K.side_stream(torch.device(DEV), 80)
    if side is None:                                  # (the runtime refused the mask: the pool stream after all)
        return DevicePrefetcher(*args, **kw)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(torch.cuda, 'Stream', lambda *a, **k: side.stream)
        pre = DevicePrefetcher(*args, **kw)
    assert pre.copy_stream is side.stream and pre.copy_stream != torch.cuda.current_stream()
    return pre


@pytest.mark.parametrize('resident', [True, False], ids=['resident', 'staged'])
def test_prefetcher_against_the_specification(resident):
    tensors = tensor_dataset()
    loader = lambda: DataLoader(TensorDataset(*tensors), batch_size=3, shuffle=True, generator=torch.Generator().manual_seed(4))
    aug = InputAugmentation(21, gcn_node=3, epoch=4, **ALL)
    plain = _prefetcher(loader(), FETCH, DEV, resident=resident)
    pre = _prefetcher(loader(), FETCH, DEV, resident=resident, augment=aug)
    for epoch in (4, 5):
        raw, got = list(plain), list(pre)
        assert len(raw) == len(got) == 3 and aug.epoch == epoch + 1
        assert aug.state(DEV).tolist() == [21, epoch + 1]
        seen = []
        for (d0, t0), (d1, t1) in zip(raw, got):
            ids = t0[0].cpu().numpy()
            seen += ids.tolist()
            assert torch.equal(t0[0], t1[0])
            cpu = lambda k: d0[k].cpu().numpy()
            xh, xo = cpu(0), cpu(1)
            R.augment(xh, xo, ids, 21, epoch, aug.kernel_options, cpu(7), cpu(2))
            assert same_bits(d1[0].cpu().numpy(), xh) and same_bits(d1[1].cpu().numpy(), xo)
            assert not same_bits(xh, cpu(0))
        assert sorted(seen) == list(range(7))


def test_call_and_epoch_writes_synchronise_nothing():
    batch = _batch('aligned')
    data = [None if a is None else torch.from_numpy(a).to(DEV) for a in (batch[0], batch[1], batch[2], None, None, None, None,
                                                                          batch[3])]
    ids = torch.from_numpy(_ids(3)).to(DEV)
    aug = InputAugmentation(SEED, gcn_node=3, epoch=EPOCH, **ALL)
    aug(data, ids)                                   # (the device words and the code object exist from here on)
    aug.set_epoch(EPOCH)
    data[0].copy_(torch.from_numpy(batch[0]).to(DEV))
    data[1].copy_(torch.from_numpy(batch[1]).to(DEV))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        aug(data, ids)
        aug.next_epoch()
        aug.set_epoch(EPOCH + 7)
        aug.next_epoch()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert aug.state(DEV).tolist() == [SEED, EPOCH + 8] and aug.epoch == EPOCH + 8
    assert aug.state('cuda') is aug.state(DEV) is aug.state(data[0].device)    # one tensor, however the device is spelt
    want = _spec(batch, _ids(3), aug.kernel_options)
    assert same_bits(data[0].cpu().numpy(), want[0]) and same_bits(data[1].cpu().numpy(), want[1])


def test_model_step_on_the_augmented_batch_equals_the_specifications():
    """One training step of a small model fed the prefetcher's augmented batch against the same model fed the specification's
    output: the same loss and gradients, bit for bit."""
    name = 'c2_stage1'
    z, meta = load_g4(name)
    kw = g4_inputs(z)
    bs, T, H = kw['x_human'].shape[:3]
    O = kw['x_objects'].shape[2]
    extra = {k: v.to(DEV) for k, v in kw.items() if k not in ('x_human', 'x_objects', 'objects_mask', 'steps_per_example')}
    noise = torch.from_numpy(z['gumbel_noise'])
    aug = InputAugmentation(31, gcn_node=meta['N'], epoch=2, **ALL)
    tensors = [kw['x_human'], kw['x_objects'], kw['objects_mask'], torch.ones(bs, T, H), torch.zeros(bs, T, H, H),
               torch.zeros(bs, T, H, O), torch.zeros(bs, T, O, O), kw['steps_per_example'], torch.arange(bs)]
    pre = _prefetcher(DataLoader(TensorDataset(*tensors), batch_size=bs), FETCH, DEV, resident=True, augment=aug)
    (data, targets), = list(pre)
    xh, xo = kw['x_human'].numpy().copy(), kw['x_objects'].numpy().copy()
    R.augment(xh, xo, np.arange(bs), 31, 2, aug.kernel_options, kw['steps_per_example'].numpy(), kw['objects_mask'].numpy())
    assert not same_bits(xh, kw['x_human'].numpy())

    def step(x_human, x_objects):
        m = build_model(meta, DEV).train()
        m._gumbel_noise_override = noise.to(DEV) if len(noise) else None
        out = m(x_human=x_human, x_objects=x_objects, objects_mask=data[2], steps_per_example=data[7], **extra)
        loss = g4_loss(name, meta, out)
        loss.backward()
        return loss.detach(), {n: p.grad for n, p in m.named_parameters()}

    loss_a, grads_a = step(data[0], data[1])
    loss_b, grads_b = step(torch.from_numpy(xh).to(DEV), torch.from_numpy(xo).to(DEV))
    assert torch.equal(loss_a, loss_b) and bool(torch.isfinite(loss_a))
    assert grads_a.keys() == grads_b.keys() and any(g is not None for g in grads_a.values())
    for n, g in grads_a.items():
        assert (g is None) == (grads_b[n] is None), n
        if g is not None:
            assert torch.equal(g, grads_b[n]), n
