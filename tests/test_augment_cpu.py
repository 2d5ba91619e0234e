"""Input augmentation without a GPU: the numpy specification of twog_augment_inputs (tests/augment_ref.py) -- its geometry in
fp64, what it must leave alone, shard invariance, where seed / epoch / clip id / element land in the generator's counter and
key, the dropout and jitter statistics -- and the host layer (augment.InputAugmentation, data_loading.DevicePrefetcher) on the
test double (tests/augment_fake.py)."""
import math
import os
import re
from functools import partial

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, Dataset, TensorDataset

import twog_gcn_amd  # noqa: F401
from twog_gcn_amd import _lib
from twog_gcn_amd import kernels as twog_kernels
from twog_gcn_amd.augment import InputAugmentation
from twog_gcn_amd.data_loading import DevicePrefetcher, _trim_collate, gcn_fetcher
from tests import augment_ref as R
from tests.augment_cases import FEATURES, GEOMETRY, OPTION_SETS, bits, kernel_options, make_batch, same_bits, tensor_dataset
from tests.augment_fake import AugmentFakeKernels
from tests.gumbel_noise_ref import philox4x32_10
from tests.helpers import ROOT

SHAPE = dict(bs=3, T=5, H=2, N=3, geo_offset=6, O=2, F_o=7)
ALL = OPTION_SETS['all']


@pytest.fixture()
def fake():
    k = AugmentFakeKernels()
    twog_kernels._set_backend_for_tests(k)
    yield k
    twog_kernels._set_backend_for_tests(None)


def _data(xh, xo, mask, steps):
    t = lambda a: None if a is None else torch.from_numpy(a.copy())
    return [t(xh), t(xo), t(mask), None, None, None, None, t(steps)]


def _spec(batch, ids, seed, epoch, opts):
    xh, xo, mask, steps = (None if a is None else a.copy() for a in batch)
    R.augment(xh, xo, ids, seed, epoch, opts, steps, mask)
    return xh, xo


# ---------------------------------------------------------------------------------------------------------------- neutral
def test_neutral_options_return_the_inputs_bits_and_launch_nothing(fake):
    batch = make_batch(**SHAPE, steps=[5, 3, 0])
    data = _data(*batch)
    aug = InputAugmentation(3, gcn_node=SHAPE['N'])
    out = aug(data, torch.arange(3))
    assert out is data and fake.augment_calls == []
    assert same_bits(data[0].numpy(), batch[0]) and same_bits(data[1].numpy(), batch[1])
    InputAugmentation(3, gcn_node=SHAPE['N'], **ALL)(data, torch.arange(3))
    assert fake.augment_calls == [(3, ('geometry', 'features'))]
    assert not same_bits(data[0].numpy(), batch[0])


# ---------------------------------------------------------------------------------------------------------------- fp64
def test_fp64_rotation_is_a_rotation():
    r = np.linspace(-1, 1, 2001)
    for deg in (1., 30., 90.):
        c, s, a, b, _, _ = R.geometry64(r, 0.37, 0., 0., math.tan(math.radians(deg) / 2), 0.2, 0.)
        assert np.abs(c * c + s * s - 1).max() <= 1e-12
        assert np.abs(a * a + b * b - (1 + 0.2 * 0.37) ** 2).max() <= 1e-12
        assert np.abs(np.degrees(np.arctan2(s, c))).max() <= deg + 1e-9       # never beyond the option


def test_fp64_velocities_stay_the_difference_of_positions():
    g = np.random.default_rng(1)
    pos = np.cumsum(g.normal(0, 0.01, (40, 6, 2)), axis=0) + 0.5
    vel = np.zeros_like(pos)
    vel[:-1] = (pos[1:] - pos[:-1]) * 100                                      # data_loading._pos_vel
    _, _, a, b, tx, ty = R.geometry64(0.8, -0.6, 0.3, -0.9, math.tan(math.radians(40.) / 2), 0.25, 0.2)
    out = R.transform64(np.concatenate([pos, vel], -1), a, b, tx, ty, cx=0.5, cy=0.4)
    assert np.abs(out[:-1, :, 2:] - (out[1:, :, :2] - out[:-1, :, :2]) * 100).max() <= 1e-12
    assert np.abs(out[-1, :, 2:]).max() == 0


@pytest.mark.parametrize('r0,want', [(1.0, (0., 1.)), (-1.0, (0., -1.))])
def test_quarter_turn_is_exact(r0, want):
    """max_rotation_deg = 90 with r0 = +-1: t = +-1, q = 1, c = 0 / 2 = 0, s = +-2 / 2 = +-1 -- the point (1, 0) about the
    origin lands on (0, +-1) and its velocity (0, 1) on (-+1, 0), in fp64 and in the fp32 specification alike."""
    assert abs(math.tan(math.radians(90.) / 2) - 1) <= 2.0 ** -52               # (libm's tan(pi / 4) is one ulp short of 1)
    c, s, a, b, tx, ty = R.geometry64(r0, 0., 0., 0., 1.0, 0., 0.)
    assert (c, s, a, b, tx, ty) == (0., r0, 0., r0, 0., 0.)
    assert R.transform64([1., 0., 0., 1.], a, b, tx, ty).tolist() == [0., want[1], -want[1], 0.]
    opts = kernel_options(1, max_rotation_deg=90.)
    assert opts['tan_half_max'] == 1.0                                         # tan(pi / 4) rounds to 1 in fp32
    assert R.params_of_units(r0, 0., 0., 0., opts).tolist() == [0., r0, 0., 0.]


# ---------------------------------------------------------------------------------------------------------------- untouched
def test_what_must_be_left_alone_keeps_its_bits():
    N, go = SHAPE['N'], SHAPE['geo_offset']
    batch = make_batch(**SHAPE, steps=[5, 3, 0])
    xh0, xo0, mask, steps = batch
    xh, xo = _spec(batch, [4, 5, 6], 11, 2, kernel_options(N, **ALL))
    nodes0, nodes = xh0[..., go:].reshape(3, 5, 2, N, 4), xh[..., go:].reshape(3, 5, 2, N, 4)
    assert same_bits(nodes[:, :, :, 1], nodes0[:, :, :, 1]) and not nodes0[0, :, :, 1].any()      # zero nodes
    for b, s in enumerate([5, 3, 0]):                                                              # frames at and beyond steps
        assert same_bits(xh[b, s:], xh0[b, s:]) and same_bits(xo[b, s:], xo0[b, s:])
        if s:
            assert not np.array_equal(bits(xh[b, :s, :, :go]), bits(xh0[b, :s, :, :go]))
            assert not np.array_equal(bits(nodes[b, :s, :, 0]), bits(nodes0[b, :s, :, 0]))
    assert same_bits(xo[0, :, 1], xo0[0, :, 1]) and not np.array_equal(bits(xo[0, :, 0]), bits(xo0[0, :, 0]))   # masked object
    assert np.array_equal(xh[:, :, 0, go:][:, :3], xh[:, :, 1, go:][:, :3], equal_nan=True)        # one transform for all H rows
    # the feature pass alone leaves the geometry tail alone, the geometry alone the feature channels
    xh, xo = _spec(batch, [4, 5, 6], 11, 2, kernel_options(N, **FEATURES))
    assert same_bits(xh[..., go:], xh0[..., go:]) and not same_bits(xh[..., :go], xh0[..., :go])
    xh, xo = _spec(batch, [4, 5, 6], 11, 2, kernel_options(N, **GEOMETRY))
    assert same_bits(xh[..., :go], xh0[..., :go]) and same_bits(xo, xo0) and not same_bits(xh[..., go:], xh0[..., go:])


# ---------------------------------------------------------------------------------------------------------------- invariance
def test_shard_invariance_and_permutation():
    shape = dict(SHAPE, bs=6)
    batch = make_batch(**shape, steps=[5, 4, 3, 5, 1, 2])
    opts, ids = kernel_options(SHAPE['N'], **ALL), np.array([10, 3, 2 ** 32 - 1, 7, 0, 99])
    full = _spec(batch, ids, 5, 1, opts)
    for sl in (slice(0, 2), slice(2, 3), slice(3, 6)):
        part = _spec(tuple(a[sl] for a in batch), ids[sl], 5, 1, opts)
        assert same_bits(part[0], full[0][sl]) and same_bits(part[1], full[1][sl])
    perm = np.array([4, 0, 5, 2, 1, 3])
    moved = _spec(tuple(a[perm] for a in batch), ids[perm], 5, 1, opts)
    assert same_bits(moved[0], full[0][perm]) and same_bits(moved[1], full[1][perm])


def test_seed_epoch_and_id_each_decide_the_draw():
    batch = make_batch(**SHAPE)
    opts = kernel_options(SHAPE['N'], **ALL)
    base = _spec(batch, [1, 2, 3], 5, 1, opts)
    again = _spec(batch, [1, 2, 3], 5, 1, opts)
    assert same_bits(base[0], again[0]) and same_bits(base[1], again[1])
    for ids, seed, epoch in (([1, 2, 4], 5, 1), ([1, 2, 3], 6, 1), ([1, 2, 3], 5, 2), ([1, 2, 3], 5 + 2 ** 32, 1),
                             ([1, 2, 3], 5, 1 + 2 ** 32)):
        other = _spec(batch, ids, seed, epoch, opts)
        changed = [not same_bits(other[k][b], base[k][b]) for k in (0, 1) for b in range(3)]
        assert changed == ([i != j for i, j in zip(ids, [1, 2, 3])] * 2 if (seed, epoch) == (5, 1) else [True] * 6)
    assert same_bits(_spec(batch, [1, 2, 3], 5 - 2 ** 64, 1, opts)[0], base[0])                    # modulo 2^64


def test_large_ids_epochs_and_elements_reach_their_counter_words():
    seed, epoch, clip = 0x89abcdef01234567, 2 ** 32 + 2 ** 31 + 9, 2 ** 32 - 2
    key = lambda tag: (seed & 0xffffffff, (seed >> 32) ^ tag)
    ctr = lambda index: (epoch & 0xffffffff, epoch >> 32, clip, index)
    assert ctr(0)[:3] == (2 ** 31 + 9, 1, 2 ** 32 - 2)
    opts = kernel_options(1, **GEOMETRY)
    want = R.params_of_units(*(R.signed_unit(w) for w in philox4x32_10(ctr(0), key(R.TAG_GEOMETRY))), opts)
    assert same_bits(R.clip_params(seed, epoch, [clip], opts)[0], want)
    assert same_bits(R.clip_params(seed - 2 ** 64, epoch, np.array([clip], dtype=np.int64), opts)[0], want)
    for tag in (R.TAG_HUMAN, R.TAG_OBJECT):
        for e in (0, 1, 2, 2 ** 32 + 5, 2 ** 33 - 1):                          # the last element a clip's block may hold
            w = philox4x32_10(ctr(e >> 1), key(tag))
            got = R.feature_words(seed, epoch, clip, [e], tag)
            assert (int(got[0][0]), int(got[1][0])) == (int(w[2 * (e & 1)]), int(w[2 * (e & 1) + 1])), (tag, e)
    assert len({R.TAG_GEOMETRY, R.TAG_HUMAN, R.TAG_OBJECT, 0}) == 4            # apart from each other and from the Gumbel key
    header = open(os.path.join(ROOT, 'include', 'twog_gcn.h')).read()
    stated = {n: int(v, 16) for n, v in re.findall(r'#define TWOG_AUGMENT_TAG_(\w+)\s+0x([0-9A-Fa-f]+)u', header)}
    assert stated == dict(GEOMETRY=R.TAG_GEOMETRY, HUMAN=R.TAG_HUMAN, OBJECT=R.TAG_OBJECT)
    assert (_lib.AUGMENT_TAG_GEOMETRY, _lib.AUGMENT_TAG_HUMAN, _lib.AUGMENT_TAG_OBJECT) == (R.TAG_GEOMETRY, R.TAG_HUMAN, R.TAG_OBJECT)


# ---------------------------------------------------------------------------------------------------------------- statistics
N_STAT = 2 ** 20


def test_dropout_keeps_the_fraction_it_names():
    p = 0.3
    x = np.ones((1, 1, N_STAT), dtype=np.float32)
    opts = kernel_options(0, feature_dropout=p)
    assert opts['drop_threshold'] == round(p * 2 ** 24) and opts['amp'] == 0
    R.features_block(x, 2024, 0, 17, R.TAG_OBJECT, N_STAT, opts)
    kept = x != 0
    assert np.array_equal(np.unique(x), np.array([0, opts['keep_scale']], dtype=np.float32))
    frac = kept.mean()
    print(f'kept fraction {frac:.6f}, expected {1 - p}, bound {5 * math.sqrt(p * (1 - p) / N_STAT):.6f}')
    assert abs(frac - (1 - p)) <= 5 * math.sqrt(p * (1 - p) / N_STAT)


def test_jitter_is_centred_bounded_and_of_the_named_variance():
    std = 0.25
    x0 = np.random.default_rng(2).standard_normal((1, 1, N_STAT)).astype(np.float32)
    x = x0.copy()
    opts = kernel_options(0, feature_noise_std=std)
    assert opts['drop_threshold'] == 0 and opts['keep_scale'] == 1 and opts['amp'] == np.float32(std * math.sqrt(3))
    R.features_block(x, 2024, 0, 17, R.TAG_HUMAN, N_STAT, opts)
    d = x.astype(np.float64) - x0
    print(f'jitter mean {d.mean():.3e} (bound {5 * std / math.sqrt(N_STAT):.3e}), std {d.std():.5f}, max {np.abs(d).max():.5f}')
    assert abs(d.mean()) <= 5 * std / math.sqrt(N_STAT)
    assert np.abs(d).max() <= opts['amp']
    assert abs(d.std() - std) <= 0.01 * std


# ---------------------------------------------------------------------------------------------------------------- host layer
def test_option_ranges_are_validated():
    for bad in (dict(max_rotation_deg=-1.), dict(max_rotation_deg=90.5), dict(max_scale=1.), dict(max_scale=-0.1),
                dict(feature_dropout=1.), dict(feature_dropout=-0.1), dict(feature_noise_std=-1.), dict(max_shift=float('nan'))):
        with pytest.raises(ValueError):
            InputAugmentation(0, gcn_node=3, **bad)
    k = InputAugmentation(0, gcn_node=3, max_rotation_deg=60., feature_noise_std=2., feature_dropout=0.5).kernel_options
    assert k['tan_half_max'] == np.float32(math.tan(math.radians(60.) / 2)) and k['amp'] == np.float32(2 * math.sqrt(3))
    assert k['keep_scale'] == 2.0 and k['drop_threshold'] == 2 ** 23


def test_state_dict_round_trip_continues_the_sequence(fake):
    batch = make_batch(**SHAPE)
    a = InputAugmentation(-7, gcn_node=SHAPE['N'], epoch=2 ** 32 + 1, **ALL)
    ids = torch.tensor([2, 0, 1])
    a(_data(*batch), ids)                       # (the device words exist from here on)
    a.next_epoch()
    sd = a.state_dict()
    assert sd['seed'] == 2 ** 64 - 7 and sd['epoch'] == 2 ** 32 + 2 and sd['centre'] == (0.5, 0.4)
    b = InputAugmentation(0, gcn_node=1).load_state_dict(sd)
    assert b.state_dict() == sd and b.kernel_options == a.kernel_options
    da, db = a(_data(*batch), ids), b(_data(*batch), ids)
    want = _spec(batch, ids.numpy(), -7, 2 ** 32 + 2, a.kernel_options)
    for k in (0, 1):
        assert same_bits(da[k].numpy(), want[k]) and same_bits(db[k].numpy(), want[k])
    a.set_epoch(5)
    assert a.state('cpu').tolist() == [-7, 5] and a.state_dict()['epoch'] == 5
    words = a.state('cpu')                      # loading writes into the words a captured launch would go on reading
    assert a.load_state_dict(dict(sd, seed=9, epoch=12)).state(torch.device('cpu')) is words and words.tolist() == [9, 12]


def test_non_contiguous_inputs_raise(fake):
    batch = make_batch(**SHAPE)
    data = _data(*batch)
    data[0] = data[0][..., :-1]
    with pytest.raises(ValueError, match='contiguous'):
        InputAugmentation(1, gcn_node=SHAPE['N'], **ALL)(data, torch.arange(3))
    assert same_bits(data[0].numpy(), batch[0][..., :-1])


# ---------------------------------------------------------------------------------------------------------------- prefetcher
def _loader(tensors, **kw):
    return DataLoader(TensorDataset(*tensors), batch_size=3, **kw)


FETCH = partial(gcn_fetcher, dataset_name='mphoi')


@pytest.mark.parametrize('resident', [True, False], ids=['resident', 'staged'])
@pytest.mark.parametrize('shuffle', [False, True], ids=['sequential', 'shuffled'])
def test_prefetcher_augments_every_batch_by_its_dataset_indices(fake, resident, shuffle):
    tensors = tensor_dataset()
    gen = lambda: dict(shuffle=True, generator=torch.Generator().manual_seed(4)) if shuffle else {}
    aug = InputAugmentation(21, gcn_node=3, epoch=4, **ALL)
    plain = DevicePrefetcher(_loader(tensors, **gen()), FETCH, 'cpu', resident=resident)
    pre = DevicePrefetcher(_loader(tensors, **gen()), FETCH, 'cpu', resident=resident, augment=aug)
    for epoch in (4, 5):
        raw, got = list(plain), list(pre)
        assert len(raw) == len(got) == 3 and aug.epoch == epoch + 1             # the epoch moves once per pass, behind it
        seen = []
        for (d0, t0), (d1, t1) in zip(raw, got):
            ids = t0[0].numpy()
            seen += ids.tolist()
            assert torch.equal(t0[0], t1[0])
            want = _spec((d0[0].numpy(), d0[1].numpy(), d0[2].numpy(), d0[7].numpy()), ids, 21, epoch, aug.kernel_options)
            assert same_bits(d1[0].numpy(), want[0]) and same_bits(d1[1].numpy(), want[1])
            assert not same_bits(d1[0].numpy(), d0[0].numpy())
            for k in range(2, 8):
                assert torch.equal(d0[k], d1[k])
        assert sorted(seen) == list(range(7)) and (seen != list(range(7))) == shuffle
    assert len(fake.augment_calls) == 6
    assert torch.equal(TensorDataset(*tensors).tensors[0], tensor_dataset()[0])  # the data set itself is never written


@pytest.mark.parametrize('resident', [True, False], ids=['resident', 'staged'])
def test_prefetcher_without_an_augmenter_is_what_it_was(fake, resident):
    tensors = tensor_dataset()
    a = list(DevicePrefetcher(_loader(tensors), FETCH, 'cpu', resident=resident))
    b = list(DevicePrefetcher(_loader(tensors), FETCH, 'cpu', resident=resident, augment=None))
    assert len(a) == len(b) == 3 and fake.augment_calls == []
    for (d0, t0), (d1, t1) in zip(a, b):
        assert len(d0) == len(d1) == 8 and len(t0) == len(t1) == 1
        for x, y in zip(d0 + t0, d1 + t1):
            assert x.dtype == y.dtype and torch.equal(x, y)
        assert same_bits(d0[0].numpy(), d1[0].numpy())


def test_prefetcher_refuses_an_augmenter_where_the_indices_are_unknown():
    class Rows(Dataset):
        def __init__(self, tensors):
            self.t = tensors

        def __len__(self):
            return len(self.t[0])

        def __getitem__(self, i):
            return tuple(t[i] for t in self.t)

    tensors = tensor_dataset()
    aug = InputAugmentation(1, gcn_node=3, **ALL)
    with pytest.raises(TypeError, match='indices'):
        DevicePrefetcher(DataLoader(Rows(tensors), batch_size=3), FETCH, 'cpu', augment=aug)
    with pytest.raises(TypeError, match='indices'):
        DevicePrefetcher(DataLoader(TensorDataset(*tensors), batch_size=3, collate_fn=_trim_collate), FETCH, 'cpu', augment=aug)
    with pytest.raises(TypeError):
        DevicePrefetcher(DataLoader(Rows(tensors), batch_size=3), FETCH, 'cpu', resident=True, augment=aug)
    DevicePrefetcher(DataLoader(Rows(tensors), batch_size=3), FETCH, 'cpu')     # (and is fine without one)
