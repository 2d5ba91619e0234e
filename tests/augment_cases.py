"""Shared by tests/test_augment_cpu.py and tests/test_augment_gpu.py: seeded batches in the loader's layout, the option sets
and a small TensorDataset in the slot order data_loading.gcn_fetcher reads."""
import numpy as np
import torch

from twog_gcn_amd.augment import InputAugmentation

GEOMETRY = dict(max_rotation_deg=30., max_scale=0.2, max_shift=0.1, centre=(0.5, 0.4))
FEATURES = dict(feature_noise_std=0.25, feature_dropout=0.3)
OPTION_SETS = {'rotation': dict(max_rotation_deg=30.), 'scale': dict(max_scale=0.2), 'shift': dict(max_shift=0.1),
               'rotation_about_centre': dict(max_rotation_deg=90., centre=(0.5, 0.4)), 'noise': dict(feature_noise_std=0.25),
               'dropout': dict(feature_dropout=0.3), 'all': dict(GEOMETRY, **FEATURES)}


def kernel_options(gcn_node, **options):
    return InputAugmentation(0, gcn_node=gcn_node, **options).kernel_options


def make_batch(bs, T, H, N, geo_offset, O, F_o, seed=0, steps=None):
    """x_human (bs, T, H, geo_offset + 4 N), x_objects (bs, T, O, F_o) or None, objects_mask (bs, O) or None, steps (bs,): float32
    numpy. Every H row of a frame carries the same node block, as the loaders write it; node 1 of every clip is a missing
    object (zeros), object O - 1 of clip 0 is masked out, and frames at and beyond steps[b] hold NaN (their bits must survive)."""
    g = np.random.default_rng(seed)
    x_human = g.standard_normal((bs, T, H, geo_offset + 4 * N)).astype(np.float32)
    nodes = g.uniform(0.05, 1.0, (bs, T, 1, N, 4)).astype(np.float32)
    if N > 1:
        nodes[:, :, :, 1] = 0.0
    x_human[..., geo_offset:] = np.broadcast_to(nodes, (bs, T, H, N, 4)).reshape(bs, T, H, 4 * N)
    x_objects = g.standard_normal((bs, T, O, F_o)).astype(np.float32) if O else None
    mask = np.ones((bs, O), dtype=np.float32) if O else None
    if O:
        mask[0, O - 1] = 0.0
    steps = np.full(bs, T, dtype=np.float32) if steps is None else np.asarray(steps, dtype=np.float32)
    for b in range(bs):
        x_human[b, int(steps[b]):] = np.nan
        if O:
            x_objects[b, int(steps[b]):] = np.nan
    return x_human, x_objects, mask, steps


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def tensor_dataset(n=7, T=5, H=2, N=3, geo_offset=8, O=2, F_o=8, seed=5):
    """The tensors of a data set in gcn_fetcher's slot order (x_human, x_objects, objects_mask, segmentation, three distance
    slots, steps_per_example) and one target, which holds every clip's index: a batch's target is its clip ids."""
    steps = [T - (i % 3) for i in range(n)]
    xh, xo, mask, steps = make_batch(n, T, H, N, geo_offset, O, F_o, seed=seed, steps=steps)
    xh, xo = np.nan_to_num(xh), np.nan_to_num(xo)   # (create_data_loader: padding is zeros)
    t = [xh, xo, mask, np.ones((n, T, H), np.float32), np.zeros((n, T, H, H), np.float32), np.zeros((n, T, H, O), np.float32),
         np.zeros((n, T, O, O), np.float32), steps, np.arange(n, dtype=np.int64)]
    return [torch.from_numpy(a) for a in t]
