"""The cases of the linear-chain CRF loss, shared by tests/test_crf_cpu.py, tests/test_crf_gpu.py and
tools/crf_loss_fp64.py (which measures what fp32 costs on them and records it in profiles/crf_loss_fp64.json).

A case is a dict(name, kind, bs, C, T, E, labels, values). `kind` is the class the recorded fp32 error and so the GPU gate
are kept per: 'small' (a few chunks at most), 'long' (drift over many steps), 'wide' (wide-range scores), 'sharp'
(near-deterministic emissions, where logZ - gold cancels). `make(case)` builds (input fp32 (bs, C, T, E), target int64
(bs, T, E), A fp32 (C, C), pi fp32 (C,)) from the name alone, the same on every machine.

Shapes: the smallest at which the kernels take another path. CHUNK is the staging chunk (TWOG_CRF_CHUNK), CEILINGS the
class-count template ceilings; 8 entities are one workgroup below 33 classes and 4 beyond, so E = 9 is more than one
workgroup per clip with idle waves in the last."""
import zlib

import numpy as np

CHUNK = 16
CEILINGS = (8, 16, 32, 64)
IGNORE = -1

LABELS = ('all', 'tail', 'head', 'holes', 'empty', 'oob', 'k1', 'k2')
KINDS = ('small', 'long', 'wide', 'sharp')


def _case(kind, bs, C, T, E, labels='all', values='softmax'):
    return dict(name=f'{kind}-bs{bs}-C{C}-T{T}-E{E}-{labels}-{values}', kind=kind, bs=bs, C=C, T=T, E=E, labels=labels,
                values=values)


def _cases():
    out = []
    # class counts: 1, 2, 3 and one value either side of every template ceiling, up to 64
    for i, C in enumerate((1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64)):
        out.append(_case('small', 2, C, CHUNK + 1, 3, ('holes', 'all', 'tail')[i % 3]))
    # T one step either side of the chunk and of two chunks; K = 1 and K = 2 as whole sequences
    for i, T in enumerate((1, 2, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1)):
        out.append(_case('small', (1, 3)[i % 2], 5, T, (1, 3, 9)[i % 3], 'all' if T <= 2 else ('all', 'holes', 'head')[i % 3]))
    # every label pattern, more than one workgroup per clip with an idle wave (E = 9), and the same beyond 32 classes (E = 5)
    for labels in LABELS:
        out.append(_case('small', 3, 6, CHUNK + 4, 9 if labels in ('tail', 'empty') else 3, labels))
    out.append(_case('small', 3, 40, CHUNK + 2, 5, 'tail'))
    out.append(_case('small', 1, 4, 2 * CHUNK + 3, 9, 'holes'))
    # drift
    out.append(_case('long', 1, 4, 4096, 2, 'holes'))
    out.append(_case('long', 1, 64, 512, 2, 'tail'))
    out.append(_case('long', 2, 9, 1000, 3, 'all'))
    out.append(_case('long', 1, 20, 700, 3, 'holes'))
    # wide-range scores: log-probabilities down to -80, A in [-20, 5], pi in [-10, 0]
    out.append(_case('wide', 3, 6, 2 * CHUNK + 1, 3, 'holes', 'wide'))
    out.append(_case('wide', 2, 33, CHUNK + 1, 3, 'tail', 'wide'))
    out.append(_case('wide', 1, 13, 200, 2, 'all', 'wide'))
    out.append(_case('wide', 3, 64, CHUNK - 1, 2, 'head', 'wide'))
    # near-deterministic emissions: one class at -1e-6, the others at -15, the labels on that class
    out.append(_case('sharp', 3, 6, 2 * CHUNK + 1, 3, 'holes', 'sharp'))
    out.append(_case('sharp', 1, 17, 200, 2, 'all', 'sharp'))
    out.append(_case('sharp', 2, 3, CHUNK, 3, 'tail', 'sharp'))
    out.append(_case('sharp', 1, 40, 100, 2, 'head', 'sharp'))
    return out


CASES = _cases()
BY_NAME = {c['name']: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def make(case):
    rng = np.random.default_rng(zlib.crc32(case['name'].encode()))
    bs, C, T, E = case['bs'], case['C'], case['T'], case['E']
    target = rng.integers(0, C, size=(bs, T, E)).astype(np.int64)
    if case['values'] == 'softmax':
        z = rng.normal(size=(bs, C, T, E)) * 2.0
        x = z - np.log(np.exp(z).sum(1, keepdims=True))
        A, pi = rng.normal(size=(C, C)), rng.normal(size=C)
    elif case['values'] == 'wide':
        x = rng.uniform(-80.0, 0.0, size=(bs, C, T, E))
        A, pi = rng.uniform(-20.0, 5.0, size=(C, C)), rng.uniform(-10.0, 0.0, size=C)
    elif case['values'] == 'sharp':
        x = np.full((bs, C, T, E), -15.0)
        np.put_along_axis(x, target[:, None], -1e-6, axis=1)
        A, pi = np.zeros((C, C)), np.zeros(C)
    else:
        raise ValueError(case['values'])
    labels = case['labels']
    t = np.arange(T)[None, :, None]
    if labels == 'tail':        # padding of a different length per clip
        keep = t < np.maximum(1, T - 2 * np.arange(bs) - 1)[:, None, None]
        target = np.where(keep, target, IGNORE)
    elif labels == 'head':
        target = np.where(t >= min(3, T - 1), target, IGNORE)
    elif labels == 'holes':
        target = np.where(rng.random(size=target.shape) < 0.3, IGNORE, target)
    elif labels == 'empty':     # a sequence with nothing kept beside full ones, and a whole clip's tail entity absent
        target[0, :, 0] = IGNORE
        target[-1, :, -1] = IGNORE
    elif labels == 'oob':       # labels outside [0, C) that are not the ignore value are removed all the same
        r = rng.random(size=target.shape)
        target = np.where(r < 0.15, C + 2, np.where(r < 0.3, -5, target))
    elif labels in ('k1', 'k2'):
        k = int(labels[1])
        keep = np.zeros_like(target, dtype=bool)
        for b in range(bs):
            for e in range(E):
                keep[b, rng.choice(T, size=k, replace=False), e] = True
        target = np.where(keep, target, IGNORE)
    elif labels != 'all':
        raise ValueError(labels)
    return x.astype(np.float32), target.astype(np.int64), A.astype(np.float32), pi.astype(np.float32)


def run_kernel_layer(K, tensors, device, weight=1.0, before_g=True):
    """The four launches of the kernel layer (kernels.crf_nll_fwd / crf_nll_bwd) on the tensors of `make`, as a
    tests.crf_ref.CrfResult in numpy. before_g: the upstream gradient is the term's own count, so that g = 1 exactly (the
    count is an integer below 2^24) and the gradients come out before the factor g, as crf_nll(..., g=1) gives them."""
    import torch
    from tests.crf_ref import CrfResult
    x, y, A, pi = (torch.from_numpy(a).to(device) for a in tensors)
    term = dict(input=x, target=y, transitions=A, initial=pi, weight=weight, ignore=IGNORE)
    losses = torch.empty(1, dtype=torch.float32, device=device)
    stats = torch.empty(1, 2, dtype=torch.float64, device=device)
    K.crf_nll_fwd([term], losses, stats)
    dl = stats[:, 1].to(torch.float32) if before_g else torch.ones(1, dtype=torch.float32, device=device)
    dinput = torch.empty_like(x)
    (dA, dpi), = K.crf_nll_bwd([term], stats, dl.contiguous(), [dinput], [False], [True])
    bs, _, _, E = x.shape
    seq = term['seq'].cpu()
    return CrfResult(seq[:, 2].numpy().reshape(bs, E), seq[:, 0].numpy().reshape(bs, E), seq[:, 1].numpy().reshape(bs, E),
                     seq[:, 3].contiguous().view(torch.int32).numpy().astype(np.int64).reshape(bs, E),
                     float(losses[0]), float(stats[0, 1]), dinput.cpu().numpy(), dA.cpu().numpy(), dpi.cpu().numpy())
