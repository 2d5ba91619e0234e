"""The cases of the semi-Markov CRF loss, shared by tests/test_semicrf_cpu.py, tests/test_semicrf_gpu.py and
tools/semicrf_loss_fp64.py (which measures what fp32 costs on them and records it in profiles/semicrf_loss_fp64.json).

A case is a dict(name, kind, claim, bs, C, T, E, D, labels, values). `claim` names the branch the case is there for. `kind` is
the class the recorded fp32 error and so the GPU gate are kept per: 'small' (a few chunks at most), 'long' (drift over many
steps), 'wide' (wide-range scores), 'sharp' (near-deterministic emissions, where logZ - gold cancels). `make(case)` builds
(input fp32 (bs, C, T, E), target int64 (bs, T, E), A fp32 (C, C), pi fp32 (C,), dur fp32 (C, D)) from the name alone, the
same on every machine.

Labels come in runs (a fresh label after a random number of steps), cut so that no run is longer than `longest`; the
removal patterns of tests/crf_cases.py are laid over them. The two plan cases are found from twog_semicrf_plan of the loaded
library (launch-free), not from constants: the first shape of a fixed ladder whose plan has every wave the entities ask for,
and the first whose plan gives waves up for LDS."""
import zlib

import numpy as np

CHUNK = 16
IGNORE = -1
KINDS = ('small', 'long', 'wide', 'sharp')
LABELS = ('all', 'head', 'tail', 'holes', 'absent', 'none', 'runD1', 'run2D', 'run2D1')


def _case(kind, claim, bs, C, T, E, D, labels='all', values='softmax'):
    return dict(name=f'{kind}-bs{bs}-C{C}-T{T}-E{E}-D{D}-{labels}-{values}', kind=kind, claim=claim, bs=bs, C=C, T=T, E=E, D=D,
                labels=labels, values=values)


def plan(bs, C, T, E, D):
    """twog_semicrf_plan of the loaded library: no device is touched."""
    from twog_gcn_amd import _lib
    return _lib.semicrf_plan(_lib.load(), bs, C, T, E, D)


def _plan_cases():
    full = lds = None
    for C, D in ((6, 8), (20, 16), (33, 32), (40, 64), (64, 128)):
        T, E = D + 5, 9
        p = plan(1, C, T, E, D)
        most_f, most_b = min(E, 8), min(E, 4 if C > 32 else 8)
        if full is None and p['fwd_waves'] == most_f and p['bwd_waves'] == most_b:
            full = _case('small', 'plan: every wave the entities ask for', 1, C, T, E, D, 'holes')
        if lds is None and p['fwd_waves'] < most_f and p['bwd_waves'] < most_b:
            lds = _case('small', 'plan: waves given up for LDS, both directions', 1, C, T, E, D, 'tail')
    assert full is not None and lds is not None
    return [full, lds]


def _cases():
    out = []
    # class counts one either side of every template edge
    for i, C in enumerate((8, 9, 16, 17, 32, 33, 64)):
        out.append(_case('small', f'class template edge, C = {C}', 2, C, CHUNK + 1, 3, 5, ('holes', 'all', 'tail')[i % 3]))
    # K = T kept steps around the chunk, the entities around one workgroup
    for i, K in enumerate((1, 15, 16, 17, 33)):
        out.append(_case('small', f'K = {K}', (1, 3)[i % 2], 5, K, (1, 3, 9)[i % 3], 4))
    # the duration range against K = 20: one length, two, a chunk, one more, exactly K, beyond K, the limit
    for D in (1, 2, 16, 17, 20, 23, 128):
        out.append(_case('small', f'D = {D} at K = 20', 2, 6, 20, 2, D))
    # every removed-step pattern; E = 9 is more than one workgroup per clip with idle waves in the last
    for labels in ('all', 'head', 'tail', 'holes', 'absent', 'none'):
        out.append(_case('small', f'removed steps: {labels}', 3, 6, CHUNK + 4, 9 if labels in ('tail', 'absent') else 3, 6, labels))
    # gold runs longer than D: cut into pieces joined by A[c, c]
    for labels, what in (('runD1', 'D + 1'), ('run2D', '2 D'), ('run2D1', '2 D + 1')):
        out.append(_case('small', f'a gold run of {what} steps', 2, 4, 14, 2, 4, labels))
    # -inf in contract
    out.append(_case('small', '-inf diagonal, D >= the longest run', 2, 6, 33, 3, 8, 'holes', 'infdiag'))
    out.append(_case('small', '-inf minimum durations and a -inf initial score', 2, 5, 33, 2, 8, 'all', 'mindur'))
    out.append(_case('small', '-inf diagonal beyond 32 classes', 1, 40, 18, 5, 6, 'tail', 'infdiag'))
    out += _plan_cases()
    # drift
    out.append(_case('long', '4096 steps at D = 128', 1, 4, 4096, 2, 128, 'holes'))
    out.append(_case('long', 'the widest template at D = 128', 1, 64, 300, 2, 128, 'tail'))
    out.append(_case('long', 'many steps, middle D', 2, 9, 500, 3, 32, 'all'))
    # wide-range scores: log-probabilities down to -80, A in [-20, 5], pi in [-10, 0], dur in [-10, 2]
    out.append(_case('wide', 'wide-range scores', 3, 6, 2 * CHUNK + 1, 3, 7, 'holes', 'wide'))
    out.append(_case('wide', 'wide-range scores beyond 32 classes', 2, 33, CHUNK + 1, 3, 20, 'tail', 'wide'))
    out.append(_case('wide', 'wide-range scores over many steps', 1, 13, 200, 2, 16, 'all', 'wide'))
    # near-deterministic emissions: one class at -1e-6, the others at -15, the labels on that class
    out.append(_case('sharp', 'near-deterministic emissions', 3, 6, 2 * CHUNK + 1, 3, 7, 'holes', 'sharp'))
    out.append(_case('sharp', 'near-deterministic emissions over many steps', 1, 17, 200, 2, 16, 'all', 'sharp'))
    return out


def _runs(rng, shape, C, longest, shortest=1):
    """int64 labels of `shape` = (bs, T, E) in runs of shortest .. longest steps; with C > 1 neighbouring runs differ."""
    bs, T, E = shape
    y = np.zeros(shape, np.int64)
    for b in range(bs):
        for e in range(E):
            t, last = 0, -1
            while t < T:
                n = int(rng.integers(shortest, longest + 1))
                if T - t - n < shortest:                  # no stub shorter than `shortest` at the end
                    n = T - t
                c = int(rng.integers(0, C))
                if C > 1 and c == last:
                    c = (c + 1) % C
                y[b, t:t + n, e] = c
                t, last = t + n, c
    return y


def longest_run(y, C):
    """The longest run of equal labels over the kept steps of (bs, T, E) labels."""
    best = 0
    for b in range(y.shape[0]):
        for e in range(y.shape[2]):
            k = y[b, :, e]
            k = k[(k != IGNORE) & (k >= 0) & (k < C)]
            n = 0
            for i in range(k.size):
                n = n + 1 if i and k[i] == k[i - 1] else 1
                best = max(best, n)
    return best


def make(case):
    rng = np.random.default_rng(zlib.crc32(case['name'].encode()))
    bs, C, T, E, D = case['bs'], case['C'], case['T'], case['E'], case['D']
    labels, values = case['labels'], case['values']
    # the diagonal is -inf: no run may exceed D, also where a hole joins its neighbours (checked below); minimum durations:
    # runs of 3 .. D steps. Elsewhere runs of up to 6 steps, longer than D where D is small.
    if values == 'infdiag':
        target = _runs(rng, (bs, T, E), C, max(1, min(D, 6) // 2))
    elif values == 'mindur':
        target = _runs(rng, (bs, T, E), C, D - 2, 3)
    else:
        target = _runs(rng, (bs, T, E), C, 6)
    if labels in ('runD1', 'run2D', 'run2D1'):
        n = {'runD1': D + 1, 'run2D': 2 * D, 'run2D1': 2 * D + 1}[labels]
        target[:, 2:2 + n] = (target[:, 1:2] + 1) % C
        target[:, 2 + n:] = (target[:, 2:3] + 1 + (target[:, 2 + n:] % (C - 1))) % C   # the run ends where it is meant to
    if values in ('softmax', 'infdiag', 'mindur'):
        z = rng.normal(size=(bs, C, T, E)) * 2.0
        x = z - np.log(np.exp(z).sum(1, keepdims=True))
        A, pi, dur = rng.normal(size=(C, C)), rng.normal(size=C), rng.normal(size=(C, D))
        if values == 'infdiag':
            np.fill_diagonal(A, -np.inf)
        if values == 'mindur':
            dur[:, :2] = -np.inf
            free = [c for c in range(C) if c not in set(target[:, 0].ravel().tolist())]
            pi[free[0]] = -np.inf                         # a class no sequence starts with
    elif values == 'wide':
        x = rng.uniform(-80.0, 0.0, size=(bs, C, T, E))
        A, pi, dur = rng.uniform(-20.0, 5.0, size=(C, C)), rng.uniform(-10.0, 0.0, size=C), rng.uniform(-10.0, 2.0, size=(C, D))
    elif values == 'sharp':
        x = np.full((bs, C, T, E), -15.0)
        np.put_along_axis(x, target[:, None], -1e-6, axis=1)
        A, pi, dur = np.zeros((C, C)), np.zeros(C), np.zeros((C, D))
    else:
        raise ValueError(values)
    t = np.arange(T)[None, :, None]
    if labels == 'tail':        # padding of a different length per clip
        keep = t < np.maximum(1, T - 2 * np.arange(bs) - 1)[:, None, None]
        target = np.where(keep, target, IGNORE)
    elif labels == 'head':
        target = np.where(t >= min(3, T - 1), target, IGNORE)
    elif labels == 'holes':     # the ignore value, and labels outside [0, C) that are removed all the same
        r = rng.random(size=target.shape)
        target = np.where(r < 0.2, IGNORE, np.where(r < 0.3, C + 2, target))
    elif labels == 'absent':    # a sequence with nothing kept beside full ones, and a whole clip's tail entity absent
        target[0, :, 0] = IGNORE
        target[-1, :, -1] = IGNORE
    elif labels == 'none':      # all removed
        target[:] = IGNORE
    elif labels not in ('all', 'runD1', 'run2D', 'run2D1'):
        raise ValueError(labels)
    assert values not in ('infdiag', 'mindur') or longest_run(target, C) <= D, 'the gold score would be -inf'
    return (x.astype(np.float32), target.astype(np.int64), A.astype(np.float32), pi.astype(np.float32),
            dur.astype(np.float32))


CASES = _cases()
BY_NAME = {c['name']: c for c in CASES}
assert len(BY_NAME) == len(CASES), 'two cases share a name'


def run_kernel_layer(K, tensors, device, weight=1.0, before_g=True):
    """The four launches of the kernel layer (kernels.semicrf_nll_fwd / semicrf_nll_bwd) on the tensors of `make`, as a
    tests.semicrf_ref.SemiCrfResult in numpy. before_g: the upstream gradient is the term's own count, so that g = 1 exactly
    (the count is an integer below 2^24) and the gradients come out before the factor g, as semicrf_nll(..., g=1) gives them."""
    import torch
    from tests.semicrf_ref import SemiCrfResult
    x, y, A, pi, dur = (torch.from_numpy(a).to(device) for a in tensors)
    term = dict(input=x, target=y, transitions=A, initial=pi, durations=dur, weight=weight, ignore=IGNORE)
    losses = torch.empty(1, dtype=torch.float32, device=device)
    stats = torch.empty(1, 2, dtype=torch.float64, device=device)
    K.semicrf_nll_fwd([term], losses, stats)
    dl = stats[:, 1].to(torch.float32) if before_g else torch.ones(1, dtype=torch.float32, device=device)
    dinput = torch.empty_like(x)
    (dA, dpi, ddur), = K.semicrf_nll_bwd([term], stats, dl.contiguous(), [dinput], [False], [True])
    bs, _, _, E = x.shape
    seq = term['seq'].cpu()
    return SemiCrfResult(seq[:, 2].numpy().reshape(bs, E), seq[:, 0].numpy().reshape(bs, E), seq[:, 1].numpy().reshape(bs, E),
                         seq[:, 3].contiguous().view(torch.int32).numpy().astype(np.int64).reshape(bs, E),
                         float(losses[0]), float(stats[0, 1]), dinput.cpu().numpy(), dA.cpu().numpy(), dpi.cpu().numpy(),
                         ddur.cpu().numpy())
