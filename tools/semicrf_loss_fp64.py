#!/usr/bin/env python3
"""What fp32 costs the semi-Markov CRF loss, and what the kernels cost beyond that: profiles/semicrf_loss_fp64.json.

Step 1 (any machine, no GPU): over the cases of tests/semicrf_cases.py, the numpy definition at fp32 (tests/semicrf_ref.py,
dtype=np.float32: the log domain with the maximum subtracted, one rounding per operation) against the same at fp64, the
largest error per compared quantity and per case, and per case kind -- loss and per-sequence nll relative to max(1, |logZ|),
the four gradients in absolute terms before the factor g. The gate of tests/test_semicrf_gpu.py for a quantity is FACTOR
times the largest over the cases of the kind.
    python tools/semicrf_loss_fp64.py --spec
Step 2 (GPU): the kernels' own errors against fp64 on the same cases, written beside them.
    python tools/semicrf_loss_fp64.py --kernel
Both steps rewrite only their own part of the file.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FACTOR = 4   # the device's expf / logf are a few ulp from numpy's, and a different but valid summation order


def worst(per_case, cases):
    from tests.semicrf_cases import KINDS
    from tests.semicrf_ref import QUANTITIES
    return {kind: {q: max(per_case[c['name']][q] for c in cases if c['kind'] == kind) for q in QUANTITIES} for kind in KINDS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--spec', action='store_true')
    ap.add_argument('--kernel', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'semicrf_loss_fp64.json'))
    ap.add_argument('--base', default=None, help='the file whose other part is kept (default: --out)')
    args = ap.parse_args()
    import numpy as np
    import twog_gcn_amd  # noqa: F401  (the plan cases ask the loaded library)
    from tests import semicrf_ref as R
    from tests.semicrf_cases import CASES, make
    base = args.base or args.out
    res = json.load(open(base)) if os.path.exists(base) else {}
    res['cases'] = {c['name']: c['claim'] for c in CASES}
    res['factor'] = FACTOR
    res['quantities'] = ('loss and nll: |got - fp64| / max(1, |logZ|); dinput, dA, dpi, ddur: |got - fp64| before the factor g '
                         '(both evaluated with g = 1)')
    specs = {c['name']: R.semicrf_nll(*make(c), dtype=np.float64, g=1.0) for c in CASES}
    if args.spec:
        per_case = {c['name']: R.errors(R.semicrf_nll(*make(c), dtype=np.float32, g=1.0), specs[c['name']]) for c in CASES}
        res['fp32_spec_per_case'] = per_case
        res['fp32_spec'] = worst(per_case, CASES)
        res['gate'] = {kind: {q: FACTOR * v for q, v in d.items()} for kind, d in res['fp32_spec'].items()}
        for q in R.QUANTITIES:
            assert any(e[q] > 0 for e in per_case.values()), f'no case measures {q}: its gate would be vacuous'
    if args.kernel:
        import torch
        from twog_gcn_amd.kernels import get_kernels
        from tests.semicrf_cases import run_kernel_layer
        assert torch.cuda.is_available(), 'the kernels need the GPU: there is no fallback'
        K = get_kernels()
        per_case = {}
        for c in CASES:
            got = run_kernel_layer(K, make(c), torch.device('cuda', 0))
            assert (got.K == specs[c['name']].K).all(), c['name']
            per_case[c['name']] = R.errors(got, specs[c['name']])
        res['kernel_per_case'] = per_case
        res['kernel'] = worst(per_case, CASES)
        res['kernel_device'] = torch.cuda.get_device_name(0)
        if 'gate' in res:
            res['kernel_above_gate'] = {n: {q: v for q, v in e.items() if v > res['gate'][c['kind']][q]}
                                        for c in CASES for n, e in [(c['name'], per_case[c['name']])]
                                        if any(v > res['gate'][c['kind']][q] for q, v in e.items())}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: res.get(k) for k in ('fp32_spec', 'gate', 'kernel', 'kernel_above_gate')}, indent=1))


if __name__ == '__main__':
    main()
