"""GPU: `bench.py --gpus N` started BARE (no torchrun, no WORLD_SIZE) must start N ranks by itself and report them.
Two ranks share the one visible MI355X here (TWOG_BENCH_BACKEND=gloo for the collectives -- RCCL needs one GPU per
rank; the driver's 8-GPU run uses the default nccl backend through exactly the same launch path)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*flags, timeout=900):
    env = dict(os.environ, TWOG_BENCH_BACKEND='gloo')
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), *flags], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-1500:]   # exactly ONE JSON line, from rank 0
    return json.loads(lines[0])


def test_bench_gpus_2_launches_two_ranks_weak():
    d = _bench('--gpus', '2', '--steps', '2', '--warmup', '1', '--workload', 'c5', '--full', '--no-cpu-baseline')
    assert d['n_gpus'] == 2 and d['scaling'] == 'weak'
    assert len(d['config']['devices']) == 2 and d['config']['devices'][0].startswith('rank0:')
    assert d['config']['per_gpu_batch'] == 16 and d['config']['global_batch'] == 32
    assert d['config']['collective_backend'] == 'gloo'
    assert d['value'] > 0 and d['forward_only_clips_per_s'] > 0
    assert abs(d['value'] - 32 * 2 / (d['ms_per_step'] * 2e-3)) < 1e-6 * d['value']
    # the same line carries the other scaling mode: fixed GLOBAL batch of the workload (16 clips -> 8 per GPU)
    st = d['strong_scaling']
    assert st['scaling'] == 'strong' and st['per_gpu_batch'] == 8 and st['global_batch'] == 16 and st['value'] > 0
    assert 'weak scaling' in d['value_is']


def test_bench_strong_scaling_splits_the_global_batch():
    d = _bench('--gpus', '2', '--steps', '2', '--warmup', '1', '--workload', 'c5', '--scaling', 'strong', '--full',
               '--no-cpu-baseline')
    assert d['n_gpus'] == 2 and d['scaling'] == 'strong'
    assert d['config']['per_gpu_batch'] == 8 and d['config']['global_batch'] == 16
    wk = d['weak_scaling']
    assert wk['scaling'] == 'weak' and wk['per_gpu_batch'] == 16 and wk['global_batch'] == 32 and wk['value'] > 0


def test_bench_plain_run_leaves_the_full_figures_out():
    """A plain run reports the headline and the figures of its own timed steps; what takes runs of its own (GCN
    roofline, forward-only rate, CPU baseline) comes with --full."""
    plain = _bench('--gpus', '1', '--steps', '2', '--warmup', '1', '--workload', 'c5')
    assert plain['value'] > 0 and plain['unit'] == 'clips/s' and plain['higher_is_better'] is True
    assert abs(plain['value'] - 16 * 2 / (plain['ms_per_step'] * 2e-3)) < 1e-6 * plain['value']
    assert plain['roofline']['achieved'] > 0 and plain['roofline_chain']['ms_per_step'] > 0
    for key in ('roofline_gcn', 'forward_only_clips_per_s', 'cpu_baseline'):
        assert key not in plain, key
    full = _bench('--gpus', '1', '--steps', '2', '--warmup', '1', '--workload', 'c5', '--full', '--no-cpu-baseline')
    assert full['roofline_gcn']['ms_per_batch'] > 0 and full['forward_only_clips_per_s'] > 0
    assert 'cpu_baseline' not in full


def test_bench_world_size_mismatch_is_refused():
    env = dict(os.environ, WORLD_SIZE='1')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2'], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and 'WORLD_SIZE' in r.stderr


def test_bench_dump_outputs_same_in_every_run(tmp_path):
    """--dump-outputs: the last timed step's outputs, identical in two runs with the same arguments (the warm-up phase
    runs a variable number of steps; the timed steps start from the restored initial state), and --steps is honoured."""
    import numpy as np
    runs = []
    for d in ('a', 'b'):
        r = _bench('--gpus', '1', '--steps', '3', '--warmup', '1', '--workload', 'c5', '--no-cpu-baseline',
                   '--dump-outputs', str(tmp_path / d))
        assert r['steps'] == 3 and r['ms_per_step'] > 0
        runs.append(tmp_path / d)
    names = sorted(p.name for p in runs[0].iterdir())
    assert names == sorted(p.name for p in runs[1].iterdir())
    assert {'loss.npy', 'parameters.npy', 'gradients.npy', 'output_4.npy', 'output_5.npy'} <= set(names)
    total = 0
    for n in names:
        a, b = np.load(runs[0] / n), np.load(runs[1] / n)
        assert a.dtype == np.float32 and np.isfinite(a).all(), n
        assert np.array_equal(a, b), n
        total += a.nbytes
    assert total <= 64 << 20
