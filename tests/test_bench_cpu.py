"""CPU: the launch logic of bench.py that needs no GPU -- a --gpus / WORLD_SIZE mismatch is refused with the exact
torchrun command, and a bare `--gpus N` start becomes a launcher of N child ranks (checked by substituting the child)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_world_size_mismatch_is_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '4'], cwd=ROOT,
                       env=dict(os.environ, WORLD_SIZE='2'), capture_output=True, text=True, timeout=300)
    assert r.returncode == 2
    assert '--nproc-per-node 4' in r.stderr and 'WORLD_SIZE=2' in r.stderr


def test_bare_start_launches_n_ranks(monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    seen = {}

    def fake_run(cmd, env=None, **kw):
        seen['cmd'], seen['env'] = cmd, env

        class R:
            returncode = 7
        return R()

    monkeypatch.setattr(subprocess, 'run', fake_run)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '8', '--steps', '3'])
    assert bench.launch_ranks(8) == 7          # the launcher exits with the children's code
    cmd = seen['cmd']
    assert cmd[1:4] == ['-m', 'torch.distributed.run', '--nnodes=1'] and '--nproc-per-node=8' in cmd
    assert cmd[cmd.index('--master-addr') + 1] == '127.0.0.1'
    assert cmd[-4:] == ['--gpus', '8', '--steps', '3'] and cmd[-5].endswith('bench.py')
    assert seen['env'].get('HSA_ENABLE_IPC_MODE_LEGACY') == '0'


def test_dump_outputs_float32_within_budget_fixed_sample(tmp_path):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import bench
    big = torch.arange(20_000_000, dtype=torch.float64)
    arrays = [('loss', torch.tensor(2.5)), ('out', torch.randn(3, 4).t()), ('big', big)]
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), arrays)
    total = 0
    for name, t in arrays:
        a, b = np.load(tmp_path / 'a' / f'{name}.npy'), np.load(tmp_path / 'b' / f'{name}.npy')
        assert a.dtype == np.float32 and np.array_equal(a, b)
        total += a.nbytes
        if name != 'big':   # small arrays are written whole, in their shape
            assert a.shape == tuple(t.shape) and np.array_equal(a, t.float().numpy())
    assert total <= 64 << 20
    s = np.load(tmp_path / 'a' / 'big.npy')   # the sample: elements in ascending index order
    assert 0 < s.size < big.numel() and np.all(np.diff(s) >= 0) and s[0] < s[-1]


def test_steps_below_one_is_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '0'], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and '--steps' in r.stderr
