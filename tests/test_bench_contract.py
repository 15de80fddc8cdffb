"""bench.py driver contract: single-process run emits ONE JSON line with
the required fields (the round driver parses this exactly)."""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_json_contract():
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, 'bench.py'),
         '--steps', '2', '--warmup', '1', '--batch-size', '4',
         '--network', 'LeNet', '--dataset', 'MNIST'],
        capture_output=True, text=True, timeout=300, cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.strip().splitlines()
             if l.startswith('{')]
    assert len(lines) == 1, out.stdout
    j = json.loads(lines[0])
    for key in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup',
                'ms_per_step', 'higher_is_better', 'scaling',
                'vs_baseline', 'dtype', 'data', 'config'):
        assert key in j, key
    assert j['n_gpus'] == 1
    assert j['steps'] == 2 and j['warmup'] == 1
    assert j['higher_is_better'] is True
    assert j['scaling'] == 'weak'
    assert j['value'] > 0
    cfg = j['config']
    for key in ('model', 'global_batch', 'per_worker_batch', 'parallelism'):
        assert key in cfg, key


def _run_dump(out_dir, extra=()):
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, 'bench.py'),
         '--steps', '2', '--warmup', '1', '--batch-size', '4',
         '--network', 'LeNet', '--dataset', 'MNIST',
         '--dump-outputs', str(out_dir), *extra],
        capture_output=True, text=True, timeout=300, cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.strip().splitlines()
             if l.startswith('{')]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_bench_dump_outputs_repeatable(tmp_path):
    """--dump-outputs writes the last timed step's outputs as float32 .npy
    files; same arguments -> same inputs -> (on CPU, fp32) identical arrays.
    --full is accepted and leaves the result line's meaning unchanged."""
    import numpy as np
    ja = _run_dump(tmp_path / 'a')
    jb = _run_dump(tmp_path / 'b', extra=('--full',))
    assert ja['metric'] == jb['metric'] and ja['steps'] == jb['steps'] == 2
    names = sorted(os.listdir(tmp_path / 'a'))
    assert names == ['grads.npy', 'loss.npy', 'master_weights.npy']
    assert sorted(os.listdir(tmp_path / 'b')) == names
    total = 0
    for n in names:
        a = np.load(tmp_path / 'a' / n)
        b = np.load(tmp_path / 'b' / n)
        assert a.dtype == np.float32 and a.size > 0
        assert np.isfinite(a).all()
        assert a.shape == b.shape and np.isfinite(b).all()
        if ja['dtype'] == 'fp32':
            # CPU path is deterministic: identical inputs -> identical bits
            # (GPU kernels reduce with atomics, so only shapes are compared)
            np.testing.assert_array_equal(a, b)
        total += a.nbytes
    assert total <= 64 * 10 ** 6
    assert np.abs(np.load(tmp_path / 'a' / 'grads.npy')).max() > 0
