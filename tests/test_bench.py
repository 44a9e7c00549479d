"""bench.py's plain run: the result line's contract and --dump-outputs (the full line is exercised through its N > 1
half in test_distributed_gpu.py::test_bench_multi_gpu_half_runs_unattended)."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_line_and_dump_outputs(tmp_path):
    """A plain run prints the headline only (no roofline, cfg3 line or CPU baseline), times exactly --steps steps, and
    --dump-outputs leaves the last step's losses and sampled parameters as float32 .npy files within 64 MB."""
    out_dir = tmp_path / 'dump'
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--batch', '32',
           '--dump-outputs', str(out_dir)]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out['steps'] == 3 and out['warmup'] == 1 and out['n_gpus'] == 1
    assert out['ms_per_step'] > 0 and out['value'] > 0 and out['unit'] == 'sequences/s' and out['higher_is_better'] is True
    assert abs(out['value'] - 32 * 1e3 / out['ms_per_step']) <= 0.01 * out['value']
    assert out['dtype'] == 'bf16' and out['metric'].startswith('pre-train samples/sec')
    assert not {'roofline', 'also', 'cpu_baseline', 'comm'} & set(out)
    files = sorted(glob.glob(str(out_dir / '*.npy')))
    names = [os.path.basename(f)[:-4] for f in files]
    assert 'loss' in names and any(n.startswith('loss.CMLM') for n in names) and 'param.embeddings.weight' in names
    assert sum(os.path.getsize(f) for f in files) <= 64 << 20
    arrays = {n: np.load(f) for n, f in zip(names, files)}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert float(arrays['loss'][0]) > 0
