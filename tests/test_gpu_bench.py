"""GPU: bench.py's plain single-GPU run -- exactly the K timed steps, the headline keys of the result line and nothing of what
--full adds -- and --dump-outputs (the last timed step's loss, logits, gradients, parameters and buffers as float32 .npy)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_plain_run_and_dump_outputs(hip, tmp_path):
    out_dir = tmp_path / 'outputs'
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '2', '--n-sp', '200',
           '--n-edges', '800', '--dump-outputs', str(out_dir)]
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d['n_gpus'] == 1 and d['steps'] == 3 and d['warmup'] == 2 and d['unit'] == 'superpoints/s'
    assert d['higher_is_better'] is True and d['dtype'] == 'f32' and d['config']['superpoints_per_step'] == 200
    assert abs(d['value'] - 200 / (d['ms_per_step'] * 1e-3)) < 1e-6 * d['value']
    assert d['self_check']['persistent_errors'] == 0 and d['self_check']['grads_finite']
    for k in ('roofline', 'ms_per_step_min', 'sustained', 'trainer_window', 'forward_only', 'other_workloads'):
        assert k not in d, k                                          # side measurements: --full only
    arrays = {p.stem: np.load(p) for p in out_dir.glob('*.npy')}
    assert set(arrays) == {'loss', 'logits', 'grads', 'params', 'buffers'}
    for name, a in arrays.items():
        assert a.dtype == np.float32 and np.isfinite(a).all(), name
    assert arrays['logits'].shape == (200, 13) and arrays['grads'].shape == arrays['params'].shape
    assert arrays['grads'].size > 0 and arrays['buffers'].size > 0
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
