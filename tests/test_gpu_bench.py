"""GPU test of a plain `bench.py` run (pytest -m gpu): without --full it times the steps, dumps and prints the headline line, and
measures nothing beside it."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_run_prints_the_headline_only(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1',
           '--per_gpu_batch', '16', '--image_size', '64', '--dump-outputs', str(tmp_path)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d['metric'].startswith('images/sec') and d['unit'] == 'images/s' and d['higher_is_better'] is True
    assert d['dtype'] == 'f32' and d['f32_matmul'] == 'f16x3_3' and d['steps'] == 2 and d['warmup'] == 1
    assert d['value'] > 0 and d['ms_per_step'] > 0 and abs(d['value'] - 16 * 1e3 / d['ms_per_step']) < 1e-2 * d['value']
    assert d['step_ms']['n'] == 2 and d['train_metrics']
    for k in ('roofline', 'families', 'ntxent', 'speed_mode', 'f32_mode', 'parity_mode_bf16x6', 'parity', 'north_star_met',
              'allgather', 'augment', 'cpu_baseline'):
        assert d[k] is None, k
    assert not d['kernels']
    assert {p.name for p in tmp_path.iterdir()} >= {'total_loss.npy', 'embeddings.npy', 'variables.npy', 'gradients.npy'}
