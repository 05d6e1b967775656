"""bench.py as it is run for every change: a plain run prints the headline alone, `--steps` sets the timed
steps, and `--dump-outputs` writes the last timed step's outputs from inputs that are the same run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = {'metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'}
FULL_ONLY = {'epoch', 'bf16_variant', 'collective', 'roofline', 'roofline_forward_recurrence', 'roofline_attention',
             'roofline_gemm', 'roofline_frontend', 'config4', 'config5', 'cpu_baseline'}


def _plain_bench(dump, steps):
    env = dict(os.environ)
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'SSASR_DIST_SINGLE', 'SSASR_DIST_BACKEND'):
        env.pop(k, None)
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(steps),
                          '--warmup', '1', '--dump-outputs', dump], env=env, cwd=ROOT,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert res.returncode == 0, (res.stdout + res.stderr)[-3000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_plain_bench_prints_the_headline_and_dumps_the_last_step(tmp_path):
    # 1,000 steps: enough training for the run-to-run rounding of the gradient reductions to grow far past rounding
    # (logits 37 % apart) had the last step not started from the seeded initial state
    a, b = str(tmp_path / 'a'), str(tmp_path / 'b')
    line = _plain_bench(a, 1000)
    assert HEADLINE <= set(line) and not FULL_ONLY & set(line), sorted(line)
    assert line['steps'] == 1000 and line['warmup'] == 1 and line['ms_per_step'] > 0 and line['value'] > 0
    assert line['unit'] == 'utterances/sec' and line['higher_is_better'] is True and line['dtype'] == 'f32'
    assert abs(line['value'] - 32 * 1000.0 / line['ms_per_step']) < 0.01 * line['value']
    names = sorted(os.listdir(a))
    assert {'loss.npy', 'logits.npy', 'grad_norm.npy', 'update_skipped.npy'} <= set(names)
    assert sum(os.path.getsize(os.path.join(a, n)) for n in names) <= 64 << 20
    assert float(np.load(os.path.join(a, 'loss.npy'))[0]) == pytest.approx(line['final_loss'], abs=1e-5)
    assert np.load(os.path.join(a, 'update_skipped.npy'))[0] == 0
    # the same arguments again: the same inputs, so the same outputs up to the run-to-run rounding of the
    # gradient reductions' atomics
    line_b = _plain_bench(b, 1000)
    assert line_b['final_loss'] == pytest.approx(line['final_loss'], abs=1e-5)
    assert sorted(os.listdir(b)) == names
    for n in names:
        x, y = np.load(os.path.join(a, n)), np.load(os.path.join(b, n))
        assert x.dtype in (np.float32, np.float64) and x.shape == y.shape, n
        assert np.allclose(x, y, rtol=1e-4, atol=1e-5), (n, float(np.abs(x - y).max()))
