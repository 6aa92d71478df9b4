"""-m gpu: a plain bench.py run (no --full) and its --dump-outputs files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, steps, warmup):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
           "--rec_iters", "4", "--dump-outputs", out_dir]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_dumps_the_last_timed_step(tmp_path):
    """Without --full the line carries the headline keys but no CPU baseline and no per-kernel pass; the dumped arrays are
    those of the last timed step: the same step index reached through other step / warm-up counts gives the same bits."""
    a = _bench(str(tmp_path / "a"), steps=2, warmup=1)
    b = _bench(str(tmp_path / "b"), steps=1, warmup=2)
    for res, steps in ((a, 2), (b, 1)):
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert k in res, k
        assert res["steps"] == steps and res["ms_per_step"] > 0 and res["value"] > 0
        assert "cpu_baseline" not in res and res["kernels"] == [] and res["roofline"]["profiled_step_ms"] is None
    B, R = a["config"]["batch_per_gpu"], a["config"]["rec_rr"]
    shapes = {"rec": (B, 28, 28, 1), "idx": (B,), "loss": (B * R,), "z": (B * R, 128)}
    assert sorted(os.listdir(str(tmp_path / "a"))) == sorted(n + ".npy" for n in shapes)
    for n, shape in shapes.items():
        xa, xb = np.load(str(tmp_path / "a" / (n + ".npy"))), np.load(str(tmp_path / "b" / (n + ".npy")))
        assert xa.shape == shape and xa.dtype in (np.float32, np.float64) and np.isfinite(xa).all(), n
        assert np.array_equal(xa, xb), n
    assert abs(np.load(str(tmp_path / "a" / "loss.npy")).reshape(B, R).min(axis=1).mean() - a["mean_best_loss"]) < 1e-5
