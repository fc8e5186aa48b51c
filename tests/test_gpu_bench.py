"""bench.py end to end on the GPU (C1, the smallest config): the plain result line, --dump-outputs, and the restart
of the trajectory every bench.RESTART_PERIOD steps, which keeps a long run's state finite and makes its state after
n steps that of a fresh run after (n - 1) % RESTART_PERIOD + 1."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("displacement", "velocity", "acceleration")


def _run(out, steps, warmup):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "c1", "--steps",
                        str(steps), "--warmup", str(warmup), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), {f: np.load(os.path.join(out, f + ".npy")) for f in FIELDS}


def test_long_run_restarts_and_dumps_the_fresh_runs_state(tmp_path):
    P = bench.RESTART_PERIOD
    short, a = _run(tmp_path / "short", 6, 2)  # 8 steps, no restart
    long_, b = _run(tmp_path / "long", 2 * P + 6, 2)  # 2 P + 8 steps: two restarts, then the same 8
    for d, steps in ((short, 6), (long_, 2 * P + 6)):
        assert (d["steps"], d["warmup"], d["unit"], d["higher_is_better"]) == (steps, 2, "DOF-it/s", True)
        assert d["value"] > 0 and d["ms_per_step"] > 0 and d["steps_converged"] == steps
        for k in ("cpu_baseline", "roofline_hbm", "roofline_general", "general", "parity"):
            assert d[k] is None  # --full only
    assert sorted(os.listdir(tmp_path / "long")) == sorted(f + ".npy" for f in FIELDS)
    for f in FIELDS:
        assert b[f].dtype == np.float32 and b[f].shape == (4158,)
        assert np.isfinite(b[f]).all() and np.abs(b[f]).max() > 0
        assert np.array_equal(a[f], b[f]), f
