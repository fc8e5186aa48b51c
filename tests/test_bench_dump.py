"""bench.py --dump-outputs on the CPU: file names, dtypes, the 64 MB budget and the fixed sample (no GPU: a stand-in
stepper serves get_state)."""
import os
import sys

import numpy as np
import pytest

import bench


class _State:
    DISPLACEMENT, VELOCITY, ACCELERATION = 0, 1, 2

    def __init__(self, n):
        self.dof_count = n

    def get_state(self, which):
        return np.arange(self.dof_count, dtype=np.float32) * np.float32(which + 1)


def _load(d):
    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_small_output_is_written_whole(tmp_path):
    bench.dump_outputs(_State(1029), str(tmp_path))
    got = _load(tmp_path)
    assert sorted(got) == ["acceleration.npy", "displacement.npy", "velocity.npy"]
    for k, name in enumerate(("displacement.npy", "velocity.npy", "acceleration.npy")):
        assert got[name].dtype == np.float32
        assert np.array_equal(got[name], _State(1029).get_state(k))


def test_large_output_is_the_same_sample_within_the_budget(tmp_path):
    n = bench.DUMP_BUDGET_BYTES // 12 + 1  # the first size over the budget
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(_State(n), str(a))
    bench.dump_outputs(_State(n), str(b), rank=1)
    assert sum(os.path.getsize(a / f) for f in os.listdir(a)) <= bench.DUMP_BUDGET_BYTES
    ga, gb = _load(a), _load(b)
    assert sorted(gb) == ["acceleration_rank1.npy", "displacement_rank1.npy", "velocity_rank1.npy"]
    idx = ga["displacement.npy"].astype(np.int64)  # arange * 1: the kept DOFs themselves (n < 2^24)
    assert idx.size < n and np.all(np.diff(idx) > 0)
    assert np.array_equal(ga["velocity.npy"], 2.0 * ga["displacement.npy"])  # the same DOFs of every field
    for f in ga:
        assert ga[f].dtype == np.float32
        assert np.array_equal(ga[f], gb[f.replace(".npy", "_rank1.npy")])  # and in every run


def test_steps_must_be_positive(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    args = bench.parse()
    assert (args.steps, args.warmup, args.full, args.dump_outputs) == (7, 3, False, None)
