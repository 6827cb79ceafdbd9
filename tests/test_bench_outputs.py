"""bench.py: a plain run prints the headline only, `--full` adds the secondary figures, `--dump-outputs DIR` writes what the last
timed step computed (the same arrays with or without `--full`)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import ROOT

SECONDARY = ("ms_per_step_median_hipevent", "ms_per_step_min_max_hipevent", "host_enqueue_ms_per_step",
             "host_enqueue_ms_per_step_in_region", "roofline", "kernel_classes_ms_per_step", "cpu_baseline")


def test_dump_sample_positions_are_fixed_and_inside_the_trainable_runs():
    sys.path.insert(0, ROOT)
    import bench
    runs = [(0, 10), (64, 70), (128, 1000)]
    every = bench.sample_positions(runs, 10 ** 6)
    assert every.tolist() == list(range(0, 10)) + list(range(64, 70)) + list(range(128, 1000))
    a = bench.sample_positions(runs, 100)
    b = bench.sample_positions(runs, 100)
    assert np.array_equal(a, b) and len(a) == 100 and len(np.unique(a)) == 100 and np.all(np.diff(a) > 0)
    assert all(any(s <= p < e for s, e in runs) for p in a.tolist())
    assert bench.DUMP_SAMPLE * 4 * 2 <= 64 << 20          # parameters + gradients, float32, within the 64 MB budget


def _bench(tmp_path, name, extra):
    out = str(tmp_path / name)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--layers", "50",
           "--size", "256", "--batch", "4", "--dump-outputs", out] + extra
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert res.returncode == 0, "bench.py %s failed (rc %d):\n%s" % (" ".join(extra), res.returncode, res.stderr[-3000:])
    lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, res.stdout[-2000:]
    arrays = {f[:-4]: np.load(os.path.join(out, f)) for f in sorted(os.listdir(out))}
    return json.loads(lines[0]), arrays


@pytest.mark.gpu
def test_plain_line_is_lean_full_line_adds_the_rest_and_both_dump_the_same_last_step(tmp_path):
    plain, dp = _bench(tmp_path, "plain", [])
    full, df = _bench(tmp_path, "full", ["--full", "--no-cpu-baseline", "--instr-steps", "1"])
    for out in (plain, full):
        assert out["steps"] == 3 and out["warmup"] == 1 and out["unit"] == "images/sec" and out["higher_is_better"] is True
        assert out["dtype"] == "bf16" and out["ms_per_step"] > 0 and out["value"] > 0
        assert abs(out["value"] - 4 * 1000.0 / out["ms_per_step"]) <= 1e-2 * out["value"]
    assert not [k for k in SECONDARY if k in plain], plain.keys()
    assert all(k in full for k in SECONDARY if k != "cpu_baseline"), full.keys()
    assert {"loss", "params_sample", "grads_sample", "log_total_loss", "log_heatmap_loss"} <= set(dp)
    assert sorted(dp) == sorted(df)
    assert sum(a.nbytes for a in dp.values()) <= 64 << 20
    for k, a in dp.items():
        assert a.dtype in (np.float32, np.float64) and a.size > 0 and np.isfinite(a).all(), k
        assert np.array_equal(a, df[k]), "%s differs between the plain and the --full run" % k
    for k in ("heatmap_loss", "total_loss"):
        assert round(float(dp["log_" + k][0]), 6) == plain["last_step_log"][k], k
    assert float(dp["loss"][0]) > 0 and np.abs(dp["grads_sample"]).max() > 0
