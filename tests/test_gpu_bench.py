"""bench.py itself on the GPU box: the N > 1 path (one process per rank, row gather every step, max-over-ranks timing, rank 0's JSON
line) must not rot before its first real 8-GPU run.  Two ranks share the one card of the box under SOFTSPOKEN_DIST_BACKEND=gloo
(RCCL wants one device per rank); the device work per rank is the single-GPU step.  A plain run (no --full) times the steps and
nothing else, and --dump-outputs writes what its last step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args, env=None, timeout=900):
    e = dict(os.environ)
    e.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    e.update(env or {})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], cwd=ROOT, env=e, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.stdout[-800:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]                   # ONE JSON line, from rank 0
    return json.loads(lines[0])


def test_bench_two_ranks_on_one_card(build_all):
    common = ["--files", "4", "--steps", "1", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-secondary"]
    one = _bench("--gpus", "1", *common)
    assert one["n_gpus"] == 1 and one["config"]["rccl_world_size"] == 1 and one["value"] > 0 and one["rows_last_step"] > 0
    assert one["roofline"]["frac"] > 0 and one["roofline"]["kernel"].startswith("conv3x3")
    assert one["roofline"]["mfma"]["issued_tflops"] >= one["roofline"]["mfma"]["achieved_tflops_algorithmic"]
    # the traffic figure is either measured for exactly this kernel at this duration, or null with the reason beside it
    ts = one["roofline"]["traffic_source"]
    assert (one["roofline"]["traffic"] is None) == ("traffic_null_because" in ts)
    two = _bench("--gpus", "2", *common, env={"SOFTSPOKEN_DIST_BACKEND": "gloo"})
    assert two["n_gpus"] == 2 and two["config"]["rccl_world_size"] == 2 and two["config"]["backend"] == "gloo"
    assert two["scaling"] == "weak" and two["steps"] == 1 and two["warmup"] == 1
    assert two["rows_last_step"] == 2 * one["rows_last_step"]  # every rank's rows reach rank 0 (weak scaling: each has its own 4 files)
    assert two["value"] > 0 and two["config"]["windows_per_step_per_gpu"] == one["config"]["windows_per_step_per_gpu"]


def test_bench_plain_run_dumps_what_the_full_run_computes(build_all, tmp_path):
    args = ["--gpus", "1", "--files", "4", "--steps", "2", "--warmup", "1"]
    plain = _bench(*args, "--dump-outputs", str(tmp_path / "plain"))
    assert plain["full"] is False and plain["steps"] == 2 and plain["warmup"] == 1 and plain["value"] > 0 and plain["ms_per_step"] > 0
    assert plain["unit"] == "audio-seconds/s" and plain["higher_is_better"] is True and plain["dtype"] == "f16x2"
    assert all(plain[k] is None for k in ("roofline", "stft_stage", "cpu_baseline", "secondary", "kernels", "layers"))
    full = _bench(*args, "--full", "--no-cpu-baseline", "--no-secondary", "--dump-outputs", str(tmp_path / "full"))
    assert full["full"] is True and full["roofline"]["kernel"].startswith("conv3x3")
    total = 0
    for name in ("rows", "window_logits", "avg"):
        got = np.load(str(tmp_path / "plain" / (name + ".npy")))
        total += os.path.getsize(str(tmp_path / "plain" / (name + ".npy")))
        assert got.dtype in (np.float32, np.float64) and got.size > 0 and np.isfinite(got).all(), name
        np.testing.assert_array_equal(got, np.load(str(tmp_path / "full" / (name + ".npy"))), err_msg=name)   # seeded inputs, same outputs
    assert total <= 64 * 10 ** 6
    rows = np.load(str(tmp_path / "plain" / "rows.npy"))
    assert rows.shape == (plain["rows_last_step"], 3) and set(np.unique(rows[:, 0])) <= set(range(4))
    windows = plain["config"]["windows_per_step_per_gpu"]
    assert np.load(str(tmp_path / "plain" / "window_logits.npy")).shape == (min(4096, windows), 256)
