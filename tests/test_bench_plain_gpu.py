"""`bench.py --gpus 1` without --full (-m gpu): the headline alone -- one JSON line with the contract keys, the roofline
quoted beside them, the dumped outputs when asked, and none of what only --full measures or checks (the parity check, the
CPU baselines, config.others, host_to_host, the sustained loop, the side file)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_plain_bench_run_is_the_headline_alone(gpu_lib, tmp_path):
    dump = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--dump-outputs", str(dump)]
    try:
        res = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    except subprocess.TimeoutExpired:
        pytest.fail("bench.py --gpus 1 did not finish within 300 s")
    assert res.returncode == 0, res.stderr[-1500:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-1500:]
    line = json.loads(lines[0])
    assert line["unit"] == "frames/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1 and line["value"] > 0
    frames = (3600 * 16000 - 800) // 400 + 1
    assert line["config"]["frames_per_step_job"] == frames and line["config"]["kernel"] == "st_fast_800_w8"
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 / frames - 1.0) < 1e-3
    assert line["roofline"]["kernel_avg_ms"] > 0
    for key in ("parity_check", "cpu_baseline", "host_to_host", "sustained", "full_record"):
        assert key not in line, key
    assert "others" not in line["config"] and list(line["configs"]) == ["cfg2"]
    assert not list(tmp_path.glob("bench_full_n*.json"))
    F = np.load(dump / "features.npy")
    idx = np.load(dump / "frame_index.npy")
    assert F.shape[0] == 34 and F.shape[1] == idx.shape[0] and np.all(np.isfinite(F))
