"""-m gpu: what a plain `bench.py` run does and what --full adds, on a small configuration.  A plain run times the steps, writes
--dump-outputs and prints the line -- the contract's keys and the decoder's own counters, no roofline, CPU baseline, parity or legs --
and no detail file unless asked for one; --full adds the checks and measurements on top of the same timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "6", "--frames", "60", "--states", "20000", "--pdfs", "1000"]


def _run(args, cwd):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + args, capture_output=True, text=True, timeout=600, cwd=cwd)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_plain_run_is_the_headline_only(tmp_path):
    d = _run(["--dump-outputs", str(tmp_path / "dump")], str(tmp_path))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus"):
        assert k in d, k
    assert d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"] == "f32" and d["steps"] == 2 and d["warmup"] == 1
    assert abs(d["value"] - 6 * 60 * 2 / (2e-3 * d["ms_per_step"])) / d["value"] < 1e-6   # frames / timed seconds
    assert d["config"]["global_batch"] == 6
    for k in ("roofline", "cpu_baseline", "legs", "detail"):
        assert k not in d, k
    assert "parity" not in d["config"]
    ok = np.load(str(tmp_path / "dump" / "ok.npy"))
    assert ok.shape == (6,) and ok.sum() == d["config"]["utterances_with_path"] > 0


def test_full_run_adds_the_checks(tmp_path):
    detail = str(tmp_path / "detail.json")
    d = _run(["--full", "--no-legs", "--no-service-point", "--no-traffic", "--cpu-sample", "6", "--no-cpu-baseline", "--detail-out", detail],
             str(tmp_path))
    assert d["config"]["parity"] == "6/6" and d["roofline"]["kernel"].endswith("_kernel") and d["roofline"]["profiled_step_ms"] > 0
    assert d["detail"] == "detail.json"
    with open(detail) as f:
        full = json.load(f)
    assert full["config"]["work_counts_sample"]["gpu"]["N"] > 0
