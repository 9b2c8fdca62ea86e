"""bench.py's final stdout line: strict JSON, under 4 KB, the contract's keys, scalars only per leg (round 4's
29 KB line was not parsed by the driver).  Fed with a full result of the shape main() builds -- round 4's own, re-nested."""
import importlib.util
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _canned():
    with open(os.path.join(ROOT, "profiles", "r04_default_bench_line.json")) as f:
        o = json.load(f)
    legs = {}
    for k in ("biglm", "lattice_beam13", "lattice_beam15_no_determinizer", "lattice_beam15", "lattice_beam15_pipelined"):
        legs[k] = o.pop(k)
    sp = o["service_point"]
    legs["service_point_7000_200"] = {k: v for k, v in sp.items() if not k.endswith("_at_7000_200")}
    legs["calibrated_7000_200"] = sp["calibrated_workload_at_7000_200"]
    legs["headline_at_7000_200"] = sp["headline_workload_at_7000_200"]
    legs["reference_default_limits"] = o.pop("reference_default_limits")
    legs["biglm"]["cpu_baseline"] = dict(o["cpu_baseline"], determinizer_ms_per_lattice=np.float64(41.25))
    legs["broken"] = {"error": "TimeoutExpired(" + "x" * 500 + ")", "stderr_tail": "y" * 600}
    o["legs"] = legs
    o["roofline"]["profiled_step_ms"] = np.float32(19.5)
    o["config"]["mean_active_tokens_per_frame"] = float("nan")   # must not reach the line as NaN
    return o


def _strict(line):
    def no_constants(x):
        raise ValueError("non-finite constant %s in the bench line" % x)

    return json.loads(line, parse_constant=no_constants)


def test_line_is_small_strict_json():
    b = _bench()
    line = b.summary_line(_canned(), "bench_detail.json")
    assert "\n" not in line
    assert len(line.encode()) < 4096
    d = _strict(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert isinstance(d["config"]["workload"], str) and "model" not in d["config"]
    for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "algorithmic_bytes_per_launch", "avg_launch_ms", "whole_path_frac",
              "profiled_step_ms"):
        assert k in d["roofline"], k
    assert abs(d["roofline"]["frac"] - d["roofline"]["achieved"] / d["roofline"]["peak"]) < 1e-5
    for k in ("value", "unit", "cores", "kind", "single_thread_value", "cpu_model", "sample"):
        assert k in d["cpu_baseline"], k
    scalar = (int, float, str, bool, type(None))
    for part in ("config", "roofline", "cpu_baseline"):
        assert all(isinstance(v, scalar) for v in d[part].values()), part
    assert set(d["legs"]) >= {"biglm", "lattice_beam15", "lattice_beam15_pipelined", "calibrated_7000_200"}
    for name, leg in d["legs"].items():
        assert all(isinstance(v, scalar) for v in leg.values()), name
    assert d["legs"]["biglm"]["cpu_baseline_value"] > 0 and d["legs"]["biglm"]["parity"] == "8/8"
    assert d["legs"]["calibrated_7000_200"]["bit_identical"] == "112/128"
    assert "error" in d["legs"]["broken"] and len(d["legs"]["broken"]["error"]) <= 120
    assert "mean_active_tokens_per_frame" not in d["config"]   # NaN dropped, not printed


def test_line_shrinks_instead_of_overflowing():
    b = _bench()
    o = _canned()
    for i in range(40):   # many more legs than the real run has
        o["legs"]["extra_%d" % i] = dict(o["legs"]["lattice_beam15"])
    line = b.summary_line(o, "bench_detail.json")
    assert len(line.encode()) < 4096
    _strict(line)
    o["legs"].update({"filler_%d" % i: dict(o["legs"]["lattice_beam15"]) for i in range(400)})
    line = b.summary_line(o, None)   # (never refuses to print: drops legs from the line, says how many)
    assert len(line.encode()) < 4096
    d = _strict(line)
    assert d["legs_dropped_from_line"] > 0 and "biglm" in d["legs"] and "roofline" in d and "cpu_baseline" in d


def test_detail_file_is_strict_json(tmp_path):
    b = _bench()
    p = str(tmp_path / "detail.json")
    assert b.write_detail(_canned(), p) == p
    with open(p) as f:
        d = _strict(f.read())
    assert d["legs"]["biglm"]["roofline"]["kernel"].endswith("_kernel")
    assert d["config"]["mean_active_tokens_per_frame"] is None


def test_traffic_is_per_launch_of_this_run():
    """the line's traffic over its algorithmic bytes per launch must be the counter passes' bytes per whole-batch
    launch over the algorithmic whole-batch bytes (round 5's was 2x that: the child pass ran two steps, its launches were taken for one
    step's).  Canned: round 5's own figures -- one-group child, 300 expansion launches of 109.4 MB per step; the run: three channel
    groups, 900 launches per step, 47.45 MB algorithmic per whole-batch launch."""
    b = _bench()
    child_bpl, child_lps, run_lps = 109435074.45, 300, 900
    alg_whole_batch = 47.45e6
    alg_per_launch = alg_whole_batch * child_lps / run_lps
    t = b.traffic_per_launch(child_bpl, child_lps, run_lps)
    assert abs(t / alg_per_launch - child_bpl / alg_whole_batch) < 1e-9
    assert abs(t / alg_per_launch - 2.306) < 0.01
    # the stored passes of the rounds before ran two steps ("launches"); since round 6 they store launches_per_step
    assert b.stored_launches_per_step({"launches": {"expand": 600}}, "expand", 900) == 300
    assert b.stored_launches_per_step({"launches_per_step": {"expand": 300}}, "expand", 900) == 300
    o = _canned()
    o["roofline"]["traffic"] = t
    o["roofline"]["algorithmic_bytes_per_launch"] = alg_per_launch
    o["roofline"]["traffic_over_algorithmic"] = t / alg_per_launch
    d = _strict(b.summary_line(o, None))
    assert abs(d["roofline"]["traffic"] / d["roofline"]["algorithmic_bytes_per_launch"] - child_bpl / alg_whole_batch) < 1e-3
    assert abs(d["roofline"]["traffic_over_algorithmic"] - 2.306) < 0.01


def test_metric_is_short():
    b = _bench()
    o = _canned()
    o["metric"] = "m" * 300
    assert len(_strict(b.summary_line(o, None))["metric"]) <= 100


def test_gpus_n_launches_its_own_ranks(monkeypatch, capsys):
    """VERDICT r5 missing #1: `python bench.py --gpus 8` with no rank environment starts torch.distributed.run itself, as a child
    process, before torch is imported; relays rank 0's JSON line as the last stdout line and exits with the child's code."""
    import subprocess
    import sys
    import types

    b = _bench()
    seen = {}

    class FakePopen:
        def __init__(self, cmd, stdout=None, env=None):
            seen["cmd"], seen["env"] = cmd, env
            self.stdout = [b"[rank 0] some log\n", b'{"metric":"m","value":1.0,"n_gpus":8}\n']

        def wait(self):
            return 0

    monkeypatch.setattr(subprocess, "Popen", FakePopen)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "8", "--steps", "3", "--warmup", "1"])
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    before = "torch" in sys.modules
    with pytest.raises(SystemExit) as e:
        b.main()
    assert e.value.code == 0
    assert ("torch" in sys.modules) == before   # the parent did not import torch on the way
    cmd = seen["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node" in cmd and cmd[cmd.index("--nproc-per-node") + 1] == "8"
    assert "--master-addr" in cmd and cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-6:] == ["--gpus", "8", "--steps", "3", "--warmup", "1"] and cmd[-7].endswith("bench.py")
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0" or "HSA_ENABLE_IPC_MODE_LEGACY" in os.environ
    out = capsys.readouterr().out.strip().splitlines()
    assert json.loads(out[-1])["n_gpus"] == 8 and len(out) == 1


def test_plain_run_line(monkeypatch):
    """A plain run (no --full) fills the contract's keys and its own counters only: the line then carries no roofline, CPU baseline,
    legs or detail file, and is still strict JSON."""
    import sys

    b = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = b.parse()
    assert a.full is False and a.work_dir == ""
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full"])
    assert b.parse().full is True
    o = _canned()
    plain = {k: o[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                               "vs_baseline", "dtype", "data")}
    plain["config"] = {k: o["config"][k] for k in ("workload", "global_batch", "frames_per_utt", "rtfx", "utterances_with_path")}
    d = _strict(b.summary_line(plain, None))
    assert d["value"] == o["value"] and d["ms_per_step"] == o["ms_per_step"] and d["unit"] == "frames/s" and d["higher_is_better"] is True
    assert d["config"]["global_batch"] == o["config"]["global_batch"]
    for k in ("roofline", "cpu_baseline", "legs", "detail"):
        assert k not in d, k
