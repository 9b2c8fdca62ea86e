"""Who owns the HIP resources of the host library (asr-decoder_amd/csrc/wfst_capi.cc), checked without a device: the real wfst_capi.cc
and wfst_openfst.cc are linked against a TEST DOUBLE of the HIP runtime (tests/hip_double/fake_hip.cc: "device" and page-locked memory
from calloc, streams / events / graphs / graph executables as small heap objects, no-op launch wrappers, a live count per kind; a double
free or a handle it never handed out aborts) and run under AddressSanitizer + UBSan by tests/hip_double/own_main.cc.

The sequence, for a 128-channel best-path decoder (three channel groups), a lattice decoder on a stream of its caller's and a biglm
decoder with two tiny LMs, all on a six-state graph with small wfst_limits: create, init, advance calls of 4 and more frames (each a
graph capture per channel group; on the 128-channel decoder more than the 64 executables the cache holds, so it is flushed), finalize,
init again, advance_host with 300 and then 700 frames (the history slab regrows; the lattice decoder's rows are page-locked), finalize,
free of the decoder, the LMs and the graph.  The best-path decoder also makes its lazily created results stream and staging
(best_path_enqueue / _fetch) and its endpoint buffers (set_endpoint_config); what those calls return is not looked at -- the no-op
kernels leave every control block zero, and the double fakes no results.  No call of the issue's sequence had to be dropped.

lifecycle: every live count is zero at the end.  sweep: the k-th creating call (hipMalloc, hipHostMalloc, hipEventCreate*,
hipStreamCreate*, hipGraphInstantiate) fails for k = 1, 2, ... until a run completes unfaulted; every faulted run returns WFST_E_DEVICE
and, once what was handed out is freed, leaves nothing live."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:allocator_may_return_null=1:max_allocation_size_mb=512", UBSAN_OPTIONS="halt_on_error=1")
KINDS = ["best", "lattice", "biglm"]


def _hip_include():
    for d in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"), "/opt/rocm/include"):
        if os.path.exists(os.path.join(d, "hip", "hip_runtime.h")):
            return d
    raise RuntimeError("hip/hip_runtime.h not found (ROCM_PATH)")


@pytest.fixture(scope="module")
def own_main(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("own") / "own_main")
    csrc = os.path.join(ROOT, "asr-decoder_amd", "csrc")
    dbl = os.path.join(ROOT, "tests", "hip_double")
    subprocess.check_call(["g++", "-std=c++17"] + SAN + ["-D__HIP_PLATFORM_AMD__", "-I" + _hip_include(),
                                                         os.path.join(csrc, "wfst_capi.cc"), os.path.join(csrc, "wfst_openfst.cc"),
                                                         os.path.join(dbl, "fake_hip.cc"), os.path.join(dbl, "own_main.cc"), "-o", exe])
    return exe


def _run(exe, mode):
    p = subprocess.run([exe, mode], capture_output=True, text=True, env=ENV, timeout=600)
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr and "FAKE HIP" not in p.stderr, p.stderr[-3000:]
    assert p.returncode == 0, (p.returncode, p.stdout[-3000:], p.stderr[-1500:])
    return p.stdout


def _creating(out):
    got = dict(re.findall(r"^lifecycle (\w+) rc 0 creating (\d+) live 0$", out, flags=re.M))
    assert sorted(got) == sorted(KINDS), out
    return {k: int(v) for k, v in got.items()}


def test_lifecycle_leaves_nothing_live(own_main):
    made = _creating(_run(own_main, "lifecycle"))
    # streams, events and executables beyond the buffers: the 128-channel decoder makes well over a hundred resources
    assert made["best"] > 100 and made["lattice"] > 50 and made["biglm"] > 50


def test_failed_creating_call_leaks_nothing(own_main):
    made = _creating(_run(own_main, "lifecycle"))
    out = _run(own_main, "sweep")
    swept = {k: (int(f), int(l), int(w)) for k, f, l, w in re.findall(r"^sweep (\w+) faulted (\d+) leaks (\d+) wrong_rc (\d+)$", out, flags=re.M)}
    assert sorted(swept) == sorted(KINDS), out
    for kind in KINDS:
        faulted, leaks, wrong_rc = swept[kind]
        assert leaks == 0 and wrong_rc == 0, out[-3000:]
        assert faulted >= made[kind], (kind, faulted, made[kind])   # (the sweep did not end early: it failed every creating call of the sequence)
