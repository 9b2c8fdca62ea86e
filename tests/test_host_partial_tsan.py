"""GpuChannelPool's partial-words request kind (asr-decoder_amd/host/wfst-host.cc) under ThreadSanitizer, without a device: the pool,
its batcher thread and N x GpuLatticeDecoder(pool) over a TEST DOUBLE of the C ABI (tests/partial_double/fake_partial.cc: the
double of tests/pool_double plus the partial halves, whose words derive from the channel and its frame count).  Worker threads ask
for their partial words between chunks: every request is answered with its own channel's words at its own frame count, the batcher
issues at most one wfst_decoder_partial_enqueue per pass and never a second while one is outstanding, it batches, a misuse comes back
to the misusing thread alone, and the sanitizer has nothing to say.  Also: the CLI's usage text names --partial-words."""
import os
import platform
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = os.path.join(ROOT, "tests", "partial_double")


@pytest.fixture(scope="module")
def partial_tsan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tsan") / "partial_tsan")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-g", "-pthread", "-fsanitize=thread", os.path.join(D, "partial_tsan_main.cc"),
                           os.path.join(D, "fake_partial.cc"), os.path.join(ROOT, "asr-decoder_amd", "host", "wfst-host.cc"), "-o", exe,
                           "-Wl,--unresolved-symbols=ignore-all"], stderr=subprocess.DEVNULL)
    return exe


def _run(args):
    """(setarch -R: ThreadSanitizer's fixed shadow layout and randomised mmap do not always agree, see test_host_pool_tsan.py)"""
    pre = ["setarch", platform.machine(), "-R"] if shutil.which("setarch") else []
    return subprocess.run(pre + args, capture_output=True, text=True, timeout=300,
                          env=dict(os.environ, TSAN_OPTIONS="halt_on_error=0:second_deadlock_stack=1"))


@pytest.mark.parametrize("threads,utts", [(16, 96), (3, 20), (1, 5)])
def test_partial_requests_are_batched_without_races(partial_tsan, threads, utts):
    p = _run([partial_tsan, str(threads), str(utts)])
    assert "ThreadSanitizer" not in p.stderr, p.stderr[-3000:]
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr[-1500:])
    out = dict(zip(p.stdout.split()[0::2], p.stdout.split()[1::2]))
    assert out["bad"] == "0" and out["misuse_caught"] == "1"
    assert out["fake_overlapping"] == "0" and int(out["max_per_pass"]) <= 1
    # every request reached the double (the misuse probe's list was refused before it counted)
    assert int(out["asked"]) > 0 and int(out["partial_requests"]) >= int(out["asked"])
    if threads >= 8:
        assert int(out["partial_requests"]) >= 2 * int(out["fake_enqueues"])   # it batched


def test_cli_usage_names_partial_words():
    host = os.path.join(ROOT, "asr-decoder_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host])
    p = subprocess.run([os.path.join(host, "wfst-decode")], capture_output=True, text=True)
    assert p.returncode == 1 and "--partial-words" in p.stderr
