"""GpuChannelPool's kNbestWords request (asr-decoder_amd/host/wfst-host.cc) under ThreadSanitizer, without a device: the pool, its
batcher thread and N x GpuLatticeDecoder(pool) linked against a double of the C ABI of their own (tests/nbwords_double/: the pool's
double plus wfst_decoder_get_nbest_words, which echoes the channel, its frames and the question asked).  Threads ask GetNbestWords
after every chunk with two different questions: every answer is the asking thread's own, the batcher issues one call per question and
pass (fewer calls than requests), and the sanitizer has nothing to say."""
import os
import platform
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = os.path.join(ROOT, "tests", "nbwords_double")


@pytest.fixture(scope="module")
def nbwords_tsan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tsan") / "nbwords_tsan")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-g", "-pthread", "-fsanitize=thread", os.path.join(D, "nbwords_tsan_main.cc"),
                           os.path.join(D, "fake_wfstdec_nbwords.cc"), os.path.join(ROOT, "asr-decoder_amd", "host", "wfst-host.cc"), "-o", exe,
                           "-Wl,--unresolved-symbols=ignore-all"], stderr=subprocess.DEVNULL)
    return exe


def _run(args):
    pre = ["setarch", platform.machine(), "-R"] if shutil.which("setarch") else []
    return subprocess.run(pre + args, capture_output=True, text=True, timeout=300,
                          env=dict(os.environ, TSAN_OPTIONS="halt_on_error=0:second_deadlock_stack=1"))


@pytest.mark.parametrize("threads,utts", [(16, 64), (3, 12), (1, 4)])
def test_pool_groups_nbest_words_requests_without_races(nbwords_tsan, threads, utts):
    p = _run([nbwords_tsan, str(threads), str(utts)])
    assert "ThreadSanitizer" not in p.stderr, p.stderr[-3000:]
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr[-1500:])
    out = dict(zip(p.stdout.split()[0::2], p.stdout.split()[1::2]))
    assert out["bad"] == "0" and out["asked"] == out["requests"] == out["fake_channels"] and out["calls"] == out["fake_calls"]
    if threads >= 8:
        assert int(out["calls"]) < int(out["requests"])
