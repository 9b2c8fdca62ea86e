"""CPU: how the word queries (wfst_decoder_align_words, wfst_decoder_nearest_words, wfst_decoder_word_confidence) cut their channels
into rounds under a cell budget -- cut_round of asr-decoder_amd/csrc/wfst_capi_align.h, the one piece of their shared driver that no GPU
test reaches: the budgets are 32 Mi and 64 Mi cells, and every call the suite makes is one round.

tests/hip_double/rounds_main.cc is a program of its own that includes the header and calls the function; it is built with g++ under
AddressSanitizer + UBSan and run as an executable.  It holds the function to a restatement of the rule and to the rule's properties
(every runnable entry in exactly one round, in order; the others in none; no empty round; a round over the budget has one member; the
driver's loop ends on an all-skipped tail) for: empty input, nothing runnable, one entry over the budget alone, such an entry between
small ones, entries that fill the budget exactly and by one cell too many, zero-cell entries, skipped entries, and 400 random vectors
with budgets from 1 to their total."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1")


def _hip_include():
    for d in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"), "/opt/rocm/include"):
        if os.path.exists(os.path.join(d, "hip", "hip_runtime.h")):
            return d
    raise RuntimeError("hip/hip_runtime.h not found (ROCM_PATH)")


def test_round_cutting_follows_its_rule(tmp_path):
    exe = str(tmp_path / "rounds_main")
    subprocess.check_call(["g++", "-std=c++17"] + SAN + ["-D__HIP_PLATFORM_AMD__", "-I" + _hip_include(),
                                                         "-I" + os.path.join(ROOT, "asr-decoder_amd", "csrc"),
                                                         os.path.join(ROOT, "tests", "hip_double", "rounds_main.cc"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, env=ENV, timeout=60)
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    assert p.returncode == 0, (p.returncode, p.stdout[-3000:], p.stderr[-1500:])
    m = re.search(r"^rounds ok (\d+) (\d+)$", p.stdout, flags=re.M)
    assert m, p.stdout[-3000:]
    # the 13 cases by hand and 400 x 6 random ones; more than one round each on average (the budgets do cut)
    assert int(m.group(1)) == 13 + 400 * 6 and int(m.group(2)) > int(m.group(1))

