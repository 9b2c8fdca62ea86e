"""CPU: the host side of wfst_decoder_set_live_lattice_prune / _get_live_lattice_prune without a device -- the real wfst_capi.cc,
wfst_capi_liveprune.cc and wfst_openfst.cc linked against the test double of the HIP runtime (tests/hip_double/fake_hip.cc, unchanged:
wfst_capi.cc calls no launch wrapper the double lacks) and run under AddressSanitizer + UBSan by a stand-alone program
(tests/hip_double/liveprune_main.cc): argument and state errors, the scratch allocated once by the first mode 1 and owned by the
decoder (8 bytes x arena_tokens x channels, one device buffer more, the same one after 1 -> 0 -> 1, given back with the decoder), a
failed allocation returned with the mode left at 0 and nothing held, FinalizeDecoding in mode 1."""
import os
import subprocess

from test_host_ownership import ENV, ROOT, SAN, _hip_include


def test_live_prune_scratch_is_owned_and_a_failed_allocation_leaves_mode_0(tmp_path):
    exe = str(tmp_path / "liveprune_main")
    csrc = os.path.join(ROOT, "asr-decoder_amd", "csrc")
    dbl = os.path.join(ROOT, "tests", "hip_double")
    subprocess.check_call(["g++", "-std=c++17"] + SAN + ["-D__HIP_PLATFORM_AMD__", "-I" + _hip_include(),
                                                         os.path.join(csrc, "wfst_capi.cc"), os.path.join(csrc, "wfst_capi_liveprune.cc"),
                                                         os.path.join(csrc, "wfst_openfst.cc"), os.path.join(dbl, "fake_hip.cc"),
                                                         os.path.join(dbl, "liveprune_main.cc"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, env=ENV, timeout=300)
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr and "FAKE HIP" not in p.stderr, p.stderr[-3000:]
    assert p.returncode == 0 and "failed 0" in p.stdout and "FAILED" not in p.stdout, (p.returncode, p.stdout, p.stderr[-1500:])
    assert p.stdout.count("\nok ") + p.stdout.startswith("ok ") >= 19, p.stdout
