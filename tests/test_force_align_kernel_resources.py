"""CPU: what the compiler makes of forced_align_kernel (wfst_forced.hip), read from hipcc's kernel-resource-usage remarks
(asr-decoder_amd/build.py: kernel_resources(source=...), the library's own flags, device code only; no GPU needed).

The kernel's dependent chain per frame is LDS read -> min -> barrier: a spilled vector register or a byte of scratch would put HBM
round trips into it.  The figures are those of the finished build (profiles/forced_kernel_resources.txt): the two cost rows and the
staged scores in static LDS, inside the 64 KiB a workgroup gets without opting in to more, and the waves per SIMD that LDS leaves."""
import importlib
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# lds bytes, scratch bytes per lane, vgpr_spill, occupancy in waves per SIMD
PINNED = {"forced_align_kernel": (40960, 0, 0, 4)}


@pytest.fixture(scope="module")
def usage():
    build = importlib.import_module("asr-decoder_amd").build
    return build.kernel_resources(source=os.path.join(ROOT, "asr-decoder_amd", "csrc", "wfst_forced.hip"))


def test_forced_align_kernel_keeps_its_footprint(usage):
    lds, scratch, vgpr_spill, occupancy = PINNED["forced_align_kernel"]
    assert "forced_align_kernel" in usage, sorted(usage)
    u = usage["forced_align_kernel"]
    print(u)
    assert u["lds"] == lds and u["lds"] <= 64 * 1024
    assert u["scratch"] == scratch
    assert u["vgpr_spill"] == vgpr_spill
    assert u["occupancy"] >= occupancy


def test_the_pinned_figures_are_the_recorded_ones():
    text = open(os.path.join(ROOT, "profiles", "forced_kernel_resources.txt")).read()
    lds, scratch, vgpr_spill, occupancy = PINNED["forced_align_kernel"]
    assert "forced_align_kernel" in text
    for part in ("lds=%d" % lds, "scratch=%d" % scratch, "vgpr_spill=%d" % vgpr_spill, "occupancy=%d" % occupancy):
        assert part in text, part
