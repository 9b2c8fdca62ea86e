"""CPU: what the compiler makes of the kernels of wfst_graphpost.hip, read from hipcc's kernel-resource-usage remarks
(asr-decoder_amd/build.py: kernel_resources(source=...), the library's own flags, device code only; no GPU needed).

graphpost_kernel's dependent chain per frame and level is LDS read -> log-sum -> barrier: a spilled vector register or a byte of
scratch would put HBM round trips into it.  The figures are those of the finished build (profiles/graphpost_kernel_resources.txt): the
two float64 rows and the staged scores in static LDS, inside the 64 KiB a workgroup gets without opting in to more."""
import importlib
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# lds bytes, scratch bytes per lane, vgpr_spill, occupancy in waves per SIMD
PINNED = {"graphpost_kernel": (40960, 0, 0, 4), "graphpost_pack_kernel": (1024, 0, 0, 8), "graphpost_dense_kernel": (0, 0, 0, 8)}


@pytest.fixture(scope="module")
def usage():
    build = importlib.import_module("asr-decoder_amd").build
    return build.kernel_resources(source=os.path.join(ROOT, "asr-decoder_amd", "csrc", "wfst_graphpost.hip"))


@pytest.mark.parametrize("name", sorted(PINNED))
def test_the_kernels_keep_their_footprint(usage, name):
    lds, scratch, vgpr_spill, occupancy = PINNED[name]
    assert name in usage, sorted(usage)
    u = usage[name]
    print(name, u)
    assert u["lds"] == lds and u["lds"] <= 65536
    assert u["scratch"] == scratch == 0
    assert u["vgpr_spill"] == vgpr_spill == 0
    assert u["occupancy"] >= occupancy


def test_the_pinned_figures_are_the_recorded_ones():
    text = open(os.path.join(ROOT, "profiles", "graphpost_kernel_resources.txt")).read()
    for name, (lds, scratch, vgpr_spill, occupancy) in PINNED.items():
        line = [x for x in text.splitlines() if x.startswith(name + " ")]
        assert len(line) == 1, name
        for part in ("lds=%d" % lds, "scratch=%d" % scratch, "vgpr_spill=%d" % vgpr_spill, "occupancy=%d" % occupancy):
            assert part in line[0].split(), (name, part)
