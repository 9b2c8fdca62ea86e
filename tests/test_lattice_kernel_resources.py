"""CPU: what the compiler makes of the lattice-query kernels that share wfst_lattice_sweep.h (the levelled sweep, the log-sum, the
block primitives, the frame-class reduction), read from hipcc's kernel-resource-usage remarks (asr-decoder_amd/build.py:
kernel_resources(source=...), the library's own flags, device code only; no GPU needed).

The figures are those of the kernels as they stood before they shared that header, each with its own copy of every piece
(profiles/lattice_kernel_resources.txt).  A shared template must not cost a kernel what its own copy did not: no more LDS, no more
scratch, no spilled vector register more, and no wave per SIMD less.  Register counts may move inside that."""
import importlib
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# kernel: (source, lds bytes, scratch bytes per lane, vgpr_spill, occupancy in waves per SIMD)
PINNED = {
    "posterior_kernel": ("wfst_posterior.hip", 4352, 36, 0, 7),
    "confidence_kernel": ("wfst_posterior.hip", 49160, 0, 0, 8),
    "seqpost_kernel": ("wfst_seqpost.hip", 41216, 0, 0, 5),
    "slot_mass_kernel": ("wfst_altern.hip", 40968, 0, 0, 8),
    "slot_none_kernel": ("wfst_altern.hip", 41216, 0, 0, 6),
    "frame_post_kernel": ("wfst_framepost.hip", 15360, 0, 0, 7),
    "frame_pack_kernel": ("wfst_framepost.hip", 1024, 0, 0, 8),
    "acc_kernel": ("wfst_seqstat.hip", 16896, 0, 0, 7),
    "seqstat_frame_kernel": ("wfst_seqstat.hip", 25600, 0, 0, 6),
    "seqstat_pack_kernel": ("wfst_seqstat.hip", 1024, 0, 0, 8),
    "seqstat_dense_kernel": ("wfst_seqstat.hip", 0, 0, 0, 8),
}


@pytest.fixture(scope="module")
def usage():
    build = importlib.import_module("asr-decoder_amd").build
    out = {}
    for src in sorted({v[0] for v in PINNED.values()}):
        out.update(build.kernel_resources(source=os.path.join(ROOT, "asr-decoder_amd", "csrc", src)))
    return out


@pytest.mark.parametrize("kernel", sorted(PINNED))
def test_lattice_kernels_keep_their_footprint(usage, kernel):
    _, lds, scratch, vgpr_spill, occupancy = PINNED[kernel]
    assert kernel in usage, sorted(usage)
    u = usage[kernel]
    print(kernel, u)
    assert u["lds"] <= lds
    assert u["scratch"] <= scratch
    assert u["vgpr_spill"] <= vgpr_spill
    assert u["occupancy"] >= occupancy
