"""CPU: what the compiler makes of the two kernels of the headline step, read from hipcc's kernel-resource-usage remarks
(asr-decoder_amd/build.py: kernel_resources(), the library's own flags, device code only; no GPU needed).

The bounds are those of a compute unit shared by both kernels (512 VGPRs per SIMD lane, 160 KB of LDS): an insert workgroup is
two waves per SIMD of at most 80 registers, an expansion workgroup one wave per SIMD; at no more than 96 registers 1 insert + 3
expansion workgroups take 448 registers and 2 + 2 take 512, and four expansion images of at most 40 960 bytes are a CU's LDS.
A spilled register is 0.2 ms per step (NOTES.md), so neither kernel may spill or use scratch.  An edit that loses one of these
loses a workgroup per CU without any test of results noticing."""
import importlib

import pytest


@pytest.fixture(scope="module")
def usage():
    return importlib.import_module("asr-decoder_amd").build.kernel_resources()


@pytest.mark.parametrize("kernel,max_vgprs", [("expand_kernel_staged_row", 96), ("insert_kernel_fused", 80)])
def test_headline_kernels_keep_their_residency(usage, kernel, max_vgprs):
    assert kernel in usage, sorted(usage)
    u = usage[kernel]
    print(kernel, u)
    assert u["vgpr_spill"] == 0
    assert u["scratch"] == 0
    assert u["vgprs"] + u["agprs"] <= max_vgprs
    assert u["lds"] <= 40960
