"""CPU: the surface of the pruned live lattices (wfst_decoder_set_live_lattice_prune / wfst_decoder_get_live_lattice_prune): the header,
the binding's symbol list and the library agree on the two names; the argument checks that need no device; the entry points are a
translation unit of their own, listed in build.SRCS; the snapshot's launch sits inside launch_lattice_emit, so wfst_capi.cc names no
launch wrapper it did not name before (tests/hip_double/fake_hip.cc doubles exactly those: tests/test_host_ownership.py shows it by
passing unchanged)."""
import ctypes
import importlib
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["wfst_decoder_set_live_lattice_prune", "wfst_decoder_get_live_lattice_prune"]
CSRC = os.path.join(ROOT, "asr-decoder_amd", "csrc")


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module("asr-decoder_amd")
    p.build.build()
    return p


def test_header_binding_and_library_agree(pkg):
    src = open(os.path.join(ROOT, "include", "wfst_decoder.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(wfst_[a-z0-9_]+)\s*\(", src))
    lib = ctypes.CDLL(pkg.wfstdec.LIB_PATH)
    for name in NAMES:
        assert name in declared, name
        assert name in pkg.wfstdec.SYMBOLS, name
        assert hasattr(lib, name), name
    for method in ("set_live_lattice_prune", "live_lattice_prune"):
        assert callable(getattr(pkg.wfstdec.BatchDecoder, method)), method


def test_header_cites_the_reference_and_says_what_differs():
    src = open(os.path.join(ROOT, "include", "wfst_decoder.h")).read()
    block = src[src.index("pruned live lattices"):src.index("int wfst_decoder_get_live_lattice_prune")]
    for cite in ("online-decoder-base-inl.h:725-847", "kaldi-online-nnet3-my-decoder.cc:50-89", "determinizes the UNPRUNED live lattice",
                 "WFST_E_STATE", "WFST_E_ARG"):
        assert cite in block, cite


def test_argument_checks_without_a_device(pkg):
    L = pkg.wfstdec.lib()
    assert L.wfst_decoder_set_live_lattice_prune(None, 1) == -1
    assert b"NULL decoder" in L.wfst_last_error()
    m, b = ctypes.c_int32(7), ctypes.c_int64(7)
    assert L.wfst_decoder_get_live_lattice_prune(None, ctypes.byref(m), ctypes.byref(b)) == -1
    assert b"NULL decoder" in L.wfst_last_error()
    assert (m.value, b.value) == (7, 7)


def _launch_wrappers(text):
    return set(re.findall(r"\b(launch_[a-z0-9_]+|prune_raw_[a-z_]+|insert_kernel_set_lds|words_chain_lds)\s*\(", text))


def test_the_entry_points_are_a_translation_unit_of_their_own(pkg):
    unit = os.path.join(CSRC, "wfst_capi_liveprune.cc")
    assert unit in pkg.build.SRCS and os.path.join(CSRC, "wfst_capi_liveprune.h") in pkg.build.HDRS
    text = open(unit).read()
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, text, flags=re.M), name
        assert not re.search(r"^int %s\(" % name, open(os.path.join(CSRC, "wfst_capi.cc")).read(), flags=re.M), name
    assert not _launch_wrappers(text)   # the setter launches nothing: the mode is two fields of the DecoderDev the launches are handed


def test_wfst_capi_names_no_new_launch_wrapper():
    """every launch wrapper wfst_capi.cc calls is one the double of the HIP side (tests/hip_double/fake_hip.cc) defines; the snapshot's
    kernel is launched by launch_lattice_emit, keyed by DecoderDev::live_prune / snap_extra"""
    used = _launch_wrappers(open(os.path.join(CSRC, "wfst_capi.cc")).read())
    doubled = _launch_wrappers(open(os.path.join(ROOT, "tests", "hip_double", "fake_hip.cc")).read())
    assert used and used <= doubled, sorted(used - doubled)
    kern = open(os.path.join(CSRC, "wfst_kernels.hip")).read()
    emit = kern[kern.index("void launch_lattice_emit(const DecoderDev &D, const int32_t *chans, int n, int use_final, hipStream_t s) {"):]
    emit = emit[:emit.index("\n}\n")]
    assert "lattice_snapshot_kernel" in emit and "D.live_prune" in emit and "D.snap_extra" in emit
    assert "lattice_snapshot_kernel" not in open(os.path.join(CSRC, "wfst_capi.cc")).read()
    dev = open(os.path.join(CSRC, "wfst_device.h")).read()
    assert "launch_lattice_snapshot" not in dev and "int32_t live_prune;" in dev and "uint2 *snap_extra;" in dev
