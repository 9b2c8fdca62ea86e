"""CPU: the surface of wfst_decoder_graph_posteriors -- the header, the binding's symbol list and the library agree, the header's
constant is the restatement's and the kernel's, the LDS budget holds, and the call refuses NULL arguments before any device."""
import ctypes as C
import importlib
import inspect
import os
import re

import pytest

import graph_post_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1
NAMES = ["wfst_decoder_graph_posteriors", "wfst_decoder_graph_posteriors_workspace"]


@pytest.fixture(scope="module")
def W():
    p = importlib.import_module("asr-decoder_amd")
    p.build.build()
    return p.wfstdec


def test_header_binding_and_library_agree(W):
    hdr = open(os.path.join(ROOT, "include", "wfst_decoder.h")).read()
    lib = C.CDLL(W.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, hdr) and name in W.SYMBOLS and hasattr(lib, name), name
    decl = re.search(r"int wfst_decoder_graph_posteriors\((.*?)\);", hdr, flags=re.S)
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")]
    assert args == ["wfst_decoder *d", "const int32_t *channels", "int32_t n", "const wfst_align_graphs *graphs", "const int32_t *graph_of",
                    "const int32_t *n_frames_in", "const int32_t *label_map", "int32_t n_tid", "double graph_scale", "double acoustic_scale",
                    "double min_post", "int64_t max_cells", "int32_t cap_frames", "int32_t cap_entries", "int32_t cap_arcs",
                    "void *const *grad", "const int64_t *grad_pitch", "const int32_t *grad_frames", "int32_t n_cols", "double grad_scale",
                    "void *consumer_stream", "int32_t *status", "int32_t *found", "int32_t *n_frames", "double *log_like",
                    "int32_t *n_entries", "int32_t *n_arcs", "int32_t *frame_off", "int32_t *n_distinct", "double *frame_mass",
                    "int32_t *entry_class", "double *entry_post", "double *arc_occ"]
    sig = inspect.signature(W.BatchDecoder.graph_posteriors).parameters
    assert list(sig)[:15] == ["self", "graphs", "graph_of", "channels", "n_frames", "label_map", "graph_scale", "acoustic_scale", "min_post",
                              "arc_occupancy", "grad", "grad_scale", "n_cols", "consumer_stream", "max_cells"]
    assert set(W.GraphPosteriors.__slots__) >= {"status", "found", "n_frames", "log_like", "frame_off", "classes", "posts", "n_distinct",
                                                "frame_mass", "arc_occ"}
    # the two older calls point at this one
    assert "Per-arc posteriors of the numerator graph: wfst_decoder_graph_posteriors" in hdr
    assert "The MMI numerator's log-probability: wfst_decoder_graph_posteriors' log_like" in hdr
    for left_out in ("a beam", "add into the rows", "soft-numerator MMI in one call", "half-precision dense output", "graph compilation"):
        assert left_out in hdr[hdr.index("graph posteriors: forward-backward"):hdr.index("#define WFST_GPOST_LDS_STATES")], left_out


def test_the_constant_and_the_lds_budget():
    hdr = open(os.path.join(ROOT, "include", "wfst_decoder.h")).read()
    dev = open(os.path.join(ROOT, "asr-decoder_amd", "csrc", "wfst_device.h")).read()
    assert int(re.search(r"#define WFST_GPOST_LDS_STATES (\d+)", hdr).group(1)) == U.WFST_GPOST_LDS_STATES
    assert int(re.search(r"kGpostLdsStates = (\d+);", dev).group(1)) == U.WFST_GPOST_LDS_STATES
    # two float64 rows and the staged float32 scores stay inside the 64 KiB a workgroup gets without opting in to more
    labels = int(re.search(r"kFalignLdsLabels = (\d+);", dev).group(1))
    assert 2 * 8 * U.WFST_GPOST_LDS_STATES + 2 * 4 * labels <= 64 * 1024


def test_a_translation_unit_of_its_own():
    srcs = [os.path.basename(s) for s in importlib.import_module("asr-decoder_amd").build.SRCS]
    assert "wfst_graphpost.hip" in srcs and "wfst_capi_graphpost.cc" in srcs
    core = open(os.path.join(ROOT, "asr-decoder_amd", "csrc", "wfst_capi.cc")).read()
    assert "wfst_decoder_graph_posteriors(" not in core and "launch_graph_post" not in core


def test_null_arguments_are_refused(W):
    lib = W.lib()
    z, d = C.c_double(0.0), C.c_double(1.0)
    assert lib.wfst_decoder_graph_posteriors(None, None, 0, None, None, None, None, 0, d, d, z, C.c_int64(0), 1, 1, 0, None, None, None, 0, d,
                                             None, *([None] * 12)) == E_ARG
    assert "NULL" in lib.wfst_last_error().decode()
    assert lib.wfst_decoder_graph_posteriors_workspace(None, None) == E_ARG
