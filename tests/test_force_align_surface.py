"""CPU: the surface of wfst_align_graphs_* / wfst_decoder_force_align -- the header, the binding's symbol list and the library agree, the
header's constants are the restatement's, and a graph set is validated on the HOST before any device is touched: a host that runs
these tests may have no GPU at all, where an epsilon cycle is still refused as a format error and a valid set then answers that there
is no device."""
import ctypes as C
import importlib
import inspect
import os
import re

import numpy as np
import pytest

import force_align_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_DEVICE, E_FORMAT = -1, -3, -6
NAMES = ["wfst_align_graphs_create", "wfst_align_graphs_load", "wfst_align_graphs_info", "wfst_align_graphs_free", "wfst_decoder_force_align",
         "wfst_decoder_force_align_workspace"]


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
    decl = re.search(r"int wfst_decoder_force_align\((.*?)\);", hdr, flags=re.S)
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")]
    assert args == ["wfst_decoder *d", "const int32_t *channels", "int32_t n", "const wfst_align_graphs *graphs", "const int32_t *graph_of",
                    "const int32_t *n_frames_in", "const int32_t *label_map", "int32_t n_tid", "int64_t max_cells", "int32_t cap_frames",
                    "int32_t cap_hops", "int32_t cap_words", "int32_t *status", "int32_t *found", "int32_t *n_frames", "float *path_cost",
                    "float *tot_score", "float *lm_score", "int32_t *n_hops", "int32_t *hop_arc", "int32_t *alignment", "int32_t *n_words",
                    "int32_t *words", "int32_t *word_frame"]
    const = lambda name: int(re.search(r"#define %s (\d+)" % name, hdr).group(1))
    assert const("WFST_FALIGN_LDS_STATES") == U.WFST_FALIGN_LDS_STATES
    dev = open(os.path.join(ROOT, "asr-decoder_amd", "csrc", "wfst_device.h")).read()
    assert int(re.search(r"kFalignLdsStates = (\d+);", dev).group(1)) == U.WFST_FALIGN_LDS_STATES
    # two float32 rows and the staged scores stay inside the 64 KiB a workgroup gets without opting in to more
    labels = int(re.search(r"kFalignLdsLabels = (\d+);", dev).group(1))
    assert 2 * 4 * U.WFST_FALIGN_LDS_STATES + 2 * 4 * labels <= 64 * 1024
    sig = inspect.signature(W.BatchDecoder.force_align).parameters
    assert list(sig)[:6] == ["self", "graphs", "graph_of", "channels", "n_frames", "label_map"]
    assert all(sig[k].default is None for k in ("graph_of", "channels", "n_frames", "label_map"))
    # a translation unit of its own, which the library's core does not call into
    assert "wfst_decoder_force_align(" not in open(os.path.join(ROOT, "asr-decoder_amd", "csrc", "wfst_capi.cc")).read()
    srcs = [os.path.basename(s) for s in importlib.import_module("asr-decoder_amd").build.SRCS]
    assert "wfst_forced.hip" in srcs and "wfst_capi_forced.cc" in srcs


def _cycle_graph():
    B = U.Builder()
    s = B.states(5)
    B.arc(s[0], 3, 1, 0.5, s[1])
    B.arc(s[1], 0, 0, 0.25, s[2])
    B.arc(s[2], 0, 0, -0.25, s[3])
    B.arc(s[3], 0, 0, 0.0, s[1])    # 1 -> 2 -> 3 -> 1
    B.arc(s[3], 4, 0, 1.0, s[4])
    return B.build(s[0], s[4])


def test_an_epsilon_cycle_is_refused_before_any_device(W):
    good = U.transcript_graph([1, 2], seed=3, n_tid=8)
    with pytest.raises(W.WfstError) as ei:
        W.AlignGraphs.from_arrays([U.as_tuple(good), U.as_tuple(_cycle_graph())])
    assert ei.value.code == E_FORMAT
    msg = str(ei.value)
    assert "align graph 1" in msg and "cycle" in msg
    assert re.search(r"state ([123])\b", msg), msg   # a state OF the cycle, not one behind it


def test_format_errors_come_first_too(W):
    g = U.transcript_graph([1], seed=4, n_tid=8)
    arcs = g.arcs.copy()
    arcs["to"][0] = g.n_states   # out of range
    with pytest.raises(W.WfstError) as ei:
        W.AlignGraphs.from_arrays([(g.start, g.final_state, g.state_info, arcs)])
    assert ei.value.code == E_FORMAT
    arcs = g.arcs.copy()
    arcs["olabel"][0] = -1
    with pytest.raises(W.WfstError) as ei:
        W.AlignGraphs.from_arrays([(g.start, g.final_state, g.state_info, arcs)])
    assert ei.value.code == E_FORMAT
    with pytest.raises(W.WfstError) as ei:
        W.AlignGraphs.from_arrays([(g.n_states, g.final_state, g.state_info, g.arcs)])
    assert ei.value.code == E_ARG
    assert W.lib().wfst_decoder_force_align(None, None, 0, None, None, None, None, 0, C.c_int64(0), 1, 1, 1, *([None] * 12)) == E_ARG


def test_a_valid_set_without_a_device_says_so(W):
    if W.device_count() > 0:
        pytest.skip("a GPU is visible here")
    with pytest.raises(W.WfstError) as ei:
        W.AlignGraphs.from_arrays([U.as_tuple(U.transcript_graph([1, 2], seed=3, n_tid=8))])
    assert ei.value.code == E_DEVICE and "no HIP device" in str(ei.value)
