"""CPU: the surface of wfst_decoder_frame_posteriors -- the header, the binding's symbol list and the library agree on it, the
argument errors that need no decoder are raised before any device work (this machine may have no GPU at all: a call that got as far
as the device would fail with WFST_E_DEVICE or crash, not answer WFST_E_ARG), the CLI's usage errors and the host mirror."""
import ctypes as C
import importlib
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import framepost_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1
NAME = "wfst_decoder_frame_posteriors"


@pytest.fixture(scope="module")
def W():
    p = importlib.import_module("asr-decoder_amd")
    p.build.build()
    return p.wfstdec


def test_header_binding_and_library_agree(W):
    hdr = open(os.path.join(ROOT, "include", "wfst_decoder.h")).read()
    decl = re.search(r"int %s\((.*?)\);" % NAME, hdr, flags=re.S)
    assert decl, "the header declares the entry point"
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")]
    assert args == ["wfst_decoder *d", "const int32_t *channels", "int32_t n", "int32_t use_final_probs", "double graph_scale",
                    "double acoustic_scale", "const int32_t *label_map", "int32_t n_tid", "double min_post", "int64_t max_cells",
                    "int32_t cap_frames", "int32_t cap_entries", "int32_t *status", "double *log_z", "int32_t *n_frames", "int32_t *n_entries",
                    "int32_t *frame_off", "int32_t *n_distinct", "double *frame_mass", "int32_t *entry_class", "double *entry_post"]
    assert NAME in W.SYMBOLS and hasattr(C.CDLL(W.LIB_PATH), NAME)
    # the LDS capacity the GPU tests build their lattices around
    assert int(re.search(r"#define WFST_FRAMEPOST_LDS_RECS (\d+)", hdr).group(1)) == framepost_util.LDS_RECS
    dev = open(os.path.join(ROOT, "asr-decoder_amd", "csrc", "wfst_device.h")).read()
    assert int(re.search(r"kFramePostLdsRecs = (\d+);", dev).group(1)) == framepost_util.LDS_RECS
    assert callable(W.BatchDecoder.frame_posteriors) and callable(W.frame_post_lookup)
    sig = inspect.signature(W.BatchDecoder.frame_posteriors).parameters
    assert list(sig) == ["self", "channels", "use_final_probs", "graph_scale", "acoustic_scale", "label_map", "min_post", "max_cells"]
    assert sig["channels"].default is None and sig["use_final_probs"].default is True and sig["graph_scale"].default == 1.0
    assert sig["acoustic_scale"].default == 1.0 and sig["label_map"].default is None and sig["min_post"].default == 0.0 and sig["max_cells"].default == 0
    assert list(inspect.signature(W.frame_post_lookup).parameters) == ["result", "classes_per_frame"]
    # the semantics are stated in full in the header
    for phrase in ("post(f, v)    = the sum of gamma(a) over the emitting arcs a (ilabel > 0) whose SOURCE state's frame is f and whose class is v",
                   "class(a)      = ilabel(a) where label_map is NULL, label_map[ilabel(a)] otherwise", "by class id ASCENDING",
                   "frame_mass[f] = the sum of post(f, v) over all v, before any threshold", "n_distinct[f] = the number of classes with post(f, v) > 0",
                   "An arc with ilabel 0 stays inside its frame; every other arc goes from frame f to f + 1", "NOT bit for bit",
                   "n_frames = 0, log_z = 0 and no entries", "the room needed", "lattice-to-post"):
        assert phrase in hdr, phrase
    # the three older calls keep their own wording and point to this one
    assert hdr.count("wfst_decoder_word_alternatives', below") == 2
    assert hdr.count("(The per-frame transition-id posteriors are wfst_decoder_frame_posteriors'") == 3
    assert "Not computed here: minimum Bayes risk decoding and confusion networks, per-frame transition-id posteriors (lattice-to-post)." in hdr
    # a translation unit of its own, which the library's core does not call into
    assert NAME not in open(os.path.join(ROOT, "asr-decoder_amd", "csrc", "wfst_capi.cc")).read()
    srcs = [os.path.basename(s) for s in importlib.import_module("asr-decoder_amd").build.SRCS]
    assert "wfst_framepost.hip" in srcs and "wfst_capi_framepost.cc" in srcs


def call(W, d=None, channels=True, gs=1.0, as_=1.0, label_map=None, n_tid=0, min_post=0.0, max_cells=0, capf=8, cape=64):
    I = C.POINTER(C.c_int32)
    ch = np.array([0], np.int32)
    m = None if label_map is None else np.ascontiguousarray(label_map, np.int32)
    rc = W.lib().wfst_decoder_frame_posteriors(d, ch.ctypes.data_as(I) if channels else None, 1, 1, C.c_double(gs), C.c_double(as_),
                                               None if m is None else m.ctypes.data_as(I), n_tid, C.c_double(min_post), C.c_int64(max_cells), capf, cape,
                                               *([None] * 9))
    return rc, W.lib().wfst_last_error().decode()


def test_argument_errors_come_before_any_device_work(W):
    # a decoder that is never looked at: these checks come before the first use of it (the fake one has no channels, so a call that
    # passed them still ends in WFST_E_ARG at the channel list, never on the device)
    fake = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    assert call(W, None)[0] == E_ARG and call(W, fake, channels=False)[0] == E_ARG
    for gs, as_ in ((-1.0, 1.0), (1.0, -1e-300), (float("nan"), 1.0), (1.0, float("nan")), (float("inf"), 1.0), (1.0, float("-inf"))):
        rc, msg = call(W, fake, gs=gs, as_=as_)
        assert rc == E_ARG and "scale" in msg, (gs, as_, msg)
    for mp in (float("nan"), -1e-300, 1.0000001, float("inf")):
        rc, msg = call(W, fake, min_post=mp)
        assert rc == E_ARG and "min_post" in msg, (mp, msg)
    for kw, word in ((dict(capf=0), "cap_frames"), (dict(capf=-2), "cap_frames"), (dict(cape=0), "cap_entries"), (dict(max_cells=-1), "max_cells"),
                     (dict(label_map=[0, 1, 2], n_tid=0), "n_tid"), (dict(label_map=[0, 1, 2], n_tid=-5), "n_tid"),
                     (dict(label_map=[0, 1, -2], n_tid=2), "negative")):
        rc, msg = call(W, fake, **kw)
        assert rc == E_ARG and word in msg, (kw, msg)
    # what passes them ends at the fake decoder's channel list; entry 0 of a map is unused and may hold anything
    for kw in (dict(), dict(min_post=0.0), dict(min_post=1.0), dict(label_map=[-7, 1, 2], n_tid=2), dict(gs=0.0, as_=0.0)):
        rc, msg = call(W, fake, **kw)
        assert rc == E_ARG and "channel" in msg, (kw, msg)


def test_cli_flags_and_the_host_mirror(tmp_path):
    host = os.path.join(ROOT, "asr-decoder_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host])
    cli = os.path.join(host, "wfst-decode")
    run = lambda *a: subprocess.run([cli] + list(a) + ["a", "b", "c"], capture_output=True, text=True)
    p = subprocess.run([cli], capture_output=True, text=True)
    assert p.returncode == 1 and "[--frame-post=FILE [--frame-post-class=tid|pdf|phone] [--frame-post-scales=GS,AS] [--frame-post-min=X]]" in p.stderr
    p = run("--frame-post=x", "--frame-post-class=pdf")
    assert p.returncode == 1 and "--frame-post-class=pdf needs --tid2pdf=FILE" in p.stderr
    p = run("--frame-post=x", "--frame-post-class=phone")
    assert p.returncode == 1 and "--frame-post-class=phone needs --tid2phone=FILE" in p.stderr
    p = run("--frame-post=x", "--frame-post-class=word")
    assert p.returncode == 1 and "--frame-post-class=tid|pdf|phone" in p.stderr
    for lone in ("--frame-post-class=pdf", "--frame-post-scales=1,1", "--frame-post-min=0.1"):
        p = run(lone)
        assert p.returncode == 1 and "go with --frame-post=FILE" in p.stderr, lone
    for bad in ("--frame-post-scales=1", "--frame-post-scales=1,x", "--frame-post-scales=-1,1", "--frame-post-scales=1,nan", "--frame-post-scales=1,2,3",
                "--frame-post-min=2", "--frame-post-min=-0.5", "--frame-post-min=x", "--frame-post-min="):
        p = run("--frame-post=x", bad)
        assert p.returncode == 1 and "--frame-post-scales=GS,AS" in p.stderr and "--frame-post-min=X" in p.stderr, bad
    p = run("--frame-post=x", "--threads=2")
    assert p.returncode == 1 and "--frame-post goes with the batch shape or --single-stream" in p.stderr
    # --tid2phone given for the phone classes alone is no endpointing: the run gets past that check, to the graph that is not there
    conf = tmp_path / "decoder.conf"
    conf.write_text("--beam=12\n--lattice-beam=5\n")
    with_conf = lambda *a: subprocess.run([cli] + list(a) + [str(conf), str(tmp_path / "no-graph"), "c"], capture_output=True, text=True)
    p = with_conf("--frame-post=" + str(tmp_path / "post.txt"), "--frame-post-class=phone", "--tid2phone=nowhere")
    assert p.returncode != 0 and "endpointing" not in p.stderr, p.stderr
    p = with_conf("--tid2phone=nowhere")
    assert p.returncode == 1 and "endpointing needs" in p.stderr
    hdr = open(os.path.join(host, "wfst-host.h")).read()
    assert "struct FramePosteriors {" in hdr and hdr.count("void FramePosteriors(") == 2
    assert "#pragma weak wfst_decoder_frame_posteriors" in open(os.path.join(host, "wfst-host.cc")).read()
