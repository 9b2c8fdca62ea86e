"""CPU: the surface of wfst_decoder_sequence_stats -- the header, the binding's symbol list and the library agree on it, the header's
constants are the restatement's, the argument errors that need no decoder are raised before any device work (a host that runs these tests may have no
GPU at all: a call that got as far as the device would fail with WFST_E_DEVICE or crash, not answer WFST_E_ARG), the CLI's usage
errors and the host mirror."""
import ctypes as C
import importlib
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import seqstat_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1
NAME = "wfst_decoder_sequence_stats"


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
    assert args == ["wfst_decoder *d", "const int32_t *channels", "int32_t n", "int32_t criterion", "int32_t use_final_probs", "double graph_scale",
                    "double acoustic_scale", "const int32_t *label_map", "int32_t n_tid", "const int32_t *ref", "const int32_t *n_ref",
                    "int32_t cap_ref", "const int32_t *sil_classes", "int32_t n_sil", "int32_t drop_frames", "int64_t max_cells",
                    "int32_t cap_frames", "int32_t cap_entries", "void *const *grad", "const int64_t *grad_pitch", "const int32_t *grad_frames",
                    "int32_t n_cols", "double grad_scale", "void *consumer_stream", "int32_t *status", "double *log_z", "double *tot_acc",
                    "int32_t *n_frames", "int32_t *n_ref_frames", "int32_t *n_dropped", "int32_t *n_entries", "int32_t *frame_off",
                    "int32_t *entry_class", "double *entry_post", "double *entry_value"]
    assert NAME in W.SYMBOLS and hasattr(C.CDLL(W.LIB_PATH), NAME)
    # the constants the restatement and the GPU tests are built around
    const = lambda name: int(re.search(r"#define %s (\d+)" % name, hdr).group(1))
    assert const("WFST_SEQSTAT_LDS_RECS") == seqstat_util.LDS_RECS and const("WFST_SEQSTAT_MAX_SIL") == seqstat_util.MAX_SIL
    assert const("WFST_SEQ_MMI") == seqstat_util.SEQ_MMI == W.WFST_SEQ_MMI and const("WFST_SEQ_SMBR") == seqstat_util.SEQ_SMBR == W.WFST_SEQ_SMBR
    dev = open(os.path.join(ROOT, "asr-decoder_amd", "csrc", "wfst_device.h")).read()
    assert int(re.search(r"kSeqStatLdsRecs = (\d+);", dev).group(1)) == seqstat_util.LDS_RECS
    assert int(re.search(r"kSeqStatMaxSil = (\d+);", dev).group(1)) == seqstat_util.MAX_SIL
    assert re.search(r"kSeqMmi = 0, kSeqSmbr = 1;", dev)
    sig = inspect.signature(W.BatchDecoder.sequence_stats).parameters
    assert list(sig) == ["self", "refs", "channels", "criterion", "use_final_probs", "graph_scale", "acoustic_scale", "label_map", "sil_classes",
                         "drop_frames", "grad", "grad_scale", "stream", "max_cells", "lists"]
    assert sig["channels"].default is None and sig["criterion"].default == "smbr" and sig["use_final_probs"].default is True
    assert sig["graph_scale"].default == 1.0 and sig["acoustic_scale"].default == 1.0 and sig["label_map"].default is None
    assert sig["sil_classes"].default == () and sig["drop_frames"].default is False and sig["grad"].default is None
    assert sig["grad_scale"].default == 1.0 and sig["stream"].default == "current" and sig["max_cells"].default == 0 and sig["lists"].default is True
    # the semantics are stated in full in the header, with Kaldi's tool named
    for phrase in ("LatticeForwardBackwardMpeVariants", "fa[0] = 0, fa[t] = sum over in-arcs  a: s -> t of p_in(a)  * (fa[s] + acc(a))",
                   "fb[s] = sum over out-arcs a: s -> t of p_out(a) * (fb[t] + acc(a))", "tot_acc    = fb[0]",
                   "w(a)       = gamma(a) * (fa[s] + acc(a) + fb[t] - tot_acc), signed", "value(f, v) = [v == ref[f]] - post(f, v)",
                   "one more entry (ref[f], 0, 1)", "--drop-frames", "by class id ASCENDING", "NOT bit for bit", "the room needed",
                   "float32(grad_scale * value(f, v)) at column v", "Not computed here: minimum Bayes risk decoding"):
        assert phrase in hdr, phrase
    # a translation unit of its own, which the library's core does not call into
    assert NAME not in open(os.path.join(ROOT, "asr-decoder_amd", "csrc", "wfst_capi.cc")).read()
    srcs = [os.path.basename(s) for s in importlib.import_module("asr-decoder_amd").build.SRCS]
    assert "wfst_seqstat.hip" in srcs and "wfst_capi_seqstat.cc" in srcs


def call(W, d=None, channels=True, crit=1, gs=1.0, as_=1.0, label_map=None, n_tid=0, ref=(1, 2), n_ref=None, sil=(), max_cells=0, capf=8, cape=64,
         grad=None, pitch=None, rows=(4,), n_cols=0, grad_scale=1.0):
    I = C.POINTER(C.c_int32)
    ch = np.array([0], np.int32)
    m = None if label_map is None else np.ascontiguousarray(label_map, np.int32)
    r = np.ascontiguousarray(ref, np.int32)
    nr = np.array([len(r) if n_ref is None else n_ref], np.int32)
    s = np.ascontiguousarray(list(sil), np.int32)
    g = None if grad is None else (C.c_void_p * 1)(grad)
    pt = None if pitch is None else np.array([pitch], np.int64)
    rw = np.ascontiguousarray(rows, np.int32)
    rc = W.lib().wfst_decoder_sequence_stats(d, ch.ctypes.data_as(I) if channels else None, 1, crit, 1, C.c_double(gs), C.c_double(as_),
                                             None if m is None else m.ctypes.data_as(I), n_tid, r.ctypes.data_as(I), nr.ctypes.data_as(I), len(r),
                                             s.ctypes.data_as(I) if len(s) else None, len(s), 0, C.c_int64(max_cells), capf, cape, g,
                                             None if pt is None else pt.ctypes.data_as(C.POINTER(C.c_int64)), rw.ctypes.data_as(I) if grad is not None else None,
                                             n_cols, C.c_double(grad_scale), C.c_void_p(W.WFST_STREAM_NONE), *([None] * 11))
    return rc, W.lib().wfst_last_error().decode()


def test_argument_errors_come_before_any_device_work(W):
    # a decoder that is never looked at: these checks come before the first use of it (the fake one has no channels, so a call that
    # passed them still ends in WFST_E_ARG at the channel list, never on the device)
    fake = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    assert call(W, None)[0] == E_ARG and call(W, fake, channels=False)[0] == E_ARG
    for gs, as_ in ((-1.0, 1.0), (1.0, -1e-300), (float("nan"), 1.0), (1.0, float("nan")), (float("inf"), 1.0), (1.0, float("-inf"))):
        rc, msg = call(W, fake, gs=gs, as_=as_)
        assert rc == E_ARG and "scale" in msg, (gs, as_, msg)
    for kw, word in ((dict(crit=2), "criterion"), (dict(crit=-1), "criterion"), (dict(capf=0), "cap_frames"), (dict(capf=-2, cape=0), "cap_frames"),
                     (dict(cape=0), "cap_entries"), (dict(max_cells=-1), "max_cells"),
                     (dict(label_map=[0, 1, 2], n_tid=0), "n_tid"), (dict(label_map=[0, 1, -2], n_tid=2), "negative"),
                     (dict(sil=[2, 2]), "ascending"), (dict(sil=[3, 1]), "ascending"), (dict(sil=[-1]), "sil_classes"), (dict(sil=list(range(65))), "MAX_SIL"),
                     (dict(n_ref=-1), "n_ref"), (dict(n_ref=3), "n_ref"),
                     (dict(grad=4096, n_cols=8, grad_scale=float("nan")), "grad_scale"), (dict(grad_scale=float("inf")), "grad_scale"),
                     (dict(grad=4096, n_cols=0), "n_cols"), (dict(grad=4098, n_cols=8), "aligned"), (dict(grad=4096, n_cols=8, pitch=7), "pitch"),
                     (dict(grad=4096, n_cols=8, rows=(-1,)), "grad_frames"), (dict(grad=4096, n_cols=2), "ref class"),
                     (dict(grad=4096, n_cols=8, label_map=[0, 1, 8], n_tid=2), "label_map class")):
        rc, msg = call(W, fake, **kw)
        assert rc == E_ARG and word in msg, (kw, msg)
    # what passes them ends at the fake decoder's channel list
    for kw in (dict(), dict(crit=0), dict(capf=0, cape=0), dict(sil=list(range(64))), dict(ref=(-1, -5)), dict(n_ref=0), dict(grad=4096, n_cols=8, pitch=8),
               dict(label_map=[-7, 1, 2], n_tid=2), dict(gs=0.0, as_=0.0)):
        rc, msg = call(W, fake, **kw)
        assert rc == E_ARG and "channel" in msg, (kw, msg)


def test_cli_flags_and_the_host_mirror(tmp_path):
    host = os.path.join(ROOT, "asr-decoder_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host])
    cli = os.path.join(host, "wfst-decode")
    run = lambda *a: subprocess.run([cli] + list(a) + ["a", "b", "c"], capture_output=True, text=True)
    p = subprocess.run([cli], capture_output=True, text=True)
    assert p.returncode == 1 and ("[--seq-stats=FILE --seq-ref=FILE [--seq-criterion=smbr|mmi] [--seq-class=tid|pdf|phone] [--seq-scales=GS,AS] "
                                  "[--seq-silence=a:b:c] [--seq-drop-frames]]") in p.stderr
    for lone in ("--seq-ref=x", "--seq-criterion=mmi", "--seq-class=pdf", "--seq-scales=1,1", "--seq-silence=1:2", "--seq-drop-frames"):
        p = run(lone)
        assert p.returncode == 1 and "go with --seq-stats=FILE" in p.stderr, lone
    p = run("--seq-stats=x")
    assert p.returncode == 1 and "--seq-stats=FILE needs --seq-ref=FILE" in p.stderr
    p = run("--seq-stats=x", "--seq-ref=y", "--seq-class=pdf")
    assert p.returncode == 1 and "--seq-class=pdf needs --tid2pdf=FILE" in p.stderr
    p = run("--seq-stats=x", "--seq-ref=y", "--seq-class=phone")
    assert p.returncode == 1 and "--seq-class=phone needs --tid2phone=FILE" in p.stderr
    p = run("--seq-stats=x", "--seq-ref=y", "--seq-class=word")
    assert p.returncode == 1 and "--seq-class=tid|pdf|phone" in p.stderr
    p = run("--seq-stats=x", "--seq-ref=y", "--seq-criterion=mpe")
    assert p.returncode == 1 and "--seq-criterion=smbr|mmi" in p.stderr
    for bad in ("--seq-scales=1", "--seq-scales=1,x", "--seq-scales=-1,1", "--seq-scales=1,nan", "--seq-scales=1,2,3", "--seq-silence=", "--seq-silence=2:1",
                "--seq-silence=1:1", "--seq-silence=-1", "--seq-silence=1:", "--seq-silence=a", "--seq-silence=" + ":".join(str(i) for i in range(65))):
        p = run("--seq-stats=x", "--seq-ref=y", bad)
        assert p.returncode == 1 and "--seq-scales=GS,AS" in p.stderr and "--seq-silence=a:b:c" in p.stderr, bad
    p = run("--seq-stats=x", "--seq-ref=y", "--threads=2")
    assert p.returncode == 1 and "--seq-stats goes with the batch shape or --single-stream" in p.stderr
    # --tid2phone given for the phone classes alone is no endpointing: the run gets past that check, to the graph that is not there
    conf = tmp_path / "decoder.conf"
    conf.write_text("--beam=12\n--lattice-beam=5\n")
    ref = tmp_path / "ref.txt"
    ref.write_text("utt1 1 2 3\n")
    p = subprocess.run([cli, "--seq-stats=" + str(tmp_path / "s.txt"), "--seq-ref=" + str(ref), "--seq-class=phone", "--tid2phone=nowhere", str(conf),
                        str(tmp_path / "no-graph"), "c"], capture_output=True, text=True)
    assert p.returncode != 0 and "endpointing" not in p.stderr, p.stderr
    hdr = open(os.path.join(host, "wfst-host.h")).read()
    assert "struct SequenceStats {" in hdr and "struct SequenceStatsOptions {" in hdr and hdr.count("void SequenceStats(") == 2
    assert "#pragma weak wfst_decoder_sequence_stats" in open(os.path.join(host, "wfst-host.cc")).read()
