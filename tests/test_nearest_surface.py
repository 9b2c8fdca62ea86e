"""CPU: the surface of the lattice edit distance (wfst_decoder_nearest_words): the header, the binding's symbol list and the library
agree on the name; the header states the recurrence, the kind order and max_cells and cites the reference; the argument checks that need
no device; the entry point is a translation unit of its own, which alone launches the new kernel and calls the existing index launch
(wfst_capi.cc stays linkable against the doubles of the HIP runtime and of the launches it always used); the host mirror builds with it
and refers to the symbol weakly (wfst-host.cc stays linkable against the C-ABI doubles of tests/pool_double and tests/partial_double)."""
import ctypes
import importlib
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "wfst_decoder_nearest_words"


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
    assert NAME in declared and NAME in pkg.wfstdec.SYMBOLS and hasattr(lib, NAME)
    assert callable(pkg.wfstdec.BatchDecoder.nearest_words)
    # the declaration's parameters, in the order the binding passes them
    decl = src[src.index("int " + NAME):]
    decl = decl[:decl.index(";")]
    names = re.findall(r"(\w+)\s*(?:,|\))", decl)
    assert names == ["d", "channels", "n", "use_final_probs", "n_refs", "cap_words", "ref_words", "ref_len", "cap_hyp", "max_cells", "status",
                     "found", "n_err", "n_cor", "n_sub", "n_ins", "n_del", "n_arcs", "n_hyp", "hyp_words", "begin_frame", "end_frame", "ref_hyp",
                     "tot_score", "lm_score"]


def test_header_states_the_definition_and_cites_the_reference():
    src = open(os.path.join(ROOT, "include", "wfst_decoder.h")).read()
    block = src[src.index("lattice edit distance: the lattice path nearest a transcript"):src.index("int " + NAME)]
    block = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", block))   # (the comment's line breaks fall anywhere)
    for cite in ("kaldi-bin/bin/nbest-compute-wer.cc:111-167", "oracle error", "lattice-oracle",
                 "v[0][0] = (0, +0.0f)", "d' = (d + c(a)) + 0.0f", "(e + (olabel != r[k]), d')", "(e + 1, d')", "(e + 1, d)", "there are no others",
                 "OLABEL, not by ilabel", "least graph state among equals", "exact equality of both halves",
                 "0: match / substitution, from (s, k - 1); 1: free arc,", "2: insertion, from (s, k); 3: the deletion step, from (t, k - 1)",
                 "ilabel == 0 last, graph state of the source token, ilabel, olabel, bits of graph, bits of acoustic", "biglm",
                 "sub + ins + del == n_err", "cor + sub + del == L", "cor + sub + ins == n_hyp", "ref_hyp", "strictly increasing",
                 "max_cells", "65 536 states x 65", "8 bytes", "32.5 MiB", "256 MiB", "n_hyp > cap_hyp", "n_refs outside 1..64"):
        assert cite in block, cite


def test_a_call_fails_loudly_without_a_device(pkg):
    L = pkg.wfstdec.lib()
    one = (ctypes.c_int32 * 1)(0)
    assert L.wfst_decoder_nearest_words(None, one, 1, 1, 1, 4, one, one, 4, ctypes.c_int64(0), *([None] * 15)) == -1
    assert b"NULL decoder" in L.wfst_last_error()
    if pkg.wfstdec.device_count() == 0:   # no decoder can exist here: the only way in is the graph upload, which refuses
        s = pkg.synth.make_hclg_like(50, seed=1, n_tid=20, n_words=5)
        with pytest.raises(pkg.wfstdec.WfstError) as e:
            pkg.wfstdec.Graph.from_arrays(s.start, s.final_state, s.state_info, s.arcs)
        assert e.value.code == -3


def test_the_entry_point_is_a_translation_unit_of_its_own(pkg):
    csrc = os.path.join(ROOT, "asr-decoder_amd", "csrc")
    unit, kernels = os.path.join(csrc, "wfst_capi_nearest.cc"), os.path.join(csrc, "wfst_nearest.hip")
    assert unit in pkg.build.SRCS and kernels in pkg.build.SRCS
    for h in ("wfst_capi_nearest.h", "wfst_align_index.h"):
        assert os.path.join(csrc, h) in pkg.build.HDRS, h
    capi, entry, text = open(os.path.join(csrc, "wfst_capi.cc")).read(), open(unit).read(), open(kernels).read()
    assert "launch_nearest(" in entry and "launch_align_index(" in entry, "the new kernel, over the index the existing launch builds"
    assert "nearest" not in capi.lower(), "wfst_capi.cc launches nothing new and knows nothing of the call"
    assert "void nearest_kernel(" in text and "align_index_kernel" not in re.sub(r"//.*", "", text), "the index kernel is not copied"
    assert text.count("__global__") == 1
    code = re.sub(r"//.*", "", text)
    assert "asm" not in code, "no inline assembly"
    for rmw in ("atomicMin", "atomicAdd", "atomicCAS", "atomicExch", "atomicMax", "fetch_"):
        assert rmw not in code, "no atomic read-modify-write: a cell pulls its minimum"
    # the carving of the index is shared with align_kernel, not copied
    assert "aln_carve(" in open(os.path.join(csrc, "wfst_align_index.h")).read()
    for f in ("wfst_align.hip", "wfst_nearest.hip"):
        t = open(os.path.join(csrc, f)).read()
        assert '#include "wfst_align_index.h"' in t and "AlnIndex aln_carve(" not in t, f


def test_host_mirror_builds_and_refers_to_the_symbol_weakly(pkg):
    host = os.path.join(ROOT, "asr-decoder_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host])
    assert "#pragma weak " + NAME in open(os.path.join(host, "wfst-host.cc")).read()
    so = os.path.join(ROOT, "asr-decoder_amd", "lib", "libwfsthost.so")
    syms = subprocess.run(["nm", "-DC", so], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bw " + NAME + r"\b", syms), "a weak reference"
    for name in ("datemoon::GpuBatchDecoder::NearestWords(", "datemoon::GpuLatticeDecoder::NearestWords("):
        assert name in syms, name
    cli = os.path.join(host, "wfst-decode")
    p = subprocess.run([cli], capture_output=True, text=True)
    assert p.returncode == 1 and "--nearest-words=FILE" in p.stderr
    # refused before any device work: an unreadable file, the --threads shape, more than 64 references for a key
    p = subprocess.run([cli, "--nearest-words=/nonexistent", "a", "b", "c"], capture_output=True, text=True)
    assert p.returncode == 1 and "cannot read /nonexistent" in p.stderr
    p = subprocess.run([cli, "--nearest-words=/nonexistent", "--threads=2", "a", "b", "c"], capture_output=True, text=True)
    assert p.returncode == 1 and "--nearest-words goes with the batch shape or --single-stream" in p.stderr


def test_more_than_64_references_for_a_key_are_refused(pkg, tmp_path):
    host = os.path.join(ROOT, "asr-decoder_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host])
    f = tmp_path / "refs.txt"
    f.write_text("".join("utt 1 2 3\n" for _ in range(65)))
    p = subprocess.run([os.path.join(host, "wfst-decode"), "--nearest-words=" + str(f), "a", "b", "c"], capture_output=True, text=True)
    assert p.returncode == 1 and "--nearest-words: more than 64 sequences for utt" in p.stderr
