"""CPU: the surface of wfst_decoder_word_alternatives -- the header, the binding's symbol list and the library agree on it, and the
argument errors that need no decoder are raised before any device work (this machine may have no GPU at all: a call that got as
far as the device would fail with WFST_E_DEVICE or crash, not answer WFST_E_ARG)."""
import ctypes as C
import importlib
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import altern_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1
NAME = "wfst_decoder_word_alternatives"


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
                    "double acoustic_scale", "int32_t n_alts", "int32_t n_seqs", "int32_t cap_words", "const int32_t *seq_words",
                    "const int32_t *seq_len", "int64_t max_cells", "int32_t *status", "double *log_z", "int32_t *found", "int32_t *n_arcs",
                    "int32_t *begin_frame", "int32_t *end_frame", "double *word_post", "double *none_post", "int32_t *n_distinct",
                    "int32_t *alt_word", "double *alt_post", "double *path_logpost", "float *tot_score", "float *lm_score"]
    assert NAME in W.SYMBOLS and hasattr(C.CDLL(W.LIB_PATH), NAME)
    # the LDS capacity the GPU tests build their lattices around, and the most alternatives of a slot
    assert int(re.search(r"#define WFST_ALTERN_LDS_KEYS (\d+)", hdr).group(1)) == altern_util.LDS_KEYS
    assert int(re.search(r"#define WFST_ALTERN_MAX_ALTS (\d+)", hdr).group(1)) == altern_util.MAX_ALTS == 16
    assert callable(W.BatchDecoder.word_alternatives)
    sig = inspect.signature(W.BatchDecoder.word_alternatives).parameters
    assert sig["n_alts"].default == 5 and sig["max_cells"].default == 0 and sig["use_final_probs"].default is True
    assert inspect.signature(W.BatchDecoder.nbest_words_conf).parameters["alternatives"].default == 0
    # the semantics are stated in full in the header
    for phrase in ("mass(k, v) = the sum of gamma(a) over the arcs a with olabel(a) == v whose SOURCE state's frame lies in cell k",
                   "mass DESCENDING and then by word id ASCENDING", "UNCLAMPED", "none_post[k] + P(some word in the cell) = 1",
                   "an empty cell (lo >= hi", "a word on an arc that ENTERS the cell belongs to the cell before",
                   "exp(-(A_k[s] + c(a) + beta[t] + log_z))", "the paths that ended before the cell began", "NOT bit for bit",
                   "found = 0: every new output is zero"):
        assert phrase in hdr, phrase
    # the two older calls point to this one, their own wording kept
    assert hdr.count("wfst_decoder_word_alternatives', below") == 2
    assert "minimum Bayes risk / confusion networks.  (The sentence posterior is wfst_decoder_sequence_posterior's" in hdr
    assert "Not computed here: minimum Bayes risk decoding and confusion networks, per-frame transition-id posteriors (lattice-to-post)." in hdr


def call(W, d=None, channels=True, gs=1.0, as_=1.0, n_alts=5, n_seqs=1, cap=2, words=True, lens=True, max_cells=0, length=1, word=1):
    I = C.POINTER(C.c_int32)
    ch, w, ln = np.array([0], np.int32), np.array([word, 1], np.int32), np.array([length], np.int32)
    p = lambda a, on: a.ctypes.data_as(I) if on else None
    rc = W.lib().wfst_decoder_word_alternatives(d, p(ch, channels), 1, 1, C.c_double(gs), C.c_double(as_), n_alts, n_seqs, cap, p(w, words),
                                                p(ln, lens), C.c_int64(max_cells), *([None] * 14))
    return rc, W.lib().wfst_last_error().decode()


def test_argument_errors_come_before_any_device_work(W):
    # a decoder that is never looked at: these checks come before the first use of it (the fake one has no channels, so a call that
    # passed them would still end in WFST_E_ARG at the channel list, never on the device)
    fake = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    assert call(W, None)[0] == E_ARG and call(W, fake, channels=False)[0] == E_ARG
    for gs, as_ in ((-1.0, 1.0), (1.0, -1e-300), (float("nan"), 1.0), (1.0, float("nan")), (float("inf"), 1.0), (1.0, float("-inf"))):
        rc, msg = call(W, fake, gs=gs, as_=as_)
        assert rc == E_ARG and "scale" in msg, (gs, as_, msg)
    for n_alts in (0, -1, 17, 1 << 20):
        rc, msg = call(W, fake, n_alts=n_alts)
        assert rc == E_ARG and "n_alts" in msg, (n_alts, msg)
    for kw in (dict(n_seqs=0), dict(n_seqs=65), dict(cap=0), dict(cap=-3), dict(words=False), dict(lens=False), dict(max_cells=-1),
               dict(length=3), dict(word=0)):
        rc, msg = call(W, fake, **kw)
        assert rc == E_ARG and "n_alts" not in msg, (kw, msg)


def test_cli_flags_and_the_host_mirror():
    host = os.path.join(ROOT, "asr-decoder_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host])
    cli = os.path.join(host, "wfst-decode")
    p = subprocess.run([cli], capture_output=True, text=True)
    assert p.returncode == 1 and "[--word-alternatives[=K]]" in p.stderr
    p = subprocess.run([cli, "--word-alternatives", "a", "b", "c"], capture_output=True, text=True)
    assert p.returncode == 1 and "--word-alternatives goes with --nbest-word-times or --align-words=FILE" in p.stderr
    p = subprocess.run([cli, "--word-alternatives=3", "--word-confidence", "a", "b", "c"], capture_output=True, text=True)
    assert p.returncode == 1 and "goes with --nbest-word-times or --align-words=FILE" in p.stderr
    for bad in ("--word-alternatives=0", "--word-alternatives=17", "--word-alternatives=x", "--word-alternatives="):
        p = subprocess.run([cli, bad, "--nbest=2", "--nbest-word-times", "a", "b", "c"], capture_output=True, text=True)
        assert p.returncode == 1 and "--word-alternatives=K, 1 <= K <= 16" in p.stderr, bad
    hdr = open(os.path.join(host, "wfst-host.h")).read()
    assert "struct WordAlternatives : WordConfidence {" in hdr and hdr.count("void WordAlternatives(") == 2
    assert "#pragma weak wfst_decoder_word_alternatives" in open(os.path.join(host, "wfst-host.cc")).read()
