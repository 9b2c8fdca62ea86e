"""CPU: the surface of phrase boosting (wfst_bias_compile, wfst_bias_lists_*, wfst_decoder_biased_words) -- the header, the
binding's symbol list and the library agree on it, the header states the arithmetic, wfst_bias_compile equals the numpy automaton of
tests/bias_util.py (the node numbering included), the argument errors are raised before any device work (this machine may have no GPU
at all), and what the compiler made of bias_kernel."""
import ctypes as C
import importlib
import inspect
import os
import re

import numpy as np
import pytest

import bias_util as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_DEVICE, E_CAPACITY = -1, -3, -4
NAME = "wfst_decoder_biased_words"
NEW = ["wfst_bias_compile", "wfst_bias_lists_create", "wfst_bias_lists_info", "wfst_bias_lists_free", NAME]


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module("asr-decoder_amd")
    p.build.build()
    return p


def test_header_binding_and_library_agree(pkg):
    W = pkg.wfstdec
    hdr = open(os.path.join(ROOT, "include", "wfst_decoder.h")).read()
    decl = re.search(r"int %s\((.*?)\);" % NAME, hdr, flags=re.S)
    assert decl, "the header declares the entry point"
    args = [" ".join(a.split()) for a in re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")]
    assert args == ["wfst_decoder *d", "const int32_t *channels", "int32_t n", "int32_t use_final_probs", "const wfst_bias_lists *lists",
                    "const int32_t *list_of", "int32_t n_set", "const double *settings", "int32_t cap_words", "int32_t cap_hits", "int64_t max_cells",
                    "int32_t *status", "int32_t *found", "int32_t *n_arcs", "int32_t *n_hyp", "int32_t *n_hits", "int32_t *hyp_words",
                    "int32_t *begin_frame", "int32_t *end_frame", "int32_t *hit_phrase", "int32_t *hit_word", "double *biased_cost", "double *bonus",
                    "float *tot_score", "float *lm_score"]
    lib = C.CDLL(W.LIB_PATH)
    for name in NEW:
        assert name in W.SYMBOLS and hasattr(lib, name) and re.search(r"\b%s\(" % name, hdr), name
    assert "#define WFST_BIAS_MAX_NODES 256" in hdr and "#define WFST_BIAS_MAX_WORDS 16" in hdr
    sig = inspect.signature(W.BatchDecoder.biased_words).parameters
    assert list(sig) == ["self", "lists", "list_of", "settings", "channels", "use_final_probs", "cap_words", "cap_hits", "max_cells"]
    assert sig["list_of"].default is None and sig["settings"].default == ((1, 1, 0, 1),) and sig["channels"].default is None
    assert sig["use_final_probs"].default is True and sig["cap_words"].default == 256 and sig["cap_hits"].default == 64 and sig["max_cells"].default == 0
    assert hasattr(W.BiasLists, "from_phrases") and hasattr(W.BiasLists, "info") and callable(W.bias_compile)


def test_the_header_states_the_definition():
    hdr = open(os.path.join(ROOT, "include", "wfst_decoder.h")).read()
    block = hdr[hdr.index("phrase boosting: biased best paths of the raw lattice"):hdr.index("int " + NAME)]
    block = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", block))   # (the comment's line breaks fall anywhere)
    for phrase in ("a phrase that lattice_beam pruned away is not brought back", "1..WFST_BIAS_MAX_WORDS word ids (> 0)", "finite and >= 0",
                   "no two phrases of one list are equal", "J <= WFST_BIAS_MAX_NODES", "breadth-first order, root 0",
                   "(depth, parent's number, word id) ascending", "the numbering is part of the definition because the tie rule uses it",
                   "the longest proper suffix of str(j) that is a node", "the longest suffix of str(i) . w that is a node", "the root if none is",
                   "beta(0) = 0.0 and beta(j) = own(j) + beta(fail(j))", "computed in node order in float64",
                   "overlapping and nested occurrences each count, and nothing is retracted",
                   "(graph_scale gs, acoustic_scale as, word_penalty wip, boost_scale bs)", "n_set = 1..16",
                   "exactly wfst_decoder_rescaled_words'", "j_k = delta(j_{k-1}, olabel(a_k))", "d = c_q(a) - r", "r = bs * beta(j_k) on a word arc and 0.0 otherwise",
                   "the product and the difference each rounded on its own", "no fused multiply-add", "v[0][0] = +0.0", "(v[s][i] + d) + 0.0",
                   "a sum that is not finite is no transition", "Float addition is monotone", "R is a DAG", "whatever the order of the arc index",
                   "bit for bit", "Totals may be negative", "then the least graph state, then the least node",
                   "found = 0 only if no final state is reached", "(v[s][i] + d) + 0.0 == v[t][j]", "then the least source node", "biglm",
                   "the float64 sequential sum of r in hop order", "UNSCALED", "LatticeToVector", "unchanged by the bias",
                   "ordered by hit_word ascending", "the longest phrase comes first", "-1 (or list_of NULL) means no list: J = 1",
                   "bit for bit wfst_decoder_rescaled_words' scaled_cost at (gs, as, wip)", "the counts are the room needed",
                   "n_set outside 1..16", "cap_words <= 0", "cap_hits < 0", "Any output pointer may be NULL", "The decoder's state is only read",
                   "Synchronous", "before any device is touched", "names list and phrase", "more than 256 nodes is WFST_E_CAPACITY",
                   "biasing the first-pass search", "lists beyond 256 nodes or a sparse table", "n-best lists under a bias", "transition-id output",
                   "class or subword biasing"):
        assert phrase in block, phrase


def test_the_entry_points_are_a_translation_unit_of_their_own(pkg):
    csrc = os.path.join(ROOT, "asr-decoder_amd", "csrc")
    unit, kernels = os.path.join(csrc, "wfst_capi_bias.cc"), os.path.join(csrc, "wfst_bias.hip")
    assert unit in pkg.build.SRCS and kernels in pkg.build.SRCS and os.path.join(csrc, "wfst_capi_bias.h") in pkg.build.HDRS
    capi, entry, text = open(os.path.join(csrc, "wfst_capi.cc")).read(), open(unit).read(), open(kernels).read()
    for word in NEW + ["biased_words", "launch_bias", "bias_kernel", "wfst_capi_bias", "BiasDev", "bias_lists"]:
        assert word not in capi, "wfst_capi.cc launches nothing new and knows nothing of the call"
    assert "launch_bias(" in entry and "launch_align_index(" in entry and "word_query_run(" in entry and "wfst_hip_own.h" in open(
        os.path.join(csrc, "wfst_capi_align.h")).read() and "DevBuf<" in open(os.path.join(csrc, "wfst_capi_bias.h")).read()
    code = re.sub(r"//.*", "", text)
    assert "void bias_kernel(" in code and code.count("__global__") == 1 and "align_index_kernel" not in code, "the index kernel is not copied"
    assert '#include "wfst_align_index.h"' in text and "aln_carve(" in code
    assert "#pragma clang fp contract(off)" in code, "neither the arc cost nor the bonus is contracted"
    assert "asm" not in code, "no inline assembly"
    for rmw in ("atomicMin", "atomicAdd", "atomicCAS", "atomicExch", "atomicMax", "fetch_"):
        assert rmw not in code, "no atomic read-modify-write: a cell pulls its minimum"


def test_the_kernel_uses_no_scratch_and_its_lds_fits(pkg):
    res = pkg.build.kernel_resources(source=os.path.join(ROOT, "asr-decoder_amd", "csrc", "wfst_bias.hip"))
    assert "bias_kernel" in res, sorted(res)
    r = res["bias_kernel"]
    print("bias_kernel:", r)
    assert r["vgpr_spill"] == 0 and r["scratch"] == 0, "nothing goes to scratch memory (scalar registers that wait in vector lanes do not)"
    assert 0 < r["lds"] <= 64 * 1024


def flat(phrases):
    ln = np.ascontiguousarray([len(ws) for ws, _ in phrases], np.int32)
    words = np.ascontiguousarray([w for ws, _ in phrases for w in ws], np.int32)
    bonus = np.ascontiguousarray([b for _, b in phrases], np.float64)
    return ln, words, bonus


def compile_raw(W, phrases, cap_nodes=256):
    I, D = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    ln, words, bonus = flat(phrases)
    n = C.c_int32(-7)
    v = [np.full(max(cap_nodes, 1), -9, np.int32) for _ in range(4)]
    beta = np.full(max(cap_nodes, 1), -9.0)
    rc = W.lib().wfst_bias_compile(len(ln), ln.ctypes.data_as(I), words.ctypes.data_as(I), bonus.ctypes.data_as(D), cap_nodes, C.byref(n),
                                   *([x.ctypes.data_as(I) for x in v] + [beta.ctypes.data_as(D)]))
    return rc, n.value, v, beta, W.lib().wfst_last_error().decode()


def same_automaton(W, phrases):
    A = B.compile_list(phrases)
    got = W.bias_compile(phrases)
    assert got["n_nodes"] == A.J
    for key in ("parent", "word", "fail", "phrase"):
        assert np.array_equal(got[key], getattr(A, key)), (key, phrases)
    assert got["beta"].tobytes() == A.beta.tobytes(), "beta bit for bit: the sums taken in node order"
    return A


def chain_list(nodes):
    """a list of exactly `nodes` nodes: chains of 16 words over a small alphabet (failure links that go somewhere), the last one cut"""
    out, left, k = [], nodes - 1, 0
    while left > 0:
        n = min(16, left)
        out.append((tuple(10 * k + 1 + (i * i + k) % 3 for i in range(n)), 0.1 * (k + 1)))
        left -= n
        k += 1
    return out


def test_bias_compile_equals_the_numpy_automaton(pkg):
    W = pkg.wfstdec
    rs = np.random.RandomState(5)
    same_automaton(W, [])
    same_automaton(W, [((1, 2, 3), 1.0), ((1, 2, 4), 0.5), ((2, 3), 0.25), ((2,), 0.125), ((5, 1, 2, 4, 6), 2.0), ((1, 1), 4.0)])
    for _ in range(200):
        phrases, seen = [], set()
        for _ in range(rs.randint(1, 9)):
            ws = tuple(int(w) for w in rs.randint(1, rs.randint(2, 6), size=rs.randint(1, 7)))
            if ws not in seen:
                seen.add(ws)
                phrases.append((ws, float(rs.rand() * 3.0)))   # (arbitrary float64 bonuses: beta's order of summation shows)
        same_automaton(W, phrases)
    # at the limit: 255 and 256 nodes stand, 257 are refused with the count
    for nodes in (255, 256):
        A = same_automaton(W, chain_list(nodes))
        assert A.J == nodes and int(A.depth.max()) == 16
    rc, n, _, _, msg = compile_raw(W, chain_list(257), cap_nodes=300)
    assert rc == E_CAPACITY and n == 257 and "257 nodes" in msg
    # the caller's rows too short: the count, nothing else
    rc, n, v, _, msg = compile_raw(W, chain_list(40), cap_nodes=39)
    assert rc == E_CAPACITY and n == 40 and "cap_nodes" in msg and np.all(v[0] == -9)


def create_raw(W, lists, device=0):
    I, D = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    n_ph = np.ascontiguousarray([len(p) for p in lists], np.int32)
    ln, words, bonus = flat([x for p in lists for x in p])
    h = C.c_void_p()
    rc = W.lib().wfst_bias_lists_create(len(lists), n_ph.ctypes.data_as(I), ln.ctypes.data_as(I), words.ctypes.data_as(I), bonus.ctypes.data_as(D),
                                        device, C.byref(h))
    return rc, h, W.lib().wfst_last_error().decode()


def test_bad_lists_are_refused_on_the_host(pkg):
    W = pkg.wfstdec
    good = [((1, 2), 1.0), ((3,), 0.5)]
    nan, inf = float("nan"), float("inf")
    for bad, word in (([((1, 0), 1.0)], "word id"), ([((-4,), 1.0)], "word id"), ([((), 1.0)], "length"), ([(tuple(range(1, 18)), 1.0)], "length"),
                      ([((1,), -0.5)], "bonus"), ([((1,), nan)], "bonus"), ([((1,), inf)], "bonus"), ([((7, 8), 1.0), ((7, 8), 2.0)], "duplicate")):
        rc, h, msg = create_raw(W, [good, good + bad])
        assert rc == E_ARG and not h and word in msg and "bias list 1 " in msg and "phrase %d" % (len(good) + len(bad) - 1) in msg, (bad, msg)
        rc, _, _, _, msg = compile_raw(W, good + bad)
        assert rc == E_ARG and word in msg, (bad, msg)
    rc, h, msg = create_raw(W, [good, chain_list(257)])
    assert rc == E_CAPACITY and not h and "bias list 1 " in msg and "257 nodes" in msg
    rc, h, msg = create_raw(W, [])
    assert rc == E_ARG and not h
    assert W.lib().wfst_bias_lists_create(1, None, None, None, None, 0, None) == E_ARG
    assert W.lib().wfst_bias_lists_info(None, *([None] * 7)) == E_ARG
    W.lib().wfst_bias_lists_free(None)
    # a valid set gets as far as the device: on a machine without one that is the answer
    if W.device_count() == 0:
        rc, h, msg = create_raw(W, [good, chain_list(256), []])
        assert rc == E_DEVICE and not h, msg


def call(W, d=None, channels=True, n_set=1, settings=(1.0, 1.0, 0.0, 1.0), cap_words=8, cap_hits=4, max_cells=0):
    I, D = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    ch = np.array([0], np.int32)
    st = None if settings is None else np.ascontiguousarray(settings, np.float64)
    rc = W.lib().wfst_decoder_biased_words(d, ch.ctypes.data_as(I) if channels else None, 1, 1, None, None, n_set,
                                           None if st is None else st.ctypes.data_as(D), cap_words, cap_hits, C.c_int64(max_cells), *([None] * 14))
    return rc, W.lib().wfst_last_error().decode()


def test_argument_errors_come_before_any_device_work(pkg):
    W = pkg.wfstdec
    # a decoder that is never looked at: these checks come before the first use of it (the fake one has no channels, so a call that
    # passed them still ends in WFST_E_ARG at the channel list, never on the device)
    fake = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    nan, inf = float("nan"), float("inf")
    assert call(W, None)[0] == E_ARG and call(W, fake, channels=False)[0] == E_ARG
    for gs, as_ in ((-1.0, 1.0), (1.0, -1e-300), (nan, 1.0), (1.0, nan), (inf, 1.0), (1.0, -inf)):
        rc, msg = call(W, fake, settings=(gs, as_, 0.0, 1.0))
        assert rc == E_ARG and "scale" in msg, (gs, as_, msg)
    for wip in (nan, inf, -inf):
        rc, msg = call(W, fake, settings=(1.0, 1.0, wip, 1.0))
        assert rc == E_ARG and "penalty" in msg, (wip, msg)
    for bs in (nan, inf, -inf, -1e-300):
        rc, msg = call(W, fake, settings=(1.0, 1.0, 0.0, bs))
        assert rc == E_ARG and "boost_scale" in msg, (bs, msg)
    rc, msg = call(W, fake, n_set=2, settings=(1.0, 1.0, 0.0, 1.0, 1.0, 1.0, 0.0, nan))
    assert rc == E_ARG and "boost_scale" in msg
    for kw, word in ((dict(n_set=0), "n_set"), (dict(n_set=17, settings=[1.0, 1.0, 0.0, 1.0] * 17), "n_set"), (dict(n_set=-1), "n_set"),
                     (dict(settings=None), "NULL settings"), (dict(cap_words=0), "cap_words"), (dict(cap_words=-3), "cap_words"),
                     (dict(cap_hits=-1), "cap_hits"), (dict(max_cells=-1), "max_cells")):
        rc, msg = call(W, fake, **kw)
        assert rc == E_ARG and word in msg, (kw, msg)
    # what passes them ends at the fake decoder's channel list
    for kw in (dict(), dict(settings=(0.0, 0.0, -5.0, 0.0)), dict(n_set=16, settings=[1.0, 0.1, 0.5, 2.0] * 16), dict(cap_hits=0)):
        rc, msg = call(W, fake, **kw)
        assert rc == E_ARG and "channel" in msg, (kw, msg)


def test_cli_flags_and_the_host_mirror(pkg, tmp_path):
    import subprocess

    host = os.path.join(ROOT, "asr-decoder_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host])
    cli = os.path.join(host, "wfst-decode")
    run = lambda *a: subprocess.run([cli] + list(a) + ["a", "b", "c"], capture_output=True, text=True)
    p = subprocess.run([cli], capture_output=True, text=True)
    assert p.returncode == 1 and "[--bias=FILE [--bias-settings=GS,AS,WIP,BS[:GS,AS,WIP,BS...]]]" in p.stderr
    good = tmp_path / "bias.txt"
    good.write_text("* 1.5 4 5\nutt1 0.25 7\n\n")
    flag = "--bias=" + str(good)
    for bad in ("--bias-settings=", "--bias-settings=1,1,0", "--bias-settings=1,1,0,1,1", "--bias-settings=1,x,0,1", "--bias-settings=-1,1,0,1",
                "--bias-settings=1,nan,0,1", "--bias-settings=1,1,inf,1", "--bias-settings=1,1,0,-0.5", "--bias-settings=1,1,0,inf",
                "--bias-settings=1,1,0,1:", "--bias-settings=1,1,0,1::1,1,0,1", "--bias-settings=1,1,0,1:2,2", "--bias-settings=1,1,0,1;1,1,1,1"):
        p = run(flag, bad)
        assert p.returncode == 1 and "--bias-settings=GS,AS,WIP,BS[:GS,AS,WIP,BS...]:" in p.stderr, bad
    p = run(flag, "--bias-settings=" + ":".join(["1,1,0,1"] * 17))
    assert p.returncode == 1 and "--bias-settings: more than 16 settings" in p.stderr
    p = run("--bias-settings=1,1,0,1")
    assert p.returncode == 1 and "--bias-settings goes with --bias=FILE" in p.stderr
    p = run("--bias=")
    assert p.returncode == 1 and "--bias=FILE:" in p.stderr
    p = run(flag, "--threads=2")
    assert p.returncode == 1 and "--bias goes with the batch shape or --single-stream" in p.stderr
    p = run("--bias=" + str(tmp_path / "none.txt"))
    assert p.returncode == 1 and "cannot read" in p.stderr
    for text in ("utt1 x 5\n", "utt1 1.5\n", "utt1 -1 5\n", "utt1 nan 5\n", "utt1 1.0 5 0\n", "utt1 1.0 5 six\n", "utt1 1.0 " + " ".join(["7"] * 17) + "\n"):
        (tmp_path / "bad.txt").write_text("* 1.0 4 5\n" + text)
        p = run("--bias=" + str(tmp_path / "bad.txt"))
        assert p.returncode == 1 and "--bias: line 2 of" in p.stderr and "KEY bonus w1 w2 ..." in p.stderr, (text, p.stderr)
    # well-formed flags get past the checks, to the config file that is not there
    for args in ((flag,), (flag, "--bias-settings=1,1,0,1"), (flag, "--bias-settings=0,0,-3.5,0:1e0,0.1,2,7.5"), (flag, "--bias-settings=" + ":".join(["1,1,0,1"] * 16)),
                 (flag, "--single-stream"), (flag, "--batch=4")):
        p = run(*args)
        assert p.returncode != 0 and "--bias" not in p.stderr, (args, p.stderr)
    hdr = open(os.path.join(host, "wfst-host.h")).read()
    assert "class BiasLists {" in hdr and "struct BiasedWords {" in hdr and "struct BiasSetting {" in hdr and hdr.count("void BiasedWords(") == 2
    src = open(os.path.join(host, "wfst-host.cc")).read()
    for name in ("wfst_bias_lists_create", "wfst_bias_lists_free", NAME):
        assert "#pragma weak " + name in src
    so = os.path.join(ROOT, "asr-decoder_amd", "lib", "libwfsthost.so")
    syms = subprocess.run(["nm", "-DC", so], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bw " + NAME + r"\b", syms), "a weak reference"
    for name in ("datemoon::GpuBatchDecoder::BiasedWords(", "datemoon::GpuLatticeDecoder::BiasedWords(", "datemoon::BiasLists::Set("):
        assert name in syms, name
    assert "kCall" in src and "BiasedWordsCall(_dec, std::vector<int32_t>(1, _chan)" in src, "over a pool the call runs in the batcher thread"
