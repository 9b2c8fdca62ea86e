"""CPU: the surface of phrase boosting for large lists (wfst_bias_book_compile, wfst_bias_books_*, wfst_decoder_biased_words_sparse) --
the header, the binding's symbol list and the library agree on it, the header states the definition, wfst_bias_book_compile equals
the automaton of tests/bias_sparse_util.py at 257 and 4 096 nodes and keeps the cap of 65 536, the argument errors are raised before
any device work, and what the compiler made of the two kernels."""
import ctypes as C
import importlib
import inspect
import os
import re

import numpy as np
import pytest

import bias_sparse_util as S
from test_bias_surface import chain_list, flat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_DEVICE, E_CAPACITY = -1, -3, -4
NAME = "wfst_decoder_biased_words_sparse"
NEW = ["wfst_bias_book_compile", "wfst_bias_books_create", "wfst_bias_books_info", "wfst_bias_books_free", NAME]


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
    assert args == ["wfst_decoder *d", "const int32_t *channels", "int32_t n", "int32_t use_final_probs", "const wfst_bias_books *books",
                    "const int32_t *book_of", "int32_t n_set", "const double *settings", "int32_t cap_words", "int32_t cap_hits", "int64_t max_cells",
                    "int64_t round_cells", "int32_t *status", "int64_t *n_cells", "int32_t *found", "int32_t *n_arcs", "int32_t *n_hyp",
                    "int32_t *n_hits", "int32_t *hyp_words", "int32_t *begin_frame", "int32_t *end_frame", "int32_t *hit_phrase", "int32_t *hit_word",
                    "double *biased_cost", "double *bonus", "float *tot_score", "float *lm_score"]
    lib = C.CDLL(W.LIB_PATH)
    for name in NEW:
        assert name in W.SYMBOLS and hasattr(lib, name) and re.search(r"\b%s\(" % name, hdr), name
    assert "#define WFST_BIAS_BOOK_MAX_NODES 65536" in hdr and "#define WFST_BIAS_MAX_NODES 256" in hdr
    sig = inspect.signature(W.BatchDecoder.biased_words_sparse).parameters
    assert list(sig) == ["self", "books", "book_of", "settings", "channels", "use_final_probs", "cap_words", "cap_hits", "max_cells", "round_cells"]
    assert sig["book_of"].default is None and sig["settings"].default == ((1, 1, 0, 1),) and sig["channels"].default is None
    assert sig["use_final_probs"].default is True and sig["cap_words"].default == 256 and sig["cap_hits"].default == 64
    assert sig["max_cells"].default == 0 and sig["round_cells"].default == 0
    assert hasattr(W.BiasBooks, "from_phrases") and hasattr(W.BiasBooks, "info") and hasattr(W.BiasBooks, "free") and callable(W.bias_book_compile)


def test_the_header_states_the_definition():
    hdr = open(os.path.join(ROOT, "include", "wfst_decoder.h")).read()
    block = hdr[hdr.index("phrase boosting for large lists: sparse cells over reachable nodes"):hdr.index("int " + NAME)]
    assert hdr.index("int wfst_decoder_biased_words(") < hdr.index("phrase boosting for large lists"), "below the dense call's block"
    block = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", block))
    for phrase in ("A BOOK is a bias list without the 256-node cap", "J <= WFST_BIAS_BOOK_MAX_NODES = 65 536", "exactly wfst_decoder_biased_words'",
                   "breadth first, root 0, by (depth, parent's number, word id)", "then the least source node", "word for word",
                   "this call's answer equals that call's in every byte", "which does not depend on the settings", "R(0) = {0}",
                   "its float32 graph + acoustic sum is finite", "R(t) contains R(s) if olabel(a) == 0", "{delta(i, olabel(a)) : i in R(s)}",
                   "the least fixed point", "v[t][j] finite implies j in R(t)", "holds the same bits as the dense one",
                   "A cell inside R may still be +inf", "n_cells[i] = the sum over t of |R(t)|", "an exact integer",
                   "bias_reach_kernel", "bias_sparse_kernel", "recomputing the node track from the automaton itself", "a binary search among i's children",
                   "max_cells bounds ONE channel's n_cells", "0 = 4 Mi cells", "n_cells[i] = -1", "the others' answers stand", "four times as large",
                   "log4(max_cells / first size) + 1", "round_cells is the number of cost cells", "0 = 32 Mi cells = 256 MiB",
                   "The answers do not depend on max_cells, round_cells or the growth", "round_cells < 0 is WFST_E_ARG", "Any output pointer may be NULL",
                   "n_nodes is set even on WFST_E_CAPACITY", "before any device is touched", "\"bias book K phrase P\"", "more than 65 536 nodes is WFST_E_CAPACITY"):
        assert phrase in block, phrase


def test_the_entry_points_are_a_translation_unit_of_their_own(pkg):
    csrc = os.path.join(ROOT, "asr-decoder_amd", "csrc")
    unit, kernels = os.path.join(csrc, "wfst_capi_bias_sparse.cc"), os.path.join(csrc, "wfst_bias_sparse.hip")
    assert unit in pkg.build.SRCS and kernels in pkg.build.SRCS and os.path.join(csrc, "wfst_capi_bias_sparse.h") in pkg.build.HDRS
    capi, entry, text = open(os.path.join(csrc, "wfst_capi.cc")).read(), open(unit).read(), open(kernels).read()
    driver = open(os.path.join(csrc, "wfst_capi_wordquery.cc")).read()
    for word in NEW + ["biased_words_sparse", "launch_bias_reach", "bias_books", "BiasReachDev"]:
        assert word not in capi and word not in driver, "neither wfst_capi.cc nor the siblings' driver knows the call"
    for piece in ("align_begin(", "align_emit(", "cut_round(", "launch_align_index(", "launch_bias_reach(", "launch_bias_sparse("):
        assert piece in entry, piece
    code = re.sub(r"//.*", "", text)
    assert "void bias_reach_kernel(" in code and "void bias_sparse_kernel(" in code and code.count("__global__") == 2
    assert "align_index_kernel" not in code and "bias_kernel" not in code.replace("bias_reach_kernel", "").replace("bias_sparse_kernel", "")
    assert '#include "wfst_align_index.h"' in text and "aln_carve(" in code
    assert code.count("#pragma clang fp contract(off)") == 4, "the arc cost, the bonus, their difference and the sum onto a cell"
    assert "asm" not in code, "no inline assembly"
    sweep = code[code.index("void bias_sparse_kernel("):]
    for rmw in ("atomicMin", "atomicAdd", "atomicCAS", "atomicExch", "atomicMax", "fetch_"):
        assert rmw not in sweep, "no atomic read-modify-write in the sweep: a cell pulls its minimum"
    assert "sp_delta(" not in sweep[:sweep.index("__builtin_amdgcn_fence")], "the sweep and the walk back never evaluate delta: only the forward reading does"


def test_the_kernels_use_no_scratch_and_little_lds(pkg):
    res = pkg.build.kernel_resources(source=os.path.join(ROOT, "asr-decoder_amd", "csrc", "wfst_bias_sparse.hip"))
    for name in ("bias_reach_kernel", "bias_sparse_kernel"):
        assert name in res, sorted(res)
        r = res[name]
        print(name + ":", r)
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0, "nothing goes to scratch memory"
        assert 0 < r["lds"] <= 1024, "the automaton and the sets stay in global memory: LDS holds the scans' partial sums only"


def compile_raw(W, phrases, cap_nodes=65536):
    I, D = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    ln, words, bonus = flat(phrases)
    n = C.c_int32(-7)
    v = [np.full(max(cap_nodes, 1), -9, np.int32) for _ in range(4)]
    beta = np.full(max(cap_nodes, 1), -9.0)
    rc = W.lib().wfst_bias_book_compile(len(ln), ln.ctypes.data_as(I), words.ctypes.data_as(I), bonus.ctypes.data_as(D), cap_nodes, C.byref(n),
                                        *([x.ctypes.data_as(I) for x in v] + [beta.ctypes.data_as(D)]))
    return rc, n.value, v, beta, W.lib().wfst_last_error().decode()


def random_book(rs, nodes, alphabet):
    """random phrases over a small alphabet (failure links that lead somewhere), the last ones one word long, to exactly `nodes` nodes"""
    out, seen, trie = [], set(), {()}
    while len(trie) < nodes - 6:
        ws = tuple(int(w) for w in rs.randint(1, alphabet + 1, size=rs.randint(1, 7)))
        if ws not in seen:
            seen.add(ws)
            out.append((ws, float(rs.rand() * 3.0)))
            trie.update(ws[:k] for k in range(1, len(ws) + 1))
    out += [((1000 + k,), 0.5) for k in range(nodes - len(trie))]
    return out


def test_book_compile_equals_the_automaton(pkg):
    W = pkg.wfstdec
    rs = np.random.RandomState(7)
    for phrases in ([], [((1, 2, 3), 1.0), ((2, 3), 0.25), ((1, 1), 4.0)], chain_list(256), chain_list(257), random_book(rs, 257, 4),
                    random_book(rs, 4096, 12)):
        A = S.compile_book(phrases)
        got = W.bias_book_compile(phrases)
        assert got["n_nodes"] == A.J
        for key in ("parent", "word", "fail", "phrase"):
            assert np.array_equal(got[key], getattr(A, key)), key
        assert got["beta"].tobytes() == A.beta.tobytes(), "beta bit for bit"
    assert A.J == 4096 and int((A.fail != 0).sum()) > 1000
    # the dense compile still refuses 257 nodes
    with pytest.raises(W.WfstError) as e:
        W.bias_compile(chain_list(257), cap_nodes=300)
    assert e.value.code == E_CAPACITY
    # the caller's rows too short: the count, nothing else
    rc, n, v, _, msg = compile_raw(W, chain_list(300), cap_nodes=299)
    assert rc == E_CAPACITY and n == 300 and "cap_nodes" in msg and np.all(v[0] == -9)


def test_the_cap_of_65536_nodes(pkg):
    W = pkg.wfstdec
    ones = lambda nodes: [((w,), 0.25) for w in range(1, nodes)]   # one-word phrases: nodes - 1 of them and the root
    for nodes in (65535, 65536):
        rc, n, v, beta, msg = compile_raw(W, ones(nodes), cap_nodes=65536)
        assert rc == 0 and n == nodes, msg
        assert np.array_equal(v[1][:nodes], np.arange(nodes)) and not v[0][1:nodes].any() and not v[2][:nodes].any()
        assert np.array_equal(v[3][1:nodes], np.arange(nodes - 1)) and np.all(beta[1:nodes] == 0.25)
    rc, n, v, _, msg = compile_raw(W, ones(65537), cap_nodes=70000)
    assert rc == E_CAPACITY and n == 65537 and "65537 nodes" in msg and "a book holds 65536" in msg and np.all(v[0] == -9)
    rc, h, msg = create_raw(W, [[((1,), 1.0)], ones(65537)])
    assert rc == E_CAPACITY and not h and "bias book 1 " in msg and "65537 nodes" in msg


def create_raw(W, books, device=0):
    I, D = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    n_ph = np.ascontiguousarray([len(p) for p in books], np.int32)
    ln, words, bonus = flat([x for p in books for x in p])
    h = C.c_void_p()
    rc = W.lib().wfst_bias_books_create(len(books), n_ph.ctypes.data_as(I), ln.ctypes.data_as(I), words.ctypes.data_as(I), bonus.ctypes.data_as(D),
                                        device, C.byref(h))
    return rc, h, W.lib().wfst_last_error().decode()


def test_bad_books_are_refused_on_the_host(pkg):
    W = pkg.wfstdec
    good = [((1, 2), 1.0), ((3,), 0.5)]
    nan, inf = float("nan"), float("inf")
    for bad, word in (([((1, 0), 1.0)], "word id"), ([((-4,), 1.0)], "word id"), ([((), 1.0)], "length"), ([(tuple(range(1, 18)), 1.0)], "length"),
                      ([((1,), -0.5)], "bonus"), ([((1,), nan)], "bonus"), ([((1,), inf)], "bonus"), ([((7, 8), 1.0), ((7, 8), 2.0)], "duplicate")):
        rc, h, msg = create_raw(W, [good, good + bad])
        assert rc == E_ARG and not h and word in msg and "bias book 1 phrase %d" % (len(good) + len(bad) - 1) in msg, (bad, msg)
        rc, _, _, _, msg = compile_raw(W, good + bad)
        assert rc == E_ARG and word in msg, (bad, msg)
    rc, h, msg = create_raw(W, [])
    assert rc == E_ARG and not h
    assert W.lib().wfst_bias_books_create(1, None, None, None, None, 0, None) == E_ARG
    assert W.lib().wfst_bias_books_info(None, *([None] * 7)) == E_ARG
    assert compile_raw(W, good, cap_nodes=-1)[0] == E_ARG
    W.lib().wfst_bias_books_free(None)
    # a valid set gets as far as the device: on a machine without one that is the answer
    if W.device_count() == 0:
        rc, h, msg = create_raw(W, [good, chain_list(300), []])
        assert rc == E_DEVICE and not h, msg


def call(W, d=None, channels=True, n_set=1, settings=(1.0, 1.0, 0.0, 1.0), cap_words=8, cap_hits=4, max_cells=0, round_cells=0):
    I, D = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    ch = np.array([0], np.int32)
    st = None if settings is None else np.ascontiguousarray(settings, np.float64)
    rc = W.lib().wfst_decoder_biased_words_sparse(d, ch.ctypes.data_as(I) if channels else None, 1, 1, None, None, n_set,
                                                  None if st is None else st.ctypes.data_as(D), cap_words, cap_hits, C.c_int64(max_cells),
                                                  C.c_int64(round_cells), *([None] * 15))
    return rc, W.lib().wfst_last_error().decode()


def test_argument_errors_come_before_any_device_work(pkg):
    W = pkg.wfstdec
    # a decoder that is never looked at, as in test_bias_surface.py: what passes the checks ends at the fake decoder's channel list
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
    for kw, word in ((dict(n_set=0), "n_set"), (dict(n_set=17, settings=[1.0, 1.0, 0.0, 1.0] * 17), "n_set"), (dict(n_set=-1), "n_set"),
                     (dict(settings=None), "NULL settings"), (dict(cap_words=0), "cap_words"), (dict(cap_words=-3), "cap_words"),
                     (dict(cap_hits=-1), "cap_hits"), (dict(max_cells=-1), "max_cells"), (dict(max_cells=(1 << 30) + 1), "max_cells"),
                     (dict(round_cells=-1), "round_cells")):
        rc, msg = call(W, fake, **kw)
        assert rc == E_ARG and word in msg, (kw, msg)
    for kw in (dict(), dict(settings=(0.0, 0.0, -5.0, 0.0)), dict(n_set=16, settings=[1.0, 0.1, 0.5, 2.0] * 16), dict(cap_hits=0),
               dict(max_cells=1 << 30, round_cells=1)):
        rc, msg = call(W, fake, **kw)
        assert rc == E_ARG and "channel" in msg, (kw, msg)


def test_cli_flags_and_the_host_mirror(pkg, tmp_path):
    import subprocess

    host = os.path.join(ROOT, "asr-decoder_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host])
    cli = os.path.join(host, "wfst-decode")
    run = lambda *a: subprocess.run([cli] + list(a) + ["a", "b", "c"], capture_output=True, text=True)
    p = subprocess.run([cli], capture_output=True, text=True)
    assert p.returncode == 1 and "[--bias=FILE [--bias-settings=GS,AS,WIP,BS[:GS,AS,WIP,BS...]]] [--bias-sparse]" in p.stderr
    p = run("--bias-sparse")
    assert p.returncode == 1 and "--bias-sparse goes with --bias=FILE" in p.stderr
    good = tmp_path / "bias.txt"
    good.write_text("* 1.5 4 5\nutt1 0.25 7\n" + "".join("* 0.5 %d\n" % (1000 + k) for k in range(300)))
    flag = "--bias=" + str(good)
    # well-formed flags get past the checks (a list of more than 256 nodes included), to the config file that is not there
    for args in ((flag,), (flag, "--bias-sparse"), (flag, "--bias-sparse", "--bias-settings=1,1,0,1"), (flag, "--bias-sparse", "--single-stream")):
        p = run(*args)
        assert p.returncode != 0 and "--bias" not in p.stderr, (args, p.stderr)
    p = run(flag, "--bias-sparse", "--threads=2")
    assert p.returncode == 1 and "--bias goes with the batch shape or --single-stream" in p.stderr
    hdr = open(os.path.join(host, "wfst-host.h")).read()
    assert "class BiasBooks {" in hdr and hdr.count("void BiasedWordsSparse(") == 2 and "long long n_cells" in hdr
    src = open(os.path.join(host, "wfst-host.cc")).read()
    for name in ("wfst_bias_books_create", "wfst_bias_books_free", NAME):
        assert "#pragma weak " + name in src
    so = os.path.join(ROOT, "asr-decoder_amd", "lib", "libwfsthost.so")
    syms = subprocess.run(["nm", "-DC", so], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bw " + NAME + r"\b", syms), "a weak reference"
    for name in ("datemoon::GpuBatchDecoder::BiasedWordsSparse(", "datemoon::GpuLatticeDecoder::BiasedWordsSparse(", "datemoon::BiasBooks::Set("):
        assert name in syms, name
    assert "kCall" in src and "BiasedWordsSparseCall(_dec, std::vector<int32_t>(1, _chan)" in src, "over a pool the call runs in the batcher thread"
