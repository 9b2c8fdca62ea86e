"""-m gpu: wfst_decoder_graph_posteriors (graphpost_kernel, graphpost_pack_kernel, graphpost_dense_kernel) -- the forward-backward pass
of a channel's scores over the utterance's own graph, in float64.

The reference of every comparison is the header's recursion restated in numpy (tests/graph_post_util.py) on the same scores, within
the tolerance derived there: tol_log = 8 (n_levels + 2) 2^-52 max(1, A) for log_like, 4 tol_log max(1, |v|) + k 2^-52 for a posterior
over k arcs, T + 1 times that for an occupancy.  Every test prints the largest difference / tolerance it reached."""
import ctypes as C
import json
import os
import re
import threading

import numpy as np
import pytest

import graph_post_util as U
from golden_util import GOLDEN_DIR

pytestmark = pytest.mark.gpu

E_ARG, E_CAPACITY, E_STATE = -1, -4, -5
N_TID = 600
N_PDF = N_TID // 2
LIM = dict(max_frames=192, max_tokens_per_frame=32768, arena_tokens=1 << 20)
LAT = dict(lattice_links=1 << 21)
CFG = dict(beam=12.0, max_active=1000000, min_active=0, lattice_beam=6.0, prune_interval=10)


@pytest.fixture(scope="module")
def world(synth, tmp_path_factory):
    import gpu_util as G

    W = G.wfstdec
    g = synth.make_hclg_like(3000, seed=21, n_tid=N_TID, n_words=500)
    m = synth.default_tid2pdf(N_TID)
    path = str(tmp_path_factory.mktemp("gpost") / "g.bin")
    g.write(path)
    graph = W.Graph.load(path)
    graph.set_tid2pdf(m)
    mats = [synth.make_loglikes(g, T, N_PDF, m, seed=s, mu=-2.2)[0] for T, s in ((40, 700), (97, 701), (150, 702))]
    yield dict(G=G, W=W, graph=graph, m=m, mats=mats, T=[x.shape[0] for x in mats], path=path)
    graph.free()


def decoder(world, n, lattice=False, **kw):
    lim = dict(LIM)
    if lattice:
        lim.update(LAT)
    lim.update(kw)
    return world["W"].BatchDecoder(world["graph"], world["G"].gpu_config(CFG), n, **lim)


def scores(T, seed, cols=N_PDF):
    return np.random.default_rng(seed).normal(-2.5, 1.2, size=(T, cols)).astype(np.float32)


def feed_host(dec, mats, channels=None, decode=True):
    """InitDecoding, then the rows of every listed channel that has any; decode=False: handed over, not decoded"""
    ch = list(range(len(mats))) if channels is None else list(channels)
    dec.init(ch)
    have = [(c, x) for c, x in zip(ch, mats) if x.shape[0] > 0]
    if have:
        dec.advance_host([x for _, x in have], [x.shape[0] for _, x in have], [c for c, _ in have], max_num_frames=-1 if decode else 0)


def check(world, dec, graphs, channels, lls, graph_of=None, n_frames=None, label_map=None, tid2pdf="world", gs=1.0, as_=1.0, min_post=0.0,
          what="", ag=None, **kw):
    """graph_posteriors of the list against the restatement on lls[i]; returns (got, want)"""
    W = world["W"]
    m = world["m"] if isinstance(tid2pdf, str) else tid2pdf
    own = ag is None
    if own:
        ag = W.AlignGraphs.from_arrays([U.as_tuple(g) for g in graphs])
    try:
        got = dec.graph_posteriors(ag, graph_of, channels, n_frames, label_map, gs, as_, min_post, arc_occupancy=True, **kw)
    finally:
        if own:
            ag.free()
    want, worst = [], 0.0
    for i, c in enumerate(channels):
        g = graphs[graph_of[i] if graph_of is not None else i]
        T = n_frames[i] if n_frames is not None and n_frames[i] is not None and n_frames[i] >= 0 else lls[i].shape[0]
        want.append(U.graph_posteriors(g, lls[i], T, m, label_map, gs, as_, min_post))
        worst = max(worst, U.compare(got[i], want[-1], "%s channel %d" % (what, c), min_post))
    print("%s: largest difference / tolerance %.4f" % (what, worst))
    return got, want


def raw_bytes(r):
    return (r.status, r.found, r.n_frames, np.float64(r.log_like).tobytes(), r.frame_off.tobytes(), r.classes.tobytes(), r.posts.tobytes(),
            r.n_distinct.tobytes(), r.frame_mass.tobytes(), None if r.arc_occ is None else r.arc_occ.tobytes())


# ---- 1. mixed list ---------------------------------------------------------------------------------------------------------------------
def test_mixed_list(world):
    """eight channels with different graphs through graph_of, 50 .. 300 states, T in {0, 1, 2, 37, 150}"""
    Ts = [0, 1, 2, 37, 150, 37, 150, 2]
    graphs = [U.transcript_graph(range(1, 31), seed=1, n_tid=N_TID),                   # 0: T = 150
              U.hclg_graph(299, 5, N_TID),                                              # 1: T = 37
              U.transcript_graph(range(1, 13), seed=2, n_tid=N_TID, bypass=True),       # 2: T = 0
              U.transcript_graph(range(1, 8), seed=3, n_tid=N_TID),                     # 3: T = 37
              U.transcript_graph(range(1, 14), seed=4, n_tid=N_TID, bypass=True),       # 4: T = 1
              U.hclg_graph(120, 6, N_TID),                                              # 5: T = 2
              U.transcript_graph(range(1, 26), seed=7, n_tid=N_TID),                    # 6: T = 150
              U.transcript_graph(range(1, 15), seed=8, n_tid=N_TID, bypass=True)]       # 7: T = 2
    assert all(50 <= g.n_states <= 300 for g in graphs), [g.n_states for g in graphs]
    graph_of = [2, 4, 5, 3, 0, 1, 6, 7]
    lls = [scores(T, 100 + i) for i, T in enumerate(Ts)]
    dec = decoder(world, 8)
    ag = world["W"].AlignGraphs.from_arrays([U.as_tuple(g) for g in graphs])
    try:
        feed_host(dec, lls)
        got, want = check(world, dec, graphs, list(range(8)), lls, graph_of, what="mixed", ag=ag)
        found = [g.found for g in got]
        print("mixed: states %s, T %s, found %s" % ([graphs[k].n_states for k in graph_of], Ts, found))
        assert found[0] and found[1] and found[3] and found[4] and found[6] and found[7] and not all(found)
        assert got[0].n_frames == 0 and got[0].n_entries == 0 and got[0].log_like != 0.0 and got[0].arc_occ.sum() > 0   # T = 0: epsilon arcs only
        # a sublist in another order: a channel's bytes do not depend on the list
        sub = dec.graph_posteriors(ag, [6, 4, 0], [6, 1, 4], arc_occupancy=True)
        for r, c in zip(sub, [6, 1, 4]):
            assert raw_bytes(r) == raw_bytes(got[c]), c
        # fewer frames than held
        check(world, dec, graphs, [6, 1, 4], [lls[6], lls[1], lls[4]], [6, 4, 0], n_frames=[100, -1, 120], what="sublist", ag=ag)
    finally:
        ag.free()
        dec.free()


# ---- 2. the state count around WFST_GPOST_LDS_STATES ----------------------------------------------------------------------------------
def test_state_count_edges(world):
    L = U.WFST_GPOST_LDS_STATES
    graphs = [U.fan_graph(n, 40 + k, N_TID) for k, n in enumerate((L - 1, L, L + 1))]
    assert [g.n_states for g in graphs] == [L - 1, L, L + 1]
    lls = [scores(3, 200 + i) for i in range(3)]
    dec = decoder(world, 3)
    try:
        feed_host(dec, lls)
        got, _ = check(world, dec, graphs, [0, 1, 2], lls, what="state edges")
        assert all(g.found and g.n_frames == 3 for g in got)
        # the answers do not depend on where the rows live: the same scores, the graphs swapped between the channels
        check(world, dec, [graphs[2], graphs[0], graphs[1]], [0, 1, 2], lls, what="state edges swapped")
    finally:
        dec.free()


def kernel_constants():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dev = open(os.path.join(root, "asr-decoder_amd", "csrc", "wfst_device.h")).read()
    hip = open(os.path.join(root, "asr-decoder_amd", "csrc", "wfst_graphpost.hip")).read()
    return int(re.search(r"kFalignLdsLabels = (\d+);", dev).group(1)), int(re.search(r"kGpThreads = (\d+);", hip).group(1))


# ---- 3. the distinct ilabels around the staging constant ------------------------------------------------------------------------------
def test_distinct_label_count_edges(synth, tmp_path):
    """one label less than the staged scores hold, exactly that many and one more, on either side of WFST_GPOST_LDS_STATES too"""
    import gpu_util as G

    W = G.wfstdec
    NL, _ = kernel_constants()
    L = U.WFST_GPOST_LDS_STATES
    n_tid = NL + 176
    g = synth.make_hclg_like(1000, seed=23, n_tid=n_tid, n_words=100)
    m = synth.default_tid2pdf(n_tid)
    path = str(tmp_path / "g.bin")
    g.write(path)
    graph = W.Graph.load(path)
    graph.set_tid2pdf(m)
    shapes = [(NL // 2 + 8, NL - 1), (NL // 2 + 8, NL), (NL // 2 + 8, NL + 1), (L + 3, NL - 1), (L + 3, NL), (L + 3, NL + 1)]
    graphs = [U.label_fan_graph(S, n, 300 + k) for k, (S, n) in enumerate(shapes)]
    lls = [scores(3 + k % 2, 310 + k, cols=n_tid // 2) for k in range(len(shapes))]
    dec = W.BatchDecoder(graph, G.gpu_config(CFG), len(shapes), **LIM)
    ag = W.AlignGraphs.from_arrays([U.as_tuple(x) for x in graphs])
    world = dict(W=W, m=m)
    try:
        assert list(ag.info()["n_labels"]) == [n for _, n in shapes] and list(ag.info()["n_states"]) == [S for S, _ in shapes]
        feed_host(dec, lls)
        got, _ = check(world, dec, graphs, list(range(6)), lls, what="label edges", ag=ag)
        assert all(r.found for r in got)
        check(world, dec, graphs, list(range(6)), lls, [2, 0, 1, 5, 3, 4], what="label edges swapped", ag=ag)
    finally:
        ag.free()
        dec.free()
        graph.free()


# ---- 4. epsilon structure ---------------------------------------------------------------------------------------------------------------
def eps_chain_graph(k, seed, detour=False):
    """chains of k epsilon arcs of either sign out of start at frame 0, in mid-utterance and into final_state at frame T, with
    emitting self-loops between them: epsilon depth k; detour: a second way of two arcs round every chain's first link (depth k + 1)"""
    rng = np.random.default_rng(seed)
    B = U.Builder()
    w = lambda: float(np.float32(rng.uniform(-0.5, 1.5)))
    tid = lambda: int(rng.integers(1, N_TID + 1))

    def eps_chain(s, word):
        for j in range(k):
            t = B.state()
            B.arc(s, 0, word if j == k - 1 else 0, w(), t)
            if j == 0 and detour:   # two paths: the sum differs from the minimum
                u = B.state()
                B.arc(s, 0, 0, w(), u)
                B.arc(u, 0, 0, w(), t)
            s = t
        return s

    start = B.state()
    a = eps_chain(start, 11)
    b = B.state()
    B.arc(a, tid(), 0, w(), b)
    B.arc(b, tid(), 0, w(), b)
    c = eps_chain(b, 12)
    d = B.state()
    B.arc(c, tid(), 13, w(), d)
    B.arc(d, tid(), 0, w(), d)
    return B.build(start, eps_chain(d, 14))


def test_epsilon_structure(world):
    _, lanes = kernel_constants()
    graphs = [eps_chain_graph(k, 60 + k) for k in (1, 2, 4)] + [U.eps_fan_graph(lanes + 37, 70, N_TID),
                                                                  U.transcript_graph(range(1, 12), seed=5, n_tid=N_TID, bypass=True),
                                                                  eps_chain_graph(2, 66, detour=True)]
    assert [int(U.eps_levels(g).max()) for g in graphs[:3] + graphs[5:]] == [1, 2, 4, 3] and int(np.bincount(U.eps_levels(graphs[3]))[1]) > lanes
    Ts = [9, 9, 9, 4, 0, 9]
    lls = [scores(T, 300 + i) for i, T in enumerate(Ts)]
    dec = decoder(world, 6)
    try:
        feed_host(dec, lls)
        got, want = check(world, dec, graphs, list(range(6)), lls, what="epsilon")
        assert all(r.found for r in got)
        assert got[4].n_frames == 0 and got[4].n_entries == 0 and got[4].log_like != 0.0       # the bypass at T = 0
        assert np.any((got[5].arc_occ > 0.01) & (got[5].arc_occ < 0.99))                      # the sum is over more than one path
    finally:
        dec.free()


# ---- 5. the "no arc" rule ---------------------------------------------------------------------------------------------------------------
def test_no_arc_rule(world):
    import torch

    g = U.transcript_graph(range(1, 6), seed=10, n_tid=N_TID)
    ll = scores(20, 400)
    clean = U.force_align(g, ll, 20, world["m"])
    assert clean["found"]
    cols = world["m"][clean["alignment"]]
    bad = ll.copy()
    bad[:, cols[3]] = -np.inf          # a column of -inf: the arcs that read it are no arcs at any frame
    bad[10, cols[10]] = np.nan         # on the best path
    bad[15, cols[15]] = np.inf
    dead = ll.copy()
    dead[7, :] = -np.inf               # a frame at which every arc dies
    B = U.Builder()                    # a non-finite arc weight: the only way round it is the dearer one
    s = B.states(4)
    B.arc(s[0], 5, 0, float("inf"), s[1])
    B.arc(s[0], 6, 0, 2.0, s[1])
    B.arc(s[1], 7, 0, float("nan"), s[1])
    B.arc(s[1], 8, 0, 0.5, s[1])
    B.arc(s[1], 0, 0, float("-inf"), s[3])
    B.arc(s[1], 0, 0, 0.25, s[2])
    B.arc(s[2], 0, 0, 0.0, s[3])
    gw = B.build(s[0], s[3])
    dec = decoder(world, 4)
    sentinel = 7.5
    grad = [torch.full((20, N_TID + 1), sentinel, device="cuda:0") for _ in range(4)]
    try:
        feed_host(dec, [ll, bad, dead, ll])
        got, want = check(world, dec, [g, g, g, gw], [0, 1, 2, 3], [ll, bad, dead, ll], what="no arc", grad=grad)
        assert got[0].found and got[3].found and not got[2].found and got[2].status == 0
        assert got[2].n_frames == 0 and got[2].log_like == 0.0 and got[2].n_entries == 0 and not np.any(got[2].arc_occ)
        assert got[1].log_like < got[0].log_like or not got[1].found
        assert got[3].arc_occ[0] == 0.0 and abs(got[3].arc_occ[1] - 1.0) < 1e-9
        torch.cuda.synchronize()
        assert bool((grad[2] == sentinel).all())          # its dense rows untouched
        assert bool((grad[0] != sentinel).all())
    finally:
        dec.free()


# ---- 6. scales --------------------------------------------------------------------------------------------------------------------------
def test_scales(world):
    graphs = [U.transcript_graph(range(1, 9), seed=12, n_tid=N_TID), U.transcript_graph([1], seed=13, n_tid=N_TID, states_per_word=(2, 2))]
    lls = [scores(40, 410), scores(5, 411)]
    dec = decoder(world, 2)
    ag = world["W"].AlignGraphs.from_arrays([U.as_tuple(g) for g in graphs])
    try:
        feed_host(dec, lls)
        ll_of = {}
        for gs, as_ in ((1.0, 1.0), (0.0, 1.0), (1.0, 0.0), (0.3, 2.5), (0.0, 0.0)):
            got, want = check(world, dec, graphs, [0, 1], lls, gs=gs, as_=as_, what="scales (%g, %g)" % (gs, as_), ag=ag)
            assert got[0].found and got[1].found
            ll_of[(gs, as_)] = got[0].log_like
        assert len(set(ll_of.values())) == 5
        n = U.enumerate_posteriors(graphs[1], lls[1], 5, world["m"], None, 0.0, 0.0)["n_paths"]
        assert n > 1 and abs(got[1].log_like - np.log(n)) <= want[1]["tol_log"], (got[1].log_like, n)
    finally:
        ag.free()
        dec.free()


# ---- 7. classes -------------------------------------------------------------------------------------------------------------------------
def test_classes(world):
    W = world["W"]
    graphs = [U.transcript_graph(range(1, 12), seed=14, n_tid=N_TID), U.transcript_graph(range(1, 6), seed=15, n_tid=N_TID, bypass=True)]
    lls = [scores(60, 420), scores(30, 421)]
    phone = ((np.arange(N_TID + 1) + 3) // 4).astype(np.int32)
    dec = decoder(world, 2)
    ag = W.AlignGraphs.from_arrays([U.as_tuple(g) for g in graphs])
    try:
        feed_host(dec, lls)
        for name, m in (("tid", None), ("pdf", world["m"]), ("phone", phone)):
            got, want = check(world, dec, graphs, [0, 1], lls, label_map=m, what="classes %s" % name, ag=ag)
            thin, _ = check(world, dec, graphs, [0, 1], lls, label_map=m, min_post=0.05, what="classes %s, min_post" % name, ag=ag)
            for r, t, w in zip(got, thin, want):
                assert r.found
                assert t.n_entries < r.n_entries and np.all(t.posts >= 0.05)
                assert np.array_equal(t.n_distinct, r.n_distinct) and t.frame_mass.tobytes() == r.frame_mass.tobytes()
                assert np.all(np.abs(r.frame_mass - 1.0) <= U.post_tol(w, 1.0, w["k_class"].sum()))
                # frame_post_lookup reads the result as it stands: the largest class of every frame, and one that is not listed
                dense = U.dense_of(r, w["post"].shape[1])
                top = dense.argmax(axis=1)
                assert np.array_equal(W.frame_post_lookup(r, top), dense[np.arange(len(top)), top])
                assert not np.any(W.frame_post_lookup(r, np.full(len(top), dense.shape[1] + 3)))
    finally:
        ag.free()
        dec.free()


def raw_call(W, dec, ag, channels, graph_of, capf, cape, capa=0, n_frames=None, label_map=None, n_tid=0, gs=1.0, as_=1.0, min_post=0.0,
             max_cells=0, grad=None, pitch=None, rows=None, n_cols=0, grad_scale=1.0, stream=-1, d=True, occ=True):
    """the C entry point itself, with rows of the caller's size: dict of the raw output arrays and the return code"""
    I, D = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    ch = None if channels is None else np.ascontiguousarray(channels, np.int32)
    gof = None if graph_of is None else np.ascontiguousarray(graph_of, np.int32)
    n = len(channels) if channels is not None else 1
    i32 = lambda *s: np.full(s, 99, np.int32)
    f64 = lambda *s: np.full(s, 9.0, np.float64)
    o = dict(status=i32(n), found=i32(n), n_frames=i32(n), log_like=f64(n), n_entries=i32(n), n_arcs=i32(n), off=i32(n, max(capf, 0) + 1),
             nd=i32(n, max(capf, 1)), mass=f64(n, max(capf, 1)), cls=i32(n, max(cape, 1)), post=f64(n, max(cape, 1)), occ=f64(n, max(capa, 1)))
    p = lambda a: None if a is None else a.ctypes.data_as({np.dtype(np.int32): I, np.dtype(np.float64): D, np.dtype(np.int64): C.POINTER(C.c_int64)}[a.dtype])
    nfi = None if n_frames is None else np.ascontiguousarray(n_frames, np.int32)
    lm = None if label_map is None else np.ascontiguousarray(label_map, np.int32)
    ptrs = None
    if grad is not None:
        ptrs = (C.c_void_p * n)(*[None if x is None else int(x) for x in grad])
    pitch = None if pitch is None else np.ascontiguousarray(pitch, np.int64)
    rows = None if rows is None else np.ascontiguousarray(rows, np.int32)
    o["rc"] = W.lib().wfst_decoder_graph_posteriors(
        dec.h if d else None, p(ch), n, ag.h if ag is not None else None, p(gof), p(nfi), p(lm), n_tid, C.c_double(gs), C.c_double(as_),
        C.c_double(min_post), C.c_int64(max_cells), capf, cape, capa, ptrs, p(pitch), p(rows), n_cols, C.c_double(grad_scale), C.c_void_p(stream),
        p(o["status"]), p(o["found"]), p(o["n_frames"]), p(o["log_like"]), p(o["n_entries"]), p(o["n_arcs"]), p(o["off"]), p(o["nd"]), p(o["mass"]),
        p(o["cls"]), p(o["post"]), p(o["occ"]) if occ and capa > 0 else None)
    return o


# ---- 8. arc occupancies -----------------------------------------------------------------------------------------------------------------
def test_arc_occupancies(world):
    W = world["W"]
    graphs = [U.transcript_graph(range(1, 10), seed=16, n_tid=N_TID), U.transcript_graph(range(1, 4), seed=17, n_tid=N_TID)]
    lls = [scores(50, 430), scores(25, 431)]
    dec = decoder(world, 2)
    ag = W.AlignGraphs.from_arrays([U.as_tuple(g) for g in graphs])
    try:
        feed_host(dec, lls)
        got, want = check(world, dec, graphs, [0, 1], lls, what="occupancies", ag=ag)
        for r, w, g in zip(got, want, graphs):
            emit = g.arcs["ilabel"] != 0
            T = r.n_frames
            assert r.found and len(r.arc_occ) == g.n_arcs == r.n_arcs
            assert abs(r.arc_occ[emit].sum() - T) <= T * U.post_tol(w, 1.0, int(emit.sum()))
        # cap_arcs too small for one channel of the list: its own WFST_E_CAPACITY with the room needed, the other complete
        A = [g.n_arcs for g in graphs]
        assert A[0] > A[1]
        o = raw_call(W, dec, ag, [0, 1], [0, 1], 64, 64 * 512, capa=A[1])
        assert o["rc"] == 0 and list(o["status"]) == [E_CAPACITY, 0] and list(o["n_arcs"]) == A and not np.any(o["occ"][0])
        assert o["occ"][1].tobytes() == got[1].arc_occ.tobytes() and o["log_like"][0] == got[0].log_like and "cap_arcs" in W.lib().wfst_last_error().decode()
        o = raw_call(W, dec, ag, [0, 1], [0, 1], 64, 64 * 512, capa=A[0])
        assert list(o["status"]) == [0, 0] and o["occ"][0].tobytes() == got[0].arc_occ.tobytes()
        # ... and the binding repeats the call once
        rep = dec.graph_posteriors(ag, arc_occupancy=True, cap_arcs=3)
        assert [raw_bytes(r) for r in rep] == [raw_bytes(r) for r in got]
        assert dec.graph_posteriors(ag)[0].arc_occ is None
    finally:
        ag.free()
        dec.free()


# ---- 9. dense rows ----------------------------------------------------------------------------------------------------------------------
def test_dense_rows(world):
    import torch

    W = world["W"]
    m = world["m"]
    graphs = [U.transcript_graph(range(1, 5), seed=18 + c, n_tid=N_TID) for c in range(4)]
    Ts = [40, 33, 21, 40]
    lls = [scores(T, 440 + i) for i, T in enumerate(Ts)]
    dec = decoder(world, 4)
    ag = W.AlignGraphs.from_arrays([U.as_tuple(g) for g in graphs])
    sentinel, scale = -3.25, -0.37
    try:
        feed_host(dec, lls)
        side = torch.cuda.Stream()
        for stream in (side, W.WFST_STREAM_NONE, None):
            wide = torch.empty((44, N_PDF + 9), device="cuda:0")     # a pitch above n_cols, more rows than frames
            short = torch.empty((20, N_PDF), device="cuda:0")        # grad_frames below T
            exact = torch.empty((40, N_PDF), device="cuda:0")
            if stream is side:
                with torch.cuda.stream(side):
                    for t in (wide, short, exact):
                        t.fill_(sentinel)                            # the fill is on the consumer's stream: the writes wait for it
            else:
                for t in (wide, short, exact):
                    t.fill_(sentinel)
                torch.cuda.synchronize()
            grad = [wide[:, :N_PDF], short, None, exact]
            got = dec.graph_posteriors(ag, label_map=m, min_post=0.2, grad=grad, grad_scale=scale, consumer_stream=stream)
            full = dec.graph_posteriors(ag, label_map=m)
            if stream is side:
                side.synchronize()                                   # the stream waits behind the writes
            else:
                torch.cuda.synchronize()
            for i, t in ((0, wide), (1, short), (3, exact)):
                assert got[i].found and got[i].log_like == full[i].log_like
                dense = U.dense_of(full[i], N_PDF)[:, :N_PDF]
                have = t.cpu().numpy()
                rows = min(Ts[i], have.shape[0])
                expect = np.full(have.shape, sentinel, np.float32)
                expect[:rows, :N_PDF] = np.where(dense[:rows] > 0, (scale * dense[:rows]).astype(np.float32), np.float32(0))
                assert have.tobytes() == expect.tobytes(), (i, stream)
                assert got[i].n_entries < full[i].n_entries       # min_post thins the lists, not the rows
        # the dense output only
        exact.fill_(sentinel)
        torch.cuda.synchronize()
        only = dec.graph_posteriors(ag, label_map=m, grad=[None, None, None, exact], lists=False)
        torch.cuda.synchronize()
        assert only[3].log_like == full[3].log_like and len(only[3].classes) == 0
        assert exact.cpu().numpy().tobytes() == np.where(dense > 0, dense.astype(np.float32), np.float32(0)).tobytes()
    finally:
        ag.free()
        dec.free()


# ---- 10. where the scores come from -----------------------------------------------------------------------------------------------------
def test_chunks_in_f16_with_scale_and_priors(world):
    import torch

    T, scale = 60, 0.1
    prior = np.random.RandomState(20).normal(-5.0, 1.5, N_PDF).astype(np.float32)
    raw = [torch.from_numpy((scores(T, 500 + c) / np.float32(scale) + prior).astype(np.float32)).to(torch.float16).to("cuda:0") for c in range(2)]
    graphs = [U.transcript_graph(range(1, 9), seed=20 + c, n_tid=N_TID) for c in range(2)]
    dec = decoder(world, 2)
    try:
        dec.set_score_transform(scale, prior)
        dec.init()
        dec.advance_chunk([raw[0][:25], raw[1][:31]])
        dec.advance_chunk([raw[0][25:], raw[1][31:]], max_num_frames=0)     # the second chunks are held, not decoded
        assert dec.num_frames_decoded(0) == 25 and dec.num_frames_decoded(1) == 31
        lls = [dec.scores(c, 0, T) for c in range(2)]
        got, _ = check(world, dec, graphs, [0, 1], lls, what="chunks")
        assert all(r.found and r.n_frames == T for r in got)
    finally:
        dec.free()


def test_the_callers_matrix_and_never_decoded_channels(world):
    G = world["G"]
    mats = world["mats"]
    dev = G.upload(mats[:2])
    graphs = [U.transcript_graph(range(1, 6), seed=30 + c, n_tid=N_TID, bypass=True) for c in range(3)]
    dec = decoder(world, 3)
    try:
        dec.init()
        # channel 0: all 40 frames of the caller's matrix decoded; channel 1: 30 of 97; channel 2: rows handed over, none decoded
        dec.advance([dev[0].data_ptr(), dev[1].data_ptr()], [40, 97], N_PDF, channels=[0, 1], max_num_frames=30)
        dec.advance([dev[0].data_ptr()], [40], N_PDF, channels=[0])
        dec.advance_host([mats[2]], [150], channels=[2], max_num_frames=0)
        assert [dec.num_frames_decoded(c) for c in range(3)] == [40, 30, 0]
        got, _ = check(world, dec, graphs, [0, 1, 2], [mats[0], mats[1][:30], mats[2]], what="sources")
        assert [r.n_frames for r in got] == [40, 30, 150] and all(r.found for r in got)
        check(world, dec, graphs, [1, 2], [mats[1], mats[2]], [1, 2], n_frames=[17, 64], what="fewer frames")
    finally:
        dec.free()


def test_live_and_finalized_channels_and_the_decoder_is_untouched(world):
    """a live channel mid-utterance and a finalized one in one call; a twin without the call ends in the same best paths, bit for bit"""
    mats = world["mats"]
    graphs = [U.transcript_graph(range(1, 10), seed=40, n_tid=N_TID), U.transcript_graph(range(1, 7), seed=41, n_tid=N_TID)]
    a, b = decoder(world, 2, lattice=True), decoder(world, 2, lattice=True)
    try:
        for dec in (a, b):
            dec.init()
            dec.advance_host([mats[1], mats[2][:60]], [97, 60])
            dec.finalize([0])
        got, _ = check(world, a, graphs, [0, 1], [mats[1], mats[2][:60]], what="live + finalized")
        assert got[0].found and got[1].found and [r.n_frames for r in got] == [97, 60]
        for dec in (a, b):
            dec.advance_host([mats[2]], [150], channels=[1])
        check(world, a, graphs, [1], [mats[2]], [0], what="live, later")
        for dec in (a, b):
            dec.finalize([1])
        pa, pb = a.best_paths(), b.best_paths()
        for x, y in zip(pa, pb):
            for k in ("ilabel", "olabel"):
                assert np.array_equal(x[k], y[k])
            for k in ("graph", "ac"):
                assert np.array_equal(x[k].view(np.uint32), y[k].view(np.uint32))
            assert U.bits(x["tot_score"]) == U.bits(y["tot_score"]) and U.bits(x["lm_score"]) == U.bits(y["lm_score"])
    finally:
        a.free()
        b.free()


def test_a_biglm_decoder(world, tmp_path):
    G, W = world["G"], world["W"]
    z = np.load(os.path.join(GOLDEN_DIR, "biglm_hclg600.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    with open(tmp_path / "g.bin", "wb") as f:
        f.write(bytes(z["graph"]))
    graph = W.Graph.load(str(tmp_path / "g.bin"))
    m = np.asarray(z["tid2pdf"], np.int32)
    graph.set_tid2pdf(m)
    pname = [p for p in meta["pairs"] if p != "unigram"][0]
    lms = []
    for tag, scale in (("old", -1.0), ("new", 1.0)):
        p = str(tmp_path / ("lm_%s.bin" % tag))
        with open(p, "wb") as f:
            f.write(bytes(z["lm_%s_%s" % (pname, tag)]))
        lms.append(W.Lm.load(p, scale))
    mats = [np.asarray(z["ll_%d" % i], np.float32) for i in range(2)]
    n_tid = len(m) - 1
    dec = W.BatchDecoder(graph, G.gpu_config(dict(beam=13.0, max_active=1000000, min_active=0, lattice_beam=25.0, prune_interval=7)), 2,
                         old_lm=lms[0], new_lm=lms[1], max_frames=64, max_tokens_per_frame=32768, arena_tokens=1 << 20, lattice_links=1 << 21)
    try:
        dev = G.upload(mats)
        dec.init()
        dec.advance([t.data_ptr() for t in dev], [x.shape[0] for x in mats], int(mats[0].shape[1]))
        dec.finalize([1])
        graphs = [U.transcript_graph(range(1, 4), seed=50 + c, n_tid=n_tid, bypass=True) for c in range(2)]
        got, _ = check(world, dec, graphs, [0, 1], mats, tid2pdf=m, what="biglm")
        assert all(r.found and r.n_frames == x.shape[0] for r, x in zip(got, mats))
    finally:
        dec.free()
        for lm in lms:
            lm.free()
        graph.free()


# ---- 11. beside force_align -------------------------------------------------------------------------------------------------------------
def test_beside_force_align(world):
    m = world["m"]
    rng = np.random.default_rng(33)
    hops = [(int(rng.integers(1, N_TID + 1)), k % 3, float(np.float32(rng.uniform(0, 2)))) if k % 4 else (0, 0, -0.25) for k in range(16)]
    graphs = [U.transcript_graph(range(1, 9), seed=34, n_tid=N_TID), U.transcript_graph(range(1, 5), seed=35, n_tid=N_TID, bypass=True), U.chain_graph(hops),
              U.chain_graph(hops)]
    Ts = [50, 20, 12, 9]    # the chain takes exactly 12 frames: channel 3 is not found
    lls = [scores(T, 450 + i) for i, T in enumerate(Ts)]
    dec = decoder(world, 4)
    ag = world["W"].AlignGraphs.from_arrays([U.as_tuple(g) for g in graphs])
    try:
        feed_host(dec, lls)
        fa = dec.force_align(ag)
        got, want = check(world, dec, graphs, [0, 1, 2, 3], lls, what="beside force_align", ag=ag)
        assert [r.found for r in got] == [a.found for a in fa] == [True, True, True, False]
        for r, a, w, g, ll in zip(got, fa, want, graphs, lls):
            if not r.found:
                continue
            cost = U.hop_cost(g, ll, a.hop_arc, m)
            assert -r.log_like <= cost + w["tol_log"]
            assert np.all(world["W"].frame_post_lookup(r, a.alignment) > 0)
        # a single path: the sum is the path
        assert abs(-got[2].log_like - U.hop_cost(graphs[2], lls[2], fa[2].hop_arc, m)) <= want[2]["tol_log"]
        assert np.all(np.abs(got[2].posts - 1.0) <= U.post_tol(want[2], 1.0, 1)) and got[2].n_entries == 12
        assert -got[0].log_like < U.hop_cost(graphs[0], lls[0], fa[0].hop_arc, m) - 1e-6     # many paths: strictly more likely
    finally:
        ag.free()
        dec.free()


# ---- 12. capacities and errors ----------------------------------------------------------------------------------------------------------
def test_capacities_and_errors(world):
    import torch

    W = world["W"]
    graphs = [U.transcript_graph(range(1, 7), seed=70, n_tid=N_TID), U.transcript_graph(range(1, 31), seed=71, n_tid=N_TID),
              U.chain_graph([(N_TID + 5, 1, 0.5)])]
    lls = [scores(40, 600), scores(150, 601)]
    dec = decoder(world, 4)
    ag = W.AlignGraphs.from_arrays([U.as_tuple(g) for g in graphs])
    try:
        feed_host(dec, lls, [0, 1])
        good = dec.graph_posteriors(ag, [0, 1], [0, 1])
        assert good[0].found and good[1].found
        ne = [r.n_entries for r in good]
        assert ne[1] > ne[0]
        S1 = graphs[1].n_states

        def same(o, i, r):
            return (o["found"][i] == 1 and o["log_like"][i] == r.log_like and o["n_entries"][i] == r.n_entries and
                    o["cls"][i, :r.n_entries].tobytes() == r.classes.tobytes() and o["post"][i, :r.n_entries].tobytes() == r.posts.tobytes() and
                    o["off"][i, :r.n_frames + 1].tobytes() == r.frame_off.tobytes())

        # max_cells exceeded on one channel only
        o = raw_call(W, dec, ag, [0, 1], [0, 1], 160, ne[1], max_cells=151 * S1 - 1)
        assert o["rc"] == 0 and list(o["status"]) == [0, E_CAPACITY] and list(o["found"]) == [1, 0] and o["n_frames"][1] == 150 and o["n_entries"][1] == 0
        assert same(o, 0, good[0]) and "max_cells" in W.lib().wfst_last_error().decode()
        o = raw_call(W, dec, ag, [0, 1], [0, 1], 160, ne[1], max_cells=151 * S1)
        assert list(o["status"]) == [0, 0] and same(o, 0, good[0]) and same(o, 1, good[1])
        # cap_frames, then cap_entries, too small for channel 1: the counts are the room needed, its lists stay zero, log_like stands
        for capf, cape in ((149, ne[1]), (150, ne[1] - 1), (40, ne[0])):
            o = raw_call(W, dec, ag, [0, 1], [0, 1], capf, cape)
            assert o["rc"] == 0 and list(o["status"]) == [0, E_CAPACITY], (capf, cape)
            assert (o["n_frames"][1], o["n_entries"][1]) == (150, ne[1]) and o["log_like"][1] == good[1].log_like
            assert not np.any(o["cls"][1]) and not np.any(o["post"][1]) and not np.any(o["off"][1]) and same(o, 0, good[0])
        o = raw_call(W, dec, ag, [0, 1], [0, 1], 150, ne[1])
        assert list(o["status"]) == [0, 0] and same(o, 1, good[1])
        # ... and the binding repeats the call once
        rep = dec.graph_posteriors(ag, [0, 1], [0, 1], cap_frames=3, cap_entries=5)
        assert [raw_bytes(r) for r in rep] == [raw_bytes(r) for r in good]
        # every WFST_E_ARG / WFST_E_STATE of the header, none of which reaches the device: the workspace stays as it is
        ws = dec.graph_posteriors_workspace()
        ok = dict(channels=[0, 1], graph_of=[0, 1], capf=160, cape=ne[1])
        call = lambda **kw: raw_call(W, dec, kw.pop("ag", ag), **dict(ok, **kw))["rc"]
        assert call(d=False) == E_ARG and call(channels=None) == E_ARG
        assert call(ag=None) == E_ARG and call(graph_of=None) == E_ARG
        assert call(graph_of=[0, 3]) == E_ARG and call(graph_of=[-1, 0]) == E_ARG
        assert call(graph_of=[0, 2]) == E_ARG and "tid2pdf" in W.lib().wfst_last_error().decode()   # an ilabel beyond the map
        assert call(channels=[0, 0]) == E_ARG and call(channels=[0, 4]) == E_ARG and call(channels=[-1, 0]) == E_ARG
        assert call(channels=[0, 1, 2, 3, 0], graph_of=[0] * 5) == E_ARG
        assert call(channels=[0, 2]) == E_STATE and "InitDecoding" in W.lib().wfst_last_error().decode()   # never initialised
        assert call(n_frames=[41, -1]) == E_ARG and call(n_frames=[-2, -1]) == E_ARG
        assert call(capf=-1) == E_ARG and call(cape=-1) == E_ARG and call(capf=0) == E_ARG and call(cape=0) == E_ARG and call(capa=-1) == E_ARG
        assert call(max_cells=-1) == E_ARG
        for bad in (-0.5, float("inf"), float("nan")):
            assert call(gs=bad) == E_ARG and call(as_=bad) == E_ARG
        for bad in (-0.1, 1.5, float("nan")):
            assert call(min_post=bad) == E_ARG
        lm = np.arange(N_TID + 1, dtype=np.int32)
        assert call(label_map=lm, n_tid=0) == E_ARG
        assert call(label_map=lm[:100], n_tid=99) == E_ARG                       # shorter than the graphs' largest ilabel
        neg = lm.copy()
        neg[7] = -1
        assert call(label_map=neg, n_tid=N_TID) == E_ARG
        # the dense arguments
        t = torch.zeros((160, N_TID + 1), device="cuda:0")
        ptr = [t.data_ptr(), None]
        dense = dict(grad=ptr, rows=[160, 0], n_cols=N_TID + 1)
        assert call(**dict(dense, rows=None)) == E_ARG and call(**dict(dense, n_cols=0)) == E_ARG
        assert call(**dict(dense, rows=[-1, 0])) == E_ARG and call(**dict(dense, pitch=[N_TID, N_TID + 1])) == E_ARG
        assert call(**dict(dense, grad=[t.data_ptr() + 2, None])) == E_ARG
        assert call(**dict(dense, grad_scale=float("inf"))) == E_ARG and call(**dict(dense, grad_scale=float("nan"))) == E_ARG
        top = int(max(g.arcs["ilabel"].max() for g in graphs[:2]))
        assert call(**dict(dense, n_cols=top)) == E_ARG                          # without a map a column per transition-id
        assert call(**dict(dense, label_map=lm, n_tid=N_TID, n_cols=N_TID)) == E_ARG     # a class beyond n_cols
        torch.cuda.synchronize()
        assert not bool(t.any()) and dec.graph_posteriors_workspace() == ws
        assert call(**dense) == 0 and call(label_map=lm, n_tid=N_TID) == 0
        torch.cuda.synchronize()
        assert bool(t[:40].any()) and not bool(t[40:].any())
        # the decoder still answers
        rep = dec.graph_posteriors(ag, [0, 1], [0, 1])
        assert [raw_bytes(r) for r in rep] == [raw_bytes(r) for r in good]
        assert dec.graph_posteriors_workspace() >= 8 * 151 * S1
    finally:
        ag.free()
        dec.free()


def test_a_graph_set_on_another_device(world):
    W = world["W"]
    if W.device_count() < 2:
        pytest.skip("one device")
    g = U.transcript_graph(range(1, 4), seed=72, n_tid=N_TID)
    ll = scores(20, 610)
    dec = decoder(world, 1)
    ag = W.AlignGraphs.from_arrays([U.as_tuple(g)], device=1)
    try:
        feed_host(dec, [ll])
        o = raw_call(W, dec, ag, [0], [0], 32, 2048)
        assert o["rc"] == E_ARG and "another device" in W.lib().wfst_last_error().decode()
    finally:
        ag.free()
        dec.free()


# ---- 13. determinism and rounds ---------------------------------------------------------------------------------------------------------
def test_determinism_and_rounds(world):
    graphs = [U.transcript_graph(range(1, 12), seed=80 + c, n_tid=N_TID) for c in range(4)]
    lls = [scores(80, 700 + i) for i in range(4)]
    dec = decoder(world, 4)
    ag = world["W"].AlignGraphs.from_arrays([U.as_tuple(g) for g in graphs])
    try:
        feed_host(dec, lls)
        one = dec.graph_posteriors(ag, arc_occupancy=True, label_map=world["m"])
        two = dec.graph_posteriors(ag, arc_occupancy=True, label_map=world["m"])
        assert all(r.found for r in one) and [raw_bytes(r) for r in one] == [raw_bytes(r) for r in two]
        ws = dec.graph_posteriors_workspace()
        # max_cells = the largest table: every channel is a round of its own
        cells = max(81 * g.n_states for g in graphs)
        fresh = decoder(world, 4)
        try:
            feed_host(fresh, lls)
            per = fresh.graph_posteriors(ag, arc_occupancy=True, label_map=world["m"], max_cells=cells)
            assert [raw_bytes(r) for r in per] == [raw_bytes(r) for r in one]
            assert fresh.graph_posteriors_workspace() < ws
        finally:
            fresh.free()
    finally:
        ag.free()
        dec.free()


# ---- 14. one graph set, two decoders, two threads -----------------------------------------------------------------------------------------
def test_a_shared_graph_set(world):
    graphs = [U.transcript_graph(range(1, 10), seed=90 + c, n_tid=N_TID) for c in range(3)]
    lls = [scores(60, 800 + i) for i in range(3)]
    decs = [decoder(world, 3), decoder(world, 3)]
    ag = world["W"].AlignGraphs.from_arrays([U.as_tuple(g) for g in graphs])
    try:
        for dec in decs:
            feed_host(dec, lls)
        before = ag.info()
        out, err = [None, None], []
        gate = threading.Barrier(2)

        def work(k):
            try:
                gate.wait()
                out[k] = decs[k].graph_posteriors(ag, arc_occupancy=True)   # the set's first use: the by-source tables are built once
            except Exception as e:   # noqa: BLE001
                err.append(e)

        threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not err, err
        assert [raw_bytes(r) for r in out[0]] == [raw_bytes(r) for r in out[1]]
        worst = 0.0
        for i in range(3):
            worst = max(worst, U.compare(out[0][i], U.graph_posteriors(graphs[i], lls[i], None, world["m"]), "shared set channel %d" % i))
        print("shared set: largest difference / tolerance %.4f" % worst)
        after = ag.info()
        assert all(np.array_equal(before[k], after[k]) for k in before)
        fa = decs[0].force_align(ag)
        assert all(a.found for a in fa)
    finally:
        ag.free()
        for dec in decs:
            dec.free()
