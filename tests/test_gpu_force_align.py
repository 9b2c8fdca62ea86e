"""-m gpu: wfst_decoder_force_align (forced_align_kernel) -- exact float32 Viterbi of a channel's scores against the utterance's own
graph.

The reference of every comparison is the header's semantics restated in numpy (tests/force_align_util.py) on the same scores, and
everything is compared BIT FOR BIT: found, path_cost, hop_arc, alignment, words, word frames and the two sums."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import force_align_util as U
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
    path = str(tmp_path_factory.mktemp("falign") / "g.bin")
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


def check(world, dec, graphs, channels, lls, graph_of=None, n_frames=None, label_map=None, tid2pdf="world", what=""):
    """force_align of the list against the restatement on lls[i]; returns (got, want)"""
    W = world["W"]
    m = world["m"] if isinstance(tid2pdf, str) else tid2pdf
    ag = W.AlignGraphs.from_arrays([U.as_tuple(g) for g in graphs])
    try:
        got = dec.force_align(ag, graph_of, channels, n_frames, label_map)
    finally:
        ag.free()
    want = []
    for i, c in enumerate(channels):
        g = graphs[graph_of[i] if graph_of is not None else i]
        T = n_frames[i] if n_frames is not None and n_frames[i] is not None and n_frames[i] >= 0 else lls[i].shape[0]
        want.append(U.force_align(g, lls[i], T, m, label_map))
        U.compare(got[i], want[-1], "%s channel %d" % (what, c))
    return got, want


# ---- 1. mixed small cases ------------------------------------------------------------------------------------------------------------
def test_mixed_small_cases(world):
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
    try:
        feed_host(dec, lls)
        got, want = check(world, dec, graphs, list(range(8)), lls, graph_of, what="mixed")
        found = [g.found for g in got]
        print("mixed: states %s, T %s, found %s, hops %s" % ([graphs[k].n_states for k in graph_of], Ts, found, [g.n_hops for g in got]))
        assert found[0] and found[1] and found[3] and found[4] and found[6] and found[7] and not all(found)
        assert got[0].n_frames == 0 and got[0].n_hops > 0 and len(got[0].alignment) == 0   # T = 0: epsilon arcs only
        # the same list in another order, a sublist, and fewer frames than held
        check(world, dec, graphs, [6, 1, 4], [lls[6], lls[1], lls[4]], [6, 4, 0], n_frames=[100, -1, 120], what="sublist")
    finally:
        dec.free()


# ---- 2. the state count around WFST_FALIGN_LDS_STATES ----------------------------------------------------------------------------------
def test_state_count_edges(world):
    L = U.WFST_FALIGN_LDS_STATES
    graphs = [U.fan_graph(n, 40 + k, N_TID) for k, n in enumerate((L - 1, L, L + 1))]
    assert [g.n_states for g in graphs] == [L - 1, L, L + 1]
    lls = [scores(3, 200 + i) for i in range(3)]
    dec = decoder(world, 3)
    try:
        feed_host(dec, lls)
        got, _ = check(world, dec, graphs, [0, 1, 2], lls, what="edges")
        assert all(g.found and g.n_frames == 3 and g.n_words == 1 for g in got)
        # the answers do not depend on where the rows live: the same fan with one state more or less, the same scores
        check(world, dec, [graphs[2], graphs[0], graphs[1]], [0, 1, 2], lls, what="edges swapped")
    finally:
        dec.free()


def kernel_constants():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dev = open(os.path.join(root, "asr-decoder_amd", "csrc", "wfst_device.h")).read()
    hip = open(os.path.join(root, "asr-decoder_amd", "csrc", "wfst_forced.hip")).read()
    return int(re.search(r"kFalignLdsLabels = (\d+);", dev).group(1)), int(re.search(r"kFaThreads = (\d+);", hip).group(1))


def test_distinct_label_count_edges(synth, tmp_path):
    """The scores of up to kFalignLdsLabels distinct ilabels are staged in LDS a frame ahead, beyond that they are gathered from the
    frame's row: graphs of one label less, exactly that many and one more in one call, on either side of WFST_FALIGN_LDS_STATES too,
    so that staged and gathered scores each meet rows in LDS and rows in the workspace.  The answers do not depend on which."""
    import gpu_util as G

    W = G.wfstdec
    NL, _ = kernel_constants()
    L = U.WFST_FALIGN_LDS_STATES
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
    try:
        assert list(ag.info()["n_labels"]) == [n for _, n in shapes] and list(ag.info()["n_states"]) == [S for S, _ in shapes]
        feed_host(dec, lls)
        got = dec.force_align(ag)
        for k, (S, n) in enumerate(shapes):
            r = got[k]
            U.compare(r, U.force_align(graphs[k], lls[k], None, m), "%d states, %d distinct ilabels" % (S, n))
            assert r.found and r.n_words == 1
        # the same scores against a graph on the other side of the label edge: another graph, so another answer, held the same way
        got = dec.force_align(ag, graph_of=[2, 0, 1, 5, 3, 4])
        for k, j in enumerate([2, 0, 1, 5, 3, 4]):
            U.compare(got[k], U.force_align(graphs[j], lls[k], None, m), "graph %d on channel %d" % (j, k))
    finally:
        ag.free()
        dec.free()
        graph.free()


def test_an_epsilon_level_wider_than_the_workgroup(world):
    """one level of the epsilon DAG with more states than the workgroup has lanes (and with a remainder): the level pass strides"""
    _, lanes = kernel_constants()
    graphs = [U.eps_fan_graph(2 * lanes + 37, 70, N_TID), U.eps_fan_graph(lanes + 1, 71, N_TID)]
    assert all(int(np.bincount(U.eps_levels(x))[1]) > lanes for x in graphs)
    lls = [scores(4, 320), scores(2, 321)]
    dec = decoder(world, 2)
    try:
        feed_host(dec, lls)
        got, _ = check(world, dec, graphs, [0, 1], lls, what="wide epsilon level")
        assert all(x.found and x.n_words == 1 for x in got) and got[0].n_hops == 4 + 2
    finally:
        dec.free()


# ---- 3. epsilon depth -------------------------------------------------------------------------------------------------------------------
def eps_chain_graph(k, seed):
    """chains of k epsilon arcs out of start at frame 0, in mid-utterance and into final_state at frame T"""
    rng = np.random.default_rng(seed)
    B = U.Builder()
    w = lambda: float(np.float32(rng.uniform(-0.5, 1.5)))
    tid = lambda: int(rng.integers(1, N_TID + 1))

    def eps_chain(s, word):
        for j in range(k):
            t = B.state()
            B.arc(s, 0, word if j == k - 1 else 0, w(), t)
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


def winner_graph():
    """(a) a negative epsilon weight that changes the winner: s -> t directly at 1.0, or over u at 2.0 and an epsilon arc of -1.5;
    (b) a state reached by an emitting and by an epsilon arc at the same cost: 1.0 against 0.5 + 0.5 on scores that are multiples of
    1/4 -- the emitting arc keeps the backpointer"""
    B = U.Builder()
    s, t, u, v, x, fin = B.states(6)
    B.arc(s, 5, 1, 1.0, t)
    B.arc(s, 5, 2, 2.0, u)
    B.arc(u, 0, 3, -1.5, t)
    B.arc(t, 6, 4, 0.5, x)
    B.arc(x, 0, 5, 0.5, v)
    B.arc(t, 6, 6, 1.0, v)
    B.arc(v, 0, 0, 0.0, fin)
    return B.build(s, fin)


def test_epsilon_depth(world):
    graphs = [eps_chain_graph(k, 60 + k) for k in (1, 2, 7)] + [winner_graph()]
    Ts = [9, 9, 9, 2]
    lls = [scores(T, 300 + i) for i, T in enumerate(Ts)]
    lls[3] = np.round(lls[3] * 4) / np.float32(4)
    dec = decoder(world, 4)
    try:
        feed_host(dec, lls)
        got, want = check(world, dec, graphs, [0, 1, 2, 3], lls, what="eps")
        for i, k in enumerate((1, 2, 7)):
            assert got[i].found and got[i].n_hops == 9 + 3 * k and list(got[i].words) == [11, 12, 13, 14]
            assert got[i].word_frame[0] == 0 and got[i].word_frame[3] == 9
        # (a): over u and the negative epsilon arc; (b): both arrivals of v cost the same, the emitting one wins
        assert list(got[3].words) == [2, 3, 6], got[3].words
        V, g = want[3]["V"], graphs[3]
        assert V[1, 1] == V[1, 2] + np.float32(-1.5) and V[1, 1] < (np.float32(0) + -lls[3][0, world["m"][5]]) + np.float32(1.0)
        assert V[2, 3] == V[2, 4] + np.float32(0.5)
    finally:
        dec.free()


# ---- 4. all ties, unreachable, non-finite scores ------------------------------------------------------------------------------------
def test_all_ties(world):
    g = U.transcript_graph(range(1, 9), seed=9, n_tid=N_TID, weights=False)
    ll = np.full((40, N_PDF), -1.0, np.float32)
    dec = decoder(world, 1)
    try:
        feed_host(dec, [ll])
        got, want = check(world, dec, [g], [0], [ll], what="ties")
        assert got[0].found and float(got[0].path_cost) == 40.0
        V = want[0]["V"]
        assert all(V[f, s] == f for f in range(41) for s in range(g.n_states) if np.isfinite(V[f, s]))   # every arrival ties
    finally:
        dec.free()


def test_unreachable_and_non_finite(world):
    rng = np.random.default_rng(11)
    chain = U.chain_graph([(int(rng.integers(1, N_TID + 1)), k % 3, 0.5) for k in range(12)])   # no self-loop: exactly 12 frames
    g = U.transcript_graph(range(1, 6), seed=10, n_tid=N_TID)
    ll = scores(20, 400)
    clean = U.force_align(g, ll, 20, world["m"])
    assert clean["found"]
    cols = world["m"][clean["alignment"]]
    bad = ll.copy()
    bad[:, cols[3]] = -np.inf          # a column of -inf: the arcs that read it are no arcs at any frame
    bad[10, cols[10]] = np.nan         # on the clean scores' own path
    bad[15, cols[15]] = np.inf
    dec = decoder(world, 3)
    try:
        feed_host(dec, [ll, ll[:12], bad])
        got, want = check(world, dec, [chain, chain, g], [0, 1, 2], [ll, ll[:12], bad], what="unreachable / non-finite")
        assert not got[0].found and got[0].status == 0 and got[0].n_frames == 0
        assert got[1].found and got[1].n_hops == 12
        # the non-finite scores lie on the clean scores' path: the answer is another one (or none)
        assert not got[2].found or not np.array_equal(got[2].hop_arc, clean["hop_arc"])
        assert not np.array_equal(want[2]["V"], clean["V"])
    finally:
        dec.free()


# ---- 5. where the scores come from -------------------------------------------------------------------------------------------------
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
        ag = world["W"].AlignGraphs.from_arrays([U.as_tuple(g) for g in graphs])
        got = dec.force_align(ag)
        ag.free()
        for c in range(2):
            ll = dec.scores(c, 0, T)
            U.compare(got[c], U.force_align(graphs[c], ll, T, world["m"]), "chunk channel %d" % c)
            assert got[c].found and got[c].n_frames == T
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
        assert [g.n_frames for g in got] == [40, 30, 150]
        check(world, dec, graphs, [1, 2], [mats[1], mats[2]], [1, 2], n_frames=[17, 64], what="fewer frames")
        ag = world["W"].AlignGraphs.from_arrays([U.as_tuple(g) for g in graphs])
        with pytest.raises(world["W"].WfstError) as ei:   # more than the frames decoded of the caller's matrix
            dec.force_align(ag, [1], [1], [31])
        assert ei.value.code == E_ARG
        ag.free()
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
        assert got[0].found and got[1].found and [g.n_frames for g in got] == [97, 60]
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
        assert all(g.found and g.n_frames == x.shape[0] for g, x in zip(got, mats))
    finally:
        dec.free()
        for lm in lms:
            lm.free()
        graph.free()


# ---- 6. ties to the search and to training -------------------------------------------------------------------------------------------
def test_a_chain_of_the_best_path_gives_the_best_path_and_feeds_sequence_stats(world):
    mats = world["mats"]
    dec = decoder(world, 2, lattice=True)
    try:
        feed_host(dec, mats[:2])
        dec.finalize()
        bps = dec.best_paths()
        assert all(bp["ok"] for bp in bps)
        # the graph that accepts exactly the channel's own hop sequence, with its weights
        graphs = [U.chain_graph(list(zip(bp["ilabel"], bp["olabel"], bp["graph"]))) for bp in bps]
        got, _ = check(world, dec, graphs, [0, 1], mats[:2], label_map=None, what="best path chain")
        for g, bp, x in zip(got, bps, mats):
            assert g.found and np.array_equal(g.alignment, bp["tids"]) and np.array_equal(g.words, bp["words"])
            assert U.bits(g.tot_score) == U.bits(bp["tot_score"]) and U.bits(g.lm_score) == U.bits(bp["lm_score"])
        # the alignment under tid2pdf is sequence_stats' ref as it stands
        m = world["m"]
        got, _ = check(world, dec, graphs, [0, 1], mats[:2], label_map=m, what="pdf alignment")
        st = dec.sequence_stats([g.alignment for g in got], criterion="mmi", label_map=m)
        for s, x in zip(st, mats):
            assert s["status"] == 0 and s["n_frames"] == x.shape[0] and s["n_ref_frames"] == x.shape[0]
    finally:
        dec.free()


# ---- 7. the oracle, built on this machine --------------------------------------------------------------------------------------------
def test_against_the_oracle(world, oracle, tmp_path):
    import pyoracle

    n = 12
    rng = np.random.default_rng(91)
    graphs = [U.transcript_graph([int(w) for w in rng.integers(1, 9, size=int(rng.integers(1, 5)))], seed=900 + i, n_tid=N_TID) for i in range(n)]
    lls = [scores(int(rng.integers(20, 50)), 910 + i) for i in range(n)]
    dec = decoder(world, n)
    oracle.set_tie_rule(1)
    try:
        feed_host(dec, lls)
        got, _ = check(world, dec, graphs, list(range(n)), lls, what="oracle")
        cfg = pyoracle.Config(beam=1.0e30, max_active=2147483647, min_active=0, lattice_beam=1.0e30)
        same = 0
        for i in range(n):
            path = str(tmp_path / ("g%d.flat" % i))
            graphs[i].write(path)
            h = oracle.load_graph(path)
            try:
                o = oracle.decode(h, cfg, lls[i], tid2pdf=world["m"])
            finally:
                oracle.free_graph(h)
            assert o.ok and got[i].found, i
            cost = np.float32(0)
            for il, gc, ac in zip(o.path_ilabel, o.path_graph, o.path_ac):
                cost = np.float32(np.float32(cost + ac) + gc) if il != 0 else np.float32(cost + gc)
            assert U.bits(cost) == U.bits(got[i].path_cost), i
            if o.extra["ties"] == 0:
                same += 1
                a = graphs[i].arcs
                mine = [(int(a["ilabel"][k]), int(a["olabel"][k]), U.bits(a["w"][k])) for k in got[i].hop_arc]
                theirs = [(int(x), int(y), U.bits(w)) for x, y, w in zip(o.path_ilabel, o.path_olabel, o.path_graph)]
                assert theirs[0] == (0, 0, 0) and mine == theirs[1:], i
                assert U.bits(o.tot_score) == U.bits(got[i].tot_score) and U.bits(o.lm_score) == U.bits(got[i].lm_score), i
        assert same >= n - 1
    finally:
        oracle.set_tie_rule(0)
        dec.free()


# ---- 8. the error surface ------------------------------------------------------------------------------------------------------------
def raw_call(W, dec, ag, channels, graph_of, capf, caph, capw, n_frames=None, label_map=None, n_tid=0, max_cells=0, d=True):
    """the C entry point itself, with rows of the caller's size: dict of the raw output arrays and the return code"""
    I, F = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    ch, gof = np.ascontiguousarray(channels, np.int32), np.ascontiguousarray(graph_of, np.int32)
    n = len(ch)
    o = dict(status=np.full(n, 99, np.int32), found=np.full(n, 99, np.int32), n_frames=np.full(n, 99, np.int32), cost=np.full(n, 9.0, np.float32),
             tot=np.full(n, 9.0, np.float32), lm=np.full(n, 9.0, np.float32), n_hops=np.full(n, 99, np.int32), hops=np.full((n, max(caph, 1)), 99, np.int32),
             ali=np.full((n, max(capf, 1)), 99, np.int32), n_words=np.full(n, 99, np.int32), words=np.full((n, max(capw, 1)), 99, np.int32),
             wf=np.full((n, max(capw, 1)), 99, np.int32))
    p = lambda a: None if a is None else a.ctypes.data_as({np.dtype(np.int32): I, np.dtype(np.float32): F}[a.dtype])
    nfi = None if n_frames is None else np.ascontiguousarray(n_frames, np.int32)
    lm = None if label_map is None else np.ascontiguousarray(label_map, np.int32)
    o["rc"] = W.lib().wfst_decoder_force_align(dec.h if d else None, p(ch), n, ag.h if ag is not None else None, p(gof), p(nfi), p(lm), n_tid,
                                               C.c_int64(max_cells), capf, caph, capw, p(o["status"]), p(o["found"]), p(o["n_frames"]), p(o["cost"]),
                                               p(o["tot"]), p(o["lm"]), p(o["n_hops"]), p(o["hops"]), p(o["ali"]), p(o["n_words"]), p(o["words"]), p(o["wf"]))
    return o


def test_error_surface(world, monkeypatch):
    W = world["W"]
    graphs = [U.transcript_graph(range(1, 7), seed=70, n_tid=N_TID), U.transcript_graph(range(1, 31), seed=71, n_tid=N_TID),
              U.chain_graph([(N_TID + 5, 1, 0.5)])]
    lls = [scores(40, 600), scores(150, 601)]
    want = [U.force_align(graphs[i], lls[i], None, world["m"]) for i in range(2)]
    assert want[0]["found"] and want[1]["found"]
    dec = decoder(world, 4)
    ag = W.AlignGraphs.from_arrays([U.as_tuple(g) for g in graphs])
    info = ag.info()
    assert info["n_graphs"] == 3 and list(info["n_states"]) == [g.n_states for g in graphs] and list(info["n_arcs"]) == [g.n_arcs for g in graphs]
    assert list(info["max_ilabel"]) == [int(g.arcs["ilabel"].max()) for g in graphs] and list(info["eps_depth"]) == [int(U.eps_levels(g).max()) for g in graphs]
    assert info["device_bytes"] > 32 * info["total_arcs"]
    try:
        feed_host(dec, lls, [0, 1])
        S1 = graphs[1].n_states
        # max_cells exceeded on one channel only
        o = raw_call(W, dec, ag, [0, 1], [0, 1], 160, 400, 64, max_cells=151 * S1 - 1)
        assert o["rc"] == 0 and list(o["status"]) == [0, E_CAPACITY] and list(o["found"]) == [1, 0] and o["n_frames"][1] == 150 and o["n_hops"][1] == 0
        assert U.bits(o["cost"][0]) == U.bits(want[0]["path_cost"]) and "max_cells" in W.lib().wfst_last_error().decode()
        o = raw_call(W, dec, ag, [0, 1], [0, 1], 160, 400, 64, max_cells=151 * S1)
        assert list(o["status"]) == [0, 0] and list(o["found"]) == [1, 1]
        # capacities too small: the counts are the room needed, what fits is written, the scores stand
        nh, nw = [len(w["hop_arc"]) for w in want], [len(w["words"]) for w in want]
        o = raw_call(W, dec, ag, [0, 1], [0, 1], 40, nh[0], nw[0])
        assert o["rc"] == 0 and list(o["status"]) == [0, E_CAPACITY]
        assert (o["n_frames"][1], o["n_hops"][1], o["n_words"][1]) == (150, nh[1], nw[1]) and U.bits(o["cost"][1]) == U.bits(want[1]["path_cost"])
        assert np.array_equal(o["hops"][1], want[1]["hop_arc"][:nh[0]]) and np.array_equal(o["ali"][1], want[1]["alignment"][:40])
        assert np.array_equal(o["words"][1], want[1]["words"][:nw[0]]) and np.array_equal(o["hops"][0], want[0]["hop_arc"])
        for caps in ((150, nh[1] - 1, nw[1]), (150, nh[1], nw[1] - 1), (149, nh[1], nw[1])):
            assert raw_call(W, dec, ag, [1], [1], *caps)["status"][0] == E_CAPACITY, caps
        assert raw_call(W, dec, ag, [1], [1], 150, nh[1], nw[1])["status"][0] == 0
        # ... and the binding repeats the call once
        got = dec.force_align(ag, [0, 1], [0, 1], cap_frames=3, cap_hops=3, cap_words=1)
        for i in range(2):
            U.compare(got[i], want[i], "the binding's repeat")
        # every WFST_E_ARG / WFST_E_STATE of the header, none of which leaves a mark
        ok = dict(channels=[0, 1], graph_of=[0, 1], capf=160, caph=400, capw=64)
        call = lambda **kw: raw_call(W, dec, kw.pop("ag", ag), **dict(ok, **kw))["rc"]
        assert call(d=False) == E_ARG
        assert call(ag=None) == E_ARG
        assert call(graph_of=[0, 3]) == E_ARG and call(graph_of=[-1, 0]) == E_ARG
        assert call(graph_of=[0, 2]) == E_ARG and "tid2pdf" in W.lib().wfst_last_error().decode()   # an ilabel beyond the map
        assert call(channels=[0, 0]) == E_ARG and call(channels=[0, 4]) == E_ARG and call(channels=[-1, 0]) == E_ARG
        assert call(channels=[0, 1, 2, 3, 0], graph_of=[0] * 5) == E_ARG
        assert call(channels=[0, 2]) == E_STATE and "InitDecoding" in W.lib().wfst_last_error().decode()   # never initialised
        assert call(n_frames=[41, -1]) == E_ARG and call(n_frames=[-2, -1]) == E_ARG
        assert call(capf=-1) == E_ARG and call(caph=-1) == E_ARG and call(capw=-1) == E_ARG and call(max_cells=-1) == E_ARG
        lm = np.arange(N_TID + 1, dtype=np.int32)
        assert call(label_map=lm, n_tid=0) == E_ARG
        assert call(label_map=lm[:100], n_tid=99) == E_ARG                       # shorter than the graphs' largest ilabel
        neg = lm.copy()
        neg[7] = -1
        assert call(label_map=neg, n_tid=N_TID) == E_ARG
        assert call(label_map=lm, n_tid=N_TID) == 0
        # without a map on the decoder's graph the column is the transition-id: beyond the score stride
        plain = W.Graph.load(world["path"])
        d2 = W.BatchDecoder(plain, world["G"].gpu_config(CFG), 1, **LIM)
        try:
            wide = np.zeros((8, N_TID + 4), np.float32)
            d2.init()
            d2.advance_host([wide], [8])
            assert raw_call(W, d2, ag, [0], [0], 8, 64, 8)["rc"] == 0
            assert raw_call(W, d2, ag, [0], [2], 8, 64, 8)["rc"] == E_ARG and "stride" in W.lib().wfst_last_error().decode()
        finally:
            d2.free()
            plain.free()
        # the decoder still answers
        got = dec.force_align(ag, [0, 1], [0, 1])
        for i in range(2):
            U.compare(got[i], want[i], "after the errors")
        assert dec.force_align_workspace() >= 4 * 151 * S1
    finally:
        ag.free()
        dec.free()


def test_rounds(world):
    """an explicit max_cells also bounds what one round holds: four channels of 4 097 x 151 cells each under max_cells = one table
    are four rounds, the workspace stays below two tables, and the answers are those of one round"""
    L = U.WFST_FALIGN_LDS_STATES
    g = U.fan_graph(L + 1, 80, N_TID)
    n, cells = 4, 151 * (L + 1)
    lls = [scores(150, 700 + i) for i in range(n)]
    dec = decoder(world, n)
    ag = world["W"].AlignGraphs.from_arrays([U.as_tuple(g)])
    try:
        feed_host(dec, lls)
        want = [U.force_align(g, ll, None, world["m"]) for ll in lls]
        got = dec.force_align(ag, [0] * n, max_cells=cells + cells // 2)
        assert 4 * cells <= dec.force_align_workspace() < 4 * 2 * cells
        for i in range(n):
            assert got[i].found
            U.compare(got[i], want[i], "rounds channel %d" % i)
        got = dec.force_align(ag, [0] * n)
        assert dec.force_align_workspace() >= 4 * n * cells
        for i in range(n):
            U.compare(got[i], want[i], "one round channel %d" % i)
    finally:
        ag.free()
        dec.free()
