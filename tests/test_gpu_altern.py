"""-m gpu: wfst_decoder_word_alternatives (slot_mass_kernel / slot_none_kernel behind wfst_decoder_word_confidence's launches) -- per
word of a sequence the alignment places in time, the words the lattice says in that word's cell with their posterior mass, and the
mass of the paths that say nothing there.

The reference of every comparison is the definition restated in numpy (tests/altern_util.py) over dec.raw_lattice(channel,
use_final_probs) fetched at the same moment.  The alignment's own outputs and n_distinct are compared exactly; alt_post, word_post
and none_post at the restatement's tolerances, derived from the lattice at hand; the lists by altern_util.compare's rule, which
survives near ties.  Every test prints the largest difference / tolerance it saw; a ratio above 1 is a bug."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import pyoracle
from align_util import align_many, from_gpu
from altern_util import LDS_KEYS, alternatives_many, compare
from golden_util import GOLDEN_DIR, Golden, bits
from posterior_util import cuts_of, posteriors

pytestmark = pytest.mark.gpu

E_ARG, E_CAPACITY, E_STATE = -1, -4, -5
N_TID = 600
LIM = dict(max_frames=192, max_tokens_per_frame=32768, arena_tokens=1 << 20, lattice_links=1 << 21)
NO_WORD = 777   # a word id the graph (500 words) does not have
SCALES = [(1.0, 1.0), (0.1, 0.1), (1.0, 0.0)]
WIDE = dict(beam=200.0, max_active=1000000, min_active=0, lattice_beam=100.0, prune_interval=10)


def cfg(lattice_beam):
    return dict(beam=12.0, max_active=1000000, min_active=0, lattice_beam=lattice_beam, prune_interval=10)


@pytest.fixture(scope="module")
def world(synth, tmp_path_factory):
    import gpu_util as G

    W = G.wfstdec
    g = synth.make_hclg_like(3000, seed=21, n_tid=N_TID, n_words=500)
    m = synth.default_tid2pdf(N_TID)
    path = str(tmp_path_factory.mktemp("altern") / "g.bin")
    g.write(path)
    graph = W.Graph.load(path)
    graph.set_tid2pdf(m)
    graph.set_tid2phone(np.arange(N_TID + 1, dtype=np.int32))
    mats = [synth.make_loglikes(g, T, N_TID // 2, m, seed=s, mu=-2.2)[0] for T, s in ((40, 700), (97, 701), (150, 702))]
    dev = G.upload(mats)
    yield dict(G=G, W=W, graph=graph, mats=mats, dev=dev, ptrs=[t.data_ptr() for t in dev], T=[x.shape[0] for x in mats])
    graph.free()


def decoder(world, lattice_beam, n=3, **kw):
    lim = dict(LIM)
    lim.update(kw)
    return world["W"].BatchDecoder(world["graph"], world["G"].gpu_config(cfg(lattice_beam)), n, **lim)


def decode_all(world, dec):
    dec.init()
    dec.advance(world["ptrs"], world["T"], N_TID // 2)
    dec.finalize()


def check(dec, channels, seqs, ufp=True, scales=(1.0, 1.0), n_alts=5, what="", max_cells=0, lattices=None, aligned=None):
    """word_alternatives of the list against the restatement on each channel's raw lattice now; returns (got, want, worst ratio).
    lattices / aligned: the channels' lattices / align_many() of their sequences, where the caller has fetched them at this moment"""
    got = dec.word_alternatives(seqs, channels, use_final_probs=ufp, graph_scale=scales[0], acoustic_scale=scales[1], n_alts=n_alts,
                                max_cells=max_cells)
    want, worst = [], 0.0
    for i, c in enumerate(channels):
        L = lattices[i] if lattices is not None else from_gpu(dec.raw_lattice(int(c), ufp))
        assert len(got[i]) == len(seqs[i])
        if L is None or L.n_states == 0:
            want.append([None if s is None else dict(found=False) for s in seqs[i]])
            P = None
        else:
            P = posteriors(L, scales[0], scales[1])
            want.append(alternatives_many(L, seqs[i], scales[0], scales[1], post=P, aligned=aligned[i] if aligned is not None else None))
        for q in range(len(seqs[i])):
            tag = "%s channel %d sequence %d scales %s n_alts %d" % (what, c, q, scales, n_alts)
            assert got[i][q]["status"] == 0, tag
            if P is None:
                assert not got[i][q]["found"] and got[i][q]["log_z"] == 0.0 and not any(got[i][q]["alts"]), tag
                continue
            worst = max(worst, compare(got[i][q], want[i][q], P, L, n_alts, tag))
            if np.isfinite(P["log_z"]):
                worst = max(worst, abs(got[i][q]["log_z"] - P["log_z"]) / P["tol_log"])
            else:
                assert got[i][q]["log_z"] == P["log_z"], tag
    assert worst <= 1.0, "%s: difference / tolerance = %g" % (what, worst)
    return got, want, worst


def variants(words):
    """beside the real sequences: a word replaced by one the graph does not have, the empty sequence, a skip"""
    bad = [int(w) for w in words]
    if bad:
        bad[len(bad) // 2] = NO_WORD
    return [bad if bad else [NO_WORD], [], None]


def raw_word_sequences(L, n_paths, n):
    """the first n distinct word sequences among the n_paths cheapest paths of the raw lattice itself"""
    out = []
    for p in pyoracle.nshortest_paths(L, n_paths):
        w = [int(x) for x in p["olabel"] if x]
        if w not in out:
            out.append(w)
    return out[:n]


def canonical_states(L):
    k = np.stack([L.st_frame, L.st_gstate, L.st_final], axis=1)
    return k[np.lexsort(k.T[::-1])]


def canonical_arcs(L):
    f, g = L.st_frame, L.st_gstate
    k = np.stack([f[L.a_src], g[L.a_src], f[L.a_dst], g[L.a_dst], L.a_il, L.a_ol, bits(L.a_graph), bits(L.a_ac)], axis=1)
    return k[np.lexsort(k.T[::-1])]


def small_decoder(synth, tmp_path, name, n_states, arcs, finals, n_pdf, T, tid2pdf=None):
    """a hand-made graph decoded over T frames of equal scores with nothing pruned: (graph, decoder), both to be freed"""
    import gpu_util as G

    g = synth.graph_from_arc_lists(n_states, 0, arcs, finals)
    path = str(tmp_path / (name + ".bin"))
    g.write(path)
    graph = G.wfstdec.Graph.load(path)
    graph.set_tid2pdf(tid2pdf if tid2pdf is not None else synth.default_tid2pdf(n_pdf * 2))
    x = np.full((T, n_pdf), -0.5, np.float32)
    dec = G.wfstdec.BatchDecoder(graph, G.gpu_config(WIDE), 1, max_frames=96, max_tokens_per_frame=4096, arena_tokens=1 << 16, lattice_links=1 << 16)
    dev = G.upload([x])
    dec.init()
    dec.advance([dev[0].data_ptr()], [T], n_pdf)
    dec.finalize()
    return graph, dec


def one_to_one(n_tid):
    """tid2pdf: transition-id t reads column t - 1"""
    m = np.arange(n_tid + 1, dtype=np.int32) - 1
    m[0] = 0
    return m


# ---- 1. finalized channels ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lattice_beam", [4.0, 8.0])
def test_finalized_channels(world, lattice_beam):
    """5 sequences per channel -- nbest_words(5)'s, or where the determinizer refuses the lattice the distinct word sequences among the
    40 cheapest raw paths -- at the three pairs of scales; the restatement finds every one of them"""
    dec = decoder(world, lattice_beam)
    try:
        decode_all(world, dec)
        ch = [2, 0, 1]
        nb = dec.nbest_words(5, channels=ch)
        lat = [from_gpu(dec.raw_lattice(c, True)) for c in ch]
        seqs = []
        for i, c in enumerate(ch):
            assert nb[i][0] in (0, E_CAPACITY)
            five = [p["words"] for p in nb[i][1]] if nb[i][0] == 0 else raw_word_sequences(lat[i], 40, 5)
            assert len(five) >= 1
            seqs.append([[int(w) for w in s] for s in five] + variants(five[0]))
        worst, keys, between = 0.0, 0, 0
        al = [align_many(L, s) for L, s in zip(lat, seqs)]
        for sc, n_alts in zip(SCALES, (5, 16, 1)):
            got, want, r = check(dec, ch, seqs, True, sc, n_alts, "lattice_beam %g" % lattice_beam, lattices=lat, aligned=al)
            worst = max(worst, r)
            for i in range(len(ch)):
                k = len(seqs[i]) - 3
                assert all(want[i][j]["found"] and got[i][j]["found"] for j in range(k))
                assert not got[i][k]["found"] and got[i][k + 1]["found"] == bool(want[i][k + 1]["found"]) and not got[i][k + 2]["found"]
                keys = max(keys, max(int(got[i][j]["n_distinct"].sum()) for j in range(k)))
                between += sum(int(((got[i][j]["none_post"] > 1e-6) & (got[i][j]["none_post"] < 1 - 1e-6)).sum()) for j in range(k))
        print("finalized, lattice_beam %g: largest difference / tolerance %.3g; most (cell, word) pairs of a sequence %d, none_post strictly "
              "inside (0, 1) in %d cells" % (lattice_beam, worst, keys, between))
        assert between > 0
    finally:
        dec.free()


# ---- 2. live channels, read-only ----------------------------------------------------------------------------------------------
def test_live_channels_and_the_call_is_read_only(world):
    """the 150-frame utterance at lattice_beam 8: at frame 40 a frame of about 405 states, at frame 75 frames of about 2 600 (the
    strided lanes); both use_final_probs, both live-prune modes.  Channel 0 is queried, channel 1 is its twin that never is."""
    dec = decoder(world, 8.0, 2)
    try:
        p, stride = world["ptrs"][2], N_TID // 2
        dec.init()
        sizes, worst = [], 0.0
        for upto in (40, 75):
            dec.advance([p, p], [upto, upto], stride)
            for mode in (0, 1):
                dec.set_live_lattice_prune(mode)
                for ufp in (False, True):
                    w = [int(x) for x in dec.words([0], use_final_probs=ufp)[0][0]]
                    seqs = [[w, w[1:]] + variants(w)]
                    L = from_gpu(dec.raw_lattice(0, ufp))
                    sc = SCALES[(upto // 40 + mode + ufp) % 3]
                    got, _, r = check(dec, [0], seqs, ufp, sc, 5, "frame %d mode %d ufp %d" % (upto, mode, ufp), lattices=[L])
                    worst = max(worst, r)
                    sizes.append((upto, mode, int(ufp), L.n_states, int(np.bincount(L.st_frame).max()), got[0][0]["found"]))
            dec.set_live_lattice_prune(0)
        print("(frame, mode, ufp, states, widest frame, best words found):", sizes)
        print("live: largest difference / tolerance %.3g" % worst)
        assert any(256 < s[4] < 1024 for s in sizes) and any(s[4] > 1024 for s in sizes) and all(s[5] for s in sizes)
        dec.advance([p, p], [150, 150], stride)
        dec.finalize()
        a, b = dec.best_paths([0, 1])
        for k in ("ilabel", "olabel"):
            assert np.array_equal(a[k], b[k]), k
        for k in ("graph", "ac"):
            assert np.array_equal(bits(a[k]), bits(b[k])), k
        La, Lb = from_gpu(dec.raw_lattice(0)), from_gpu(dec.raw_lattice(1))
        assert La.n_states == Lb.n_states and len(La.a_src) == len(Lb.a_src)
        assert np.array_equal(canonical_states(La), canonical_states(Lb)) and np.array_equal(canonical_arcs(La), canonical_arcs(Lb))
    finally:
        dec.free()


# ---- 3. the goldens: epsilon chains, dead ends, negative costs --------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lattice_eps_chains", "dead_end", "neg_hclg600"])
def test_golden_fixtures(name, tmp_path):
    import gpu_util as G

    g = Golden(name)
    graph = G.wfstdec.Graph.load(g.write_graph(str(tmp_path / "g.bin")))
    if g.tid2pdf is not None:
        graph.set_tid2pdf(g.tid2pdf)
    cd = dict(g.meta["cfgs"][g.meta["cases"][0]["cfg"]])
    mats = list(g.utts)
    dec = G.wfstdec.BatchDecoder(graph, G.gpu_config(cd), len(mats), max_frames=64, max_tokens_per_frame=32768, arena_tokens=1 << 20, lattice_links=1 << 21)
    try:
        dev = G.upload(mats)
        dec.init()
        dec.advance([t.data_ptr() for t in dev], [x.shape[0] for x in mats], mats[0].shape[1])
        dec.finalize()
        ch = list(range(len(mats)))
        lat = [from_gpu(dec.raw_lattice(c, True)) for c in ch]
        seqs, n_eps_words, depth = [], 0, 0
        for c in ch:
            w = [int(x) for x in dec.words([c])[0][0]]
            L = lat[c]
            if L is None:
                seqs.append([w] + variants(w))
                continue
            n_eps_words += int(((L.a_il == 0) & (L.a_ol != 0)).sum())
            depth = max(depth, posteriors(L)["n_levels"] - len(np.unique(L.st_frame)))
            listed = {tuple(int(x) for x in p["olabel"] if x) for p in pyoracle.nshortest_paths(L, 12)}
            seqs.append([w] + [list(s) for s in sorted(listed)][:4] + variants(w))
        worst = 0.0
        al = [None if L is None else align_many(L, s) for L, s in zip(lat, seqs)]
        for sc in SCALES[:2]:
            got, want, r = check(dec, ch, seqs, True, sc, 5, name, lattices=lat, aligned=al)
            worst = max(worst, r)
            assert all(got[i][0]["found"] == (lat[i] is not None) for i in ch)
        print("%s: largest difference / tolerance %.3g; words on epsilon arcs %d, epsilon levels beyond the frames' own %d" % (name, worst, n_eps_words, depth))
        if name == "lattice_eps_chains":
            assert n_eps_words > 0 and depth >= 2, "the fixture's point: the level rounds exceed 1"
    finally:
        dec.free()
        graph.free()


# ---- 4. fans: lists shorter than, as long as and longer than n_alts; an exact tie -----------------------------------------------------
FANS = [1, 2, 4, 5, 6, 15, 16, 17]


def test_fans_around_n_alts_and_an_exact_tie(synth, tmp_path):
    """eight fans in a row, one per frame: hub f --N emitting arcs, N distinct words, graph costs i / 8--> N middle states --wordless
    arcs inside the frame--> hub f + 1.  The hypothesis takes each fan's cheapest arc, so cell f is frame f and holds fan f alone:
    N = n_alts - 1, n_alts, n_alts + 1 for n_alts = 1 (N = 1, 2), 5 and 16.  In every fan of 4 arcs or more, arcs 2 and 3 cost the same
    to the last bit: the exact tie goes to the lower word id."""
    arcs, state, tid = {}, 0, 0
    words = []
    for f, N in enumerate(FANS):
        hub, nxt = state, state + N + 1
        arcs[hub] = []
        row = []
        for i in range(N):
            tid += 1
            cost = 0.125 * (2 if (i == 3 and N >= 4) else i)
            word = 100 * (f + 1) + (N - i)          # (the cheaper the arc, the HIGHER its word id: the order is the masses', not the ids')
            arcs[hub].append((tid, word, cost, hub + 1 + i))
            arcs[hub + 1 + i] = [(0, 0, 0.25, nxt)]
            row.append(word)
        words.append(row)
        state = nxt
    graph, dec = small_decoder(synth, tmp_path, "fans", state + 1, arcs, {state: 0.0}, tid, len(FANS), one_to_one(tid))
    try:
        seq = [row[0] for row in words]
        L = from_gpu(dec.raw_lattice(0, True))
        worst = 0.0
        for n_alts in (1, 5, 16):
            got, want, r = check(dec, [0], [[seq, seq[:3] + [seq[3] - 1] + seq[4:], []]], True, (1.0, 1.0), n_alts, "fans", lattices=[L])
            worst = max(worst, r)
            a, b, _ = got[0]
            assert a["found"] and b["found"] and cuts_of(a["begin"])[:-1] == list(range(len(FANS)))
            assert a["n_distinct"].tolist() == FANS and [len(x) for x in a["alts"]] == [min(N, n_alts) for N in FANS]
            assert a["alts"] == b["alts"], "the slots are the same: the list does not depend on which word the hypothesis took"
            for f, N in enumerate(FANS):
                assert np.all(np.abs(a["none_post"]) < 1e-12)
                lst = a["alts"][f]
                assert lst[0][0] == words[f][0]
                if N >= 4 and n_alts >= 4:   # arcs 2 and 3: the same mass to the last bit, the lower word id (arc 3's) first
                    assert lst[2][1] == lst[3][1] and (lst[2][0], lst[3][0]) == (words[f][3], words[f][2]) and lst[2][0] < lst[3][0]
        print("fans: largest difference / tolerance %.3g" % worst)
    finally:
        dec.free()
        graph.free()


# ---- 5. the 70-step chain and a fan: the (cell, word) keys around the LDS table's capacity ---------------------------------------------
CHAIN = 70
_CHAIN_SEEN = {}   # fan -> the chain's part of the answer, for the cases that come after


@pytest.mark.parametrize("fan", [LDS_KEYS - CHAIN - 1, LDS_KEYS - CHAIN, LDS_KEYS - CHAIN + 1], ids=["one_below", "capacity", "one_above"])
def test_the_chain_and_a_fan_around_the_lds_capacity(fan, synth, tmp_path):
    """test_gpu_posterior.py's chain -- word s + 1 or nothing on step s -- and behind it a fan of `fan` arcs with as many words: a
    sequence over all 71 steps has 70 + fan distinct (cell, word) pairs, WFST_ALTERN_LDS_KEYS - 1, exactly it, and one more, where the
    table in the workspace takes over.  The chain's part of the answer is the same in all three to rounding."""
    T = CHAIN
    arcs = {s: [(2 * s + 1, s + 1, 0.5, s + 1), (2 * s + 2, 0, 0.25, s + 1)] for s in range(T)}
    arcs[T] = [(2 * T + 1 + i, 1000 + i, i / 128.0, T + 1 + i) for i in range(fan)]
    finals = {T + 1 + i: 0.0 for i in range(fan)}
    n_pdf = 2 * T + fan
    graph, dec = small_decoder(synth, tmp_path, "chain", T + 1 + fan, arcs, finals, n_pdf, T + 1, one_to_one(n_pdf))
    try:
        every = list(range(1, T + 1))
        tail = [1000]
        seqs = [[every + tail, every[:63] + tail, every[2:66] + tail, [35] + tail, tail, every]]
        L = from_gpu(dec.raw_lattice(0, True))
        assert len(np.unique(L.a_ol[L.a_ol > 0])) == T + fan
        got, want, worst = check(dec, [0], seqs, True, (1.0, 1.0), 16, "chain + fan %d" % fan, lattices=[L])
        assert [r["found"] for r in got[0]] == [True] * 5 + [False]
        assert [len(r["word_post"]) for r in got[0][:3]] == [71, 64, 65]
        full = got[0][0]
        assert int(full["n_distinct"].sum()) == T + fan == LDS_KEYS + (fan - (LDS_KEYS - CHAIN)) and full["n_distinct"][-1] == fan
        assert [w for w, _ in full["alts"][-1]] == list(range(1000, 1016))
        # word s + 1 sits on one arc only, at frame s, beside the wordless arc: the slot holds it alone, and none_post is the rest
        for k in range(T):
            assert full["alts"][k][0][0] == k + 1 and abs(full["alts"][k][0][1] + full["none_post"][k] - 1.0) < 1e-9
        assert abs(full["none_post"][-1]) < 1e-12 and abs(got[0][4]["none_post"][0]) < 1e-12 and got[0][4]["n_distinct"][0] == T + fan
        # the chain's slots do not see the fan: the same answer from the LDS table and from the workspace's
        part = np.array([full["alts"][k][0][1] for k in range(T)] + list(full["none_post"][:T]))
        for other in _CHAIN_SEEN.values():
            assert np.allclose(part, other, rtol=0, atol=1e-9)
        _CHAIN_SEEN[fan] = part
        print("chain + fan %d: %d (cell, word) pairs, largest difference / tolerance %.3g" % (fan, T + fan, worst))
    finally:
        dec.free()
        graph.free()


# ---- 6. cell shapes: an empty cell, one cell, a word said twice -------------------------------------------------------------------------
def test_an_empty_cell_from_two_words_at_one_frame(synth, tmp_path):
    """7 and 8 on arcs inside frame 0, then one emitting arc: begin frames 0 and 0, cell 0 = [0, 0) is empty and says nothing on every
    path; cell 1 is the whole time axis"""
    graph, dec = small_decoder(synth, tmp_path, "empty", 4, {0: [(0, 7, 0.5, 1)], 1: [(0, 8, 0.5, 2), (0, 9, 1.0, 2)], 2: [(1, 0, 0.5, 3)]}, {3: 0.0}, 2, 1)
    try:
        got, want, worst = check(dec, [0], [[[7, 8], [7, 9], [7], []]], True, (1.0, 1.0), 5, "empty cell")
        a, b, c, _ = got[0]
        assert a["found"] and b["found"] and not c["found"]
        assert a["begin"].tolist() == [0, 0] and a["none_post"][0] == 1.0 and a["alts"][0] == [] and a["n_distinct"].tolist() == [0, 3]
        assert [w for w, _ in a["alts"][1]] == [7, 8, 9] and abs(a["none_post"][1]) < 1e-15
        assert abs(a["alts"][1][1][1] - 1.0 / (1.0 + np.exp(-0.5))) < 1e-12 and a["alts"][1] == b["alts"][1]
        print("empty cell: largest difference / tolerance %.3g" % worst)
    finally:
        dec.free()
        graph.free()


def test_one_cell_and_a_word_said_twice(synth, tmp_path):
    """test_gpu_posterior.py's fixture: the paths say 5 5, 5, 5 and nothing.  For [5] the one cell is the whole time axis: none_post
    is the posterior of saying nothing at all, exp of the empty sequence's sentence posterior"""
    graph, dec = small_decoder(synth, tmp_path, "twice", 5,
                               {0: [(1, 5, 0.0, 1), (2, 0, 1.0, 2)], 1: [(3, 5, 0.0, 3), (4, 0, 1.0, 4)], 2: [(3, 5, 0.0, 3), (4, 0, 1.0, 4)]},
                               {3: 0.0, 4: 0.0}, 2, 2)
    try:
        got, _, worst = check(dec, [0], [[[5], [5, 5], [], [6]]], True, (1.0, 1.0), 5, "twice")
        one, two, none, absent = got[0]
        z = (1.0 + np.exp(-1.0)) ** 2
        assert one["found"] and abs(one["none_post"][0] - np.exp(-2.0) / z) < 1e-12 and abs(one["alts"][0][0][1] - 2.0 / (1.0 + np.exp(-1.0))) < 1e-12
        assert one["alts"][0][0][1] == one["word_post"][0] > 1.0 and one["n_distinct"].tolist() == [1]
        empty = dec.sentence_posteriors([[[]]], [0])[0][0]
        assert empty["found"] and abs(one["none_post"][0] - np.exp(empty["logpost"])) < 1e-12
        assert two["found"] and np.all(np.abs(two["none_post"] - 1.0 / (1.0 + np.e)) < 1e-12)
        assert none["found"] and none["alts"] == [] and len(none["none_post"]) == 0 and not absent["found"]
        print("twice: largest difference / tolerance %.3g" % worst)
    finally:
        dec.free()
        graph.free()


# ---- 7. 64 sequences on one channel -------------------------------------------------------------------------------------------------
def test_64_sequences_on_one_channel(world):
    dec = decoder(world, 8.0, 1)
    try:
        dec.init()
        dec.advance(world["ptrs"][:1], [40], N_TID // 2)
        dec.finalize()
        L = from_gpu(dec.raw_lattice(0, True))
        real = raw_word_sequences(L, 200, 40)
        w = [int(x) for x in dec.words([0])[0][0]]
        seqs = list(real)
        while len(seqs) < 64:
            k = len(seqs)
            seqs.append(w[: k % (len(w) + 1)] if k % 2 else w[k % len(w):])
        got, _, worst = check(dec, [0], [seqs], True, (1.0, 0.1), 3, "64 sequences", lattices=[L])
        assert len(got[0]) == 64 and sum(r["found"] for r in got[0]) >= len(real) >= 2
        print("64 sequences: largest difference / tolerance %.3g" % worst)
    finally:
        dec.free()


# ---- 8. mixed lists, a channel over max_cells, nbest_words_conf -----------------------------------------------------------------------
def test_mixed_list_capacity_of_one_channel_and_nbest_words_conf(world):
    dec = decoder(world, 4.0)
    try:
        dec.init()
        dec.advance(world["ptrs"], [40, 60, 75], N_TID // 2)
        dec.finalize(channels=[0, 2])          # channel 1 stays live at frame 60
        dec.set_live_lattice_prune(1)
        ch = [1, 2, 0]
        w = [[int(x) for x in dec.words([c])[0][0]] for c in ch]
        seqs = [[w[0], w[0][:1]], [w[1], None, w[1][:-1], []], [w[2]]]
        got, _, worst = check(dec, ch, seqs, True, (1.0, 1.0), 5, "mixed")
        assert all(a[0]["found"] for a in got)
        cells = [dec.raw_lattice(c, True)["n_states"] * (1 + max(len(s) for s in sq if s is not None)) for c, sq in zip(ch, seqs)]
        big = int(np.argmax(cells))
        assert sorted(cells)[-1] > sorted(cells)[-2]
        lat = [from_gpu(dec.raw_lattice(c, True)) for c in ch]
        tight = dec.word_alternatives(seqs, ch, max_cells=cells[big] - 1)
        assert [a[0]["status"] for a in tight] == [E_CAPACITY if i == big else 0 for i in range(3)]
        for r in tight[big]:
            assert not r["found"] and not r["begin"].any() and not r["end"].any() and not r["word_post"].any()
            assert r["log_z"] == 0.0 and r["path_logpost"] == 0.0 and r["n_arcs"] == 0 and float(r["tot"]) == 0.0 and float(r["lm"]) == 0.0
            assert not any(r["alts"]) and not r["none_post"].any() and not r["n_distinct"].any()
        for i in set(range(3)) - {big}:
            P = posteriors(lat[i])
            for q, r in enumerate(alternatives_many(lat[i], seqs[i], post=P)):
                worst = max(worst, compare(tight[i][q], r, P, lat[i], 5, "beside the channel over max_cells: %d %d" % (i, q)))
        assert worst <= 1.0
        # use_final_probs = 0: the finalized channels have no lattice (found 0, status OK, log_z 0), the live one answers
        w0 = [int(x) for x in dec.words([1], use_final_probs=False)[0][0]]
        live_only = dec.word_alternatives([[w0], [w[1]], [w[2]]], ch, use_final_probs=False)
        assert [a[0]["status"] for a in live_only] == [0, 0, 0] and [a[0]["found"] for a in live_only] == [True, False, False]
        assert not any(live_only[1][0]["alts"]) and all(live_only[0][0]["alts"])
        # nbest_words_conf: alternatives = 0 is today's answer key for key, alternatives = 3 adds word_alternatives' on the same paths
        conf = dec.nbest_words_conf(3, channels=ch)
        conf0 = dec.nbest_words_conf(3, channels=ch, alternatives=0)
        conf3 = dec.nbest_words_conf(3, channels=ch, alternatives=3)
        n = 0
        for i, ((st, paths), (st0, paths0), (st3, paths3)) in enumerate(zip(conf, conf0, conf3)):
            assert st == st0 == st3 == 0 and len(paths) == len(paths0) == len(paths3) >= 1
            direct = dec.word_alternatives([[p["words"] for p in paths]], [ch[i]], n_alts=3)[0]
            for p, p0, p3, d in zip(paths, paths0, paths3, direct):
                assert set(p0) == set(p) and set(p3) - set(p) == {"alts", "none_post", "n_distinct"}
                assert set(p) >= {"conf", "word_post", "path_logpost", "log_z", "begin", "end"}
                for k in ("words", "found", "begin", "end", "n_arcs", "align_tot", "align_lm", "tot", "lm"):
                    assert np.asarray(p[k]).tobytes() == np.asarray(p0[k]).tobytes() == np.asarray(p3[k]).tobytes(), k
                assert np.array_equal(p3["n_distinct"], d["n_distinct"]) and [len(x) for x in p3["alts"]] == [len(x) for x in d["alts"]]
                assert np.allclose(p3["none_post"], d["none_post"], rtol=0, atol=1e-9) and np.allclose(p3["word_post"], p["word_post"], rtol=0, atol=1e-9)
                assert p3["found"] and len(p3["alts"]) == p3["n_words"] and all(len(x) <= 3 for x in p3["alts"])
                n += 1
        print("mixed: largest difference / tolerance %.3g; nbest_words_conf paths %d" % (worst, n))
    finally:
        dec.free()


# ---- 9. a biglm lattice decoder -----------------------------------------------------------------------------------------------
def test_biglm_lattice_decoder(tmp_path):
    import gpu_util as G

    W = G.wfstdec
    z = np.load(os.path.join(GOLDEN_DIR, "biglm_hclg600.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    with open(tmp_path / "g.bin", "wb") as f:
        f.write(bytes(z["graph"]))
    graph = W.Graph.load(str(tmp_path / "g.bin"))
    graph.set_tid2pdf(z["tid2pdf"])
    pname = [p for p in meta["pairs"] if p != "unigram"][0]
    lms = []
    for tag, scale in (("old", -1.0), ("new", 1.0)):
        p = str(tmp_path / ("lm_%s.bin" % tag))
        with open(p, "wb") as f:
            f.write(bytes(z["lm_%s_%s" % (pname, tag)]))
        lms.append(W.Lm.load(p, scale))
    cd = dict(beam=13.0, max_active=1000000, min_active=0, lattice_beam=25.0, prune_interval=7)
    mats = [z["ll_%d" % i] for i in range(int(z["n_utt"]))]
    dec = W.BatchDecoder(graph, G.gpu_config(cd), len(mats), old_lm=lms[0], new_lm=lms[1], max_frames=64, max_tokens_per_frame=32768,
                         arena_tokens=1 << 20, lattice_links=1 << 21)
    try:
        dev = G.upload(mats)
        dec.init()
        dec.advance([t.data_ptr() for t in dev], [x.shape[0] for x in mats], int(mats[0].shape[1]))
        dec.finalize()
        have = [c for c in range(len(mats)) if dec.raw_lattice(c, True) is not None]
        assert have, "no utterance kept its lattice"
        u = have[0]
        L = from_gpu(dec.raw_lattice(u, True))
        listed = {tuple(int(w) for w in p["olabel"] if w) for p in pyoracle.nshortest_paths(L, 12)}
        w = [int(x) for x in dec.words([u])[0][0]]
        seqs = [[w] + [list(s) for s in sorted(listed)][:5] + variants(w)]
        got = dec.word_alternatives(seqs, [u], graph_scale=1.0, acoustic_scale=0.1, n_alts=5)
        P = posteriors(L, 1.0, 0.1)
        want = alternatives_many(L, seqs[0], 1.0, 0.1, post=P)
        n_skipped = n_found = 0
        worst = abs(got[0][0]["log_z"] - P["log_z"]) / P["tol_log"]
        for q in range(len(seqs[0])):
            if want[q] is not None and want[q]["found"] and want[q]["tie"]:   # two tokens may share a graph state here: unspecified
                n_skipped += 1
                continue
            worst = max(worst, compare(got[0][q], want[q], P, L, 5, "biglm sequence %d" % q))
            n_found += got[0][q]["found"]
        print("biglm: %d sequences found, %d skipped for a tie; largest difference / tolerance %.3g" % (n_found, n_skipped, worst))
        assert n_skipped <= 1 and n_found >= 2 and worst <= 1.0
    finally:
        dec.free()
        for lm in lms:
            lm.free()
        graph.free()


# ---- 10. the error surface -------------------------------------------------------------------------------------------------------
def test_error_surface(world):
    W = world["W"]
    plain = decoder(world, 4.0, 2, lattice_links=0)
    try:
        plain.init()
        plain.advance(world["ptrs"][:2], [10, 10], N_TID // 2)
        with pytest.raises(W.WfstError) as e:
            plain.word_alternatives([[[1]], [[1]]])
        assert e.value.code == E_STATE
    finally:
        plain.free()
    dec = decoder(world, 4.0, 3)
    try:
        dec.init(channels=[0, 1])
        dec.advance(world["ptrs"][:2], [20, 20], N_TID // 2, channels=[0, 1])
        ok = dec.word_alternatives([[[1]]], [0], use_final_probs=False)
        assert ok[0][0]["status"] == 0
        for seqs, ch, code in (([[[1]], [[1]]], [0, 0], E_ARG), ([[[1]], [[1]]], [0, 3], E_ARG), ([[[1]], [[1]]], [0, 2], E_STATE),
                               ([[[1, 0]]], [0], E_ARG), ([[[-4]]], [0], E_ARG), ([[[1]] * 65], [0], E_ARG)):
            with pytest.raises(W.WfstError) as e:
                dec.word_alternatives(seqs, ch, use_final_probs=False)
            assert e.value.code == code, (seqs, ch)
        for gs, as_ in ((-1.0, 1.0), (1.0, -0.5), (float("nan"), 1.0), (1.0, float("inf")), (float("-inf"), 1.0)):
            with pytest.raises(W.WfstError) as e:
                dec.word_alternatives([[[1]]], [0], use_final_probs=False, graph_scale=gs, acoustic_scale=as_)
            assert e.value.code == E_ARG, (gs, as_)
        for n_alts in (0, -1, 17):
            with pytest.raises(W.WfstError) as e:
                dec.word_alternatives([[[1]]], [0], use_final_probs=False, n_alts=n_alts)
            assert e.value.code == E_ARG and "n_alts" in str(e.value), n_alts
        # through the C ABI: NULL outputs are fine
        I = C.POINTER(C.c_int32)
        one, words, length = np.array([0], np.int32), np.array([1, 1], np.int32), np.array([1], np.int32)
        p = lambda a: a.ctypes.data_as(I)
        call = lambda n_seqs, cap, ln: W.lib().wfst_decoder_word_alternatives(dec.h, p(one), 1, 0, C.c_double(1.0), C.c_double(1.0), 5, n_seqs,
                                                                              cap, p(words), p(ln), C.c_int64(0), *([None] * 14))
        assert call(0, 2, length) == E_ARG and call(1, 0, length) == E_ARG and call(1, 2, np.array([3], np.int32)) == E_ARG
        assert call(1, 2, length) == 0
    finally:
        dec.free()
