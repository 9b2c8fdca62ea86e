"""-m gpu: wfst_decoder_align_words (align_index_kernel / align_kernel) -- the cheapest path of a channel's raw lattice that spells a
given word sequence, with its word times and scores.

The reference of every comparison is the definition restated in numpy (tests/align_util.py) over dec.raw_lattice(channel,
use_final_probs) fetched at the same moment: found, n_arcs, begin and end frames equal, tot_score and lm_score equal bit for bit.
There are no tolerances."""
import importlib
import json
import os

import numpy as np
import pytest

import pyoracle
from align_util import align_many, from_gpu
from golden_util import GOLDEN_DIR, Golden, bits

pytestmark = pytest.mark.gpu

E_ARG, E_CAPACITY, E_STATE = -1, -4, -5
N_TID = 600
LIM = dict(max_frames=192, max_tokens_per_frame=32768, arena_tokens=1 << 20, lattice_links=1 << 21)
NO_WORD = 777   # a word id the graph (500 words) does not have


def cfg(lattice_beam):
    return dict(beam=12.0, max_active=1000000, min_active=0, lattice_beam=lattice_beam, prune_interval=10)


@pytest.fixture(scope="module")
def world(synth, tmp_path_factory):
    import gpu_util as G

    W = G.wfstdec
    g = synth.make_hclg_like(3000, seed=21, n_tid=N_TID, n_words=500)
    m = synth.default_tid2pdf(N_TID)
    path = str(tmp_path_factory.mktemp("align") / "g.bin")
    g.write(path)
    graph = W.Graph.load(path)
    graph.set_tid2pdf(m)
    graph.set_tid2phone(np.arange(N_TID + 1, dtype=np.int32))   # identity: a phone is a transition-id
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


def same(got, want, what):
    """one (channel, sequence) answer against the restatement's"""
    if want is None:   # skipped
        want = dict(found=False)
    assert got["found"] == bool(want["found"]), what + " found"
    if not want["found"]:
        assert got["n_arcs"] == 0 and not got["begin"].any() and not got["end"].any() and bits([got["tot"], got["lm"]]).tolist() == [0, 0], what
        return
    assert got["n_arcs"] == want["n_arcs"], what + " n_arcs"
    assert np.array_equal(got["begin"], want["begin"]), what + " begin frames"
    assert np.array_equal(got["end"], want["end"]), what + " end frames"
    assert bits([got["tot"], got["lm"]]).tolist() == bits([want["tot"], want["lm"]]).tolist(), what + " scores"


def check(dec, channels, seqs, ufp, sil_tids=None, what="", max_cells=0):
    """align_words of the list against the restatement on each channel's raw lattice now; returns (got, want)"""
    got = dec.align_words(seqs, channels, use_final_probs=ufp, max_cells=max_cells)
    want = []
    for i, c in enumerate(channels):
        L = from_gpu(dec.raw_lattice(int(c), ufp))
        want.append(align_many(L, seqs[i], sil_tids))
        assert len(got[i]) == len(seqs[i])
        for q in range(len(seqs[i])):
            assert got[i][q]["status"] == 0, "%s channel %d" % (what, c)
            same(got[i][q], want[i][q], "%s channel %d sequence %d" % (what, c, q))
    return got, want


def variants(words):
    """the sequences every test asks beside the real ones: a word replaced by one the graph does not have, the empty sequence, a skip"""
    bad = [int(w) for w in words]
    if bad:
        bad[len(bad) // 2] = NO_WORD
    return [bad if bad else [NO_WORD], [], None]


def canonical_states(L):
    """rows (frame, graph state, final), sorted"""
    k = np.stack([L.st_frame, L.st_gstate, L.st_final], axis=1)
    return k[np.lexsort(k.T[::-1])]


def canonical_arcs(L):
    """rows (src frame, src graph state, dst frame, dst graph state, ilabel, olabel, graph bits, acoustic bits), sorted: equal for two
    lattices iff they are the same up to state numbering (pyoracle.RawLattice.labelled_arcs)"""
    f, g = L.st_frame, L.st_gstate
    k = np.stack([f[L.a_src], g[L.a_src], f[L.a_dst], g[L.a_dst], L.a_il, L.a_ol, bits(L.a_graph), bits(L.a_ac)], axis=1)
    return k[np.lexsort(k.T[::-1])]


def hops(il, ol, g, a):
    rows = [(int(i), int(o), int(x), int(y)) for i, o, x, y in zip(il, ol, bits(g), bits(a))]
    return rows[1:] if rows and rows[0] == (0, 0, 0, 0) else rows   # (GetBestPath's hop list starts with the root's (0, 0, One) arc)


# ---- 1. finalized channels ----------------------------------------------------------------------------------------------------
def raw_word_sequences(L, n_paths, n):
    """the first n distinct word sequences among the n_paths cheapest paths of the raw lattice itself"""
    out = []
    for p in pyoracle.nshortest_paths(L, n_paths):
        w = [int(x) for x in p["olabel"] if x]
        if w not in out:
            out.append(w)
    return out[:n]


def test_finalized_channels(world):
    """The sequences: the words of the best path; the 5 paths of nbest_words(5); a sequence with a word the graph does not have; the
    empty sequence; a skipped one.  On this synthetic graph the determinizer refuses the longer utterances' lattices (WFST_E_CAPACITY
    in nbest_words' status: the subset construction outgrows its workspace, with or without this call); for such a channel the 5
    sequences are the distinct word sequences among the 40 cheapest paths of the raw lattice instead."""
    n_channels = n_waived = n_paths = n_from_nbest = 0
    worst = 0.0
    for lb in (4.0, 8.0):
        dec = decoder(world, lb)
        try:
            decode_all(world, dec)
            ch = [2, 0, 1]
            best = dec.words(ch)
            nb = dec.nbest_words(5, channels=ch)
            bps = dec.best_paths(ch)
            seqs, alt = [], []
            for i, c in enumerate(ch):
                assert nb[i][0] in (0, E_CAPACITY), (lb, c, nb[i][0])
                alt.append([p["words"] for p in nb[i][1]] if nb[i][0] == 0 else raw_word_sequences(from_gpu(dec.raw_lattice(c, True)), 40, 5))
                assert len(alt[i]) >= 1
                n_from_nbest += nb[i][0] == 0
                seqs.append([best[i][0]] + alt[i] + variants(best[i][0]))
            got, want = check(dec, ch, seqs, True, what="lattice_beam %g" % lb)
            for i, c in enumerate(ch):
                k = len(alt[i])
                assert got[i][0]["found"] and all(got[i][1 + j]["found"] for j in range(k)), "every n-best sequence is in the raw lattice"
                assert not got[i][1 + k]["found"] and not got[i][3 + k]["found"], "an unknown word / a skipped sequence"
                if nb[i][0] == 0:
                    for j in range(k):   # (the determinizer re-associates the sums: recorded, not asserted)
                        worst = max(worst, abs(float(got[i][1 + j]["tot"]) - float(nb[i][1][j]["tot"])))
                n_paths += k
                # the alignment of the best path's words IS the best path, and then everything wfst_decoder_get_words says is equal
                L = from_gpu(dec.raw_lattice(c, True))
                a = want[i][0]["arcs"]
                n_channels += 1
                if hops(L.a_il[a], L.a_ol[a], L.a_graph[a], L.a_ac[a]) != hops(bps[i]["ilabel"], bps[i]["olabel"], bps[i]["graph"], bps[i]["ac"]):
                    n_waived += 1
                    continue
                w, b, e, tot, lm, _ = best[i]
                assert np.array_equal(got[i][0]["begin"], b) and np.array_equal(got[i][0]["end"], e), c
                assert bits([got[i][0]["tot"], got[i][0]["lm"]]).tolist() == bits([tot, lm]).tolist(), c
        finally:
            dec.free()
    print("sequences aligned: %d (channels served by nbest_words: %d of %d); largest |align tot - nbest_words tot| = %g; best-path check waived for %d channels"
          % (n_paths, n_from_nbest, n_channels, worst, n_waived))
    assert n_paths >= 12 and n_from_nbest >= 2 and 12 * n_waived <= n_channels


# ---- 2. live channels, read-only ----------------------------------------------------------------------------------------------
def test_live_channels_and_the_call_is_read_only(world):
    """the 150-frame utterance at lattice_beam 8: at frame 40 the live lattice has about 3 200 states and a frame of 405 (wider than a
    256-thread workgroup, narrower than align_kernel's 1024), at frame 75 about 38 600 with frames of about 2 600 (wider than both).
    Channel 0 is queried, channel 1 is its twin that never is."""
    dec = decoder(world, 8.0, 2)
    try:
        p, stride = world["ptrs"][2], N_TID // 2
        dec.init()
        sizes = []
        for upto in (40, 75):
            dec.advance([p, p], [upto, upto], stride)
            for mode in (0, 1):
                dec.set_live_lattice_prune(mode)
                for ufp in (False, True):
                    w = dec.words([0], use_final_probs=ufp)[0][0]
                    seqs = [[w, w[:-1], w[1:]] + variants(w)]
                    got, _ = check(dec, [0], seqs, ufp, what="frame %d mode %d ufp %d" % (upto, mode, ufp))
                    L = dec.raw_lattice(0, ufp)
                    sizes.append((upto, mode, int(ufp), L["n_states"], int(np.bincount(L["st_frame"]).max()), got[0][0]["found"]))
            dec.set_live_lattice_prune(0)
        print("(frame, mode, ufp, states, widest frame, best words found):", sizes)
        assert any(s[4] > 256 and s[4] < 1024 for s in sizes) and any(s[4] > 1024 for s in sizes) and all(s[5] for s in sizes)
        dec.advance([p, p], [150, 150], stride)
        dec.finalize()
        a, b = dec.best_paths([0, 1])
        for k in ("ilabel", "olabel"):
            assert np.array_equal(a[k], b[k]), k
        for k in ("graph", "ac"):
            assert np.array_equal(bits(a[k]), bits(b[k])), k
        # (tokens of a frame are numbered in the order the device created them, which differs from channel to channel: the lattices
        # are compared up to that numbering -- states and arcs by frame and graph state)
        La, Lb = from_gpu(dec.raw_lattice(0)), from_gpu(dec.raw_lattice(1))
        assert La.n_states == Lb.n_states and len(La.a_src) == len(Lb.a_src)
        assert np.array_equal(canonical_states(La), canonical_states(Lb)) and np.array_equal(canonical_arcs(La), canonical_arcs(Lb))
    finally:
        dec.free()


# ---- 3. silence lists ---------------------------------------------------------------------------------------------------------
def test_silence_lists_move_the_end_frames(world):
    dec = decoder(world, 8.0)
    try:
        decode_all(world, dec)
        ch = [0, 1, 2]
        seqs = [[dec.words([c])[0][0]] for c in ch]
        plain, want = check(dec, ch, seqs, True, what="no list")
        # the silence phones (= transition-ids here): every second emitting transition-id of the aligned paths themselves
        tids = []
        for c, w in zip(ch, want):
            L = from_gpu(dec.raw_lattice(c, True))
            il = L.a_il[w[0]["arcs"]]
            tids += [int(t) for t in il[il != 0][1::2]]
        sil = sorted(set(tids))
        dec.set_silence_phones(sil)
        trimmed, _ = check(dec, ch, seqs, True, sil_tids=np.array(sil), what="silence list")
        assert any((t[0]["end"] != p[0]["end"]).any() for t, p in zip(trimmed, plain)), "no word end moved by the silence list"
        assert all(np.array_equal(t[0]["begin"], p[0]["begin"]) for t, p in zip(trimmed, plain))
        dec.set_silence_phones([])
        again, _ = check(dec, ch, seqs, True, what="list cleared")
        assert all(np.array_equal(t[0]["end"], p[0]["end"]) for t, p in zip(again, plain))
    finally:
        dec.free()


# ---- 4. the wave-width boundary -----------------------------------------------------------------------------------------------
def test_sequences_of_1_63_64_65_and_70_words(synth, tmp_path):
    """a chain of 70 steps; every step has an emitting arc with a word (word s + 1 at step s) and one without, so a path spells any
    subsequence of 1..70: tables of 2, 64, 65, 66 and 71 columns"""
    import gpu_util as G

    T = 70
    g = synth.graph_from_arc_lists(T + 1, 0, {s: [(2 * s + 1, s + 1, 0.5, s + 1), (2 * s + 2, 0, 0.25, s + 1)] for s in range(T)}, {T: 0.0})
    m = np.arange(2 * T + 1, dtype=np.int32) - 1   # a column per transition-id
    m[0] = 0
    x = np.random.RandomState(4).normal(-2.0, 1.0, (T, 2 * T)).astype(np.float32)
    path = str(tmp_path / "chain.bin")
    g.write(path)
    graph = G.wfstdec.Graph.load(path)
    graph.set_tid2pdf(m)
    dec = G.wfstdec.BatchDecoder(graph, G.gpu_config(dict(beam=200.0, max_active=1000000, min_active=0, lattice_beam=100.0, prune_interval=10)), 1,
                                 max_frames=96, max_tokens_per_frame=4096, arena_tokens=1 << 16, lattice_links=1 << 16)
    try:
        dev = G.upload([x])
        dec.init()
        dec.advance([dev[0].data_ptr()], [T], 2 * T)
        dec.finalize()
        every = list(range(1, T + 1))
        seqs = [[[35], every[3:66], every[:64], every[2:67], every, every[:10] + every[30:40], [2, 1]]]
        got, _ = check(dec, [0], seqs, True, what="chain")
        assert [r["found"] for r in got[0]] == [True] * 6 + [False]
        assert np.array_equal(got[0][4]["begin"], np.arange(T)) and np.array_equal(got[0][4]["end"], np.arange(1, T + 1))
        assert got[0][0]["begin"].tolist() == [34] and got[0][0]["end"].tolist() == [T]
    finally:
        dec.free()
        graph.free()


# ---- 5. dense epsilon chains inside frames -------------------------------------------------------------------------------------
def test_epsilon_chains_fixture(tmp_path):
    import gpu_util as G

    g = Golden("lattice_eps_chains")
    graph = G.wfstdec.Graph.load(g.write_graph(str(tmp_path / "g.bin")))
    if g.tid2pdf is not None:
        graph.set_tid2pdf(g.tid2pdf)
    cd = dict(g.meta["cfgs"][g.meta["cases"][0]["cfg"]])
    mats = list(g.utts)
    assert sorted(x.shape[0] for x in mats) == [1, 2, 9, 30]
    dec = G.wfstdec.BatchDecoder(graph, G.gpu_config(cd), len(mats), max_frames=64, max_tokens_per_frame=32768, arena_tokens=1 << 20, lattice_links=1 << 21)
    try:
        dev = G.upload(mats)
        dec.init()
        dec.advance([t.data_ptr() for t in dev], [x.shape[0] for x in mats], mats[0].shape[1])
        dec.finalize()
        ch = list(range(len(mats)))
        seqs, n_eps_words = [], 0
        for c in ch:
            L = from_gpu(dec.raw_lattice(c, True))
            w = dec.words([c])[0][0]
            if L is None:   # (the reference's "no lattice": nothing is found)
                seqs.append([w] + variants(w))
                continue
            n_eps_words += int(((L.a_il == 0) & (L.a_ol != 0)).sum())
            listed = {tuple(int(w) for w in p["olabel"] if w) for p in pyoracle.nshortest_paths(L, 12)}   # word sequences the lattice holds
            seqs.append([w] + [list(s) for s in sorted(listed)][:6] + variants(w))
        got, want = check(dec, ch, seqs, True, what="eps chains")
        assert n_eps_words > 0, "the fixture's point: words on epsilon arcs"
        assert all(got[i][0]["found"] == (dec.raw_lattice(i, True) is not None) for i in ch) and sum(r["found"] for a in got for r in a) >= 8
    finally:
        dec.free()
        graph.free()


# ---- 6. mixed lists, a channel over max_cells, the other getters ---------------------------------------------------------------
def test_mixed_list_capacity_of_one_channel_and_the_other_getters(world):
    dec = decoder(world, 4.0)
    try:
        dec.init()
        dec.advance(world["ptrs"], [40, 60, 75], N_TID // 2)
        dec.finalize(channels=[0, 2])          # channel 1 stays live at frame 60 (lengths the determinizer takes, for the getters below)
        dec.set_live_lattice_prune(1)
        ch = [1, 2, 0]
        ufp = True
        def getters():
            return dict(words=dec.words([0, 2]), raw=[dec.raw_lattice(c) for c in (0, 2)], det=[dec.determinized_lattice(c) for c in (0, 2)],
                        nbp=[dec.nbest_paths(c, 3) for c in (0, 2)], live=dec.raw_lattice(1, ufp), nbw=dec.nbest_words(3, channels=ch))
        before = getters()
        w = [dec.words([c], use_final_probs=ufp)[0][0] for c in ch]
        seqs = [[w[0], w[0][:1]], [w[1], None, w[1][:-1], []], [w[2]]]     # differing counts and lengths per channel
        got, _ = check(dec, ch, seqs, ufp, what="mixed")
        assert all(a[0]["found"] for a in got)
        # max_cells just below the largest table of the list: that channel alone reports WFST_E_CAPACITY
        cells = [dec.raw_lattice(c, ufp)["n_states"] * (1 + max(len(s) for s in sq if s is not None)) for c, sq in zip(ch, seqs)]
        big = int(np.argmax(cells))
        assert sorted(cells)[-1] > sorted(cells)[-2]
        tight = dec.align_words(seqs, ch, use_final_probs=ufp, max_cells=cells[big] - 1)
        assert [a[0]["status"] for a in tight] == [E_CAPACITY if i == big else 0 for i in range(3)]
        assert not any(r["found"] for r in tight[big]) and all(not r["begin"].any() for r in tight[big])
        for i in set(range(3)) - {big}:
            for q in range(len(seqs[i])):
                same(tight[i][q], got[i][q], "beside the channel over max_cells: %d %d" % (i, q))
        # use_final_probs = 0: the finalized channels have no lattice (found 0, status OK), the live one answers
        w[0] = dec.words([1], use_final_probs=False)[0][0]
        live_only = dec.align_words([[x] for x in w], ch, use_final_probs=False)
        assert [a[0]["status"] for a in live_only] == [0, 0, 0] and [a[0]["found"] for a in live_only] == [True, False, False]
        # the other getters answer what they answered before
        after = getters()

        def eq(x, y):
            if isinstance(x, dict):
                return x.keys() == y.keys() and all(eq(x[k], y[k]) for k in x)
            if isinstance(x, (list, tuple)):
                return len(x) == len(y) and all(eq(a, b) for a, b in zip(x, y))
            if isinstance(x, np.ndarray) or isinstance(x, np.floating):
                return np.asarray(x).tobytes() == np.asarray(y).tobytes()
            return x == y
        for k in before:
            assert eq(before[k], after[k]), k
        # the convenience on top: nbest_words with times
        timed = dec.nbest_words_timed(3, channels=ch)
        for (st, paths), (st0, paths0) in zip(timed, before["nbw"]):
            assert st == st0 == 0 and len(paths) == len(paths0)
            for p, p0 in zip(paths, paths0):
                assert np.array_equal(p["words"], p0["words"]) and p["found"] and len(p["begin"]) == len(p["end"]) == p["n_words"]
                assert np.all(p["begin"][1:] >= p["begin"][:-1]) and np.all(p["end"] >= p["begin"])
    finally:
        dec.free()


# ---- 7. a biglm lattice decoder -----------------------------------------------------------------------------------------------
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
    # (a lattice_beam wide enough that the reference's final pruning -- its final_best_cost ranges over non-final tokens too,
    # biglm.h:186-188 -- leaves the utterances their lattices: tests/test_gpu_biglm.py)
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
        seqs = [[dec.words([u])[0][0]] + [list(s) for s in sorted(listed)][:5] + variants(dec.words([u])[0][0])]
        got = dec.align_words(seqs, [u])
        want = align_many(L, seqs[0])
        n_skipped = n_found = 0
        for q in range(len(seqs[0])):
            if want[q] is not None and want[q]["found"] and want[q]["tie"]:   # two tokens may share a graph state here: unspecified
                n_skipped += 1
                continue
            same(got[0][q], want[q], "biglm sequence %d" % q)
            n_found += got[0][q]["found"]
        print("biglm: %d sequences found, %d skipped for a tie" % (n_found, n_skipped))
        assert n_skipped <= 1 and n_found >= 2
    finally:
        dec.free()
        for lm in lms:
            lm.free()
        graph.free()


# ---- 8. the tie fixture of the restatement test, on the device -----------------------------------------------------------------
@pytest.mark.parametrize("early_on_state_1,begin", [(True, 0), (False, 1)])
def test_the_tie_rule_decides_the_times(early_on_state_1, begin, synth, tmp_path):
    """two paths 0 -> 1 -> 3 and 0 -> 2 -> 3 of equal cost (0.5 + 0.5 per arc and frame: exact) that spell the same word at different
    frames; both arrive at state 3 over emitting arcs, so the one from the lower graph state (1) wins, wherever the word sits on it"""
    import gpu_util as G

    a, b = (5, 0) if early_on_state_1 else (0, 5)
    g = synth.graph_from_arc_lists(4, 0, {0: [(1, a, 0.5, 1), (2, b, 0.5, 2)], 1: [(3, b, 0.5, 3)], 2: [(4, a, 0.5, 3)]}, {3: 0.0})
    path = str(tmp_path / "tie.bin")
    g.write(path)
    graph = G.wfstdec.Graph.load(path)
    graph.set_tid2pdf(synth.default_tid2pdf(4))
    x = np.full((2, 2), -0.5, np.float32)
    dec = G.wfstdec.BatchDecoder(graph, G.gpu_config(dict(beam=10.0, max_active=1000000, min_active=0, lattice_beam=5.0, prune_interval=10)), 1,
                                 max_frames=16, max_tokens_per_frame=4096, arena_tokens=1 << 12, lattice_links=1 << 12)
    try:
        dev = G.upload([x])
        dec.init()
        dec.advance([dev[0].data_ptr()], [2], 2)
        dec.finalize()
        got, want = check(dec, [0], [[[5], [5, 5], []]], True, what="tie")
        assert want[0][0]["tie"], "the fixture holds an exact tie"
        r = got[0][0]
        assert r["found"] and r["begin"].tolist() == [begin] and r["end"].tolist() == [2]
        assert bits([r["tot"], r["lm"]]).tolist() == bits([2.0, 1.0]).tolist()
        assert not got[0][1]["found"] and not got[0][2]["found"]
    finally:
        dec.free()
        graph.free()


# ---- 9. the error surface -------------------------------------------------------------------------------------------------------
def test_error_surface(world):
    W = world["W"]
    plain = decoder(world, 4.0, 2, lattice_links=0)
    try:
        plain.init()
        plain.advance(world["ptrs"][:2], [10, 10], N_TID // 2)
        with pytest.raises(W.WfstError) as e:
            plain.align_words([[[1]], [[1]]])
        assert e.value.code == E_STATE
    finally:
        plain.free()
    dec = decoder(world, 4.0, 3)
    try:
        dec.init(channels=[0, 1])
        dec.advance(world["ptrs"][:2], [20, 20], N_TID // 2, channels=[0, 1])
        ok = dec.align_words([[[1]]], [0], use_final_probs=False)
        assert ok[0][0]["status"] == 0
        for seqs, ch, code in (([[[1]], [[1]]], [0, 0], E_ARG), ([[[1]], [[1]]], [0, 3], E_ARG), ([[[1]], [[1]]], [0, 2], E_STATE),
                               ([[[1, 0]]], [0], E_ARG), ([[[-4]]], [0], E_ARG), ([[[1]] * 65], [0], E_ARG)):
            with pytest.raises(W.WfstError) as e:
                dec.align_words(seqs, ch, use_final_probs=False)
            assert e.value.code == code, (seqs, ch)
        # through the C ABI: n_seqs 0, cap_words 0, a seq_len above cap_words; NULL outputs are fine
        import ctypes as C
        I = C.POINTER(C.c_int32)
        one, words, length = np.array([0], np.int32), np.array([1, 1], np.int32), np.array([1], np.int32)
        p = lambda a: a.ctypes.data_as(I)
        call = lambda n_seqs, cap, ln: W.lib().wfst_decoder_align_words(dec.h, p(one), 1, 0, n_seqs, cap, p(words), p(ln), C.c_int64(0), *([None] * 7))
        assert call(0, 2, length) == E_ARG and call(1, 0, length) == E_ARG and call(1, 2, np.array([3], np.int32)) == E_ARG
        assert call(1, 2, length) == 0
    finally:
        dec.free()
