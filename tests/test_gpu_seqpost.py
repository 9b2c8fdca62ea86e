"""-m gpu: wfst_decoder_sequence_posterior (seqpost_kernel behind align_index_kernel and posterior_kernel) -- the posterior of a whole
word sequence over ALL paths of a channel's raw lattice that spell it (mode 0), and the expected number of times a path says a
phrase, with the frames at which it does (mode 1).

The reference of every comparison is the definition restated in numpy (tests/seqpost_util.py) over dec.raw_lattice(channel,
use_final_probs) fetched at the same moment.  found and n_frames are compared exactly; seq_logpost, count and every hit_mass entry at
the tolerances seqpost_util derives from the lattice at hand.  Both modes run in every case, every listed (channel, sequence) is
compared, and every test prints the largest difference / tolerance it saw; a ratio above 1 is a bug."""
import json
import os

import numpy as np
import pytest

import pyoracle
from align_util import from_gpu
from golden_util import GOLDEN_DIR, Golden, bits
from posterior_util import posteriors
from seqpost_util import compare_phrase, compare_sentence, n_frames_of, phrase_many, sentence_many

pytestmark = pytest.mark.gpu

E_ARG, E_CAPACITY, E_STATE = -1, -4, -5
N_TID = 600
LIM = dict(max_frames=192, max_tokens_per_frame=32768, arena_tokens=1 << 20, lattice_links=1 << 21)
NO_WORD = 777   # a word id the graph (500 words) does not have
SCALES = [(1.0, 1.0), (0.1, 0.1), (1.0, 0.0)]


def cfg(lattice_beam):
    return dict(beam=12.0, max_active=1000000, min_active=0, lattice_beam=lattice_beam, prune_interval=10)


@pytest.fixture(scope="module")
def world(synth, tmp_path_factory):
    import gpu_util as G

    W = G.wfstdec
    g = synth.make_hclg_like(3000, seed=21, n_tid=N_TID, n_words=500)
    m = synth.default_tid2pdf(N_TID)
    path = str(tmp_path_factory.mktemp("seqpost") / "g.bin")
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


def phrases_of(seqs):
    """the phrases a case looks for beside its sentences: the whole sequence, or a run of two words from inside it, in turn (an
    empty sequence is no phrase: skipped)"""
    out = []
    for q, w in enumerate(seqs):
        if not w:
            out.append(None)
        elif q % 2 or len(w) < 3:
            out.append(list(w))
        else:
            out.append(list(w[len(w) // 3: len(w) // 3 + 2]))
    return out


def check(dec, channels, seqs, ufp=True, scales=(1.0, 1.0), what="", max_cells=0, lattices=None, phrases=None):
    """sentence_posteriors of the list and phrase_posteriors of its phrases against the restatement on each channel's raw lattice
    now; returns (sentences got, phrases got, sentences wanted, phrases wanted, worst ratio)"""
    phrases = phrases if phrases is not None else [phrases_of(s) for s in seqs]
    kw = dict(use_final_probs=ufp, graph_scale=scales[0], acoustic_scale=scales[1], max_cells=max_cells)
    got_s = dec.sentence_posteriors(seqs, channels, **kw)
    got_p = dec.phrase_posteriors(phrases, channels, hit_mass=True, **kw)
    want_s, want_p, worst = [], [], 0.0
    for i, c in enumerate(channels):
        L = lattices[i] if lattices is not None else from_gpu(dec.raw_lattice(int(c), ufp))
        assert len(got_s[i]) == len(seqs[i]) and len(got_p[i]) == len(phrases[i])
        tag = "%s channel %d scales %s" % (what, c, scales)
        if L is None or L.n_states == 0:
            want_s.append([None] * len(seqs[i]))
            want_p.append([None] * len(phrases[i]))
            for r in got_s[i] + got_p[i]:
                assert r["status"] == 0 and not r["found"] and r["log_z"] == 0.0, tag
            assert all(r["logpost"] == 0.0 for r in got_s[i]) and all(r["count"] == 0.0 and r["n_frames"] == 0 for r in got_p[i]), tag
            continue
        P = posteriors(L, scales[0], scales[1])
        want_s.append(sentence_many(L, seqs[i], post=P))
        want_p.append(phrase_many(L, phrases[i], post=P))
        for kind, got, want in (("sequence", got_s[i], want_s[i]), ("phrase", got_p[i], want_p[i])):
            for q, (r, w) in enumerate(zip(got, want)):
                t = "%s %s %d" % (tag, kind, q)
                assert r["status"] == 0, t
                if np.isfinite(P["log_z"]):
                    worst = max(worst, abs(r["log_z"] - P["log_z"]) / P["tol_log"])
                else:
                    assert r["log_z"] == P["log_z"], t
                if kind == "phrase":
                    assert r["n_frames"] == n_frames_of(L), t
                if w is None:      # skipped
                    assert not r["found"] and (r["logpost"] == 0.0 if kind == "sequence" else r["count"] == 0.0 and not r["hit_mass"].any()), t
                elif kind == "sequence":
                    worst = max(worst, compare_sentence(r, w, t))
                else:
                    worst = max(worst, compare_phrase(r, w, L, t))
    assert worst <= 1.0, "%s: difference / tolerance = %g" % (what, worst)
    return got_s, got_p, want_s, want_p, worst


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


# ---- 1. finalized channels ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lattice_beam", [4.0, 8.0])
def test_finalized_channels(world, lattice_beam):
    """5 sequences per channel -- nbest_words(5)'s, or where the determinizer refuses the lattice the distinct word sequences among the
    40 cheapest raw paths -- at the three pairs of scales: the five posteriors sum to at most 1, and each is at least the posterior of
    the one path word_confidences aligns"""
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
        worst, mass = 0.0, []
        for sc in SCALES:
            got, gotp, want, _, r = check(dec, ch, seqs, True, sc, "lattice_beam %g" % lattice_beam, lattices=lat)
            worst = max(worst, r)
            conf = dec.word_confidences(seqs, ch, graph_scale=sc[0], acoustic_scale=sc[1])
            for i in range(len(ch)):
                k = len(seqs[i]) - 3
                assert all(want[i][j]["found"] and got[i][j]["found"] and gotp[i][j]["found"] for j in range(k))
                assert not got[i][k]["found"] and not gotp[i][k]["found"] and not got[i][k + 2]["found"]
                total = sum(np.exp(got[i][j]["logpost"]) for j in range(k))
                assert total <= 1.0 + sum(want[i][j]["tol"] for j in range(k)), (sc, i, total)
                for j in range(k):
                    assert conf[i][j]["found"] and got[i][j]["logpost"] >= conf[i][j]["path_logpost"] - want[i][j]["tol"], (sc, i, j)
                mass.append(round(float(total), 4))
        print("finalized, lattice_beam %g: largest difference / tolerance %.3g; posterior mass of the five per (scales, channel): %s"
              % (lattice_beam, worst, mass))
    finally:
        dec.free()


# ---- 2. live channels, read-only ----------------------------------------------------------------------------------------------
def test_live_channels_and_the_call_is_read_only(world):
    """the 150-frame utterance at lattice_beam 8: at frame 40 a frame of about 405 states, at frame 75 frames of about 2 600, whose
    cells stride the block several times; both use_final_probs, both live-prune modes.  Channel 0 is queried, channel 1 is its
    twin that never is."""
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
                    got, gotp, _, _, r = check(dec, [0], seqs, ufp, sc, "frame %d mode %d ufp %d" % (upto, mode, ufp), lattices=[L])
                    worst = max(worst, r)
                    sizes.append((upto, mode, int(ufp), L.n_states, int(np.bincount(L.st_frame).max()), got[0][0]["found"] and gotp[0][0]["found"]))
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
        seqs, n_eps_words, depth, n_neg = [], 0, 0, 0
        for c in ch:
            w = [int(x) for x in dec.words([c])[0][0]]
            L = lat[c]
            if L is None:
                seqs.append([w] + variants(w))
                continue
            n_eps_words += int(((L.a_il == 0) & (L.a_ol != 0)).sum())
            n_neg += int(((L.a_graph + L.a_ac) < 0).sum())
            depth = max(depth, posteriors(L)["n_levels"] - len(np.unique(L.st_frame)))
            listed = {tuple(int(x) for x in p["olabel"] if x) for p in pyoracle.nshortest_paths(L, 12)}
            seqs.append([w] + [list(s) for s in sorted(listed)][:4] + variants(w))
        worst = 0.0
        for sc in SCALES[:2]:
            got, _, _, _, r = check(dec, ch, seqs, True, sc, name, lattices=lat)
            worst = max(worst, r)
            assert all(got[i][0]["found"] == (lat[i] is not None) for i in ch)
        print("%s: largest difference / tolerance %.3g; words on epsilon arcs %d, epsilon levels beyond the frames' own %d, negative arcs %d"
              % (name, worst, n_eps_words, depth, n_neg))
        if name == "lattice_eps_chains":
            assert n_eps_words > 0 and depth >= 2, "the fixture's point: the level rounds exceed 1"
        if name == "neg_hclg600":
            assert n_neg > 0
    finally:
        dec.free()
        graph.free()


# ---- 4. the long chain: rows of 2, 64, 65, 66 and 71 cells -------------------------------------------------------------------------
def test_sequences_of_1_63_64_65_and_70_words(synth, tmp_path):
    """70 steps, each with the step's own word or none: every subsequence of 1..70 is a sentence of the lattice.  As phrases the same
    lengths start at step 0 and at step 5 (65 words are left there: the longest that fits)"""
    import gpu_util as G

    T = 70
    g = synth.graph_from_arc_lists(T + 1, 0, {s: [(2 * s + 1, s + 1, 0.5, s + 1), (2 * s + 2, 0, 0.25, s + 1)] for s in range(T)}, {T: 0.0})
    m = np.arange(2 * T + 1, dtype=np.int32) - 1
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
        assert [len(s) for s in seqs[0][:5]] == [1, 63, 64, 65, 70]
        phrases = [[every[:1], every[:63], every[:64], every[:65], every, every[5:6], every[5:68], every[5:69], every[5:70], every[:10] + every[30:40], [2, 1]]]
        got, gotp, _, _, worst = check(dec, [0], seqs, True, (1.0, 1.0), "chain", phrases=phrases)
        assert [r["found"] for r in got[0]] == [True] * 6 + [False]
        # (contiguous in the path's WORDS: the steps 11..30 have wordless arcs, so 10 and 31 are neighbours on some path)
        assert [r["found"] for r in gotp[0]] == [True] * 10 + [False]
        assert all(-700.0 < r["logpost"] < 0.0 for r in got[0][:6])
        print("chain: largest difference / tolerance %.3g" % worst)
    finally:
        dec.free()
        graph.free()


# ---- 5. a word said twice inside one cell -----------------------------------------------------------------------------------------
def test_a_word_said_twice_in_one_cell(synth, tmp_path):
    """word 5 free on either of two steps, a wordless arc at graph cost 1 beside it: the paths say 5 5, 5, 5 and nothing.  The count
    of the phrase [5] is 2 / (1 + 1/e) = 1.46, and its hit_mass over the one cell word_confidences gives [5] is that call's word_post"""
    import gpu_util as G

    g = synth.graph_from_arc_lists(5, 0, {0: [(1, 5, 0.0, 1), (2, 0, 1.0, 2)], 1: [(3, 5, 0.0, 3), (4, 0, 1.0, 4)], 2: [(3, 5, 0.0, 3), (4, 0, 1.0, 4)]},
                                   {3: 0.0, 4: 0.0})
    path = str(tmp_path / "twice.bin")
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
        seqs = [[[5], [5, 5], [], [6]]]
        got, gotp, _, _, worst = check(dec, [0], seqs, True, (1.0, 1.0), "twice", phrases=[[[5], [5, 5], None, [6]]])
        z = (1.0 + np.exp(-1.0)) ** 2
        one, two, none, absent = got[0]
        assert abs(np.exp(one["logpost"]) - 2.0 * np.exp(-1.0) / z) < 1e-12 and abs(np.exp(two["logpost"]) - 1.0 / z) < 1e-12
        assert abs(np.exp(none["logpost"]) - np.exp(-2.0) / z) < 1e-12 and not absent["found"]
        p1, p2, _, p6 = gotp[0]
        assert p1["count"] > 1.0 and abs(p1["count"] - 2.0 / (1.0 + np.exp(-1.0))) < 1e-12 and p1["conf"] == 1.0
        assert abs(p2["count"] - 1.0 / z) < 1e-12 and p2["hit_mass"][0] == 0.0 and not p6["found"]
        wp = dec.word_confidences([[[5]]], [0])[0][0]["word_post"][0]
        assert abs(p1["hit_mass"].sum() - wp) < 1e-12 and abs(p1["count"] - wp) < 1e-12
        print("twice: largest difference / tolerance %.3g" % worst)
    finally:
        dec.free()
        graph.free()


# ---- 6. 64 sequences on one channel -------------------------------------------------------------------------------------------------
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
        got, gotp, _, _, worst = check(dec, [0], [seqs], True, (1.0, 0.1), "64 sequences", lattices=[L])
        assert len(got[0]) == len(gotp[0]) == 64 and sum(r["found"] for r in got[0]) >= len(real) >= 2
        assert sum(np.exp(r["logpost"]) for r in got[0][:len(real)]) <= 1.0 + 1e-9
        print("64 sequences: largest difference / tolerance %.3g" % worst)
    finally:
        dec.free()


# ---- 7. mixed lists, a channel over max_cells, a lattice longer than cap_frames, nbest_words_conf -------------------------------------
def test_mixed_list_capacities_and_nbest_words_conf(world):
    dec = decoder(world, 4.0)
    try:
        dec.init()
        dec.advance(world["ptrs"], [40, 60, 75], N_TID // 2)
        dec.finalize(channels=[0, 2])          # channel 1 stays live at frame 60
        dec.set_live_lattice_prune(1)
        ch = [1, 2, 0]
        w = [[int(x) for x in dec.words([c])[0][0]] for c in ch]
        seqs = [[w[0], w[0][:1]], [w[1], None, w[1][:-1], []], [w[2]]]
        got, _, _, _, worst = check(dec, ch, seqs, True, (1.0, 1.0), "mixed")
        assert all(a[0]["found"] for a in got)
        lat = [from_gpu(dec.raw_lattice(c, True)) for c in ch]
        phrases = [phrases_of(s) for s in seqs]
        cells = [L.n_states * (1 + max(len(s) for s in sq if s is not None)) for L, sq in zip(lat, phrases)]
        big = int(np.argmax(cells))
        assert sorted(cells)[-1] > sorted(cells)[-2]
        # the longest lattice among the other two does not fit cap_frames
        rest = sorted(set(range(3)) - {big}, key=lambda i: n_frames_of(lat[i]))
        short, long_ = rest
        assert n_frames_of(lat[short]) < n_frames_of(lat[long_])
        tight = dec.phrase_posteriors(phrases, ch, max_cells=cells[big] - 1, hit_mass=True, cap_frames=n_frames_of(lat[long_]) - 1)
        assert [a[0]["status"] for a in tight] == [E_CAPACITY if i in (big, long_) else 0 for i in range(3)]
        for r in tight[big]:
            assert not r["found"] and r["count"] == 0.0 and r["log_z"] == 0.0 and r["n_frames"] == 0 and not r["hit_mass"].any()
        for i in (short, long_):
            P = posteriors(lat[i])
            for q, r in enumerate(phrase_many(lat[i], phrases[i], post=P)):
                g = tight[i][q]
                assert g["n_frames"] == n_frames_of(lat[i]) and abs(g["log_z"] - P["log_z"]) <= P["tol_log"]
                if r is None:
                    assert not g["found"] and g["count"] == 0.0
                    continue
                assert (g["hit_mass"] is None) == (i == long_)
                worst = max(worst, compare_phrase(g, r, lat[i], "beside the channel over max_cells: %d %d" % (i, q), rows=i == short))
        sent = dec.sentence_posteriors(seqs, ch, max_cells=max(L.n_states * (1 + max(len(s) for s in sq if s is not None))
                                                                for L, sq in zip(lat, seqs)) - 1)
        assert sorted(a[0]["status"] for a in sent) == [E_CAPACITY, 0, 0]
        assert all((not a[0]["found"] and a[0]["logpost"] == 0.0) == (a[0]["status"] != 0) for a in sent)
        assert worst <= 1.0
        # use_final_probs = 0: the finalized channels have no lattice (found 0, status OK, log_z 0), the live one answers
        w0 = [int(x) for x in dec.words([1], use_final_probs=False)[0][0]]
        live_only = dec.sentence_posteriors([[w0], [w[1]], [w[2]]], ch, use_final_probs=False)
        assert [a[0]["status"] for a in live_only] == [0, 0, 0] and [a[0]["found"] for a in live_only] == [True, False, False]
        assert live_only[1][0]["log_z"] == 0.0 and live_only[0][0]["log_z"] != 0.0
        # nbest_words_conf(sentence_post=True) = nbest_words_conf() plus sentence_posteriors of the paths' words
        conf = dec.nbest_words_conf(3, channels=ch)
        both = dec.nbest_words_conf(3, channels=ch, sentence_post=True)
        sp = dec.sentence_posteriors([[p["words"] for p in paths] for _, paths in conf], ch)
        n = 0
        for (st, paths), (st1, paths1), s in zip(conf, both, sp):
            assert st == st1 == 0 and len(paths) == len(paths1) >= 1
            for p, p1, x in zip(paths, paths1, s):
                assert set(p1) - set(p) == {"sent_logpost", "sent_found"}
                for k in ("words", "found", "begin", "end", "n_arcs", "tot", "lm", "align_tot", "align_lm"):
                    assert np.asarray(p[k]).tobytes() == np.asarray(p1[k]).tobytes(), k
                assert p1["sent_found"] and x["found"] and abs(p1["sent_logpost"] - x["logpost"]) <= 1e-9
                assert p1["path_logpost"] - 1e-9 <= p1["sent_logpost"] <= 1e-9
                n += 1
        print("mixed: largest difference / tolerance %.3g; nbest_words_conf paths %d" % (worst, n))
    finally:
        dec.free()


# ---- 8. a biglm lattice decoder -----------------------------------------------------------------------------------------------
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
        got, gotp, _, _, worst = check(dec, [u], seqs, True, (1.0, 0.1), "biglm", lattices=[L])
        n_found = sum(r["found"] for r in got[0])
        print("biglm: %d sequences found; largest difference / tolerance %.3g" % (n_found, worst))
        assert n_found >= 2 and gotp[0][0]["found"]
    finally:
        dec.free()
        for lm in lms:
            lm.free()
        graph.free()


# ---- 9. the error surface -------------------------------------------------------------------------------------------------------
def test_error_surface(world):
    W = world["W"]
    plain = decoder(world, 4.0, 2, lattice_links=0)
    try:
        plain.init()
        plain.advance(world["ptrs"][:2], [10, 10], N_TID // 2)
        for call in (plain.sentence_posteriors, plain.phrase_posteriors):
            with pytest.raises(W.WfstError) as e:
                call([[[1]], [[1]]])
            assert e.value.code == E_STATE
    finally:
        plain.free()
    dec = decoder(world, 4.0, 3)
    try:
        dec.init(channels=[0, 1])
        dec.advance(world["ptrs"][:2], [20, 20], N_TID // 2, channels=[0, 1])
        for call in (dec.sentence_posteriors, dec.phrase_posteriors):
            ok = call([[[1]]], [0], use_final_probs=False)
            assert ok[0][0]["status"] == 0
            for seqs, ch, code in (([[[1]], [[1]]], [0, 0], E_ARG), ([[[1]], [[1]]], [0, 3], E_ARG), ([[[1]], [[1]]], [0, 2], E_STATE),
                                   ([[[1, 0]]], [0], E_ARG), ([[[-4]]], [0], E_ARG), ([[[1]] * 65], [0], E_ARG)):
                with pytest.raises(W.WfstError) as e:
                    call(seqs, ch, use_final_probs=False)
                assert e.value.code == code, (seqs, ch)
            for gs, as_ in ((-1.0, 1.0), (1.0, -0.5), (float("nan"), 1.0), (1.0, float("inf")), (float("-inf"), 1.0)):
                with pytest.raises(W.WfstError) as e:
                    call([[[1]]], [0], use_final_probs=False, graph_scale=gs, acoustic_scale=as_)
                assert e.value.code == E_ARG, (gs, as_)
        assert dec.sentence_posteriors([[[]]], [0], use_final_probs=False)[0][0]["status"] == 0      # the empty sentence is one
        with pytest.raises(W.WfstError) as e:
            dec.phrase_posteriors([[[]]], [0], use_final_probs=False)                                # the empty phrase is none
        assert e.value.code == E_ARG
        # through the C ABI: NULL outputs are fine; mode, cap_frames and hit_mass are checked
        import ctypes as C
        I, D = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        one, words, length = np.array([0], np.int32), np.array([1, 1], np.int32), np.array([1], np.int32)
        rows = np.zeros(64, np.float64)
        p = lambda a: a.ctypes.data_as(I)
        call = lambda mode, n_seqs, cap, ln, capf=0, hit=None: W.lib().wfst_decoder_sequence_posterior(
            dec.h, p(one), 1, 0, C.c_double(1.0), C.c_double(1.0), mode, n_seqs, cap, p(words), p(ln), C.c_int64(0), capf,
            None, None, None, None, None, hit)
        assert call(0, 0, 2, length) == E_ARG and call(0, 1, 0, length) == E_ARG and call(1, 1, 2, np.array([3], np.int32)) == E_ARG
        assert call(2, 1, 2, length) == E_ARG and call(-1, 1, 2, length) == E_ARG and call(1, 1, 2, length, -1) == E_ARG
        assert call(1, 1, 2, length, 0, rows.ctypes.data_as(D)) == E_ARG and call(1, 1, 2, np.array([0], np.int32)) == E_ARG
        assert call(0, 1, 2, length) == 0 and call(1, 1, 2, length) == 0 and call(1, 1, 2, length, 64, rows.ctypes.data_as(D)) == 0
    finally:
        dec.free()
