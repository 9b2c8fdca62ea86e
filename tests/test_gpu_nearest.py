"""-m gpu: wfst_decoder_nearest_words (align_index_kernel / nearest_kernel) -- the path of a channel's raw lattice nearest a reference
word sequence: least word edit distance, then least cost, with the edit counts, the path's words, their times and scores.

The reference of every comparison is the definition restated in numpy (tests/nearest_util.py) over dec.raw_lattice(channel,
use_final_probs) fetched at the same moment: every integer output equal, tot_score and lm_score equal bit for bit.  There are no
tolerances."""
import json
import os

import numpy as np
import pytest

import pyoracle
import tie_util as TU
from golden_util import GOLDEN_DIR, Golden, bits
from nearest_util import from_gpu, levenshtein, nearest_many

pytestmark = pytest.mark.gpu

E_ARG, E_CAPACITY, E_STATE = -1, -4, -5
N_TID = 600
LIM = dict(max_frames=192, max_tokens_per_frame=32768, arena_tokens=1 << 20, lattice_links=1 << 21)
NO_WORD = 777   # a word id the graph (500 words) does not have
INTS = ("n_err", "n_cor", "n_sub", "n_ins", "n_del", "n_arcs", "n_hyp")
COUNT = dict(answers=0, errors=0, ties=0)


def cfg(lattice_beam):
    return dict(beam=12.0, max_active=1000000, min_active=0, lattice_beam=lattice_beam, prune_interval=10)


@pytest.fixture(scope="module")
def world(synth, tmp_path_factory):
    """test_gpu_align.py's world: the 3000-state graph of seed 21, utterances of 40 / 97 / 150 frames"""
    import gpu_util as G

    W = G.wfstdec
    g = synth.make_hclg_like(3000, seed=21, n_tid=N_TID, n_words=500)
    m = synth.default_tid2pdf(N_TID)
    path = str(tmp_path_factory.mktemp("nearest") / "g.bin")
    g.write(path)
    graph = W.Graph.load(path)
    graph.set_tid2pdf(m)
    graph.set_tid2phone(np.arange(N_TID + 1, dtype=np.int32))   # identity: a phone is a transition-id
    mats = [synth.make_loglikes(g, T, N_TID // 2, m, seed=s, mu=-2.2)[0] for T, s in ((40, 700), (97, 701), (150, 702))]
    dev = G.upload(mats)
    yield dict(G=G, W=W, graph=graph, mats=mats, dev=dev, ptrs=[t.data_ptr() for t in dev], T=[x.shape[0] for x in mats])
    print("figures: %(answers)d answers equal to the restatement's, %(errors)d of them with errors, %(ties)d through a tied decision" % COUNT)
    graph.free()


def decoder(world, lattice_beam, n=3, **kw):
    lim = dict(LIM)
    lim.update(kw)
    return world["W"].BatchDecoder(world["graph"], world["G"].gpu_config(cfg(lattice_beam)), n, **lim)


def decode_all(world, dec):
    dec.init()
    dec.advance(world["ptrs"], world["T"], N_TID // 2)
    dec.finalize()


def blank(got, what):
    assert not got["found"] and all(got[k] == 0 for k in INTS), what
    assert len(got["hyp_words"]) == 0 and not got["ref_hyp"].any() and bits([got["tot"], got["lm"]]).tolist() == [0, 0], what


def same(got, want, what):
    """one (channel, reference) answer against the restatement's"""
    if want is None or not want["found"]:   # skipped / no lattice / no final state reached
        blank(got, what)
        return
    assert got["found"], what + " found"
    for k in INTS:
        assert got[k] == want[k], "%s %s: %d, the restatement has %d" % (what, k, got[k], want[k])
    for k in ("hyp_words", "begin", "end", "ref_hyp"):
        assert np.array_equal(got[k], want[k]), "%s %s" % (what, k)
    assert bits([got["tot"], got["lm"]]).tolist() == bits([want["tot"], want["lm"]]).tolist(), what + " scores"
    COUNT["answers"] += 1
    COUNT["errors"] += want["n_err"] > 0
    COUNT["ties"] += want["tie"]


def equal_answers(a, b, what, n_words=None):
    """two answers of the device: everything equal (the hypothesis arrays of `a` against the first n_words of b's)"""
    assert all(a[k] == b[k] for k in INTS + ("found",)) and np.array_equal(a["ref_hyp"], b["ref_hyp"]), what
    assert bits([a["tot"], a["lm"]]).tolist() == bits([b["tot"], b["lm"]]).tolist(), what
    for k in ("hyp_words", "begin", "end"):
        assert np.array_equal(a[k], b[k][:n_words]), "%s %s" % (what, k)


def check(dec, channels, refs, ufp, sil_tids=None, what="", max_cells=0):
    """nearest_words of the list against the restatement on each channel's raw lattice now; returns (got, want)"""
    got = dec.nearest_words(refs, channels, use_final_probs=ufp, max_cells=max_cells)
    want = []
    for i, c in enumerate(channels):
        L = from_gpu(dec.raw_lattice(int(c), ufp))
        want.append(nearest_many(L, refs[i], sil_tids))
        assert len(got[i]) == len(refs[i])
        for q in range(len(refs[i])):
            assert got[i][q]["status"] == 0, "%s channel %d" % (what, c)
            same(got[i][q], want[i][q], "%s channel %d reference %d" % (what, c, q))
    return got, want


def variants(words):
    """the references every test asks: the words themselves, one replaced by a word the graph lacks, one dropped, one doubled, the
    words reversed, the empty reference, a skip"""
    w = [int(x) for x in words]
    mid = len(w) // 2
    replaced, dropped, doubled = list(w), list(w), list(w)
    if w:
        replaced[mid] = NO_WORD
        del dropped[mid]
        doubled.insert(mid, w[mid])
    else:
        replaced = [NO_WORD]
    return [w, replaced, dropped, doubled, w[::-1], [], None]


def canonical_states(L):
    k = np.stack([L.st_frame, L.st_gstate, L.st_final], axis=1)
    return k[np.lexsort(k.T[::-1])]


def canonical_arcs(L):
    f, g = L.st_frame, L.st_gstate
    k = np.stack([f[L.a_src], g[L.a_src], f[L.a_dst], g[L.a_dst], L.a_il, L.a_ol, bits(L.a_graph), bits(L.a_ac)], axis=1)
    return k[np.lexsort(k.T[::-1])]


# ---- 1. finalized channels ----------------------------------------------------------------------------------------------------
def test_finalized_channels(world):
    n = n_same_path = 0
    for lb in (4.0, 8.0):
        dec = decoder(world, lb)
        try:
            decode_all(world, dec)
            ch = [2, 0, 1]
            best = dec.words(ch)
            refs = [variants(best[i][0]) for i in range(3)]
            got, want = check(dec, ch, refs, True, what="lattice_beam %g" % lb)
            for i in range(3):
                w = [int(x) for x in best[i][0]]
                assert len(w) >= 2
                r = got[i]
                # the best path is a path of the lattice: its own words are there without an error, and bound every other answer
                assert r[0]["n_err"] == 0 and r[0]["hyp_words"].tolist() == w and r[0]["ref_hyp"].tolist() == list(range(len(w)))
                assert r[1]["n_err"] == 1 and r[2]["n_err"] <= 1 and r[3]["n_err"] <= 1
                for q in range(6):
                    assert r[q]["n_err"] <= levenshtein(w, refs[i][q]) and levenshtein(r[q]["hyp_words"].tolist(), refs[i][q]) == r[q]["n_err"]
                n += 6
                # where align_words finds the sequence the two agree on the cost, and -- no exact tie on the way -- on the path
                al = dec.align_words([[w]], [ch[i]])[0][0]
                assert al["found"] and bits(al["tot"]).tolist() == bits(r[0]["tot"]).tolist()
                if not want[i][0]["tie"]:
                    assert np.array_equal(al["begin"], r[0]["begin"]) and np.array_equal(al["end"], r[0]["end"])
                    assert bits(al["lm"]).tolist() == bits(r[0]["lm"]).tolist() and al["n_arcs"] == r[0]["n_arcs"]
                    n_same_path += 1
        finally:
            dec.free()
    assert n == 36 and n_same_path >= 4


# ---- 2. live channels, read-only ----------------------------------------------------------------------------------------------
def test_live_channels_and_the_call_is_read_only(world):
    """the 150-frame utterance at lattice_beam 8: at frame 40 the live lattice has a frame of about 405 states, at frame 75 frames of
    about 2 600 -- more cells than the workgroup has lanes either way, more states than lanes at 75.  Channel 0 is queried, channel 1
    is its twin that never is."""
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
                    got, _ = check(dec, [0], [variants(w)], ufp, what="frame %d mode %d ufp %d" % (upto, mode, ufp))
                    L = dec.raw_lattice(0, ufp)
                    sizes.append((upto, mode, int(ufp), L["n_states"], int(np.bincount(L["st_frame"]).max()), got[0][0]["n_err"]))
            dec.set_live_lattice_prune(0)
        print("(frame, mode, ufp, states, widest frame, errors of the best words):", sizes)
        assert any(s[4] > 256 and s[4] < 1024 for s in sizes) and any(s[4] > 1024 for s in sizes) and all(s[5] == 0 for s in sizes)
        dec.advance([p, p], [150, 150], stride)
        dec.finalize()
        a, b = dec.best_paths([0, 1])
        for k in ("ilabel", "olabel"):
            assert np.array_equal(a[k], b[k]), k
        for k in ("graph", "ac"):
            assert np.array_equal(bits(a[k]), bits(b[k])), k
        # (tokens of a frame are numbered in the order the device created them: the lattices are compared up to that numbering)
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
        refs = [variants(dec.words([c])[0][0])[:3] for c in ch]
        plain, want = check(dec, ch, refs, True, what="no list")
        # the silence phones (= transition-ids here): every second emitting transition-id of the nearest paths themselves
        tids = []
        for c, w in zip(ch, want):
            L = from_gpu(dec.raw_lattice(c, True))
            il = L.a_il[w[0]["arcs"]]
            tids += [int(t) for t in il[il != 0][1::2]]
        sil = sorted(set(tids))
        dec.set_silence_phones(sil)
        trimmed, _ = check(dec, ch, refs, True, sil_tids=np.array(sil), what="silence list")
        assert any((t[q]["end"] != p[q]["end"]).any() for t, p in zip(trimmed, plain) for q in range(3) if len(t[q]["end"]) == len(p[q]["end"]))
        assert all(np.array_equal(t[0]["begin"], p[0]["begin"]) for t, p in zip(trimmed, plain))
        dec.set_silence_phones([])
        again, _ = check(dec, ch, refs, True, what="list cleared")
        assert all(np.array_equal(t[0]["end"], p[0]["end"]) for t, p in zip(again, plain))
    finally:
        dec.free()


# ---- 4. the wave-width boundary -----------------------------------------------------------------------------------------------
def test_references_of_1_63_64_65_and_70_words(synth, tmp_path):
    """test_gpu_align.py's chain of 70 steps; every step has an emitting arc with a word (word s + 1 at step s) and one without, so a
    path spells any subsequence of 1..70: rows of 2, 64, 65, 66 and 71 cells -- the deletion scan inside a wave, up to its last
    lane, and across one and two chunk boundaries -- with references that are subsequences (no error) and ones that are not"""
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
        shifted = [NO_WORD] * 5 + every[:60]                         # 65 words: five deletions before anything matches
        holes = [w if w % 7 else NO_WORD for w in every]             # 70 words, ten of them substituted
        refs = [[[35], [NO_WORD], every[3:66], every[:64], every[2:67], every, every[::-1], shifted, holes, [2, 1], every[:64][::-1],
                 every[:31] + every[30:63]]]
        assert [len(r) for r in refs[0]] == [1, 1, 63, 64, 65, 70, 70, 65, 70, 2, 64, 64]
        got, _ = check(dec, [0], refs, True, what="chain")
        assert [r["n_err"] for r in got[0]] == [0, 1, 0, 0, 0, 0, 69, 5, 10, 1, 63, 1]
        assert np.array_equal(got[0][5]["begin"], np.arange(T)) and np.array_equal(got[0][5]["end"], np.arange(1, T + 1))
        assert got[0][0]["begin"].tolist() == [34] and got[0][0]["end"].tolist() == [T]
        assert got[0][7]["n_del"] == 5 and got[0][7]["ref_hyp"].tolist() == [-1] * 5 + list(range(60))
    finally:
        dec.free()
        graph.free()


def test_a_path_with_more_words_than_the_binding_first_makes_room_for(synth, tmp_path):
    """one path of 20 words against references of 0, 1 and 3: the binding's first call has room for 3 + 16 words, learns n_hyp = 20
    from it and asks again; a caller's own cap_hyp is taken as it is"""
    import gpu_util as G

    T = 20
    g = synth.graph_from_arc_lists(T + 1, 0, {s: [(s + 1, s + 1, 0.5, s + 1)] for s in range(T)}, {T: 0.0})
    path = str(tmp_path / "line.bin")
    g.write(path)
    graph = G.wfstdec.Graph.load(path)
    graph.set_tid2pdf(synth.default_tid2pdf(T))
    x = np.random.RandomState(6).normal(-2.0, 1.0, (T, T // 2)).astype(np.float32)   # (default_tid2pdf: two transition-ids per column)
    dec = G.wfstdec.BatchDecoder(graph, G.gpu_config(dict(beam=200.0, max_active=1000000, min_active=0, lattice_beam=100.0, prune_interval=10)), 1,
                                 max_frames=32, max_tokens_per_frame=4096, arena_tokens=1 << 12, lattice_links=1 << 12)
    try:
        dev = G.upload([x])
        dec.init()
        dec.advance([dev[0].data_ptr()], [T], x.shape[1])
        dec.finalize()
        refs = [[[5], [], [1, 2, 3]]]
        got, _ = check(dec, [0], refs, True, what="line")
        assert [(r["n_hyp"], r["n_err"], r["n_ins"]) for r in got[0]] == [(20, 19, 19), (20, 20, 20), (20, 17, 17)]
        assert all(r["hyp_words"].tolist() == list(range(1, T + 1)) and r["end"].tolist() == list(range(1, T + 1)) for r in got[0])
        short = dec.nearest_words(refs, [0], cap_hyp=19)
        assert short[0][0]["status"] == E_CAPACITY
        for q in range(3):
            equal_answers(short[0][q], got[0][q], "cap_hyp 19: %d" % q, n_words=19)
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
        refs, n_eps_words, n_eps_arcs = [], 0, 0
        for c in ch:
            L = from_gpu(dec.raw_lattice(c, True))
            w = dec.words([c])[0][0]
            refs.append(variants(w))
            if L is None:   # (the reference's "no lattice": nothing is found)
                continue
            n_eps_words += int(((L.a_il == 0) & (L.a_ol != 0)).sum())
            n_eps_arcs += int((L.a_il == 0).sum())
            listed = {tuple(int(w) for w in p["olabel"] if w) for p in pyoracle.nshortest_paths(L, 12)}   # word sequences the lattice holds
            for s in [list(s) for s in sorted(listed)][:4]:
                refs[-1] += [s, s[1:], s + s[:1]]
        got, want = check(dec, ch, refs, True, what="eps chains")
        assert n_eps_words > 0 and n_eps_arcs > n_eps_words, "the fixture's point: arcs inside frames, words on some of them"
        assert all(got[i][0]["found"] == (dec.raw_lattice(i, True) is not None) for i in ch) and sum(r["found"] for a in got for r in a) >= 20
    finally:
        dec.free()
        graph.free()


# ---- 6. mixed lists, a channel over max_cells, a channel over cap_hyp ----------------------------------------------------------
def test_mixed_list_capacity_of_one_channel_and_the_other_getters(world):
    dec = decoder(world, 4.0)
    try:
        dec.init()
        dec.advance(world["ptrs"], [40, 60, 75], N_TID // 2)
        dec.finalize(channels=[0, 2])          # channel 1 stays live at frame 60
        dec.set_live_lattice_prune(1)
        ch = [1, 2, 0]
        ufp = True

        def getters():
            return dict(words=dec.words([0, 2]), raw=[dec.raw_lattice(c) for c in (0, 2)], det=[dec.determinized_lattice(c) for c in (0, 2)],
                        nbp=[dec.nbest_paths(c, 3) for c in (0, 2)], live=dec.raw_lattice(1, ufp), nbw=dec.nbest_words(3, channels=ch),
                        aln=dec.align_words([[dec.words([c])[0][0]] for c in (0, 2)], [0, 2]))
        before = getters()
        w = [[int(x) for x in dec.words([c], use_final_probs=ufp)[0][0]] for c in ch]
        refs = [[w[0], w[0][:1]], [w[1], None, w[1][:-1], [], [NO_WORD] + w[1]], [w[2]]]     # differing counts and lengths per channel
        got, _ = check(dec, ch, refs, ufp, what="mixed")
        assert all(a[0]["found"] and a[0]["n_err"] == 0 for a in got)
        # max_cells just below the largest table of the list: that channel alone reports WFST_E_CAPACITY
        cells = [dec.raw_lattice(c, ufp)["n_states"] * (1 + max(len(s) for s in sq if s is not None)) for c, sq in zip(ch, refs)]
        big = int(np.argmax(cells))
        assert sorted(cells)[-1] > sorted(cells)[-2]
        tight = dec.nearest_words(refs, ch, use_final_probs=ufp, max_cells=cells[big] - 1)
        assert [a[0]["status"] for a in tight] == [E_CAPACITY if i == big else 0 for i in range(3)]
        for q in range(len(refs[big])):
            blank(tight[big][q], "the channel over max_cells")
        for i in set(range(3)) - {big}:
            for q in range(len(refs[i])):
                equal_answers(tight[i][q], got[i][q], "beside the channel over max_cells: %d %d" % (i, q))
        # cap_hyp one below the longest path of the list: the channels with such a path report WFST_E_CAPACITY and no other, n_hyp says
        # what it takes, the first cap_hyp words and times are there, and everything else stands
        n_hyp = [max(r["n_hyp"] for r in a) for a in got]
        room = max(n_hyp) - 1
        over = [E_CAPACITY if x > room else 0 for x in n_hyp]
        assert 0 in over and E_CAPACITY in over and room >= 1, n_hyp
        short = dec.nearest_words(refs, ch, use_final_probs=ufp, cap_hyp=room)
        assert [a[0]["status"] for a in short] == over
        for i in range(3):
            for q in range(len(refs[i])):
                equal_answers(short[i][q], got[i][q], "cap_hyp %d: %d %d" % (room, i, q), n_words=room)
        # use_final_probs = 0: the finalized channels have no lattice (found 0, status OK), the live one answers
        w[0] = dec.words([1], use_final_probs=False)[0][0]
        live_only = dec.nearest_words([[x] for x in w], ch, use_final_probs=False)
        assert [a[0]["status"] for a in live_only] == [0, 0, 0] and [a[0]["found"] for a in live_only] == [True, False, False]
        # the other getters answer what they answered before (align_words, whose workspace this call shares, among them)
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
    # (a lattice_beam wide enough that the utterances keep their lattices: tests/test_gpu_biglm.py)
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
        refs = [variants(dec.words([u])[0][0])]
        got = dec.nearest_words(refs, [u])
        want = nearest_many(L, refs[0])
        n_skipped = n_found = 0
        for q in range(len(refs[0])):
            if want[q] is not None and want[q]["found"] and want[q]["tie"]:
                # two tokens of a frame may share a graph state here: the path of a tie is unspecified, its errors and cost are not
                assert got[0][q]["n_err"] == want[q]["n_err"] and bits(got[0][q]["tot"]).tolist() == bits(want[q]["tot"]).tolist(), q
                n_skipped += 1
                continue
            same(got[0][q], want[q], "biglm reference %d" % q)
            n_found += got[0][q]["found"]
        print("biglm: %d references equal in full, %d through a tie (errors and cost equal)" % (n_found, n_skipped))
        assert n_found + n_skipped == 6 and got[0][0]["n_err"] == 0
    finally:
        dec.free()
        for lm in lms:
            lm.free()
        graph.free()


# ---- 8. exact ties -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("early_on_state_1", [True, False])
def test_the_kind_order_decides_the_times(early_on_state_1, synth, tmp_path):
    """test_gpu_align.py's fixture: two paths 0 -> 1 -> 3 and 0 -> 2 -> 3 of equal cost (0.5 + 0.5 per arc and frame: exact) that
    carry the same word, one on its first arc and one on its last.  Every reference below reaches the end state at the same cell over
    both, by different kinds: the kind order decides, whichever graph states the paths go through."""
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
        got, want = check(dec, [0], [[[5], [6], [5, 5], [], [6, 5], [5, 6]]], True, what="tie")
        assert all(w["tie"] for w in want[0]), "the fixture holds an exact tie for every reference"
        assert [r["n_err"] for r in got[0]] == [0, 1, 1, 1, 1, 1]
        # at the end state the word's arc arrives by a match (kind 0) and the other path's last arc is free (kind 1): the path with
        # the word on its LAST arc wins, whatever its graph states -- the word begins at frame 1 in both fixtures
        assert got[0][0]["begin"].tolist() == [1] and got[0][0]["end"].tolist() == [2]
        # the empty reference: both arrivals are of one kind per path (an insertion, or a free arc behind one); kind 1 wins: the
        # word sits on the first arc
        assert got[0][3]["begin"].tolist() == [0]
        assert bits([got[0][0]["tot"], got[0][0]["lm"]]).tolist() == bits([2.0, 1.0]).tolist()
    finally:
        dec.free()
        graph.free()


@pytest.mark.parametrize("wi", [1, 3])
def test_quantised_graphs_full_of_ties(wi, synth, tmp_path):
    """test_gpu_ties.py's small quantised graphs in lattice mode: exact cost ties abound, so the end state and the traceback's
    predecessors are decided by the rule, not by the costs"""
    import gpu_util as G

    W = G.wfstdec
    name, g, mats = TU.small_workloads(synth)[wi]
    p = str(tmp_path / "g.bin")
    g.write(p)
    graph = W.Graph.load(p)
    dec = W.BatchDecoder(graph, G.gpu_config(TU.SMALL_CFGS[0]), len(mats), lattice_links=1 << 18, max_frames=64, max_tokens_per_frame=4096,
                         arena_tokens=1 << 16)
    try:
        dev = G.upload(mats)
        dec.init()
        dec.advance([t.data_ptr() for t in dev], [int(x.shape[0]) for x in mats], int(mats[0].shape[1]))
        dec.finalize()
        ch = [c for c in range(len(mats)) if dec.raw_lattice(c, True) is not None]
        assert ch
        refs = []
        for c in ch:
            w = [int(x) for x in dec.words([c])[0][0]]
            refs.append([w, w[1:], w[:-1], w[::-1], [], [1, 2, 3, 1, 2, 3], w + w])
        _, want = check(dec, ch, refs, True, what=name)
        n_ties = sum(r["tie"] for a in want for r in a)
        print("%s: %d of %d answers through a tied decision" % (name, n_ties, sum(len(a) for a in want)))
        assert n_ties >= 1
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
            plain.nearest_words([[[1]], [[1]]])
        assert e.value.code == E_STATE
    finally:
        plain.free()
    dec = decoder(world, 4.0, 3)
    try:
        dec.init(channels=[0, 1])
        dec.advance(world["ptrs"][:2], [20, 20], N_TID // 2, channels=[0, 1])
        ok = dec.nearest_words([[[1]]], [0], use_final_probs=False)
        assert ok[0][0]["status"] == 0 and ok[0][0]["found"]
        for refs, ch, code in (([[[1]], [[1]]], [0, 0], E_ARG), ([[[1]], [[1]]], [0, 3], E_ARG), ([[[1]], [[1]]], [0, 2], E_STATE),
                               ([[[1, 0]]], [0], E_ARG), ([[[-4]]], [0], E_ARG), ([[[1]] * 65], [0], E_ARG)):
            with pytest.raises(W.WfstError) as e:
                dec.nearest_words(refs, ch, use_final_probs=False)
            assert e.value.code == code, (refs, ch)
        # through the C ABI: n_refs 0, cap_words 0, cap_hyp 0, a ref_len above cap_words, NULL references; NULL outputs are fine
        import ctypes as C
        I = C.POINTER(C.c_int32)
        one, words, length = np.array([0], np.int32), np.array([1, 1], np.int32), np.array([1], np.int32)
        p = lambda a: a.ctypes.data_as(I)
        call = lambda n_refs, cap, ln, hcap=4, w=words: W.lib().wfst_decoder_nearest_words(dec.h, p(one), 1, 0, n_refs, cap, None if w is None else p(w),
                                                                                          p(ln), hcap, C.c_int64(0), *([None] * 15))
        assert call(0, 2, length) == E_ARG and call(1, 0, length) == E_ARG and call(1, 2, np.array([3], np.int32)) == E_ARG
        assert call(1, 2, length, hcap=0) == E_ARG and call(1, 2, length, w=None) == E_ARG
        assert call(1, 2, length) == 0
    finally:
        dec.free()


# ---- 10. 64 references on one channel ---------------------------------------------------------------------------------------------
def test_64_references_on_one_channel(world):
    dec = decoder(world, 4.0, 1)
    try:
        dec.init()
        dec.advance(world["ptrs"][:1], [40], N_TID // 2)
        dec.finalize()
        w = [int(x) for x in dec.words([0])[0][0]]
        rs = np.random.RandomState(5)
        refs = []
        for q in range(64):   # the best words with q random edits
            r = list(w)
            for _ in range(q):
                op, at = rs.randint(3), rs.randint(len(r) + 1)
                if op == 0 or not r:
                    r.insert(at, int(rs.randint(1, 501)))
                elif op == 1:
                    del r[min(at, len(r) - 1)]
                else:
                    r[min(at, len(r) - 1)] = int(rs.randint(1, 501))
            refs.append(r)
        got, _ = check(dec, [0], [refs], True, what="64 references")
        assert all(got[0][q]["n_err"] <= q for q in range(64)) and got[0][0]["n_err"] == 0
    finally:
        dec.free()
