"""-m gpu: wfst_decoder_biased_words (bias_kernel behind align_index_kernel) -- the best path of a channel's raw lattice picked again
under scales, a word penalty and a per-channel list of boosted phrases.

The reference of every comparison is the definition restated in numpy (tests/bias_util.py on top of rescale_util.py) over
dec.raw_lattice(channel, use_final_probs) fetched at the same moment, and everything is compared BIT FOR BIT: found, the words,
their times, n_arcs, the hits, and the bits of biased_cost, bonus, tot_score and lm_score."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import bias_util as B
from align_util import from_gpu
from golden_util import GOLDEN_DIR, bits
from rescale_util import _levels, bits32, bits64

pytestmark = pytest.mark.gpu

E_ARG, E_CAPACITY, E_STATE = -1, -4, -5
N_TID = 600
LIM = dict(max_frames=192, max_tokens_per_frame=32768, arena_tokens=1 << 20, lattice_links=1 << 21)
WIDE = dict(beam=200.0, max_active=1000000, min_active=0, lattice_beam=100.0, prune_interval=10)
ABSENT = 100000   # word ids no lattice here holds
SETTINGS = [(1.0, 1.0, 0.0, 1.0), (1.0, 0.1, 0.5, 3.0), (0.0, 0.0, 0.0, 1.0), (1.0, 1.0, -3.0, 0.0), (0.7, 1.3, 0.3, 40.0)]


def cfg(lattice_beam):
    return dict(beam=12.0, max_active=1000000, min_active=0, lattice_beam=lattice_beam, prune_interval=10)


def sized_list(core, nodes, seed=0):
    """a list of exactly `nodes` nodes: the phrases of `core` (their prefixes shared as they come), then phrases of words no lattice
    holds -- one of 16 words where there is room, to the depth limit, and one-word phrases for the rest"""
    out = [(tuple(ws), float(b)) for ws, b in core]
    have = B.compile_list(out).J
    assert have <= nodes, (have, nodes)
    rs = np.random.RandomState(seed)
    if nodes - have >= 16:
        out.append((tuple(ABSENT + 5000 + k for k in range(16)), 0.5))
        have += 16
    for k in range(nodes - have):
        out.append(((ABSENT + k,), float(rs.randint(0, 9)) / 4.0))
    assert B.compile_list(out).J == nodes
    return out


def runs_of(words, rs, n, longest=3):
    """n phrases cut out of a word sequence: contiguous runs of 1..longest words, with bonuses of a few quarters"""
    out, seen = [], set()
    words = [int(w) for w in words]
    for _ in range(20 * n):
        if len(out) == n or not words:
            break
        k = rs.randint(1, min(longest, len(words)) + 1)
        at = rs.randint(0, len(words) - k + 1)
        ws = tuple(words[at:at + k])
        if ws not in seen:
            seen.add(ws)
            out.append((ws, 0.25 * rs.randint(1, 13)))
    return out


@pytest.fixture(scope="module")
def world(synth, tmp_path_factory):
    import gpu_util as G

    W = G.wfstdec
    g = synth.make_hclg_like(3000, seed=21, n_tid=N_TID, n_words=500)
    m = synth.default_tid2pdf(N_TID)
    path = str(tmp_path_factory.mktemp("bias") / "g.bin")
    g.write(path)
    graph = W.Graph.load(path)
    graph.set_tid2pdf(m)
    mats = [synth.make_loglikes(g, T, N_TID // 2, m, seed=s, mu=-2.2)[0] for T, s in ((40, 700), (97, 701), (150, 702))]
    dev = G.upload(mats)
    yield dict(G=G, W=W, graph=graph, mats=mats, dev=dev, ptrs=[t.data_ptr() for t in dev], T=[x.shape[0] for x in mats])
    graph.free()


def decoder(world, cd, n=3, **kw):
    lim = dict(LIM)
    lim.update(kw)
    return world["W"].BatchDecoder(world["graph"], world["G"].gpu_config(cd), n, **lim)


@pytest.fixture(scope="module")
def finalized(world):
    """the three utterances decoded and finalized at lattice_beam 6, their raw lattices, and per channel the words of a few paths the
    lattice holds: the 1-best at the search's scales and the best paths under other penalties"""
    dec = decoder(world, cfg(6.0))
    dec.init()
    dec.advance(world["ptrs"], world["T"], N_TID // 2)
    dec.finalize()
    lat = [from_gpu(dec.raw_lattice(c, True)) for c in range(3)]
    alt = [[r["hyp_words"].tolist() for r in row] for row in dec.rescaled_words([(1.0, 1.0, 0.0), (1.0, 0.1, -2.0), (0.1, 1.0, 0.0), (1.0, 1.0, 3.0)])]
    yield dict(dec=dec, lat=lat, alt=alt)
    dec.free()


def check(world, dec, channels, phrase_lists, list_of, settings=SETTINGS, ufp=True, what="", lattices=None, exact_path=True, **kw):
    """biased_words of the list against the restatement on each channel's raw lattice now; returns (got, want, lattices)"""
    lat = lattices if lattices is not None else [from_gpu(dec.raw_lattice(int(c), ufp)) for c in channels]
    autos = [B.compile_list(p) for p in phrase_lists]
    want = [B.bias_many(L, autos[l] if l >= 0 else B.NO_LIST, settings) for L, l in zip(lat, list_of)]
    lists = world["W"].BiasLists.from_phrases(phrase_lists) if phrase_lists else None
    try:
        got = dec.biased_words(lists, list_of, settings, channels, use_final_probs=ufp, **kw)
    finally:
        if lists is not None:
            lists.free()
    assert len(got) == len(channels)
    for i, c in enumerate(channels):
        assert len(got[i]) == len(settings)
        for q, s in enumerate(settings):
            tag = "%s channel %d setting %s" % (what, c, s)
            assert got[i][q]["status"] == 0, tag
            if not exact_path and want[i][q]["found"] and want[i][q]["ambiguous"]:
                assert got[i][q]["found"] and bits64(got[i][q]["biased_cost"]) == bits64(want[i][q]["biased_cost"]), tag
                continue
            B.same_answer(got[i][q], want[i][q], tag)
    return got, want, lat


def raw_call(W, dec, channels, lists, list_of, settings, cap_words, cap_hits, ufp=True, max_cells=0, with_hits=True):
    """the C entry point itself, with rows of the caller's size: dict of the raw output arrays and the return code"""
    I, D, F = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_float)
    ch, lo = np.ascontiguousarray(channels, np.int32), np.ascontiguousarray(list_of, np.int32)
    st = np.ascontiguousarray(settings, np.float64).reshape(-1, 4)
    n, ns = len(ch), len(st)
    pair = lambda t, fill: np.full((n, ns), fill, t)
    o = dict(status=np.full(n, 99, np.int32), found=pair(np.int32, 99), n_arcs=pair(np.int32, 99), n_hyp=pair(np.int32, 99), n_hits=pair(np.int32, 99),
             hyp_words=np.full((n, ns, cap_words), 99, np.int32), begin=np.full((n, ns, cap_words), 99, np.int32),
             end=np.full((n, ns, cap_words), 99, np.int32), hit_phrase=np.full((n, ns, max(cap_hits, 1)), 99, np.int32),
             hit_word=np.full((n, ns, max(cap_hits, 1)), 99, np.int32), biased_cost=pair(np.float64, 9.0), bonus=pair(np.float64, 9.0),
             tot=pair(np.float32, 9.0), lm=pair(np.float32, 9.0))
    p = lambda a: a.ctypes.data_as({np.dtype(np.int32): I, np.dtype(np.float64): D, np.dtype(np.float32): F}[a.dtype])
    o["rc"] = W.lib().wfst_decoder_biased_words(dec.h, p(ch), n, int(ufp), lists.h if lists is not None else None, p(lo), ns, p(st), cap_words, cap_hits,
                                                C.c_int64(max_cells), p(o["status"]), p(o["found"]), p(o["n_arcs"]), p(o["n_hyp"]), p(o["n_hits"]),
                                                p(o["hyp_words"]), p(o["begin"]), p(o["end"]), p(o["hit_phrase"]) if with_hits else None,
                                                p(o["hit_word"]) if with_hits else None, p(o["biased_cost"]), p(o["bonus"]), p(o["tot"]), p(o["lm"]))
    return o


def hand_decoder(synth, tmp_path, arcs_by_state, finals, T, n_tid, seed, name="hand"):
    """a hand-made graph with one score column per transition-id, decoded for T frames with nothing pruned and finalized"""
    import gpu_util as G

    n_states = 1 + max(max(arcs_by_state), max(a[3] for row in arcs_by_state.values() for a in row))
    g = synth.graph_from_arc_lists(n_states, 0, arcs_by_state, finals)
    m = np.arange(n_tid + 1, dtype=np.int32) - 1
    m[0] = 0
    x = np.random.RandomState(seed).normal(-2.0, 1.0, (T, n_tid)).astype(np.float32)
    path = str(tmp_path / (name + ".bin"))
    g.write(path)
    graph = G.wfstdec.Graph.load(path)
    graph.set_tid2pdf(m)
    dec = G.wfstdec.BatchDecoder(graph, G.gpu_config(WIDE), 1, max_frames=96, max_tokens_per_frame=4096, arena_tokens=1 << 16, lattice_links=1 << 16)
    dev = G.upload([x])
    dec.init()
    dec.advance([dev[0].data_ptr()], [T], n_tid)
    dec.finalize()
    return dec, graph


# ---- 1. the list sizes, a list of its own per channel --------------------------------------------------------------------------------
@pytest.mark.parametrize("nodes", [1, 2, 64, 65, 255, 256])
def test_list_sizes(world, finalized, nodes):
    """lists of exactly `nodes` nodes, another one for every channel, cut out of paths the channel's lattice holds; nodes = 1 is a
    list without phrases"""
    rs = np.random.RandomState(nodes)
    lists = []
    for c in range(3):
        pool = [w for seq in finalized["alt"][c] for w in seq]
        core = runs_of(pool, rs, min(nodes - 1, 12), longest=1 if nodes == 2 else 3) if nodes > 1 else []
        while core and B.compile_list(core).J > nodes:
            core.pop()
        lists.append(sized_list(core, nodes, seed=c))
    got, want, _ = check(world, finalized["dec"], [2, 0, 1], lists, [2, 0, 1], what="%d nodes" % nodes, lattices=[finalized["lat"][c] for c in (2, 0, 1)])
    hits = sum(g["n_hits"] for row in got for g in row)
    moved = sum(not np.array_equal(row[3]["hyp_words"], g["hyp_words"]) for row in got for g in row)
    print("%d nodes: %d hits over 15 answers, %d answers with other words than setting 3 has, %d through a tie"
          % (nodes, hits, moved, sum(w["tie"] for ws in want for w in ws)))
    assert all(g["found"] for row in got for g in row)
    assert (hits > 0) == (nodes > 1)


# ---- 2. frames of 255, 256 and 257 cells ---------------------------------------------------------------------------------------------
def test_frames_of_255_256_and_257_cells(synth, tmp_path):
    """a fan: the start state, K states one frame later, one state after them -- K x nodes cells in the middle frame, one below, at
    and one above the workgroup's lanes, with one node and with several"""
    import gpu_util as G

    n_cells = []
    for K, nodes in ((255, 1), (256, 1), (257, 1), (3, 85), (4, 64), (257, 3)):
        arcs = {0: [(1 + i, 1 + i % 5, 0.25 * (i % 7), 1 + i) for i in range(K)]}
        for i in range(K):
            arcs[1 + i] = [(K + 1 + i, 1 + (3 * i) % 5, 0.125 * (i % 3), K + 1)]
        dec, graph = hand_decoder(synth, tmp_path, arcs, {K + 1: 0.0}, 2, 2 * K, seed=K, name="fan%d_%d" % (K, nodes))
        try:
            L = from_gpu(dec.raw_lattice(0, True))
            per_frame = np.bincount(L.st_frame)
            assert per_frame[1] == K, "every middle state is in the lattice"
            n_cells.append(int(per_frame[1]) * nodes)
            core = [((1, 2), 1.5), ((2,), 0.25), ((3, 1), 0.75)] if nodes > 1 else []
            while core and B.compile_list(core).J > nodes:
                core.pop()
            lists = [sized_list(core, nodes)] if nodes > 1 else []
            check(dict(W=G.wfstdec), dec, [0], lists, [0 if nodes > 1 else -1], what="fan %d x %d" % (K, nodes), lattices=[L])
        finally:
            dec.free()
            graph.free()
    assert n_cells == [255, 256, 257, 255, 256, 771]


# ---- 3. chains inside a frame, a word on an epsilon-ilabel arc, overlapping and nested hits, the threshold of a bonus --------------------
def test_a_chain_inside_a_frame_earns_the_bonus_in_a_later_round(synth, tmp_path):
    """after the first frame two ways lead on inside the frame: one arc without a word, and a chain of two arcs with the words 7 and 8
    that costs more; the phrase (7 8) is completed on the chain's second arc, an epsilon-ilabel arc, which the sweep reaches in its
    second pass over the frame"""
    import gpu_util as G

    arcs = {0: [(1, 0, 0.5, 1)], 1: [(0, 0, 0.25, 3), (0, 7, 0.5, 2)], 2: [(0, 8, 0.5, 3)], 3: [(2, 0, 0.5, 4)]}
    dec, graph = hand_decoder(synth, tmp_path, arcs, {4: 0.0}, 2, 2, seed=1, name="chain")
    try:
        L = from_gpu(dec.raw_lattice(0, True))
        _, depth = _levels(L)
        assert int(depth.max()) >= 2 and np.any((L.a_il == 0) & (L.a_ol == 8))
        # the chain costs 0.75 more than the single arc: a bonus of 1.0 pays for it, one of 0.5 does not
        settings = [(1.0, 1.0, 0.0, 1.0), (1.0, 1.0, 0.0, 0.5), (1.0, 1.0, 0.0, 0.0)]
        got, want, _ = check(dict(W=G.wfstdec), dec, [0], [[((7, 8), 1.0)]], [0], settings, what="chain", lattices=[L])
        assert got[0][0]["hyp_words"].tolist() == [7, 8] and got[0][0]["bonus"] == 1.0 and got[0][0]["n_hits"] == 1
        assert got[0][0]["hit_phrase"].tolist() == [0] and got[0][0]["hit_word"].tolist() == [1]
        assert got[0][1]["hyp_words"].tolist() == [] and got[0][1]["bonus"] == 0.0 and got[0][1]["n_hits"] == 0
        assert got[0][2]["hyp_words"].tolist() == []
        assert abs(got[0][0]["biased_cost"] - (got[0][2]["biased_cost"] + 0.75 - 1.0)) < 1e-9
    finally:
        dec.free()
        graph.free()


def test_overlapping_and_nested_hits_and_the_bonus_that_just_flips_the_answer(synth, tmp_path):
    """a line of 8 steps; every step has an arc with a word (1 1 1 2 3 4 2 3) at 0.5 and one without at 0.25, so that a path spells
    any subsequence and every word costs 0.25 more than leaving it out, the scores being the same for both arcs of a step"""
    import gpu_util as G

    words = [1, 1, 1, 2, 3, 4, 2, 3]
    T = len(words)
    arcs = {s: [(s + 1, words[s], 0.5, s + 1), (s + 1, 0, 0.25, s + 1)] for s in range(T)}
    dec, graph = hand_decoder(synth, tmp_path, arcs, {T: 0.0}, T, T, seed=2, name="line")
    try:
        L = from_gpu(dec.raw_lattice(0, True))
        phrases = [((1, 1), 1.0), ((2, 3), 0.75), ((3,), 0.5), ((1, 2, 3), 2.0), ((9, 9), 50.0)]
        settings = [(1.0, 1.0, 0.0, 1.0), (1.0, 1.0, 0.0, 0.0), (1.0, 1.0, 0.0, 100.0)]
        got, want, _ = check(dict(W=G.wfstdec), dec, [0], [phrases], [0], settings, what="line", lattices=[L])
        g = got[0][0]
        # 1 1 1 pays twice (overlapping), 1 2 3 brings 2 3 and 3 with it (nested), 4 pays nothing and is left out, 2 3 again
        assert g["hyp_words"].tolist() == [1, 1, 1, 2, 3, 2, 3]
        assert list(zip(g["hit_phrase"].tolist(), g["hit_word"].tolist())) == [(0, 1), (0, 2), (3, 4), (1, 4), (2, 4), (1, 6), (2, 6)]
        assert g["bonus"] == 2 * 1.0 + (2.0 + 0.75 + 0.5) + (0.75 + 0.5)
        assert got[0][1]["hyp_words"].tolist() == [] and got[0][1]["n_hits"] == 0, "without a boost no word is worth 0.25"
        assert got[0][2]["biased_cost"] < 0 and got[0][2]["hyp_words"].tolist() == [1, 1, 1, 2, 3, 2, 3], "the phrase that is not there stays out"
        # the one-word phrase alone: a word costs 0.25 (up to the rounding of the float64 sums, far below 1e-7), so bs * 0.5
        # flips the answer just above bs = 0.5 and not just below
        lo, hi = 0.5 * (1.0 - 1e-6), 0.5 * (1.0 + 1e-6)
        got, want, _ = check(dict(W=G.wfstdec), dec, [0], [[((3,), 0.5)]], [0], [(1.0, 1.0, 0.0, lo), (1.0, 1.0, 0.0, hi)], what="flip", lattices=[L])
        assert got[0][0]["hyp_words"].tolist() == [] and got[0][1]["hyp_words"].tolist() == [3, 3]
    finally:
        dec.free()
        graph.free()


# ---- 4. without a list, without a boost: the rescaled words -------------------------------------------------------------------------------
def test_no_list_and_no_boost_are_the_rescaled_words(world, finalized):
    dec, lat = finalized["dec"], finalized["lat"]
    rs = np.random.RandomState(4)
    lists = [sized_list(runs_of(finalized["alt"][c][0], rs, 6), 40, seed=c) for c in range(3)]
    triples = [(1.0, 1.0, 0.0), (1.0, 0.1, 0.5), (0.7, 1.3, -0.3)]
    plain = dec.rescaled_words(triples, [0, 1, 2])
    no_list, want_a, _ = check(world, dec, [0, 1, 2], lists, [-1, -1, -1], [t + (2.0,) for t in triples], what="no list", lattices=lat)
    no_boost, want_b, _ = check(world, dec, [0, 1, 2], lists, [0, 1, 2], [t + (0.0,) for t in triples], what="no boost", lattices=lat)
    none_at_all, _, _ = check(world, dec, [0, 1, 2], [], [-1, -1, -1], [t + (2.0,) for t in triples], what="no set", lattices=lat)
    mixed, _, _ = check(world, dec, [0, 1, 2], lists, [1, -1, 0], [t + (2.0,) for t in triples], what="some", lattices=lat)
    full = 0
    for i in range(3):
        for q in range(3):
            for got, want in ((no_list[i][q], want_a[i][q]), (no_boost[i][q], want_b[i][q]), (none_at_all[i][q], want_a[i][q]), (mixed[1][q], want_a[1][q])):
                p = plain[i][q] if got is not mixed[1][q] else plain[1][q]
                assert got["found"] and bits64(got["biased_cost"]) == bits64(p["scaled_cost"]) and bits64(got["bonus"]) == bits64(0.0)
                if not want["tie"]:
                    full += 1
                    assert np.array_equal(got["hyp_words"], p["hyp_words"]) and got["n_arcs"] == p["n_arcs"]
                    assert np.array_equal(got["begin"], p["begin"]) and np.array_equal(got["end"], p["end"])
                    assert bits32(got["tot"]) == bits32(p["tot"]) and bits32(got["lm"]) == bits32(p["lm"])
            assert no_list[i][q]["n_hits"] == 0
    assert full >= 18


# ---- 5. a phrase the lattice does not hold -------------------------------------------------------------------------------------------------
def test_a_phrase_absent_from_the_lattice_changes_nothing(world, finalized):
    dec, lat = finalized["dec"], finalized["lat"]
    best = finalized["alt"][1][0]
    assert len(best) >= 2
    # words no lattice holds, and two of the best path's own words the wrong way round with a word in between that is not there
    phrases = [((ABSENT, ABSENT + 1), 1000.0), ((best[1], ABSENT + 2, best[0]), 1000.0)]
    got, want, _ = check(world, dec, [1], [phrases], [0], [(1.0, 1.0, 0.0, 1.0)], what="absent", lattices=[lat[1]])
    plain = dec.rescaled_words([(1.0, 1.0, 0.0)], [1])[0][0]
    assert got[0][0]["n_hits"] == 0 and got[0][0]["bonus"] == 0.0 and bits64(got[0][0]["biased_cost"]) == bits64(plain["scaled_cost"])
    assert np.array_equal(got[0][0]["hyp_words"], plain["hyp_words"])


# ---- 6. live channels mixed with finalized ones, live-prune mode 1, read-only, identical calls ------------------------------------------------
def test_live_channels_mixed_with_finalized_and_the_call_is_read_only(world):
    """channels 0 and 1 decode the 150-frame utterance, channel 2 the 40-frame one and is finalized; at frames 25 and 97 channels 0 and
    2 are queried under both live-prune modes; channel 1 is channel 0's twin that is never queried"""
    W = world["W"]
    dec = decoder(world, cfg(6.0))
    try:
        p, q, stride = world["ptrs"][2], world["ptrs"][0], N_TID // 2
        dec.init()
        dec.advance([p, p, q], [25, 25, 40], stride)
        dec.finalize(channels=[2])
        rs = np.random.RandomState(6)
        sizes = []
        for upto in (25, 97):
            if upto > 25:
                dec.advance([p, p], [upto, upto], stride, channels=[0, 1])
            for mode in (0, 1):
                dec.set_live_lattice_prune(mode)
                alt = [[r["hyp_words"].tolist() for r in row] for row in dec.rescaled_words([(1.0, 1.0, 0.0), (1.0, 0.1, -2.0)], [0, 2], use_final_probs=False)]
                lists = [sized_list(runs_of(alt[0][0] + alt[0][1], rs, 5), 20), sized_list(runs_of(world_words(dec), rs, 5), 30, seed=1)]
                for ufp in (False, True):
                    got, want, lat = check(world, dec, [0, 2], lists, [0, 1], SETTINGS[:3], ufp=ufp, what="frame %d mode %d ufp %d" % (upto, mode, ufp))
                    assert all(g["found"] for g in got[0])
                    if not ufp:   # a finalized channel asked without final-probs has no lattice: all zero, status OK
                        assert lat[1] is None and not any(g["found"] or g["n_hyp"] or g["n_hits"] for g in got[1])
                    sizes.append((upto, mode, int(ufp), lat[0].n_states))
                if mode == 1 and upto == 97:   # two identical calls return identical bytes
                    bl = W.BiasLists.from_phrases(lists)
                    a = raw_call(W, dec, [0, 2], bl, [0, 1], SETTINGS, 256, 128)
                    b = raw_call(W, dec, [0, 2], bl, [0, 1], SETTINGS, 256, 128)
                    bl.free()
                    assert a["rc"] == 0 and a["status"].tolist() == [0, 0] and a["n_hits"].sum() > 0
                    for key in a:
                        assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), key
            dec.set_live_lattice_prune(0)
        print("(frame, mode, ufp, states of the live lattice):", sizes)
        assert min(s[3] for s in sizes if s[1] == 1) < min(s[3] for s in sizes if s[1] == 0), "mode 1 serves a pruned lattice"
        # decoding continues bit for bit: the queried channel ends as its twin does
        dec.advance([p, p], [150, 150], stride, channels=[0, 1])
        dec.finalize(channels=[0, 1])
        a, b = dec.best_paths([0, 1])
        for key in ("ilabel", "olabel"):
            assert np.array_equal(a[key], b[key]), key
        for key in ("graph", "ac"):
            assert np.array_equal(bits(a[key]), bits(b[key])), key
        assert bits32(a["tot_score"]) == bits32(b["tot_score"]) and bits32(a["lm_score"]) == bits32(b["lm_score"])
    finally:
        dec.free()


def world_words(dec):
    """the words of finalized channel 2's best path"""
    return dec.rescaled_words([(1.0, 1.0, 0.0)], [2])[0][0]["hyp_words"].tolist()


# ---- 7. a biglm lattice decoder -------------------------------------------------------------------------------------------------------------
def test_biglm_lattice_decoder(tmp_path):
    """costs bit for bit; the answer in full where no decision of the restatement was ambiguous (two tokens of a frame may share a
    graph state here, so the order among the survivors of the tie rule is unspecified)"""
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
    mats = [z["ll_%d" % i] for i in range(int(z["n_utt"]))][:3]
    dec = W.BatchDecoder(graph, G.gpu_config(cd), len(mats), old_lm=lms[0], new_lm=lms[1], max_frames=64, max_tokens_per_frame=32768,
                         arena_tokens=1 << 20, lattice_links=1 << 21)
    try:
        dev = G.upload(mats)
        dec.init()
        dec.advance([t.data_ptr() for t in dev], [x.shape[0] for x in mats], int(mats[0].shape[1]))
        dec.finalize()
        have = [c for c in range(len(mats)) if dec.raw_lattice(c, True) is not None]
        assert have, "no utterance kept its lattice"
        rs = np.random.RandomState(8)
        alt = dec.rescaled_words([(1.0, 1.0, 0.0), (1.0, 0.1, -2.0)], have)
        lists = [sized_list(runs_of(row[0]["hyp_words"].tolist() + row[1]["hyp_words"].tolist(), rs, 6), 24, seed=i) for i, row in enumerate(alt)]
        got, want, lat = check(dict(W=W), dec, have, lists, list(range(len(have))), SETTINGS[:3], what="biglm", exact_path=False)
        n_exact = sum(not w["ambiguous"] for ws in want for w in ws)
        print("biglm: %d lattices; %d of %d answers equal in full, hits %s" % (len(have), n_exact, 3 * len(have), [[g["n_hits"] for g in row] for row in got]))
        assert n_exact >= len(have) and sum(g["n_hits"] for row in got for g in row) > 0
    finally:
        dec.free()
        for lm in lms:
            lm.free()
        graph.free()


# ---- 8. rows too short, a table over max_cells, a call split into rounds ---------------------------------------------------------------------
def test_capacities_of_one_channel(world, finalized):
    W, dec, lat = world["W"], finalized["dec"], finalized["lat"]
    rs = np.random.RandomState(9)
    ch = [1, 2, 0]
    lists = [sized_list(runs_of(finalized["alt"][c][0] + finalized["alt"][c][1], rs, 8, longest=2), 32, seed=c) for c in ch]
    settings = [(1.0, 1.0, -3.0, 2.0), (1.0, 1.0, 0.0, 1.0)]
    full, want, _ = check(world, dec, ch, lists, [0, 1, 2], settings, what="full", lattices=[lat[c] for c in ch])
    bl = W.BiasLists.from_phrases(lists)
    try:
        need = np.array([[g["n_hyp"] for g in row] for row in full])
        hits = np.array([[g["n_hits"] for g in row] for row in full])
        cap = int(need.max()) - 1
        short = need.max(axis=1) > cap
        assert cap >= 1 and short.any() and not short.all(), "the longest path is one word longer than the rows; another channel's fit"
        o = raw_call(W, dec, ch, bl, [0, 1, 2], settings, cap, 1024)
        assert o["rc"] == 0 and o["status"].tolist() == [E_CAPACITY if short[i] else 0 for i in range(3)]
        assert o["n_hyp"].tolist() == need.tolist() and o["n_hits"].tolist() == hits.tolist(), "the room needed"
        for i in range(3):
            for q in range(2):
                g, k = full[i][q], min(int(need[i, q]), cap)
                assert o["found"][i, q] == 1 and o["n_arcs"][i, q] == g["n_arcs"] and bits64(o["biased_cost"][i, q]) == bits64(g["biased_cost"])
                assert bits64(o["bonus"][i, q]) == bits64(g["bonus"]) and bits32(o["tot"][i, q]) == bits32(g["tot"]) and bits32(o["lm"][i, q]) == bits32(g["lm"])
                assert np.array_equal(o["hyp_words"][i, q, :k], g["hyp_words"][:k]) and np.array_equal(o["begin"][i, q, :k], g["begin"][:k])
                assert np.array_equal(o["end"][i, q, :k], g["end"][:k]) and not o["hyp_words"][i, q, k:].any()
                assert np.array_equal(o["hit_phrase"][i, q, :hits[i, q]], g["hit_phrase"]) and np.array_equal(o["hit_word"][i, q, :hits[i, q]], g["hit_word"])
        # the hits likewise
        hcap = int(hits.max()) - 1
        hshort = hits.max(axis=1) > hcap
        assert hcap >= 1 and hshort.any() and not hshort.all()
        o = raw_call(W, dec, ch, bl, [0, 1, 2], settings, 256, hcap)
        assert o["rc"] == 0 and o["status"].tolist() == [E_CAPACITY if hshort[i] else 0 for i in range(3)] and o["n_hits"].tolist() == hits.tolist()
        for i in range(3):
            for q in range(2):
                k = min(int(hits[i, q]), hcap)
                assert np.array_equal(o["hit_phrase"][i, q, :k], full[i][q]["hit_phrase"][:k]) and np.array_equal(o["hit_word"][i, q, :k], full[i][q]["hit_word"][:k])
                assert np.array_equal(o["hyp_words"][i, q, :need[i, q]], full[i][q]["hyp_words"])
        # with the hit rows NULL no count is held against cap_hits
        o = raw_call(W, dec, ch, bl, [0, 1, 2], settings, 256, 0, with_hits=False)
        assert o["rc"] == 0 and o["status"].tolist() == [0, 0, 0] and o["n_hits"].tolist() == hits.tolist()
        # the binding repeats the call once with the room needed
        again = dec.biased_words(bl, [0, 1, 2], settings, ch, cap_words=1, cap_hits=1)
        for i in range(3):
            for q in range(2):
                B.same_answer(again[i][q], want[i][q], "the binding's repeat")
                assert again[i][q]["status"] == 0
        # a table over max_cells: that channel's answers zero and its status alone, the others' stand; at its own size it fits
        states = [lat[c].n_states for c in ch]
        big = int(np.argmax(states))
        assert sorted(states)[-1] > sorted(states)[-2]
        tight = dec.biased_words(bl, [0, 1, 2], settings, ch, max_cells=32 * states[big] - 1)
        assert [row[0]["status"] for row in tight] == [E_CAPACITY if i == big else 0 for i in range(3)]
        for i in range(3):
            for q in range(2):
                if i == big:
                    assert not tight[i][q]["found"] and tight[i][q]["n_hyp"] == 0 and tight[i][q]["biased_cost"] == 0.0
                else:
                    B.same_answer(tight[i][q], want[i][q], "beside the channel over max_cells")
        assert [row[0]["status"] for row in dec.biased_words(bl, [0, 1, 2], settings, ch, max_cells=32 * states[big])] == [0, 0, 0]
        print("capacities: words needed %s, hits %s, states %s" % (need.tolist(), hits.tolist(), states))
    finally:
        bl.free()


def test_a_call_split_into_rounds(world):
    """two channels whose tables do not fit one round's 32 Mi cells together: 16 settings x 256 nodes x the states of a wide lattice
    each.  The 16 settings are one setting sixteen times, so that the restatement runs once per lattice"""
    dec = decoder(world, WIDE, 2)
    try:
        dec.init()
        dec.advance([world["ptrs"][0], world["ptrs"][1]], [30, 30], N_TID // 2)
        dec.finalize()
        lat = [from_gpu(dec.raw_lattice(c, True)) for c in (0, 1)]
        need = [16 * 256 * L.n_states for L in lat]
        assert sum(need) > (32 << 20) and max(L.n_states for L in lat) * 256 <= 65536 * 256, (need, "the two do not share a round; each table is within max_cells")
        rs = np.random.RandomState(10)
        alt = dec.rescaled_words([(1.0, 1.0, 0.0), (1.0, 0.1, -2.0)], [0, 1])
        lists = [sized_list(runs_of(row[0]["hyp_words"].tolist() + row[1]["hyp_words"].tolist(), rs, 8), 256, seed=i) for i, row in enumerate(alt)]
        setting = (1.0, 1.0, 0.0, 2.0)
        autos = [B.compile_list(p) for p in lists]
        want = [B.bias(L, A, setting) for L, A in zip(lat, autos)]
        bl = world["W"].BiasLists.from_phrases(lists)
        try:
            got = dec.biased_words(bl, [0, 1], [setting] * 16, [0, 1])
        finally:
            bl.free()
        for i in range(2):
            for q in range(16):
                assert got[i][q]["status"] == 0
                B.same_answer(got[i][q], want[i], "round of channel %d, setting %d" % (i, q))
        print("rounds: states %s, cells needed %s, hits %s" % ([L.n_states for L in lat], need, [got[i][0]["n_hits"] for i in range(2)]))
    finally:
        dec.free()


# ---- 9. the error surface -----------------------------------------------------------------------------------------------------------------
def test_error_surface(world):
    W = world["W"]
    bl = W.BiasLists.from_phrases([[((1, 2), 1.0)], []])
    try:
        info = bl.info()
        assert info["n_lists"] == 2 and info["n_nodes"].tolist() == [3, 1] and info["n_phrases"].tolist() == [1, 0] and info["total_nodes"] == 4
        assert info["n_words"].tolist() == [2, 0] and info["device_bytes"] > 0
        plain = decoder(world, cfg(4.0), 2, lattice_links=0)
        try:
            plain.init()
            plain.advance(world["ptrs"][:2], [10, 10], N_TID // 2)
            with pytest.raises(W.WfstError) as e:
                plain.biased_words(bl)
            assert e.value.code == E_STATE
        finally:
            plain.free()
        dec = decoder(world, cfg(4.0), 3)
        try:
            dec.init(channels=[0, 1])
            dec.advance(world["ptrs"][:2], [20, 20], N_TID // 2, channels=[0, 1])
            ok = dec.biased_words(bl, [0], channels=[0], use_final_probs=False)
            assert ok[0][0]["status"] == 0 and ok[0][0]["found"]
            for ch, code in (([0, 0], E_ARG), ([0, 3], E_ARG), ([0, 2], E_STATE)):
                with pytest.raises(W.WfstError) as e:
                    dec.biased_words(bl, [0, 0], channels=ch, use_final_probs=False)
                assert e.value.code == code, ch
            for lo in ([2], [-2]):
                with pytest.raises(W.WfstError) as e:
                    dec.biased_words(bl, lo, channels=[0], use_final_probs=False)
                assert e.value.code == E_ARG, lo
            with pytest.raises(W.WfstError) as e:
                dec.biased_words(None, [0], channels=[0], use_final_probs=False)
            assert e.value.code == E_ARG
            for bad in ([(-1.0, 1.0, 0.0, 1.0)], [(1.0, float("nan"), 0.0, 1.0)], [(1.0, 1.0, float("inf"), 1.0)], [(1.0, 1.0, 0.0, -1.0)],
                        [(1.0, 1.0, 0.0, float("inf"))], [(1.0, 1.0, 0.0, 1.0)] * 17, []):
                with pytest.raises(W.WfstError) as e:
                    dec.biased_words(bl, [0], bad, [0], use_final_probs=False)
                assert e.value.code == E_ARG, bad
            for kw in (dict(cap_words=0), dict(cap_hits=-1), dict(max_cells=-1)):
                with pytest.raises(W.WfstError) as e:
                    dec.biased_words(bl, [0], channels=[0], use_final_probs=False, **kw)
                assert e.value.code == E_ARG, kw
            # through the C ABI: NULL outputs are fine
            one, st = np.array([0], np.int32), np.array([1.0, 1.0, 0.0, 1.0])
            rc = W.lib().wfst_decoder_biased_words(dec.h, one.ctypes.data_as(C.POINTER(C.c_int32)), 1, 0, bl.h, one.ctypes.data_as(C.POINTER(C.c_int32)), 1,
                                                   st.ctypes.data_as(C.POINTER(C.c_double)), 16, 4, C.c_int64(0), *([None] * 14))
            assert rc == 0
        finally:
            dec.free()
    finally:
        bl.free()
