"""-m gpu: wfst_decoder_biased_words_sparse (bias_reach_kernel and bias_sparse_kernel behind align_index_kernel) -- phrase boosting
for books, bias lists of up to 65 536 nodes, from the cells a path can reach.

Everything is compared BIT FOR BIT: with the dense call (wfst_decoder_biased_words) where the list has at most 256 nodes, with the
dense restatement (tests/bias_util.py) where its numpy table is affordable, with the sparse restatement (tests/bias_sparse_util.py,
held to the dense one by tests/test_bias_sparse_restatement.py) everywhere; n_cells against the restatement's count of the reachable
(state, node) pairs."""
import json
import os
import time

import numpy as np
import pytest

import bias_sparse_util as S
import bias_util as B
from align_util import from_gpu
from golden_util import GOLDEN_DIR, bits
from rescale_util import _levels, bits32, bits64
from test_gpu_bias import (ABSENT, N_TID, SETTINGS, WIDE, cfg, decoder, finalized, hand_decoder, runs_of, sized_list, world,  # noqa: F401
                           world_words)

pytestmark = pytest.mark.gpu

E_ARG, E_CAPACITY, E_STATE = -1, -4, -5
KEYS = ("found", "n_arcs", "n_hyp", "hyp_words", "begin", "end", "biased_cost", "bonus", "tot", "lm", "n_hits", "hit_phrase", "hit_word", "status")


def sized_book(core, nodes, seed=0):
    """sized_list for any size: the phrases of `core`, one phrase of 16 absent words where there is room, one-word phrases of absent
    words for the rest -- exactly `nodes` nodes"""
    out = [(tuple(ws), float(b)) for ws, b in core]
    have = S.compile_book(out).J
    assert have <= nodes, (have, nodes)
    rs = np.random.RandomState(seed)
    if nodes - have >= 16:
        out.append((tuple(ABSENT + 500000 + k for k in range(16)), 0.5))
        have += 16
    out += [((ABSENT + k,), float(rs.randint(0, 9)) / 4.0) for k in range(nodes - have)]
    assert S.compile_book(out).J == nodes
    return out


def same_bytes(a, b, tag="", keys=KEYS):
    """two answers of the device, every output byte"""
    for key in keys:
        assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), (tag, key, a[key], b[key])


def check(W, dec, channels, phrase_lists, book_of, settings=SETTINGS, ufp=True, what="", lattices=None, dense_ref=True, dense_call=True,
          exact_path=True, **kw):
    """biased_words_sparse of the channels against the restatement on each channel's raw lattice now: the dense restatement
    (bias_util.bias_many over the fast automaton) where dense_ref, else the sparse one; against the dense CALL too where every list
    has at most 256 nodes.  Returns (got, want, lattices, reachable cells per channel)"""
    lat = lattices if lattices is not None else [from_gpu(dec.raw_lattice(int(c), ufp)) for c in channels]
    autos = [S.compile_book(p) for p in phrase_lists]
    none = S.compile_book([])
    pick = lambda l: autos[l] if l >= 0 else none
    want = [(B.bias_many if dense_ref else S.bias_many_sparse)(L, pick(l), settings) for L, l in zip(lat, book_of)]
    count = [S.n_cells(L, pick(l)) if L is not None else 0 for L, l in zip(lat, book_of)]
    books = W.BiasBooks.from_phrases(phrase_lists) if phrase_lists else None
    small = dense_call and all(a.J <= 256 for a in autos)
    lists = W.BiasLists.from_phrases(phrase_lists) if phrase_lists and small else None
    try:
        got = dec.biased_words_sparse(books, book_of, settings, channels, use_final_probs=ufp, **kw)
        dense = dec.biased_words(lists, book_of, settings, channels, use_final_probs=ufp) if small else None
        # (BatchDecoder.biased_words forwards a BiasBooks set here)
        fwd = dec.biased_words(books, book_of, settings, channels, use_final_probs=ufp) if books is not None else got
    finally:
        for x in (books, lists):
            if x is not None:
                x.free()
    assert len(got) == len(channels)
    for i, c in enumerate(channels):
        assert len(got[i]) == len(settings)
        for q, s in enumerate(settings):
            tag = "%s channel %d setting %s" % (what, c, s)
            g = got[i][q]
            assert g["status"] == 0, tag
            assert g["n_cells"] == count[i], (tag, g["n_cells"], count[i])
            same_bytes(g, fwd[i][q], tag + " (BatchDecoder.biased_words with books)", KEYS + ("n_cells",))
            if dense is not None:
                same_bytes(g, dense[i][q], tag + " (the dense call)")
            if not exact_path and want[i][q]["found"] and want[i][q]["ambiguous"]:
                assert g["found"] and bits64(g["biased_cost"]) == bits64(want[i][q]["biased_cost"]), tag
                continue
            B.same_answer(g, want[i][q], tag)
    return got, want, lat, count


def lists_of(finalized, nodes, size_to):
    rs = np.random.RandomState(nodes)
    lists = []
    for c in range(3):
        pool = [w for seq in finalized["alt"][c] for w in seq]
        core = runs_of(pool, rs, min(nodes - 1, 12 if nodes <= 256 else 60), longest=1 if nodes == 2 else 3) if nodes > 1 else []
        while core and S.compile_book(core).J > nodes:
            core.pop()
        lists.append(size_to(core, nodes, seed=c))
    return lists


# ---- 1. lists the dense call serves: the same bytes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("nodes", [1, 2, 64, 255, 256])
def test_lists_of_up_to_256_nodes_equal_the_dense_call_in_every_byte(world, finalized, nodes):
    lists = lists_of(finalized, nodes, sized_list)
    got, want, _, count = check(world["W"], finalized["dec"], [2, 0, 1], lists, [2, 0, 1], what="%d nodes" % nodes,
                                lattices=[finalized["lat"][c] for c in (2, 0, 1)])
    states = [finalized["lat"][c].n_states for c in (2, 0, 1)]
    print("%d nodes: states %s, reachable cells %s, hits %d, negative totals %d" % (nodes, states, count, sum(g["n_hits"] for row in got for g in row),
                                                                                  sum(g["biased_cost"] < 0 for row in got for g in row)))
    assert all(g["found"] for row in got for g in row)
    assert (sum(g["n_hits"] for row in got for g in row) > 0) == (nodes > 1)
    if nodes == 1:
        assert count == states
    if nodes >= 64:
        assert any(g["biased_cost"] < 0 for row in got for g in row), "a boost of 40 makes totals negative"


# ---- 2. books: 257, 1 024 and 4 096 nodes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nodes", [257, 1024, 4096])
def test_books_beyond_256_nodes(world, finalized, nodes):
    """phrases cut from the lattice's own alternative paths, padded with absent words.  257 and 1 024 nodes against the dense
    restatement, 4 096 against the sparse one.  At 1 024 nodes the honesty check: a dense table in disguise would have states x 1 024
    cells; the device's count, and the restatement's, must stay within an eighth of that"""
    lists = lists_of(finalized, nodes, sized_book)
    t0 = time.time()
    got, want, _, count = check(world["W"], finalized["dec"], [2, 0, 1], lists, [2, 0, 1], what="%d nodes" % nodes,
                                lattices=[finalized["lat"][c] for c in (2, 0, 1)], dense_ref=nodes <= 1024)
    states = [finalized["lat"][c].n_states for c in (2, 0, 1)]
    print("%d nodes: states %s, reachable cells %s (%.2f per state), hits %s, %.1f s" % (
        nodes, states, count, sum(count) / float(sum(states)), [[g["n_hits"] for g in row] for row in got], time.time() - t0))
    assert all(g["found"] for row in got for g in row) and sum(g["n_hits"] for row in got for g in row) > 0
    assert any(not np.array_equal(row[3]["hyp_words"], g["hyp_words"]) for row in got for g in row), "the bias moves an answer"
    if nodes == 1024:
        for i in range(3):
            assert count[i] <= states[i] * 1024 // 8 and got[i][0]["n_cells"] <= states[i] * 1024 // 8, (i, count[i], states[i])


# ---- 3. hand-made lattices ----------------------------------------------------------------------------------------------------------
def hand_check(synth, tmp_path, arcs, finals, T, n_tid, name, phrases, settings, seed=1, dense_ref=True, **kw):
    import gpu_util as G

    dec, graph = hand_decoder(synth, tmp_path, arcs, finals, T, n_tid, seed=seed, name=name)
    try:
        L = from_gpu(dec.raw_lattice(0, True))
        got, want, _, count = check(G.wfstdec, dec, [0], [phrases] if phrases else [], [0 if phrases else -1], settings, what=name, lattices=[L],
                                    dense_ref=dense_ref, **kw)
        return got[0], want[0], L, count[0]
    finally:
        dec.free()
        graph.free()


@pytest.mark.parametrize("K", [1, 2, 63, 64, 65])
def test_parallel_word_arcs_that_merge(synth, tmp_path, K):
    """K states one frame on, each behind another word that starts a phrase, merge into one state over arcs without a word: the
    merged state holds K nodes -- K + 1 with an unlisted word beside them -- and the word 900 behind it completes every phrase"""
    phrases = [((1 + i, 900), 0.25 * (1 + i % 5)) for i in range(K)]
    settings = [(1.0, 1.0, 0.0, 1.0), (1.0, 1.0, 0.0, 0.0), (1.0, 0.3, 0.5, 6.0)]
    for extra in (0, 1):
        n_mid = K + extra
        arcs = {0: [(1 + i, 1 + i if i < K else 5000, 0.25 * (i % 7), 1 + i) for i in range(n_mid)]}
        for i in range(n_mid):
            arcs[1 + i] = [(n_mid + 1 + i, 0, 0.125 * (i % 3), n_mid + 1)]
        arcs[n_mid + 1] = [(2 * n_mid + 1, 900, 0.5, n_mid + 2)]
        got, want, L, count = hand_check(synth, tmp_path, arcs, {n_mid + 2: 0.0}, 3, 2 * n_mid + 1, "merge%d_%d" % (K, extra), phrases, settings)
        R = S.reach(L, S.compile_book(phrases))
        assert max(len(r) for r in R) == K + extra and np.bincount(L.st_frame)[1] == n_mid, "every middle state is in the lattice"
        assert got[0]["hyp_words"].tolist()[-1] == 900


def test_frames_of_255_256_and_257_cells(synth, tmp_path):
    """test_gpu_bias.py's fan: K states one frame on -- with one cell each the frame has one cell below, at and above the workgroup's
    lanes; with two and three cells each, frames of 2 x 128 and 3 x 85 + 2 cells"""
    seen = []
    for K, per in ((255, 1), (256, 1), (257, 1), (128, 2), (86, 3)):
        # `per` ways into every middle state, each behind another listed word: per nodes in it
        arcs = {0: [(1 + i, 1 + i, 0.25 * (i % 7), 1 + i) for i in range(K)]}
        if per > 1:   # a frame before: `per` states behind the words 1..per, then arcs without a word into every middle state
            arcs = {0: [(1 + p, 1 + p, 0.25 * p, 1 + p) for p in range(per)]}
            for p in range(per):
                arcs[1 + p] = [(per + 1 + (i * per + p), 0, 0.125 * ((i + p) % 3), per + 1 + i) for i in range(K)]
        base = per + 1 if per > 1 else 1
        n_tid = per + K * per if per > 1 else 2 * K
        for i in range(K):
            arcs[base + i] = [(n_tid - (i % 3), 1 + (3 * i) % 5, 0.125 * (i % 3), base + K)]
        phrases = [((1 + p, 7 + p), 1.5) for p in range(max(per, 1))]
        T = 3 if per > 1 else 2
        got, want, L, count = hand_check(synth, tmp_path, arcs, {base + K: 0.0}, T, n_tid, "fan%d_%d" % (K, per), phrases, SETTINGS[:3])
        R = S.reach(L, S.compile_book(phrases))
        f = T - 1
        seen.append(sum(len(R[t]) for t in range(L.n_states) if L.st_frame[t] == f))
    assert seen == [255, 256, 257, 256, 258], seen


@pytest.mark.parametrize("N", [255, 256, 257])
def test_the_child_search_at_its_edges(synth, tmp_path, N):
    """a root with N children, a node with one child (3 -> 7) and a node with two (5 -> 8, 5 -> 9): the first, the last and an absent
    word among the root's children, and the words 7, 8 and 9, which are no child of the root"""
    phrases = [((w,), 0.25 * (1 + w % 4)) for w in range(1, N + 1)] + [((3, N + 7), 2.0), ((5, N + 8), 1.0), ((5, N + 9), 3.0)]
    words = [1, N, 3, N + 7, 5, N + 9, 5, N + 8, N + 1, N + 7, 2]
    T = len(words)
    arcs = {s: [(s + 1, words[s], 0.5, s + 1), (s + 1, 0, 0.25, s + 1)] for s in range(T)}
    settings = [(1.0, 1.0, 0.0, 1.0), (1.0, 1.0, 0.0, 0.0), (1.0, 1.0, 0.0, 100.0), (1.0, 1.0, 0.0, 0.4)]
    got, want, L, count = hand_check(synth, tmp_path, arcs, {T: 0.0}, T, T, "kids%d" % N, phrases, settings, dense_ref=False)
    assert S.compile_book(phrases).J == N + 4
    g = got[2]
    assert g["hyp_words"].tolist() == [1, N, 3, N + 7, 5, N + 9, 5, N + 8, 2], "every listed word is worth its arc; N + 1 and the lone N + 7 are not"
    assert sorted(g["hit_phrase"].tolist()) == sorted([0, N - 1, 2, N, 4, N + 2, 4, N + 1, 1])


def test_a_phrase_of_sixteen_equal_words_against_seventeen(synth, tmp_path):
    phrases = [((1,) * 16, 4.0)]
    arcs = {s: [(s + 1, 1, 0.5, s + 1), (s + 1, 0, 0.25, s + 1)] for s in range(17)}
    got, want, L, _ = hand_check(synth, tmp_path, arcs, {17: 0.0}, 17, 17, "aaaa", phrases, [(1.0, 1.0, 0.0, 1.0), (1.0, 1.0, 0.0, 0.9), (1.0, 1.0, 0.0, 0.0)])
    # 16 words cost 4.0 more than none and earn 4.0 x bs once, 17 cost 4.25 more and earn it twice
    assert got[0]["hyp_words"].tolist() == [1] * 17 and got[0]["n_hits"] == 2 and got[0]["hit_word"].tolist() == [15, 16] and got[0]["bonus"] == 8.0
    assert got[2]["hyp_words"].tolist() == [] and got[2]["n_hits"] == 0
    assert max(len(r) for r in S.reach(L, S.compile_book(phrases))) == 17


def test_failure_links_three_deep_a_fall_to_the_root_and_a_word_only_deep_in_the_trie(synth, tmp_path):
    """after 1 2 3 4 the automaton is in the node of (1 2 3 4), whose failure links lead to (2 3 4), (3 4) and (4); only (4) has a child
    over 8.  Word 5 is in a phrase, but only at depth 5: after 3 4 it finds no child along (3 4), (4) and the root"""
    phrases = [((1, 2, 3, 4, 5), 1.0), ((2, 3, 4, 6), 0.5), ((3, 4, 7), 0.25), ((4, 8), 8.0)]
    A = S.compile_book(phrases)
    at = A.strs.index((1, 2, 3, 4))
    chain = [at, int(A.fail[at]), int(A.fail[A.fail[at]]), int(A.fail[A.fail[A.fail[at]]])]
    assert [A.strs[x] for x in chain] == [(1, 2, 3, 4), (2, 3, 4), (3, 4), (4,)] and all(A.goto(x, 8) < 0 for x in chain[:3]) and A.goto(chain[3], 8) > 0
    assert A.delta(A.strs.index((3, 4)), 5) == 0 and A.goto(0, 5) < 0 and 5 in A.word_set
    words = [1, 2, 3, 4, 8, 3, 4, 5, 5]
    T = len(words)
    arcs = {s: [(s + 1, words[s], 0.5, s + 1), (s + 1, 0, 0.25, s + 1)] for s in range(T)}
    settings = [(1.0, 1.0, 0.0, 1.0), (1.0, 1.0, 0.0, 0.0), (1.0, 1.0, -1.0, 1.0)]
    got, want, L, _ = hand_check(synth, tmp_path, arcs, {T: 0.0}, T, T, "fail3", phrases, settings)
    assert want[2]["words"].tolist() == words, "with a word penalty of -1 every word is taken"
    assert want[2]["nodes"][4] == A.strs.index((4, 8)) and want[2]["nodes"][7] == 0 and want[2]["nodes"][8] == 0
    assert got[2]["hit_phrase"].tolist() == [3] and got[2]["hit_word"].tolist() == [4]
    assert got[0]["hyp_words"].tolist() == [4, 8], "the bonus of 8 pays for 4 8 alone"


def test_a_chain_of_words_inside_a_frame_settles_in_later_rounds(synth, tmp_path):
    """after the first frame two ways lead on inside the frame: one arc without a word, and a chain of three arcs with the words 7, 8
    and 9; the sets and the costs along the chain settle one arc per pass over the frame"""
    arcs = {0: [(1, 0, 0.5, 1)], 1: [(0, 0, 0.25, 4), (0, 7, 0.5, 2)], 2: [(0, 8, 0.5, 3)], 3: [(0, 9, 0.5, 4)], 4: [(2, 0, 0.5, 5)]}
    phrases = [((7, 8, 9), 2.0), ((8,), 0.125)]
    settings = [(1.0, 1.0, 0.0, 1.0), (1.0, 1.0, 0.0, 0.25), (1.0, 1.0, 0.0, 0.0)]
    import gpu_util as G

    dec, graph = hand_decoder(synth, tmp_path, arcs, {5: 0.0}, 2, 2, seed=1, name="chain3")
    try:
        L = from_gpu(dec.raw_lattice(0, True))
        _, depth = _levels(L)
        assert int(depth.max()) >= 3 and np.any((L.a_il == 0) & (L.a_ol == 9))
        got, want, _, count = check(G.wfstdec, dec, [0], [phrases], [0], settings, what="chain3", lattices=[L])
        R = S.reach(L, S.compile_book(phrases))
        assert max(len(r) for r in R) == 2 and count[0] > L.n_states
        assert got[0][0]["hyp_words"].tolist() == [7, 8, 9] and got[0][0]["n_hits"] == 2 and got[0][1]["hyp_words"].tolist() == []
    finally:
        dec.free()
        graph.free()


# ---- 4. capacities ------------------------------------------------------------------------------------------------------------------
def test_max_cells_and_round_cells(world, finalized):
    W, dec, lat = world["W"], finalized["dec"], finalized["lat"]
    ch = [1, 2, 0]
    lists = [sized_book(runs_of(finalized["alt"][c][0] + finalized["alt"][c][1], np.random.RandomState(c), 30, longest=3), 300, seed=c) for c in ch]
    settings = SETTINGS[:3]
    full, want, _, count = check(W, dec, ch, lists, [0, 1, 2], settings, what="full", lattices=[lat[c] for c in ch])
    books = W.BiasBooks.from_phrases(lists)
    try:
        info = books.info()
        assert info["n_books"] == 3 and info["n_nodes"].tolist() == [300] * 3 and info["total_nodes"] == 900 and info["device_bytes"] > 0
        big = int(np.argmax(count))
        assert sorted(count)[-1] > sorted(count)[-2]
        # one below the largest channel's cells: that channel alone is refused; at its cells it is answered
        tight = dec.biased_words_sparse(books, [0, 1, 2], settings, ch, max_cells=count[big] - 1)
        assert [row[0]["status"] for row in tight] == [E_CAPACITY if i == big else 0 for i in range(3)]
        for i in range(3):
            for q in range(len(settings)):
                if i == big:
                    g = tight[i][q]
                    assert not g["found"] and g["n_hyp"] == 0 and g["n_arcs"] == 0 and g["biased_cost"] == 0.0 and g["n_hits"] == 0 and g["n_cells"] == -1
                else:
                    same_bytes(tight[i][q], full[i][q], "beside the channel over max_cells", KEYS + ("n_cells",))
        exact = dec.biased_words_sparse(books, [0, 1, 2], settings, ch, max_cells=count[big])
        for i in range(3):
            for q in range(len(settings)):
                same_bytes(exact[i][q], full[i][q], "max_cells = the channel's cells", KEYS + ("n_cells",))
        # rounds of the sweep: two (the third channel alone) and three (every channel alone); the bytes are the one-round call's
        need = [len(settings) * c for c in count]
        for budget, rounds in ((need[0] + need[1], 2), (1, 3)):
            split = dec.biased_words_sparse(books, [0, 1, 2], settings, ch, round_cells=budget)
            for i in range(3):
                for q in range(len(settings)):
                    same_bytes(split[i][q], full[i][q], "%d rounds" % rounds, KEYS + ("n_cells",))
        # rows too short: the counts are the room needed, the binding repeats the call once with it
        again = dec.biased_words_sparse(books, [0, 1, 2], settings, ch, cap_words=1, cap_hits=1)
        for i in range(3):
            for q in range(len(settings)):
                same_bytes(again[i][q], full[i][q], "the binding's repeat", KEYS + ("n_cells",))
        print("capacities: states %s, reachable cells %s" % ([lat[c].n_states for c in ch], count))
    finally:
        books.free()


def test_a_lattice_beyond_the_first_region_is_answered_after_growth(synth, tmp_path):
    """64 nodes merge into one state and stay alive along a chain of 40 arcs without a word: far more than max(1024, 4 x states) cells"""
    K, T = 64, 40
    phrases = [((1 + i, 900), 0.25 * (1 + i % 5)) for i in range(K)]
    arcs = {0: [(1 + i, 1 + i, 0.25 * (i % 7), 1 + i) for i in range(K)]}
    for i in range(K):
        arcs[1 + i] = [(K + 1, 0, 0.125 * (i % 3), K + 1)]
    for s in range(T):
        arcs[K + 1 + s] = [(K + 2, 0, 0.5, K + 2 + s)]
    arcs[K + 1 + T] = [(K + 3, 900, 0.5, K + 2 + T)]
    got, want, L, count = hand_check(synth, tmp_path, arcs, {K + 2 + T: 0.0}, T + 3, K + 3, "grow", phrases, [(1.0, 1.0, 0.0, 1.0), (1.0, 1.0, 0.0, 0.0)])
    print("growth: %d states, %d reachable cells" % (L.n_states, count))
    assert count > max(1024, 4 * L.n_states) and got[0]["n_cells"] == count and got[0]["n_hits"] == 1


# ---- 5. live channels, biglm, no book, identical calls, decoding goes on ------------------------------------------------------------
def test_live_channels_mixed_with_finalized_and_the_call_is_read_only(world):
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
                lists = [sized_book(runs_of(alt[0][0] + alt[0][1], rs, 5), 300), sized_book(runs_of(world_words(dec), rs, 5), 30, seed=1)]
                for ufp in (False, True):
                    got, want, lat, count = check(W, dec, [0, 2], lists, [0, 1], SETTINGS[:3], ufp=ufp, what="frame %d mode %d ufp %d" % (upto, mode, ufp))
                    assert all(g["found"] for g in got[0])
                    if not ufp:   # a finalized channel asked without final-probs has no lattice: all zero, status OK
                        assert lat[1] is None and not any(g["found"] or g["n_hyp"] or g["n_hits"] or g["n_cells"] for g in got[1])
                    sizes.append((upto, mode, int(ufp), lat[0].n_states, count[0]))
                if mode == 1 and upto == 97:   # two identical calls return identical bytes
                    bk = W.BiasBooks.from_phrases(lists)
                    a = dec.biased_words_sparse(bk, [0, 1], SETTINGS, [0, 2])
                    b = dec.biased_words_sparse(bk, [0, 1], SETTINGS, [0, 2])
                    bk.free()
                    assert sum(g["n_hits"] for row in a for g in row) > 0
                    for ra, rb in zip(a, b):
                        for ga, gb in zip(ra, rb):
                            same_bytes(ga, gb, "identical calls", KEYS + ("n_cells",))
            dec.set_live_lattice_prune(0)
        print("(frame, mode, ufp, states of the live lattice, reachable cells):", sizes)
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
        lists = [sized_book(runs_of(row[0]["hyp_words"].tolist() + row[1]["hyp_words"].tolist(), rs, 6), 280, seed=i) for i, row in enumerate(alt)]
        got, want, lat, count = check(W, dec, have, lists, list(range(len(have))), SETTINGS[:3], what="biglm", exact_path=False, dense_ref=False)
        n_exact = sum(not w["ambiguous"] for ws in want for w in ws)
        print("biglm: %d lattices, reachable cells %s; %d of %d answers equal in full" % (len(have), count, n_exact, 3 * len(have)))
        assert n_exact >= len(have) and sum(g["n_hits"] for row in got for g in row) > 0
    finally:
        dec.free()
        for lm in lms:
            lm.free()
        graph.free()


def test_no_book_and_no_boost_are_the_rescaled_words(world, finalized):
    W, dec, lat = world["W"], finalized["dec"], finalized["lat"]
    rs = np.random.RandomState(4)
    lists = [sized_book(runs_of(finalized["alt"][c][0], rs, 6), 270, seed=c) for c in range(3)]
    triples = [(1.0, 1.0, 0.0), (1.0, 0.1, 0.5), (0.7, 1.3, -0.3)]
    plain = dec.rescaled_words(triples, [0, 1, 2])
    no_book, want_a, _, count = check(W, dec, [0, 1, 2], lists, [-1, -1, -1], [t + (2.0,) for t in triples], what="no book", lattices=lat, dense_ref=False)
    assert count == [L.n_states for L in lat], "without a book every state is reached at the root alone"
    no_boost, want_b, _, _ = check(W, dec, [0, 1, 2], lists, [0, 1, 2], [t + (0.0,) for t in triples], what="no boost", lattices=lat, dense_ref=False)
    none_at_all, _, _, _ = check(W, dec, [0, 1, 2], [], [-1, -1, -1], [t + (2.0,) for t in triples], what="no set", lattices=lat, dense_ref=False)
    full = 0
    for i in range(3):
        for q in range(3):
            for got, want in ((no_book[i][q], want_a[i][q]), (no_boost[i][q], want_b[i][q]), (none_at_all[i][q], want_a[i][q])):
                p = plain[i][q]
                assert got["found"] and bits64(got["biased_cost"]) == bits64(p["scaled_cost"]) and bits64(got["bonus"]) == bits64(0.0)
                if not want["tie"]:
                    full += 1
                    assert np.array_equal(got["hyp_words"], p["hyp_words"]) and got["n_arcs"] == p["n_arcs"]
                    assert np.array_equal(got["begin"], p["begin"]) and np.array_equal(got["end"], p["end"])
                    assert bits32(got["tot"]) == bits32(p["tot"]) and bits32(got["lm"]) == bits32(p["lm"])
            assert no_book[i][q]["n_hits"] == 0
    assert full >= 9, "a third of the 27 answers at least are compared in full"


# ---- 6. the error surface that needs a decoder --------------------------------------------------------------------------------------
def test_error_surface(world):
    W = world["W"]
    bk = W.BiasBooks.from_phrases([[((1, 2), 1.0)], []])
    try:
        plain = decoder(world, cfg(4.0), 2, lattice_links=0)
        try:
            plain.init()
            plain.advance(world["ptrs"][:2], [10, 10], N_TID // 2)
            with pytest.raises(W.WfstError) as e:
                plain.biased_words_sparse(bk)
            assert e.value.code == E_STATE
        finally:
            plain.free()
        dec = decoder(world, cfg(4.0), 3)
        try:
            dec.init(channels=[0, 1])
            dec.advance(world["ptrs"][:2], [20, 20], N_TID // 2, channels=[0, 1])
            ok = dec.biased_words_sparse(bk, [0], channels=[0], use_final_probs=False)
            assert ok[0][0]["status"] == 0 and ok[0][0]["found"] and ok[0][0]["n_cells"] > 0
            for ch, code in (([0, 0], E_ARG), ([0, 3], E_ARG), ([0, 2], E_STATE)):
                with pytest.raises(W.WfstError) as e:
                    dec.biased_words_sparse(bk, [0, 0], channels=ch, use_final_probs=False)
                assert e.value.code == code, ch
            for lo in ([2], [-2]):
                with pytest.raises(W.WfstError) as e:
                    dec.biased_words_sparse(bk, lo, channels=[0], use_final_probs=False)
                assert e.value.code == E_ARG, lo
            with pytest.raises(W.WfstError) as e:
                dec.biased_words_sparse(None, [0], channels=[0], use_final_probs=False)
            assert e.value.code == E_ARG
            for bad in ([(-1.0, 1.0, 0.0, 1.0)], [(1.0, float("nan"), 0.0, 1.0)], [(1.0, 1.0, float("inf"), 1.0)], [(1.0, 1.0, 0.0, -1.0)],
                        [(1.0, 1.0, 0.0, 1.0)] * 17, []):
                with pytest.raises(W.WfstError) as e:
                    dec.biased_words_sparse(bk, [0], bad, [0], use_final_probs=False)
                assert e.value.code == E_ARG, bad
            for kw in (dict(cap_words=0), dict(cap_hits=-1), dict(max_cells=-1), dict(round_cells=-1), dict(max_cells=(1 << 30) + 1)):
                with pytest.raises(W.WfstError) as e:
                    dec.biased_words_sparse(bk, [0], channels=[0], use_final_probs=False, **kw)
                assert e.value.code == E_ARG, kw
        finally:
            dec.free()
    finally:
        bk.free()
