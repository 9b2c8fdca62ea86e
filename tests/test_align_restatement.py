"""CPU: the definition of wfst_decoder_align_words as tests/align_util.py restates it -- first on hand-made lattices whose answers
are worked out by hand (in the comments), then on the C oracle's raw lattices: aligning the best path's words gives the best
path's hop list, and aligning a word sequence gives the cheapest path that spells it, bit for bit."""
import numpy as np
import pytest

import pyoracle
from align_util import align, align_many, make_lattice

F32 = np.float32


def bits(x):
    return np.asarray(x, F32).view(np.int32).tolist()


# states (frame, graph state, final); arcs (src, dst, ilabel, olabel, graph, acoustic)
def test_a_word_on_an_epsilon_arc_inside_a_frame():
    L = make_lattice([(0, 10, 0), (1, 11, 0), (1, 12, 0), (2, 13, 1)],
                     [(0, 1, 5, 0, 0.5, 1.0), (1, 2, 0, 7, 0.25, 0.0), (2, 3, 6, 0, 0.5, 2.0)])
    r = align(L, [7])
    # the word's arc leaves state 1 (frame 1); it is the last word, so it ends with the end state's frame
    assert r["found"] and r["begin"].tolist() == [1] and r["end"].tolist() == [2] and r["n_arcs"] == 3 and not r["tie"]
    assert bits([r["tot"], r["lm"]]) == bits([4.25, 1.25])   # ((0 + 1.5) + 0.25) + 2.5; 0.5 + 0.25 + 0.5


def test_a_word_on_the_last_arc_into_a_final_state():
    L = make_lattice([(0, 1, 0), (1, 2, 0), (2, 3, 1)], [(0, 1, 3, 0, 1.0, 1.0), (1, 2, 4, 9, 0.5, 0.5)])
    r = align(L, [9])
    assert r["found"] and r["begin"].tolist() == [1] and r["end"].tolist() == [2] and r["arcs"].tolist() == [0, 1]
    assert bits([r["tot"], r["lm"]]) == bits([3.0, 1.5])


def _diamond(early, late, gstates=(2, 3)):
    """word 5 either on the first arc of the upper branch (cost `early` per arc) or on the second arc of the lower one (`late`)"""
    return make_lattice([(0, 1, 0), (1, gstates[0], 0), (1, gstates[1], 0), (2, 4, 1)],
                        [(0, 1, 1, 5, early, early), (0, 2, 2, 0, late, late), (1, 3, 3, 0, early, early), (2, 3, 4, 5, late, late)])


def test_two_paths_with_the_same_words_and_different_times():
    r = align(_diamond(1.0, 0.5), [5])   # upper: 2 + 2 = 4 with the word at frame 0; lower: 1 + 1 = 2 with the word at frame 1
    assert r["found"] and r["begin"].tolist() == [1] and r["end"].tolist() == [2] and bits([r["tot"], r["lm"]]) == bits([2.0, 1.0])
    assert r["arcs"].tolist() == [1, 3] and not r["tie"]
    r = align(_diamond(0.25, 0.5), [5])  # upper: 0.5 + 0.5 = 1
    assert r["begin"].tolist() == [0] and r["end"].tolist() == [2] and bits([r["tot"], r["lm"]]) == bits([1.0, 0.5])


@pytest.mark.parametrize("gstates,begin,arcs", [((2, 3), 0, [0, 2]), ((3, 2), 1, [1, 3])])
def test_two_equal_cost_paths_the_tie_rule_decides_the_times(gstates, begin, arcs):
    """both branches cost 1.0 + 1.0 (exact in float32): at the final state both in-arcs are emitting and arrive at 2.0, so the one
    whose source token has the lower graph state wins -- whatever the states' numbers are"""
    r = align(_diamond(0.5, 0.5, gstates), [5])
    assert r["found"] and r["tie"] and bits([r["tot"], r["lm"]]) == bits([2.0, 1.0])
    assert r["begin"].tolist() == [begin] and r["end"].tolist() == [2] and r["arcs"].tolist() == arcs


def test_a_tie_between_an_emitting_and_an_epsilon_arrival_goes_to_the_emitting_arc():
    # state 2 (frame 1) is reached at 1.0 by an emitting arc from the start and at 0.5 + 0.5 through state 1 and an epsilon arc
    L = make_lattice([(0, 1, 0), (1, 2, 0), (1, 3, 0), (2, 4, 1)],
                     [(0, 1, 7, 0, 0.25, 0.25), (0, 2, 8, 0, 0.5, 0.5), (1, 2, 0, 0, 0.5, 0.0), (2, 3, 9, 6, 1.0, 1.0)])
    r = align(L, [6])
    assert r["tie"] and r["arcs"].tolist() == [1, 3] and bits([r["tot"], r["lm"]]) == bits([3.0, 1.5])


def test_a_sequence_that_is_not_in_the_lattice_and_the_empty_sequence():
    L = _diamond(1.0, 0.5)
    assert [r["found"] for r in align_many(L, [[6], [5, 5], [], [5]])] == [False, False, False, True]   # every path carries word 5
    assert align_many(L, [None, [5]])[0] is None
    plain = make_lattice([(0, 1, 0), (1, 2, 1)], [(0, 1, 1, 0, 1.0, 2.0)])
    r = align(plain, [])
    assert r["found"] and r["n_arcs"] == 1 and len(r["begin"]) == 0 and bits([r["tot"], r["lm"]]) == bits([3.0, 1.0])
    assert not align(plain, [1])["found"]


def test_the_least_graph_state_among_equal_final_states_and_no_final_state():
    L = make_lattice([(0, 1, 0), (1, 9, 1), (1, 8, 1), (1, 7, 0)], [(0, 1, 1, 3, 0.5, 0.5), (0, 2, 2, 3, 0.5, 0.5), (0, 3, 3, 3, 0.25, 0.25)])
    r = align(L, [3])
    assert r["tie"] and r["arcs"].tolist() == [1]      # states 1 and 2 are final at 1.0: graph state 8 wins; state 3 is cheaper, not final
    L.st_final[:] = 0
    assert not align(L, [3])["found"]


def test_silence_trimmed_ends():
    L = make_lattice([(0, 1, 0), (1, 2, 0), (2, 3, 0), (3, 4, 0), (4, 5, 1)],
                     [(0, 1, 10, 5, 1, 1), (1, 2, 20, 0, 1, 1), (2, 3, 21, 6, 1, 1), (3, 4, 20, 0, 1, 1)])
    assert align(L, [5, 6])["end"].tolist() == [2, 4]
    r = align(L, [5, 6], sil_tids=[20])       # word 5: its own arc is its last non-silence one; word 6 likewise
    assert r["begin"].tolist() == [0, 2] and r["end"].tolist() == [1, 3]
    assert align(L, [5, 6], sil_tids=[20, 21])["end"].tolist() == [1, 2]   # word 6 has no non-silence arc: it ends where it begins


# ---- the oracle's lattices ------------------------------------------------------------------------------------------------
GRAPHS = [(3000, 21), (600, 5)]
UTTS = [(40, 700), (97, 701), (150, 702)]


@pytest.fixture(scope="module")
def lattices(oracle, synth, tmp_path_factory):
    """(what, lattice, best path) of the twelve inputs: two graphs, lattice_beam 4 and 8, three utterances (order-free mode: the
    lattices the device path is held to)"""
    out = []
    tmp = tmp_path_factory.mktemp("align")
    m = synth.default_tid2pdf(600)
    try:
        oracle.set_order_free(True)
        for n_states, seed in GRAPHS:
            g = synth.make_hclg_like(n_states, seed=seed, n_tid=600, n_words=500)
            path = str(tmp / ("g%d.bin" % seed))
            g.write(path)
            h = oracle.load_graph(path)
            for T, ls in UTTS:
                x = synth.make_loglikes(g, T, 300, m, seed=ls, mu=-2.2)[0]
                for lb in (4.0, 8.0):
                    cfg = pyoracle.Config(beam=12.0, max_active=1000000, min_active=0, lattice_beam=lb, prune_interval=10)
                    L = pyoracle.oracle_raw_lattice(oracle, h, cfg, x, m)
                    out.append(("graph %d T %d lattice_beam %g" % (seed, T, lb), L, oracle.decode(h, cfg, x, m)))
            oracle.free_graph(h)
    finally:
        oracle.set_order_free(False)
    return out


def _hops(il, ol, g, a):
    rows = [(int(i), int(o), int(x), int(y)) for i, o, x, y in zip(il, ol, np.asarray(g, F32).view(np.int32), np.asarray(a, F32).view(np.int32))]
    return rows[1:] if rows and rows[0] == (0, 0, 0, 0) else rows   # (GetBestPath's hop list starts with the root's (0, 0, One) arc)


def test_aligning_the_best_paths_words_gives_the_best_path(lattices):
    n = 0
    for what, L, bp in lattices:
        assert L.ok and bp.ok and np.all(L.a_dst > L.a_src), what
        r = align(L, bp.words)
        assert r["found"], what
        a = r["arcs"]
        assert _hops(L.a_il[a], L.a_ol[a], L.a_graph[a], L.a_ac[a]) == _hops(bp.path_ilabel, bp.path_olabel, bp.path_graph, bp.path_ac), what
        assert bits([r["tot"], r["lm"]]) == bits([bp.tot_score, bp.lm_score]), what
        n += 1
    assert n == 12


def test_aligning_a_word_sequence_gives_its_cheapest_path(lattices):
    n = 0
    for what, L, _ in lattices:
        paths = pyoracle.nshortest_paths(L, 40)
        cheapest = {}
        for p in paths:   # (in ascending cost: the first path of a word sequence is its cheapest listed one)
            cheapest.setdefault(tuple(int(w) for w in p["olabel"] if w), F32(p["tot"]))
        seqs = list(cheapest)
        for w, r in zip(seqs, align_many(L, seqs)):
            assert r["found"] and bits(r["tot"]) == bits(cheapest[w]), (what, w, r["tot"], cheapest[w])
            n += 1
    print("distinct word sequences aligned: %d" % n)
    assert n >= 12
