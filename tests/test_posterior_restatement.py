"""CPU: the definition of wfst_decoder_word_confidence as tests/posterior_util.py restates it -- on hand-made lattices whose answers
are worked out by hand (in the comments), on random small lattices against the enumeration of every path, and on the C oracle's raw
lattices.  The tolerance is posterior_util's, derived from each lattice; the sensitivity test keeps it from hiding a failure."""
import math

import numpy as np
import pytest

import pyoracle
from align_util import make_lattice
from nearest_util import all_paths
from posterior_util import (EPS, brute_force, confidence, confidence_many, cuts_of, posteriors, random_lattice, tol_word, without_arc)

E = math.e


def close(x, y, tol=1e-14):
    return abs(float(x) - float(y)) <= tol * max(1.0, abs(float(y)))


# states (frame, graph state, final); arcs (src, dst, ilabel, olabel, graph, acoustic)
def two_parallel():
    return make_lattice([(0, 1, 0), (1, 2, 1)], [(0, 1, 1, 5, 0.5, 0.5), (0, 1, 2, 6, 0.5, 0.5)])


def eps_word():
    return make_lattice([(0, 10, 0), (1, 11, 0), (1, 12, 0), (2, 13, 1)],
                        [(0, 1, 5, 0, 0.5, 1.0), (1, 2, 0, 7, 0.25, 0.0), (2, 3, 6, 0, 0.5, 2.0)])


def eps_chain():
    """frame 1 holds a chain 1 -> 2 -> 3 -> 4 of arcs inside the frame (depth 3) and the shortcut 1 -> 4"""
    return make_lattice([(0, 1, 0), (1, 2, 0), (1, 3, 0), (1, 4, 0), (1, 5, 0), (2, 6, 1)],
                        [(0, 1, 1, 0, 1.0, 0.0), (1, 2, 0, 7, 0.5, 0.0), (2, 3, 0, 0, 0.5, 0.0), (3, 4, 0, 8, 0.5, 0.0), (1, 4, 0, 9, 2.0, 0.0),
                         (4, 5, 2, 0, 1.0, 0.0)])


def final_with_out_arc():
    return make_lattice([(0, 1, 0), (1, 2, 1), (2, 3, 1)], [(0, 1, 1, 5, 1.0, 0.0), (1, 2, 2, 6, 0.5, 0.5)])


def dead_ends():
    """state 2 is a dead end, state 3 cannot be reached, and the second arc 0 -> 1 costs +inf"""
    return make_lattice([(0, 1, 0), (1, 2, 0), (1, 3, 0), (1, 4, 0), (2, 5, 1)],
                        [(0, 1, 1, 5, 0.5, 0.5), (0, 2, 2, 5, 0.5, 0.5), (1, 4, 3, 6, 0.5, 0.5), (0, 1, 4, 5, np.inf, 0.0), (3, 4, 5, 6, 0.5, 0.5)])


def twice_in_a_cell():
    """word 5 free on either step, a wordless arc at cost 1 beside it: the paths say 5 5, 5, 5 and nothing"""
    return make_lattice([(0, 1, 0), (1, 2, 0), (2, 3, 1)],
                        [(0, 1, 1, 5, 0.0, 0.0), (0, 1, 2, 0, 1.0, 0.0), (1, 2, 3, 5, 0.0, 0.0), (1, 2, 4, 0, 1.0, 0.0)])


def negative_costs():
    return make_lattice([(0, 1, 0), (1, 2, 1)], [(0, 1, 1, 5, -0.5, -0.5), (0, 1, 2, 6, -1.5, -0.5)])


FIXTURES = [two_parallel, eps_word, eps_chain, final_with_out_arc, dead_ends, twice_in_a_cell, negative_costs]


def test_two_parallel_arcs_of_equal_cost():
    L = two_parallel()
    P = posteriors(L)
    assert P["gamma"].tolist() == [0.5, 0.5] and close(P["log_z"], math.log(2.0) - 1.0)
    r = confidence(L, [5])
    assert r["found"] and r["word_post"].tolist() == [0.5] and r["conf"].tolist() == [0.5] and close(r["path_logpost"], math.log(0.5))


def test_a_word_on_an_epsilon_arc_inside_a_frame():
    L = eps_word()   # one path: everything has posterior 1
    r = confidence(L, [7])
    assert r["found"] and r["begin"].tolist() == [1] and close(r["word_post"][0], 1.0) and close(r["log_z"], -4.25)
    assert abs(r["path_logpost"]) < 1e-15
    half = confidence(L, [7], 0.5, 2.0)   # 0.5 * (0.5 + 0.25 + 0.5) + 2 * (1 + 0 + 2)
    assert close(half["log_z"], -6.625) and close(half["word_post"][0], 1.0)


def test_an_epsilon_chain_of_depth_3_inside_one_frame():
    L = eps_chain()
    P = posteriors(L)
    assert P["n_levels"] == 6   # frame 0, four depths in frame 1, frame 2
    # the chain costs 1 + 1.5 + 1, the shortcut 1 + 2 + 1
    z = E ** -3.5 + E ** -4.0
    assert close(P["log_z"], math.log(z)) and close(P["alpha"][4], 1.0 - math.log(E ** -1.5 + E ** -2.0))
    chain, short = E ** -3.5 / z, E ** -4.0 / z
    assert all(close(g, w) for g, w in zip(P["gamma"], [1.0, chain, chain, chain, short, 1.0]))
    a, b, c = confidence_many(L, [[7, 8], [9], [8]])
    # 7 and 8 both leave frame 1: the cut m[1] = (1 + 1 + 1) >> 1 = 1 falls on that frame, so the cell of 7 is frame 0 alone and holds
    # no arc with the word -- the definition's own answer for two words on one frame
    assert a["begin"].tolist() == [1, 1] and a["word_post"][0] == 0.0 and close(a["word_post"][1], chain) and close(a["path_logpost"], math.log(chain))
    assert close(b["word_post"][0], short) and close(b["path_logpost"], math.log(short))
    assert not c["found"]      # every path with 8 says 7 first


def test_a_final_state_with_an_out_arc():
    L = final_with_out_arc()    # the paths: 5 (cost 1) and 5 6 (cost 2)
    z = E ** -1.0 + E ** -2.0
    P = posteriors(L)
    assert close(P["log_z"], math.log(z)) and close(P["gamma"][0], 1.0) and close(P["gamma"][1], E ** -2.0 / z)
    a, b = confidence_many(L, [[5], [5, 6]])
    assert a["found"] and a["n_arcs"] == 1 and close(a["word_post"][0], 1.0) and close(a["path_logpost"], math.log(E ** -1.0 / z))
    assert b["found"] and close(b["word_post"][1], 1.0 / (E + 1.0)) and close(b["path_logpost"], math.log(E ** -2.0 / z))


def test_dead_ends_and_an_infinite_arc_have_posterior_zero():
    L = dead_ends()
    P = posteriors(L)
    assert not np.isnan(P["gamma"]).any() and not np.isnan(P["alpha"]).any() and not np.isnan(P["beta"]).any()
    assert P["gamma"].tolist() == [1.0, 0.0, 1.0, 0.0, 0.0] and close(P["log_z"], -2.0)
    assert np.isinf(P["beta"][2]) and np.isinf(P["alpha"][3])
    r = confidence(L, [5, 6])
    assert r["found"] and r["word_post"].tolist() == [1.0, 1.0]
    L.st_final[:] = 0       # no path at all: log_z = -inf, every posterior 0
    P = posteriors(L)
    assert P["log_z"] == -np.inf and not P["gamma"].any() and not confidence(L, [5, 6])["found"]


def test_a_word_said_twice_in_one_cell_is_clamped():
    L = twice_in_a_cell()
    r = confidence(L, [5])     # one word, one cell: both arcs with word 5 count, each at 1 / (1 + 1/e)
    assert r["found"] and close(r["word_post"][0], 2.0 / (1.0 + 1.0 / E)) and r["word_post"][0] > 1.0 and r["conf"].tolist() == [1.0]
    assert close(r["log_z"], 2.0 * math.log(1.0 + 1.0 / E))
    both = confidence(L, [5, 5])   # begin frames 0 and 1: the cut is at (0 + 1 + 1) >> 1 = 1
    assert both["begin"].tolist() == [0, 1] and all(close(x, 1.0 / (1.0 + 1.0 / E)) for x in both["word_post"])


def test_the_empty_sequence_and_a_sequence_not_in_the_lattice():
    L = twice_in_a_cell()
    empty, absent, skipped = confidence_many(L, [[], [6], None])
    z = (1.0 + 1.0 / E) ** 2
    assert empty["found"] and len(empty["word_post"]) == 0 and close(empty["path_logpost"], math.log(E ** -2.0 / z))
    assert not absent["found"] and len(absent["word_post"]) == 0 and absent["path_logpost"] == 0.0 and skipped is None


def test_negative_costs():
    L = negative_costs()     # costs -1 and -2
    P = posteriors(L)
    assert close(P["log_z"], math.log(E + E * E)) and close(P["gamma"][0], 1.0 / (1.0 + E)) and close(P["gamma"][1], E / (1.0 + E))


def test_acoustic_scale_zero():
    L = make_lattice([(0, 1, 0), (1, 2, 1)], [(0, 1, 1, 5, 0.5, 3.0), (0, 1, 2, 6, 0.5, -7.0)])
    P = posteriors(L, 1.0, 0.0)
    assert P["gamma"].tolist() == [0.5, 0.5] and close(P["log_z"], math.log(2.0) - 0.5)
    r = confidence(L, [6], 1.0, 0.0)
    assert bool(r["found"]) and np.float32(r["tot"]) == np.float32(-6.5)   # the alignment's own score stays unscaled


# ---- random small lattices against the enumeration of every path -------------------------------------------------------------------
def test_random_lattices_against_every_path():
    rs = np.random.RandomState(17)
    n = n_conf = n_over = n_low = 0
    worst_z = worst_w = worst_fb = 0.0
    while n < 300:
        L = random_lattice(rs, quantised=bool(n % 4))
        if L is None:
            continue
        paths = all_paths(L, 20000)
        if not paths:
            continue
        n += 1
        seqs = [[int(w) for w in rs.randint(1, 4, rs.randint(0, 4))] for _ in range(2)]
        seqs += [[int(L.a_ol[a]) for a in paths[rs.randint(len(paths))] if L.a_ol[a]] for _ in range(2)]
        fr = L.st_frame[L.a_src].astype(np.int64)
        for scale in (1.0, 0.1):
            P = posteriors(L, scale, scale)
            log_z, gamma = brute_force(L, paths, scale, scale)
            assert abs(P["log_z"] - log_z) <= 1e-12 * max(1.0, abs(log_z)), n
            worst_z = max(worst_z, abs(P["log_z"] - log_z))
            # the forward total (over the final states) against the backward one
            fin = P["alpha"][np.asarray(L.st_final) != 0]
            fin = fin[np.isfinite(fin)]
            fwd = fin.min() - math.log(np.exp(-(fin - fin.min())).sum())
            assert abs(fwd - P["beta"][0]) <= P["tol_log"], n
            worst_fb = max(worst_fb, abs(fwd - P["beta"][0]) / P["tol_log"])
            for w, r in zip(seqs, confidence_many(L, seqs, scale, scale, post=P)):
                if not r["found"]:
                    continue
                m = [0] + [(int(r["begin"][k - 1]) + int(r["begin"][k]) + 1) >> 1 for k in range(1, len(w))] + [1 << 40]
                for k, word in enumerate(w):
                    want = math.fsum(gamma[(L.a_ol == word) & (fr >= m[k]) & (fr < m[k + 1])])
                    assert abs(r["word_post"][k] - want) <= 1e-12 * max(1.0, abs(want)), (n, w, k)
                    worst_w = max(worst_w, abs(r["word_post"][k] - want))
                    n_conf += 1
                    n_over += want > 1.0
                    n_low += want < 0.5
                cost = math.fsum(float(P["c"][a]) for a in r["arcs"])
                assert abs(r["path_logpost"] - (-log_z - cost)) <= 1e-12 * max(1.0, abs(log_z + cost)) and r["path_logpost"] <= 1e-12
    print("lattices %d, confidences %d (%d above 1, %d below 0.5); worst |log_z| error %.3g, worst |word_post| error %.3g, "
          "worst forward/backward difference %.3g of the tolerance" % (n, n_conf, n_over, n_low, worst_z, worst_w, worst_fb))
    assert n_conf >= 1000 and n_over >= 20 and n_low >= 200


# ---- the tolerance does not hide a missing arc ---------------------------------------------------------------------------------
@pytest.mark.parametrize("make", FIXTURES, ids=[f.__name__ for f in FIXTURES])
def test_removing_an_arc_moves_log_z_far_beyond_the_tolerance(make):
    for scale in ((0.1,) if make is eps_chain else (1.0, 0.1)):
        L = make()
        P = posteriors(L, scale, scale)
        on_a_path = np.nonzero(P["gamma"] > 0)[0]
        assert len(on_a_path) >= 2
        for a in on_a_path:
            Q = posteriors(without_arc(L, int(a)), scale, scale)
            assert abs(Q["log_z"] - P["log_z"]) > 1000.0 * P["tol_log"], (make.__name__, scale, int(a))


# ---- the oracle's lattices ------------------------------------------------------------------------------------------------
GRAPHS = [(3000, 21), (600, 5)]
UTTS = [(40, 700), (97, 701), (150, 702)]


@pytest.fixture(scope="module")
def lattices(oracle, synth, tmp_path_factory):
    """(what, lattice, best path) of the twelve inputs test_align_restatement.py builds: two graphs, lattice_beam 4 and 8, three
    utterances (order-free mode)"""
    out = []
    tmp = tmp_path_factory.mktemp("posterior")
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
                    out.append(("graph %d T %d lattice_beam %g" % (seed, T, lb), L, oracle.decode(h, cfg, x, m), T))
            oracle.free_graph(h)
    finally:
        oracle.set_order_free(False)
    return out


def says_it_twice(L, arcs):
    """some path runs over two of `arcs`"""
    by_src = np.argsort(L.a_src, kind="stable")
    for a in arcs:
        reach = np.zeros(L.n_states, bool)
        reach[L.a_dst[a]] = True
        for x in by_src:     # (every arc goes to a higher state id: sources ascending is a topological order)
            if reach[L.a_src[x]]:
                reach[L.a_dst[x]] = True
        if reach[L.a_src[arcs]].any():
            return True
    return False


def test_oracle_lattices(lattices):
    """the best path's words on each of the twelve lattices, at the scales (1, 1) and (0.1, 0.1): every word_post lies in
    (0, 1 + tolerance] -- unless some path says the word twice inside the word's cell, the one way the definition has of passing 1.
    These graphs have 500 words and an utterance repeats some (graph 5, T 150: word 282 four times on the best path), so that case
    occurs: 1.3130 at (1, 1) on graph 5, T 150, lattice_beam 4, and 1.2343 at (0.1, 0.1) on graph 21, T 150, lattice_beam 4.  A
    value above 1 is accepted only where such a path is shown to exist.  The mass per frame and path_logpost <= 0 are held throughout."""
    n = n_twice = 0
    over = 0.0
    for what, L, bp, T in lattices:
        assert L.ok and bp.ok, what
        best = [int(w) for w in bp.words]
        for scale in (1.0, 0.1):
            P = posteriors(L, scale, scale)
            r = confidence_many(L, [best], scale, scale, post=P)[0]
            assert r["found"] and len(r["word_post"]) == len(best) >= 2, what
            m = cuts_of(r["begin"])
            fr = L.st_frame[L.a_src].astype(np.int64)
            for k, x in enumerate(r["word_post"]):
                assert 0.0 < x, (what, scale, r["word_post"])
                if x > 1.0 + tol_word(P, L, 1.0):
                    sel = np.nonzero((L.a_ol == best[k]) & (fr >= m[k]) & (fr < m[k + 1]) & (P["gamma"] > 0))[0]
                    assert says_it_twice(L, sel), (what, scale, k, r["word_post"])
                    n_twice += 1
            over = max(over, float(r["word_post"].max()))
            # every path crosses from frame f to f + 1 over exactly one emitting arc
            emitting = L.a_il != 0
            mass = np.bincount(L.st_frame[L.a_src][emitting], weights=P["gamma"][emitting], minlength=T)
            assert len(mass) == T and np.all(np.abs(mass - 1.0) <= 4.0 * P["tol_log"] + len(L.a_src) * EPS), (what, scale, np.abs(mass - 1.0).max())
            assert r["path_logpost"] <= P["tol_log"], what
        n += 1
    print("largest word_post over both scales: %.4f; %d values above 1, each with a path that says the word twice in its cell" % (over, n_twice))
    assert n == 12
