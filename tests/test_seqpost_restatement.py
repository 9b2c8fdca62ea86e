"""CPU: the definition of wfst_decoder_sequence_posterior as tests/seqpost_util.py restates it -- on hand-made lattices whose answers
are worked out by hand (in the comments) and on random small lattices against the enumeration of every path.  The bar against the
enumeration is 1e-12, test_posterior_restatement.py's; the sensitivity test keeps the derived tolerance from hiding a failure."""
import math

import numpy as np
import pytest

from align_util import make_lattice
from nearest_util import all_paths
from posterior_util import confidence_many, posteriors, random_lattice, without_arc
from seqpost_util import brute_force, phrase, phrase_many, sentence, sentence_many, tol_count

E = math.e


def close(x, y, tol=1e-14):
    return abs(float(x) - float(y)) <= tol * max(1.0, abs(float(y)))


def sent(L, w, gs=1.0, as_=1.0):
    return sentence(L, w, posteriors(L, gs, as_))


def phr(L, w, gs=1.0, as_=1.0):
    return phrase(L, w, posteriors(L, gs, as_))


# states (frame, graph state, final); arcs (src, dst, ilabel, olabel, graph, acoustic)
def two_spellings():
    """two arcs say 5 (costs 1 and 2), one says 6 (cost 1)"""
    return make_lattice([(0, 1, 0), (1, 2, 1)], [(0, 1, 1, 5, 0.5, 0.5), (0, 1, 2, 5, 1.0, 1.0), (0, 1, 3, 6, 0.5, 0.5)])


def eps_word():
    return make_lattice([(0, 10, 0), (1, 11, 0), (1, 12, 0), (2, 13, 1)],
                        [(0, 1, 5, 0, 0.5, 1.0), (1, 2, 0, 7, 0.25, 0.0), (2, 3, 6, 0, 0.5, 2.0)])


def eps_chain():
    """frame 1 holds a chain 1 -> 2 -> 3 -> 4 of arcs inside the frame (depth 3, saying 7 8) and the shortcut 1 -> 4 (saying 9)"""
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


def says_a_a_a():
    return make_lattice([(0, 1, 0), (1, 2, 0), (2, 3, 0), (3, 4, 1)], [(0, 1, 1, 5, 1.0, 0.0), (1, 2, 2, 5, 0.5, 0.0), (2, 3, 3, 5, 0.25, 0.0)])


def says_5_6_7():
    return make_lattice([(0, 1, 0), (1, 2, 0), (2, 3, 0), (3, 4, 1)], [(0, 1, 1, 5, 1.0, 0.0), (1, 2, 2, 6, 0.5, 0.0), (2, 3, 3, 7, 0.25, 0.0)])


def negative_costs():
    return make_lattice([(0, 1, 0), (1, 2, 1)], [(0, 1, 1, 5, -0.5, -0.5), (0, 1, 2, 6, -1.5, -0.5)])


def test_two_paths_that_spell_the_same_word_are_added():
    L = two_spellings()
    z = 2 * E ** -1.0 + E ** -2.0
    r = sent(L, [5])
    assert r["found"] and close(r["logpost"], math.log((E ** -1.0 + E ** -2.0) / z))
    one = confidence_many(L, [[5]])[0]["path_logpost"]      # the cheaper of the two paths alone
    assert close(one, math.log(E ** -1.0 / z)) and r["logpost"] > one + 0.1
    assert close(sent(L, [6])["logpost"], math.log(E ** -1.0 / z))
    p = phr(L, [5])
    assert p["found"] and close(p["count"], (E ** -1.0 + E ** -2.0) / z) and close(p["hit_mass"][0], p["count"]) and p["hit_mass"][1] == 0.0


def test_a_word_on_an_epsilon_arc_inside_a_frame():
    L = eps_word()      # one path, which says 7 over an arc inside frame 1
    r = sent(L, [7])
    assert r["found"] and abs(r["logpost"]) < 1e-15 and not sent(L, [])["found"]
    p = phr(L, [7], 0.5, 2.0)
    assert p["found"] and close(p["count"], 1.0) and len(p["hit_mass"]) == 3 and close(p["hit_mass"][1], 1.0) and p["hit_mass"][0] == p["hit_mass"][2] == 0.0


def test_an_epsilon_chain_of_depth_3_with_a_shortcut():
    L = eps_chain()     # the chain costs 1 + 1.5 + 1 and says 7 8 inside frame 1, the shortcut 1 + 2 + 1 and says 9
    z = E ** -3.5 + E ** -4.0
    chain, short = E ** -3.5 / z, E ** -4.0 / z
    a, b, c, d = sentence_many(L, [[7, 8], [9], [8], [7]])
    assert close(a["logpost"], math.log(chain)) and close(b["logpost"], math.log(short)) and not c["found"] and not d["found"]
    p, q, r = phrase_many(L, [[8], [7, 8], [9, 8]])
    assert close(p["count"], chain) and close(q["count"], chain) and close(q["hit_mass"][1], chain) and not r["found"]


def test_a_final_state_with_an_out_arc():
    L = final_with_out_arc()    # the paths: 5 (cost 1) and 5 6 (cost 2)
    z = E ** -1.0 + E ** -2.0
    a, b = sentence_many(L, [[5], [5, 6]])
    assert close(a["logpost"], math.log(E ** -1.0 / z)) and close(b["logpost"], math.log(E ** -2.0 / z))
    assert close(phr(L, [5])["count"], 1.0) and close(phr(L, [6])["count"], E ** -2.0 / z)


def test_dead_ends_and_an_infinite_arc():
    L = dead_ends()     # one path is left: 0 -> 1 -> 4, saying 5 6
    a, b = sentence_many(L, [[5, 6], [5]])
    assert a["found"] and abs(a["logpost"]) < 1e-15 and not b["found"] and b["logpost"] == 0.0
    p = phr(L, [5])
    assert close(p["count"], 1.0) and not np.isnan(p["hit_mass"]).any()
    L.st_final[:] = 0   # no path at all
    assert not sent(L, [5, 6])["found"] and not phr(L, [5])["found"] and phr(L, [5])["count"] == 0.0


def test_the_empty_sequence_an_absent_one_and_overlapping_words():
    L = twice_in_a_cell()
    z = (1.0 + 1.0 / E) ** 2
    empty, once, twice, absent, skipped = sentence_many(L, [[], [5], [5, 5], [6], None])
    assert close(empty["logpost"], math.log(E ** -2.0 / z)) and close(once["logpost"], math.log(2.0 * E ** -1.0 / z))
    assert close(twice["logpost"], math.log(1.0 / z)) and not absent["found"] and absent["logpost"] == 0.0 and skipped is None
    assert close(math.exp(empty["logpost"]) + math.exp(once["logpost"]) + math.exp(twice["logpost"]), 1.0)
    p = phr(L, [5])     # the expected number of 5s: above 1, the word_post of test_posterior_restatement.py's fixture
    assert close(p["count"], 2.0 / (1.0 + 1.0 / E)) and p["count"] > 1.0 and p["conf"] == 1.0
    assert close(p["count"], confidence_many(L, [[5]])[0]["word_post"][0])


def test_a_phrase_twice_in_a_path_a_longer_one_and_one_cut_by_a_foreign_word():
    L = says_a_a_a()
    one, two, three, four = phrase_many(L, [[5], [5, 5], [5, 5, 5], [5, 5, 5, 5]])
    assert close(one["count"], 3.0) and close(two["count"], 2.0) and close(three["count"], 1.0) and not four["found"] and four["count"] == 0.0
    assert [round(x, 12) for x in two["hit_mass"]] == [0.0, 1.0, 1.0, 0.0]     # the begin frames of the second and the third 5
    assert two["conf"] == 1.0
    L = says_5_6_7()
    cut, run = phrase_many(L, [[5, 7], [6, 7]])
    assert not cut["found"] and close(run["count"], 1.0) and close(run["hit_mass"][2], 1.0)
    assert not sent(L, [5, 7])["found"] and sent(L, [5, 6, 7])["found"]


def test_acoustic_scale_zero_and_negative_costs():
    L = make_lattice([(0, 1, 0), (1, 2, 1)], [(0, 1, 1, 5, 0.5, 3.0), (0, 1, 2, 6, 0.5, -7.0)])
    assert close(sent(L, [5], 1.0, 0.0)["logpost"], math.log(0.5)) and close(phr(L, [6], 1.0, 0.0)["count"], 0.5)
    L = negative_costs()     # costs -1 and -2
    assert close(sent(L, [5])["logpost"], math.log(1.0 / (1.0 + E))) and close(phr(L, [6])["count"], E / (1.0 + E))


# ---- random small lattices against the enumeration of every path -------------------------------------------------------------------
def test_random_lattices_against_every_path():
    rs = np.random.RandomState(23)
    n = n_sent = n_phr = n_over = n_many = 0
    worst_s = worst_p = 0.0
    while n < 200:
        L = random_lattice(rs, quantised=bool(n % 4))
        if L is None:
            continue
        paths = all_paths(L, 20000)
        if not paths:
            continue
        n += 1
        said = sorted(set(int(x) for x in L.a_ol if x))
        phrases = [[a] for a in said] + [[a, b] for a in said for b in said] + [[a, b, c] for a in said for b in said for c in said]
        phrases += [[4], [said[0], 4] if said else [4, 4]]
        for scale in (1.0, 0.1):
            P = posteriors(L, scale, scale)
            sentences, spot = brute_force(L, paths, scale, scale)
            seqs = [list(k) for k in sentences]
            total = 0.0
            conf = confidence_many(L, seqs, scale, scale, post=P)
            for w, r, cf in zip(seqs, sentence_many(L, seqs, post=P), conf):
                want = sentences[tuple(w)]
                assert r["found"] and abs(math.exp(r["logpost"]) - want) <= 1e-12, (n, w)
                assert abs(r["logpost"] - math.log(want)) <= 1e-12 * max(1.0, abs(math.log(want))), (n, w)
                worst_s = max(worst_s, abs(math.exp(r["logpost"]) - want))
                total += math.exp(r["logpost"])
                # all paths that spell w weigh at least what the aligned one does, and at most everything
                assert cf["found"] and r["logpost"] >= cf["path_logpost"] - r["tol"] and r["logpost"] <= r["tol"], (n, w)
                n_many += r["logpost"] > cf["path_logpost"] + 1e-6
                n_sent += 1
            assert abs(total - 1.0) <= 1e-12, n
            assert not sentence(L, [4], P)["found"] and not sentence(L, seqs[0] + [4], P)["found"]
            for w, r in zip(phrases, phrase_many(L, phrases, post=P)):
                count, hit = spot(w)
                assert abs(r["count"] - count) <= 1e-12 * max(1.0, count), (n, w)
                assert len(r["hit_mass"]) == len(hit) and np.all(np.abs(r["hit_mass"] - hit) <= 1e-12 * np.maximum(1.0, hit)), (n, w)
                assert r["found"] == (count > 0.0)
                if len(w) == 1:
                    assert abs(r["count"] - P["gamma"][L.a_ol == w[0]].sum()) <= tol_count(r, L, count), (n, w)
                worst_p = max(worst_p, abs(r["count"] - count))
                n_phr += 1
                n_over += count > 1.0
    print("lattices %d, sentences %d (%d spelled by more than one path), phrases %d (%d counts above 1); worst |posterior| error %.3g, "
          "worst |count| error %.3g" % (n, n_sent, n_many, n_phr, n_over, worst_s, worst_p))
    assert n_sent >= 1000 and n_many >= 100 and n_phr >= 5000 and n_over >= 50


# ---- the tolerance does not hide a missing arc ---------------------------------------------------------------------------------
CASES = [(two_spellings, [5]), (eps_chain, [9]), (final_with_out_arc, [5, 6]), (twice_in_a_cell, [5]), (twice_in_a_cell, []),
         (negative_costs, [6])]


@pytest.mark.parametrize("make,w", CASES, ids=["%s-%s" % (f.__name__, "_".join(map(str, w))) for f, w in CASES])
def test_removing_an_arc_of_a_spelling_path_moves_the_posterior_far_beyond_the_tolerance(make, w):
    for scale in (1.0, 0.1):
        L = make()
        r = sentence(L, w, posteriors(L, scale, scale))
        assert r["found"]
        arcs = sorted(set(a for p in all_paths(L) if [int(L.a_ol[x]) for x in p if L.a_ol[x]] == w for a in p))
        assert len(arcs) >= 1
        for a in arcs:
            M = without_arc(L, int(a))
            q = sentence(M, w, posteriors(M, scale, scale))
            assert not q["found"] or abs(q["logpost"] - r["logpost"]) > 1000.0 * r["tol"], (make.__name__, scale, int(a))
