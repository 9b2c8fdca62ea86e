"""CPU: the definition of wfst_decoder_word_alternatives as tests/altern_util.py restates it -- on hand-made lattices whose answers
are worked out by hand (in the comments), on random small lattices against the enumeration of every path, on the identities that tie
it to the word confidences and the sentence posterior, and on the C oracle's raw lattices.  The sensitivity tests keep the tolerance
and the comparison rule from hiding a failure."""
import math

import numpy as np
import pytest

from align_util import make_lattice
from altern_util import TINY, alternatives, alternatives_many, assert_frames, brute_force, compare, compare_lists, none_posts, tol_none
from nearest_util import all_paths
from posterior_util import cuts_of, posteriors, random_lattice, tol_word, without_arc
from seqpost_util import sentence
from test_posterior_restatement import dead_ends, eps_word, final_with_out_arc, lattices, twice_in_a_cell, two_parallel  # noqa: F401

E = math.e


def close(x, y, tol=1e-14):
    return abs(float(x) - float(y)) <= tol * max(1.0, abs(float(y)))


# states (frame, graph state, final); arcs (src, dst, ilabel, olabel, graph, acoustic)
def chain_with_wordless_shortcut():
    """eps_chain with the shortcut 1 -> 4 wordless: the chain says 7 8 at cost 3.5, the shortcut nothing at cost 4"""
    return make_lattice([(0, 1, 0), (1, 2, 0), (1, 3, 0), (1, 4, 0), (1, 5, 0), (2, 6, 1)],
                        [(0, 1, 1, 0, 1.0, 0.0), (1, 2, 0, 7, 0.5, 0.0), (2, 3, 0, 0, 0.5, 0.0), (3, 4, 0, 8, 0.5, 0.0), (1, 4, 0, 0, 2.0, 0.0),
                         (4, 5, 2, 0, 1.0, 0.0)])


def ends_early():
    """the paths: 5 (cost 1, ends at frame 1) and 5 6 (cost 2, the 6 leaves frame 3)"""
    return make_lattice([(0, 1, 0), (1, 2, 1), (2, 3, 0), (3, 4, 0), (4, 5, 1)],
                        [(0, 1, 1, 5, 1.0, 0.0), (1, 2, 2, 0, 0.25, 0.0), (2, 3, 3, 0, 0.25, 0.0), (3, 4, 4, 6, 0.25, 0.25)])


def two_words_at_frame_0():
    """7 and 8 on arcs inside frame 0, then one emitting arc: begin frames 0 and 0, so cell 0 = [0, 0) is empty"""
    return make_lattice([(0, 1, 0), (0, 2, 0), (0, 3, 0), (1, 4, 1)],
                        [(0, 1, 0, 7, 0.5, 0.0), (1, 2, 0, 8, 0.5, 0.0), (2, 3, 1, 0, 0.5, 0.5)])


def test_two_parallel_arcs_with_different_words():
    r = alternatives(two_parallel(), [5])   # both arcs cost 1: 0.5 each, the exact tie goes to the lower word id
    assert r["found"] and r["alts"] == [[(5, 0.5), (6, 0.5)]] and r["n_distinct"].tolist() == [2] and r["none_post"].tolist() == [0.0]
    assert r["word_post"].tolist() == [0.5]
    r = alternatives(two_parallel(), [6])   # the list does not depend on which of the two is the hypothesis
    assert r["alts"] == [[(5, 0.5), (6, 0.5)]] and r["word_post"].tolist() == [0.5]


def test_a_word_on_an_epsilon_arc():
    r = alternatives(eps_word(), [7])   # one path: the word has mass 1 and nobody says nothing
    assert r["found"] and len(r["alts"]) == 1 and r["alts"][0][0][0] == 7 and close(r["alts"][0][0][1], 1.0)
    assert r["n_distinct"].tolist() == [1] and abs(r["none_post"][0]) < 1e-15


def test_an_epsilon_chain_with_a_wordless_shortcut():
    L = chain_with_wordless_shortcut()
    z = E ** -3.5 + E ** -4.0
    chain, short = E ** -3.5 / z, E ** -4.0 / z
    r = alternatives(L, [7, 8])
    # 7 and 8 both leave frame 1: the cut m[1] = 1, cell 0 is frame 0 alone -- nobody says a word there, on every path -- and cell 1
    # holds both words at the chain's posterior; the shortcut's paths say nothing in it
    assert r["begin"].tolist() == [1, 1] and r["n_distinct"].tolist() == [0, 2] and r["alts"][0] == []
    assert close(r["none_post"][0], 1.0) and close(r["none_post"][1], short)
    assert [w for w, _ in r["alts"][1]] == [7, 8] and all(close(x, chain) for _, x in r["alts"][1])
    assert r["word_post"][0] == 0.0 and close(r["word_post"][1], chain)


def test_a_final_state_with_an_out_arc():
    L = final_with_out_arc()    # the paths: 5 (cost 1) and 5 6 (cost 2); begin frames 0 and 1, the cut at 1
    r = alternatives(L, [5, 6])
    assert r["n_distinct"].tolist() == [1, 1] and close(r["alts"][0][0][1], 1.0) and close(r["alts"][1][0][1], 1.0 / (E + 1.0))
    # the path that ends in state 1 (final, frame 1: inside cell 1) says nothing there: the 5 on the arc that ENTERS belongs to cell 0
    assert abs(r["none_post"][0]) < 1e-15 and close(r["none_post"][1], E / (E + 1.0))
    one = alternatives(L, [5])   # L = 1: the cell is the whole time axis, both words are in it, every path says one
    assert one["n_distinct"].tolist() == [2] and [w for w, _ in one["alts"][0]] == [5, 6] and abs(one["none_post"][0]) < 1e-15


def test_a_path_that_ended_before_the_cell_began():
    L = ends_early()
    r = alternatives(L, [5, 6])   # begin frames 0 and 3, the cut at 2: the final state of frame 1 lies before cell 1
    assert r["begin"].tolist() == [0, 3] and cuts_of(r["begin"])[1] == 2
    assert close(r["none_post"][1], E / (E + 1.0)) and close(r["alts"][1][0][1], 1.0 / (E + 1.0)) and abs(r["none_post"][0]) < 1e-15


def test_dead_ends_and_an_infinite_arc():
    L = dead_ends()
    r = alternatives(L, [5, 6])   # the arcs off the one path have posterior 0: they add nothing and no word of their own
    assert r["found"] and r["alts"] == [[(5, 1.0)], [(6, 1.0)]] and r["n_distinct"].tolist() == [1, 1]
    assert not np.isnan(r["none_post"]).any() and np.all(np.abs(r["none_post"]) < 1e-15)
    L.st_final[:] = 0
    assert not alternatives(L, [5, 6])["found"]


def test_an_empty_cell_from_two_words_at_one_frame():
    r = alternatives(two_words_at_frame_0(), [7, 8])
    assert r["begin"].tolist() == [0, 0] and cuts_of(r["begin"])[:2] == [0, 0]
    assert r["none_post"][0] == 1.0 and r["alts"][0] == [] and r["n_distinct"].tolist() == [0, 2] and r["word_post"][0] == 0.0
    assert abs(r["none_post"][1]) < 1e-15 and [w for w, _ in r["alts"][1]] == [7, 8] and all(close(x, 1.0) for _, x in r["alts"][1])


def test_one_word_is_one_cell():
    L = twice_in_a_cell()   # the paths say 5 5 (cost 0), 5, 5 (cost 1 each) and nothing (cost 2)
    z = (1.0 + 1.0 / E) ** 2
    r = alternatives(L, [5])
    assert close(r["none_post"][0], E ** -2.0 / z) and close(r["alts"][0][0][1], 2.0 / (1.0 + 1.0 / E)) and r["n_distinct"].tolist() == [1]
    # a path says the word twice: the mass passes the share of the paths that say something
    assert 1.0 - r["none_post"][0] < r["alts"][0][0][1] - 0.1
    assert close(r["none_post"][0], math.exp(sentence(L, [], posteriors(L))["logpost"]))
    both = alternatives(L, [5, 5])   # the cut at 1: in either cell the wordless arc is taken with 1 / (e + 1)
    assert all(close(x, 1.0 / (E + 1.0)) for x in both["none_post"])


def test_the_empty_sequence_and_a_sequence_not_in_the_lattice():
    empty, absent, skipped = alternatives_many(twice_in_a_cell(), [[], [6], None])
    assert empty["found"] and empty["alts"] == [] and len(empty["none_post"]) == 0
    assert not absent["found"] and absent["alts"] == [] and len(absent["none_post"]) == 0 and skipped is None


def test_the_frame_rule_is_asserted():
    L = make_lattice([(0, 1, 0), (2, 2, 1)], [(0, 1, 1, 5, 0.5, 0.5)])
    with pytest.raises(AssertionError):
        assert_frames(L)


# ---- random small lattices against the enumeration of every path -------------------------------------------------------------------
def test_random_lattices_against_every_path():
    rs = np.random.RandomState(17)
    n = n_seq = n_cell = n_zero = n_one = n_mass = n_twice = n_whole = 0
    worst = 0.0
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
        for scale in (1.0, 0.1):
            P = posteriors(L, scale, scale)
            # L = 1: the one cell is the whole time axis, and saying nothing in it is the empty sentence
            s = sentence(L, [], P)
            whole = none_posts(L, P, [0, np.iinfo(np.int64).max])[0]
            assert abs(whole - (math.exp(s["logpost"]) if s["found"] else 0.0)) <= 1e-12, n
            n_whole += whole > 0.0
            for w, r in zip(seqs, alternatives_many(L, seqs, scale, scale, post=P)):
                if not r["found"] or not w:
                    continue
                n_seq += 1
                m = cuts_of(r["begin"])
                none, mass, some = brute_force(L, paths, scale, scale, m)
                for k in range(len(w)):
                    if m[k] >= m[k + 1]:
                        assert r["none_post"][k] == 1.0 and none[k] == 1.0
                        continue
                    x = r["none_post"][k]
                    assert abs(x - none[k]) <= 1e-12, (n, w, k, x, none[k])
                    worst = max(worst, abs(x - none[k]))
                    n_cell += 1
                    n_zero += none[k] == 0.0
                    n_one += none[k] == 1.0
                    want = {v: y for v, y in mass[k].items() if y > 0.0}
                    assert set(want) == set(r["mass"][k]), (n, w, k)
                    for v, y in want.items():
                        assert abs(r["mass"][k][v] - y) <= 1e-12 * max(1.0, y), (n, w, k, v)
                        n_mass += 1
                    # none_post + P(some word in the cell) = 1, and the masses pass that share only where a path says two words
                    total = math.fsum(r["mass"][k].values())
                    assert abs(1.0 - x - some[k]) <= 1e-12 and 1.0 - x <= total + tol_word(P, L, total)
                    twice = any(sum(1 for a in p if L.a_ol[a] and m[k] <= L.st_frame[L.a_src[a]] < m[k + 1]) > 1 for p in paths)
                    n_twice += twice
                    if not twice:
                        assert abs(1.0 - x - total) <= 1e-12, (n, w, k)
                    assert r["mass"][k].get(int(w[k]), 0.0) == r["word_post"][k]
    between = n_cell - n_zero - n_one
    print("lattices %d, sequences %d, cells %d (%d at 0, %d at 1, %d between, %d with a path that says two words), masses %d; "
          "worst |none_post| error %.3g" % (n, n_seq, n_cell, n_zero, n_one, between, n_twice, n_mass, worst))
    assert n_cell >= 500 and 4 * between >= n_cell and n_mass >= 500 and n_whole >= 20


# ---- the identities ------------------------------------------------------------------------------------------------------------
def test_identities_on_the_oracle_lattices(lattices):
    """the best path's words on each of the twelve lattices, at (1, 1) and (0.1, 0.1): 0 <= none_post <= 1 + tolerance, the lists
    ordered, n_distinct against a plain np.unique, mass(k, w[k]) == word_post[k], 1 - none_post <= the cell's masses; and for the
    one cell that is the whole time axis (L = 1) none_post = exp(the sentence posterior of the empty sequence)."""
    n = 0
    most_keys = most_cell = 0
    for what, L, bp, T in lattices:
        assert L.ok and bp.ok, what
        assert_frames(L)
        best = [int(w) for w in bp.words]
        fr = L.st_frame[L.a_src].astype(np.int64)
        for scale in (1.0, 0.1):
            P = posteriors(L, scale, scale)
            r = alternatives_many(L, [best], scale, scale, post=P)[0]
            assert r["found"], what
            m = cuts_of(r["begin"])
            keys = 0
            for k in range(len(best)):
                x = r["none_post"][k]
                assert 0.0 <= x <= 1.0 + tol_none(P, L, 1.0), (what, scale, k, x)
                lst = r["alts"][k]
                assert all(a[1] > b[1] or (a[1] == b[1] and a[0] < b[0]) for a, b in zip(lst, lst[1:])), (what, k)
                sel = (L.a_ol > 0) & (fr >= m[k]) & (fr < m[k + 1]) & (P["gamma"] > 0)
                assert r["n_distinct"][k] == len(np.unique(L.a_ol[sel])) == len(lst), (what, k)
                assert r["mass"][k].get(best[k], 0.0) == r["word_post"][k], (what, k)
                total = math.fsum(r["mass"][k].values())
                assert 1.0 - x <= total + tol_word(P, L, total) + tol_none(P, L, x), (what, scale, k)
                keys += len(lst)
                most_cell = max(most_cell, len(lst))
            most_keys = max(most_keys, keys)
            s = sentence(L, [], P)
            want = math.exp(s["logpost"]) if s["found"] else 0.0
            whole = none_posts(L, P, [0, np.iinfo(np.int64).max])[0]
            assert abs(whole - want) <= tol_none(P, L, want) + s["tol"] * want, (what, scale)
        n += 1
    print("most distinct (cell, word) pairs of a sequence %d, most words of a cell %d" % (most_keys, most_cell))
    assert n == 12


# ---- the tolerance and the comparison rule do not hide a failure -----------------------------------------------------------------
@pytest.mark.parametrize("make, seq, cell", [(chain_with_wordless_shortcut, [7, 8], 1), (twice_in_a_cell, [5], 0), (twice_in_a_cell, [5, 5], 1)],
                         ids=["shortcut", "one_cell", "second_cell"])
def test_removing_a_wordless_arc_moves_none_post_far_beyond_the_tolerance(make, seq, cell):
    for scale in (1.0, 0.1):
        L = make()
        P = posteriors(L, scale, scale)
        r = alternatives_many(L, [seq], scale, scale, post=P)[0]
        m = cuts_of(r["begin"])
        fr = L.st_frame[L.a_src]
        quiet = np.nonzero((L.a_ol == 0) & (fr >= m[cell]) & (fr < m[cell + 1]) & (P["gamma"] > 0))[0]
        moved = 0
        for a in quiet:
            M = without_arc(L, int(a))
            q = alternatives_many(M, [seq], scale, scale)[0]
            if not q["found"] or q["begin"].tolist() != r["begin"].tolist():
                continue
            assert abs(q["none_post"][cell] - r["none_post"][cell]) > 1000.0 * tol_none(P, L, r["none_post"][cell]), (make.__name__, scale, int(a))
            moved += 1
        assert moved >= 1


def _device_like(r, n_alts):
    """the restatement's answer in the shape BatchDecoder.word_alternatives returns"""
    g = dict(r)
    g["alts"] = [lst[:n_alts] for lst in r["alts"]]
    g["n_distinct"] = np.array(r["n_distinct"])
    g["none_post"] = np.array(r["none_post"])
    return g


def test_compare_accepts_the_restatement_and_rejects_what_is_wrong():
    L = make_lattice([(0, 1, 0), (1, 2, 1)], [(0, 1, 1, 5, 0.0, 0.0), (0, 1, 2, 6, 0.5, 0.0), (0, 1, 3, 7, 1.0, 0.0), (0, 1, 4, 0, 1.5, 0.0)])
    P = posteriors(L)
    want = alternatives_many(L, [[6]], post=P)[0]
    assert [w for w, _ in want["alts"][0]] == [5, 6, 7]
    for n_alts in (1, 2, 3, 5):
        assert compare(_device_like(want, n_alts), want, P, L, n_alts) == 0.0
    tol = lambda v: tol_word(P, L, v)
    lst = want["alts"][0]
    ok = lambda got, nd, n_alts: compare_lists(got, nd, want["mass"][0], n_alts, tol)
    with pytest.raises(AssertionError):      # two entries swapped: the words keep their places, the posts change hands
        ok([(lst[0][0], lst[1][1]), (lst[1][0], lst[0][1]), lst[2]], 3, 3)
    with pytest.raises(AssertionError):      # the same with the order of the list kept
        ok([lst[1], lst[0], lst[2]], 3, 3)
    with pytest.raises(AssertionError):      # the largest entry dropped from a full list
        ok([lst[1], lst[2]], 3, 2)
    with pytest.raises(AssertionError):      # an entry dropped from a list with room
        ok([lst[0], lst[2]], 3, 5)
    with pytest.raises(AssertionError):      # a wrong n_distinct
        ok(lst[:2], 4, 2)
    with pytest.raises(AssertionError):      # a word that is not in the cell
        ok(lst + [(9, 0.01)], 4, 5)
    with pytest.raises(AssertionError):      # a word twice
        ok([lst[0], lst[0], lst[2]], 3, 3)
    with pytest.raises(AssertionError):      # a post beyond the tolerance
        ok([(lst[0][0], lst[0][1] * (1 + 1e-9))] + lst[1:], 3, 3)
    bad = _device_like(want, 3)
    bad["none_post"] = want["none_post"] + 1e-9
    assert compare(bad, want, P, L, 3) > 1000.0
    # near ties: two words whose masses differ by less than the tolerance may come in either order, on the device's own values
    T = make_lattice([(0, 1, 0), (1, 2, 1)], [(0, 1, 1, 5, 1.0, 0.0), (0, 1, 2, 6, 1.0, 0.0), (0, 1, 3, 7, 3.0, 0.0)])
    PT = posteriors(T)
    wt = alternatives_many(T, [[5]], post=PT)[0]
    tie = wt["alts"][0]
    flipped = [(6, tie[1][1] + 1e-17 + 2e-16), (5, tie[0][1]), tie[2]]
    assert compare_lists(flipped, 3, wt["mass"][0], 3, lambda v: tol_word(PT, T, v)) <= 1.0
    assert compare_lists(flipped[:1], 3, wt["mass"][0], 1, lambda v: tol_word(PT, T, v)) <= 1.0
    # a word of vanishing mass may be counted or not
    faint = dict(want["mass"][0])
    faint[11] = TINY / 4
    assert compare_lists(lst + [(11, TINY / 4)], 4, faint, 5, tol) == 0.0
    assert compare_lists(lst, 3, faint, 5, tol) == 0.0
