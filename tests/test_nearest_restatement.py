"""CPU: the definition of wfst_decoder_nearest_words as tests/nearest_util.py restates it -- on hand-made lattices whose answers are
worked out by hand (in the comments), on random small lattices against the enumeration of every path, against align_util where
the two definitions meet, and on the C oracle's raw lattices.  No tolerances: costs are compared by their bits."""
import numpy as np
import pytest

import pyoracle
from align_util import align, make_lattice
from nearest_util import all_paths, brute_force, levenshtein, nearest, nearest_many

F32 = np.float32


def bits(x):
    return np.asarray(x, F32).view(np.int32).tolist()


def counts(r):
    return [r[k] for k in ("n_err", "n_cor", "n_sub", "n_ins", "n_del")]


def identities(r, ref):
    assert r["n_sub"] + r["n_ins"] + r["n_del"] == r["n_err"]
    assert r["n_cor"] + r["n_sub"] + r["n_del"] == len(ref)
    assert r["n_cor"] + r["n_sub"] + r["n_ins"] == r["n_hyp"] == len(r["hyp_words"]) == len(r["begin"]) == len(r["end"])
    m = r["ref_hyp"]
    assert len(m) == len(ref) and int((m < 0).sum()) == r["n_del"]
    assert np.all(np.diff(m[m >= 0]) > 0) and np.all(m < r["n_hyp"])
    assert sum(int(r["hyp_words"][j]) == int(ref[k]) for k, j in enumerate(m) if j >= 0) == r["n_cor"]


# states (frame, graph state, final); arcs (src, dst, ilabel, olabel, graph, acoustic)
def _chain(words, cost=0.5):
    n = len(words)
    return make_lattice([(f, f + 1, int(f == n)) for f in range(n + 1)], [(f, f + 1, f + 1, w, cost, cost) for f, w in enumerate(words)])


def test_a_substitution_beats_a_deletion_and_an_insertion():
    r = nearest(_chain([5, 6]), [5, 7])     # 5 matched, 6 against 7: one substitution (deleting 7 and inserting 6 would be two errors)
    assert r["found"] and counts(r) == [1, 1, 1, 0, 0] and r["hyp_words"].tolist() == [5, 6] and r["ref_hyp"].tolist() == [0, 1]
    assert [k for k, _ in r["ops"]] == [0, 0] and bits([r["tot"], r["lm"]]) == bits([2.0, 1.0]) and not r["tie"]
    assert r["begin"].tolist() == [0, 1] and r["end"].tolist() == [1, 2]


def test_a_word_on_an_epsilon_arc_inside_a_frame():
    L = make_lattice([(0, 10, 0), (1, 11, 0), (1, 12, 0), (2, 13, 1)],
                     [(0, 1, 5, 0, 0.5, 1.0), (1, 2, 0, 7, 0.25, 0.0), (2, 3, 6, 0, 0.5, 2.0)])
    r = nearest(L, [7])    # the kinds go by olabel: the epsilon arc carries the word
    assert counts(r) == [0, 1, 0, 0, 0] and r["begin"].tolist() == [1] and r["end"].tolist() == [2] and r["n_arcs"] == 3
    assert bits([r["tot"], r["lm"]]) == bits([4.25, 1.25])   # ((0 + 1.5) + 0.25) + 2.5; 0.5 + 0.25 + 0.5
    r = nearest(L, [8])
    assert counts(r) == [1, 0, 1, 0, 0] and r["ref_hyp"].tolist() == [0] and r["hyp_words"].tolist() == [7]
    r = nearest(L, [])     # the only path has a word: one insertion
    assert counts(r) == [1, 0, 0, 1, 0] and r["n_hyp"] == 1 and len(r["ref_hyp"]) == 0 and bits(r["tot"]) == bits(4.25)


def test_a_word_on_the_last_arc_and_references_longer_than_any_path():
    L = make_lattice([(0, 1, 0), (1, 2, 0), (2, 3, 1)], [(0, 1, 3, 0, 1.0, 1.0), (1, 2, 4, 9, 0.5, 0.5)])
    r = nearest(L, [9])
    assert counts(r) == [0, 1, 0, 0, 0] and r["begin"].tolist() == [1] and r["end"].tolist() == [2] and r["arcs"].tolist() == [0, 1]
    assert bits([r["tot"], r["lm"]]) == bits([3.0, 1.5])
    r = nearest(L, [9, 4])     # the path has one word: 4 is deleted, after the last arc
    assert counts(r) == [1, 1, 0, 0, 1] and r["ref_hyp"].tolist() == [0, -1] and [k for k, _ in r["ops"]] == [1, 0, 3]
    r = nearest(L, [4, 9])     # 4 deleted and 9 matched (one error), not 4 against 9 and 9 deleted (two)
    assert counts(r) == [1, 1, 0, 0, 1] and r["ref_hyp"].tolist() == [-1, 0]
    r = nearest(L, [1, 2, 3, 4])
    assert counts(r) == [4, 0, 1, 0, 3] and bits(r["tot"]) == bits(3.0)   # deletions cost nothing


def test_the_empty_reference():
    plain = make_lattice([(0, 1, 0), (1, 2, 1)], [(0, 1, 1, 0, 1.0, 2.0)])
    r = nearest(plain, [])
    assert r["found"] and counts(r) == [0, 0, 0, 0, 0] and r["n_arcs"] == 1 and r["n_hyp"] == 0 and bits([r["tot"], r["lm"]]) == bits([3.0, 1.0])
    r = nearest(plain, [1])
    assert r["found"] and counts(r) == [1, 0, 0, 0, 1] and r["ref_hyp"].tolist() == [-1]
    assert nearest_many(plain, [None, []])[0] is None


def _diamond(early, late, gstates=(2, 3)):
    """word 5 either on the first arc of the upper branch (cost `early` per arc) or on the second arc of the lower one (`late`)"""
    return make_lattice([(0, 1, 0), (1, gstates[0], 0), (1, gstates[1], 0), (2, 4, 1)],
                        [(0, 1, 1, 5, early, early), (0, 2, 2, 0, late, late), (1, 3, 3, 0, early, early), (2, 3, 4, 5, late, late)])


def test_a_reference_that_shares_no_word_with_the_lattice():
    L = _diamond(1.0, 0.5)      # both paths carry word 5: one substitution either way, so the cheaper path (the lower, 2.0) wins
    r = nearest(L, [6])
    assert counts(r) == [1, 0, 1, 0, 0] and r["arcs"].tolist() == [1, 3] and bits([r["tot"], r["lm"]]) == bits([2.0, 1.0])
    assert r["begin"].tolist() == [1] and r["end"].tolist() == [2]
    r = nearest(L, [6, 7, 8])
    assert r["n_err"] == 3 and r["n_sub"] == 1 and r["n_del"] == 2 and bits(r["tot"]) == bits(2.0)
    L.st_final[:] = 0
    assert not nearest(L, [5])["found"]   # found = 0 only where no final state is reached


def test_errors_come_before_cost():
    # the upper branch spells 5 at 4.0, the lower spells 6 at 2.0: for [5] the dearer path without errors wins
    L = make_lattice([(0, 1, 0), (1, 2, 0), (1, 3, 0), (2, 4, 1)],
                     [(0, 1, 1, 5, 1.0, 1.0), (0, 2, 2, 6, 0.5, 0.5), (1, 3, 3, 0, 1.0, 1.0), (2, 3, 4, 0, 0.5, 0.5)])
    assert nearest(L, [5])["arcs"].tolist() == [0, 2] and nearest(L, [6])["arcs"].tolist() == [1, 3]
    r = nearest(L, [7])
    assert r["n_sub"] == 1 and r["arcs"].tolist() == [1, 3]


def test_ties_between_kinds_go_by_the_kind_order():
    # 5 5 against [5]: the same path, the same (1, 2.0) whichever 5 is the inserted one.  At (2, 1) the match from (1, 0) is kind
    # 0 and the insertion from (1, 1) kind 2: the SECOND 5 is the matched one.
    r = nearest(_chain([5, 5]), [5])
    assert r["tie"] and counts(r) == [1, 1, 0, 1, 0] and r["ref_hyp"].tolist() == [1] and [k for k, _ in r["ops"]] == [2, 0]
    # one arc without a word against [5]: at (1, 1) the free arc from (0, 1) is kind 1 and the deletion from (1, 0) kind 3, so the
    # deletion is taken at the start state
    L = make_lattice([(0, 1, 0), (1, 2, 1)], [(0, 1, 1, 0, 1.0, 2.0)])
    r = nearest(L, [5])
    assert r["tie"] and [k for k, _ in r["ops"]] == [3, 1]
    # 5 against [6 6]: substitution + deletion; at (1, 2) kind 0 (from (0, 1): the first 6 deleted at the start) beats kind 3
    r = nearest(_chain([5]), [6, 6])
    assert r["tie"] and r["ref_hyp"].tolist() == [-1, 0] and [k for k, _ in r["ops"]] == [3, 0]


def _fork(gstates):
    """word 5 on the first arc of either branch, no word on the second: both arrivals at the final state are of one kind"""
    return make_lattice([(0, 1, 0), (1, gstates[0], 0), (1, gstates[1], 0), (2, 4, 1)],
                        [(0, 1, 1, 5, 0.5, 0.5), (0, 2, 2, 5, 0.5, 0.5), (1, 3, 3, 0, 0.5, 0.5), (2, 3, 4, 0, 0.5, 0.5)])


@pytest.mark.parametrize("gstates,arcs", [((2, 3), [0, 2]), ((3, 2), [1, 3]), ((7, 7), [0, 2])])
@pytest.mark.parametrize("ref", [[5], [6]])
def test_ties_between_arcs_go_by_the_arc_tuple(gstates, arcs, ref):
    """both branches cost 1.0 + 1.0 and both arrive at the final state over a free arc: the one whose source token has the lower graph
    state wins, whatever the states' numbers are, and between equal graph states the lower ilabel (3 before 4) -- for a match and
    for a substitution alike"""
    r = nearest(_fork(gstates), ref)
    assert r["tie"] and r["arcs"].tolist() == arcs and r["begin"].tolist() == [0] and r["end"].tolist() == [2]
    assert r["n_err"] == int(ref != [5]) and bits([r["tot"], r["lm"]]) == bits([2.0, 1.0])


def test_the_kind_order_comes_before_the_arc_tuple():
    """_diamond at equal costs against [5]: at the final state the lower branch arrives by a match (kind 0) and the upper by a free arc
    (kind 1), so the lower wins even where the upper's source token has the lower graph state"""
    for gstates in ((2, 3), (3, 2)):
        r = nearest(_diamond(0.5, 0.5, gstates), [5])
        assert r["tie"] and r["arcs"].tolist() == [1, 3] and r["begin"].tolist() == [1]


def test_silence_trimmed_ends():
    L = make_lattice([(0, 1, 0), (1, 2, 0), (2, 3, 0), (3, 4, 0), (4, 5, 1)],
                     [(0, 1, 10, 5, 1, 1), (1, 2, 20, 0, 1, 1), (2, 3, 21, 6, 1, 1), (3, 4, 20, 0, 1, 1)])
    r = nearest(L, [5, 7])
    assert r["hyp_words"].tolist() == [5, 6] and r["n_sub"] == 1 and r["begin"].tolist() == [0, 2] and r["end"].tolist() == [2, 4]
    r = nearest(L, [5, 7], sil_tids=[20])
    assert r["begin"].tolist() == [0, 2] and r["end"].tolist() == [1, 3]
    assert nearest(L, [7], sil_tids=[20, 21])["end"].tolist() == [1, 2]   # word 6 has no non-silence arc: it ends where it begins


# ---- random small lattices against the enumeration of every path -------------------------------------------------------------------
def random_lattice(rs, quantised):
    """2..5 frames of 1..3 states; emitting arcs from a frame to the next, arcs inside a frame (ilabel 0) to a higher state, with and
    without words; costs from a handful of quarters (dense exact ties) or arbitrary"""
    T = rs.randint(2, 6)
    frames = [[0]]
    states = [(0, 0, 0)]
    for f in range(1, T + 1):
        ids = []
        for _ in range(rs.randint(1, 4)):
            ids.append(len(states))
            states.append((f, rs.randint(0, 4), int(f == T and rs.rand() < 0.7)))
        frames.append(ids)
    if not any(s[2] for s in states):
        states[-1] = (T, states[-1][1], 1)
    cost = (lambda: 0.25 * rs.randint(-2, 5)) if quantised else (lambda: float(F32(rs.normal(1.0, 2.0))))
    word = lambda: int(rs.choice([0, 0, 1, 2, 3]))
    arcs = []
    for f in range(T):
        for s in frames[f]:
            for t in frames[f + 1]:
                for _ in range(rs.randint(0, 3)):
                    arcs.append((s, t, rs.randint(1, 4), word(), cost(), cost()))
    for f in range(T + 1):
        for i, s in enumerate(frames[f]):
            for t in frames[f][i + 1:]:
                if rs.rand() < 0.5:
                    arcs.append((s, t, 0, word(), cost(), 0.0))
    return make_lattice(states, arcs) if arcs else None


def test_random_lattices_against_every_path():
    rs = np.random.RandomState(11)
    n = n_found = n_ties = n_eps_words = 0
    while n < 220:
        L = random_lattice(rs, quantised=bool(n % 4))
        if L is None:
            continue
        paths = all_paths(L, 20000)
        if paths is None:
            continue
        refs = [[int(w) for w in rs.randint(1, 5, rs.randint(0, 5))] for _ in range(3)]
        if paths:
            refs.append([int(L.a_ol[a]) for a in paths[rs.randint(len(paths))] if L.a_ol[a]])   # a path's own words: no errors
        n += 1
        n_eps_words += int(((L.a_il == 0) & (L.a_ol != 0)).sum())
        for ref, r in zip(refs, nearest_many(L, refs)):
            want = brute_force(L, ref)
            assert r["found"] == (want is not None), (n, ref)
            a = align(L, ref)
            if not r["found"]:
                assert not a["found"]
                continue
            assert (r["n_err"], bits(r["tot"])) == (want[0], bits(want[1])), (n, ref, r["n_err"], r["tot"], want)
            identities(r, ref)
            assert [int(L.a_ol[x]) for x in r["arcs"] if L.a_ol[x]] == r["hyp_words"].tolist()
            assert levenshtein(r["hyp_words"].tolist(), ref) == r["n_err"]
            # where the two definitions meet: no errors iff the sequence is in the lattice, and then the same cost
            assert (r["n_err"] == 0) == a["found"], (n, ref)
            if a["found"]:
                assert bits(r["tot"]) == bits(a["tot"]), (n, ref)
            n_found += 1
            n_ties += r["tie"]
    print("lattices %d, answers %d, with a tie %d, words on arcs inside a frame %d" % (n, n_found, n_ties, n_eps_words))
    assert n_found >= 400 and n_ties >= 100 and n_eps_words >= 100


# ---- the oracle's lattices ------------------------------------------------------------------------------------------------
GRAPHS = [(3000, 21), (600, 5)]
UTTS = [(40, 700), (97, 701), (150, 702)]


@pytest.fixture(scope="module")
def lattices(oracle, synth, tmp_path_factory):
    """(what, lattice, best path) of the twelve inputs test_align_restatement.py builds: two graphs, lattice_beam 4 and 8, three
    utterances (order-free mode)"""
    out = []
    tmp = tmp_path_factory.mktemp("nearest")
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


def test_oracle_lattices_bounds_and_exact_cases(lattices):
    n = 0
    for what, L, bp in lattices:
        assert L.ok and bp.ok, what
        best = [int(w) for w in bp.words]
        assert len(best) >= 2, what
        swapped, dropped, doubled = list(best), list(best), list(best)
        swapped[len(best) // 2] = 777      # a word id the graphs (500 words) lack
        del dropped[len(best) // 2]
        doubled.insert(len(best) // 2, best[len(best) // 2])
        refs = [best, swapped, dropped, doubled, best[::-1], [], [777] * 3]
        res = nearest_many(L, refs)
        for ref, r in zip(refs, res):
            assert r["found"], what
            identities(r, ref)
            assert r["n_err"] <= levenshtein(best, ref), (what, ref)    # the best path is one of the lattice's paths
            assert levenshtein(r["hyp_words"].tolist(), ref) == r["n_err"], (what, ref)
            a = align(L, ref)
            assert (r["n_err"] == 0) == a["found"], (what, ref)
            if a["found"]:
                assert bits(r["tot"]) == bits(a["tot"]) and np.array_equal(r["begin"], a["begin"]) and np.array_equal(r["end"], a["end"]), (what, ref)
        assert res[0]["n_err"] == 0 and bits([res[0]["tot"], res[0]["lm"]]) == bits([bp.tot_score, bp.lm_score]), what
        assert res[1]["n_err"] == 1, what         # 777 can only be substituted or deleted, and the best path does it in one error
        assert res[2]["n_err"] <= 1 and res[3]["n_err"] <= 1, what
        assert res[6]["n_err"] >= 3, what
        n += 1
    assert n == 12
