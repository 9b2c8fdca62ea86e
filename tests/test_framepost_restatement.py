"""CPU: the definition of wfst_decoder_frame_posteriors as tests/framepost_util.py restates it -- on hand-made lattices whose
answers are worked out by hand (in the comments), on test_posterior_restatement.py's 300 random lattices against the enumeration
of every path, and identities on the C oracle's twelve raw lattices.  The sensitivity tests keep the tolerance and the comparison
rule from hiding a failure."""
import copy
import importlib
import math

import numpy as np
import pytest

from align_util import make_lattice
from framepost_util import band_classes, brute_force, compare, frame_posteriors
from nearest_util import all_paths
from posterior_util import posteriors, random_lattice, tol_word, without_arc
from test_posterior_restatement import lattices   # noqa: F401  (the fixture: the twelve oracle lattices)

E = math.e


def close(x, y, tol=1e-14):
    return abs(float(x) - float(y)) <= tol * max(1.0, abs(float(y)))


def lookup():
    return importlib.import_module("asr-decoder_amd").wfstdec.frame_post_lookup


# states (frame, graph state, final); arcs (src, dst, ilabel, olabel, graph, acoustic)
def test_two_parallel_arcs_with_the_same_tid_add_up():
    L = make_lattice([(0, 1, 0), (1, 2, 1)], [(0, 1, 7, 5, 0.5, 0.5), (0, 1, 7, 6, 0.5, 0.5)])
    r = frame_posteriors(L)
    assert r["n_frames"] == 1 and r["frame_off"].tolist() == [0, 1] and r["classes"].tolist() == [7] and r["posts"].tolist() == [1.0]
    assert r["n_distinct"].tolist() == [1] and r["frame_mass"].tolist() == [1.0] and close(r["log_z"], math.log(2.0) - 1.0)


def test_two_parallel_arcs_with_different_tids():
    L = make_lattice([(0, 1, 0), (1, 2, 1)], [(0, 1, 9, 5, 0.5, 0.5), (0, 1, 4, 6, 1.5, 0.5)])   # costs 1 and 2
    r = frame_posteriors(L)
    assert r["classes"].tolist() == [4, 9] and r["n_distinct"].tolist() == [2]        # by class id ascending, not by mass
    assert close(r["posts"][0], 1.0 / (1.0 + E)) and close(r["posts"][1], E / (1.0 + E)) and close(r["frame_mass"][0], 1.0)
    # min_post is taken per class; n_distinct and frame_mass are from before the threshold
    t = frame_posteriors(L, min_post=0.5)
    assert t["classes"].tolist() == [9] and t["n_distinct"].tolist() == [2] and close(t["frame_mass"][0], 1.0) and t["frame_off"].tolist() == [0, 1]
    # both tids to one class
    m = np.zeros(10, np.int32)
    m[[4, 9]] = 3
    one = frame_posteriors(L, label_map=m)
    assert one["classes"].tolist() == [3] and close(one["posts"][0], 1.0) and one["n_distinct"].tolist() == [1]


def test_a_word_carrying_epsilon_arc_between_two_frames_states_does_not_appear():
    L = make_lattice([(0, 10, 0), (1, 11, 0), (1, 12, 0), (2, 13, 1)],
                     [(0, 1, 5, 0, 0.5, 1.0), (1, 2, 0, 7, 0.25, 0.0), (2, 3, 6, 0, 0.5, 2.0)])
    r = frame_posteriors(L)     # one path: frame 0 says tid 5, frame 1 says tid 6; the arc with ilabel 0 (word 7) is in no frame
    assert r["n_frames"] == 2 and r["frame_off"].tolist() == [0, 1, 2] and r["classes"].tolist() == [5, 6]
    assert all(close(x, 1.0) for x in r["posts"]) and r["n_distinct"].tolist() == [1, 1] and all(close(x, 1.0) for x in r["frame_mass"])


def test_a_dead_end_and_an_infinite_arc_drop_out():
    # state 2 is a dead end, state 3 cannot be reached, and the second arc 0 -> 1 costs +inf
    L = make_lattice([(0, 1, 0), (1, 2, 0), (1, 3, 0), (1, 4, 0), (2, 5, 1)],
                     [(0, 1, 1, 5, 0.5, 0.5), (0, 2, 2, 5, 0.5, 0.5), (1, 4, 3, 6, 0.5, 0.5), (0, 1, 4, 5, np.inf, 0.0), (3, 4, 5, 6, 0.5, 0.5)])
    r = frame_posteriors(L)
    assert r["frame_off"].tolist() == [0, 1, 2] and r["classes"].tolist() == [1, 3] and r["posts"].tolist() == [1.0, 1.0]
    assert r["n_distinct"].tolist() == [1, 1] and r["frame_mass"].tolist() == [1.0, 1.0]
    assert sorted(r["mass"][0].items()) == [(1, 1.0), (2, 0.0), (4, 0.0)]     # the restatement knows them, at mass 0
    L.st_final[:] = 0       # no path at all: every posterior 0, nothing listed
    z = frame_posteriors(L)
    assert z["n_frames"] == 2 and z["frame_off"].tolist() == [0, 0, 0] and not z["n_distinct"].any() and not z["frame_mass"].any()


def test_a_final_state_with_an_out_arc_and_a_path_that_ends_early():
    L = make_lattice([(0, 1, 0), (1, 2, 1), (2, 3, 1)], [(0, 1, 1, 5, 1.0, 0.0), (1, 2, 2, 6, 0.5, 0.5)])
    # the paths: one arc (cost 1), both arcs (cost 2); the first ends before frame 2
    early = E ** -1.0 / (E ** -1.0 + E ** -2.0)
    r = frame_posteriors(L)
    assert r["n_frames"] == 2 and r["classes"].tolist() == [1, 2] and close(r["frame_mass"][0], 1.0)
    assert close(r["frame_mass"][1], 1.0 - early) and close(r["posts"][1], 1.0 / (E + 1.0)) and r["frame_mass"][1] == r["posts"][1]


def test_no_lattice():
    r = frame_posteriors(None)
    assert r["n_frames"] == 0 and r["log_z"] == 0.0 and r["frame_off"].tolist() == [0] and len(r["classes"]) == 0
    assert compare(dict(r), r, None, None) == 0.0


# ---- random small lattices against the enumeration of every path -------------------------------------------------------------------
def test_random_lattices_against_every_path():
    rs = np.random.RandomState(17)
    n = n_entries = n_shared = 0
    worst = 0.0
    pair = np.array([0, 1, 1, 2], np.int32)    # tids 1 and 2 share class 1
    while n < 300:
        L = random_lattice(rs, quantised=bool(n % 4))
        if L is None:
            continue
        paths = all_paths(L, 20000)
        if not paths:
            continue
        n += 1
        [rs.randint(1, 4, rs.randint(0, 4)) for _ in range(2)]   # (test_posterior_restatement.py draws its sequences here: the same 300)
        [rs.randint(len(paths)) for _ in range(2)]
        for scale in (1.0, 0.1):
            P = posteriors(L, scale, scale)
            for m in (None, pair):
                r = frame_posteriors(L, scale, scale, label_map=m, post=P)
                want = brute_force(L, paths, scale, scale, m)
                assert len(want) == r["n_frames"] == len(r["mass"])
                for f, d in enumerate(want):
                    got = {int(v): float(x) for v, x in zip(r["classes"][r["frame_off"][f]:r["frame_off"][f + 1]],
                                                             r["posts"][r["frame_off"][f]:r["frame_off"][f + 1]])}
                    assert set(got) == set(d), (n, f)
                    for v, y in d.items():
                        assert abs(got[v] - y) <= 1e-12, (n, f, v)
                        worst = max(worst, abs(got[v] - y))
                        n_entries += 1
                    cls = np.asarray(L.a_il) if m is None else m[L.a_il]
                    sel = (L.a_il > 0) & (L.st_frame[L.a_src] == f) & (P["gamma"] > 0)
                    n_shared += len(cls[sel]) > len(np.unique(cls[sel]))
                    assert abs(r["frame_mass"][f] - math.fsum(d.values())) <= 1e-12 and r["n_distinct"][f] == len(d)
    print("lattices %d, entries %d, frames where a class sums several arcs %d; worst error %.3g" % (n, n_entries, n_shared, worst))
    assert n_entries >= 3000 and n_shared >= 300


# ---- identities on the oracle's lattices ----------------------------------------------------------------------------------------
def test_oracle_lattices(lattices, synth):   # noqa: F811
    tid2pdf = np.asarray(synth.default_tid2pdf(600), np.int32)
    single = np.full(601, 42, np.int32)
    look = lookup()
    worst_mass, most_distinct, n = 0.0, 0, 0
    for what, L, bp, T in lattices:
        for scale in (1.0, 0.1):
            P = posteriors(L, scale, scale)
            r = frame_posteriors(L, scale, scale, post=P)
            assert r["n_frames"] == T, what
            # every path runs to the last frame: the mass of a frame is 1
            dev = np.abs(r["frame_mass"] - 1.0)
            assert np.all(dev <= tol_word(P, L, 1.0)), (what, scale, dev.max())
            worst_mass = max(worst_mass, float(dev.max()))
            most_distinct = max(most_distinct, int(r["n_distinct"].max()))
            # the entries of a frame sum to its frame_mass
            off = r["frame_off"]
            sums = np.array([r["posts"][off[f]:off[f + 1]].sum() for f in range(T)])
            assert np.all(np.abs(sums - r["frame_mass"]) <= tol_word(P, L, 1.0)), what
            assert np.array_equal(np.diff(off), r["n_distinct"]), what    # (no emitting arc here has gamma == 0)
            # mapping through tid2pdf equals grouping the tid entries by pdf
            by_pdf = frame_posteriors(L, scale, scale, label_map=tid2pdf, post=P)
            for f in range(T):
                grouped = {}
                for v, x in zip(r["classes"][off[f]:off[f + 1]], r["posts"][off[f]:off[f + 1]]):
                    grouped.setdefault(int(tid2pdf[v]), []).append(float(x))
                o2 = by_pdf["frame_off"]
                assert by_pdf["classes"][o2[f]:o2[f + 1]].tolist() == sorted(grouped), (what, f)
                for v, x in zip(by_pdf["classes"][o2[f]:o2[f + 1]], by_pdf["posts"][o2[f]:o2[f + 1]]):
                    assert abs(x - math.fsum(grouped[int(v)])) <= tol_word(P, L, x), (what, f, v)
            # a map to a single class: one entry per frame, equal to frame_mass
            one = frame_posteriors(L, scale, scale, label_map=single, post=P)
            assert one["frame_off"].tolist() == list(range(T + 1)) and np.all(one["classes"] == 42) and one["n_distinct"].tolist() == [1] * T
            assert np.all(np.abs(one["posts"] - r["frame_mass"]) <= tol_word(P, L, 1.0)), what
            # the best path's transition-ids are in the lattice at every frame
            tids = np.asarray(bp.tids)
            assert len(tids) == T, what
            trace = look(r, tids)
            assert trace.shape == (T,) and np.all(trace > 0.0) and np.all(trace <= 1.0 + tol_word(P, L, 1.0)), (what, scale)
            assert compare(dict(r), r, P, L, 0.0, what) == 0.0
        n += 1
    print("worst deviation of a frame's mass from 1: %.3g; most distinct transition-ids in a frame %d" % (worst_mass, most_distinct))
    assert n == 12


def test_frame_post_lookup():
    look = lookup()
    r = dict(frame_off=np.array([0, 2, 2, 3]), classes=np.array([4, 9, 4]), posts=np.array([0.25, 0.75, 1.0]))
    assert look(r, [9, 4, 4]).tolist() == [0.75, 0.0, 1.0]
    assert look(r, [4, 9, 9, 1]).tolist() == [0.25, 0.0, 0.0, 0.0]         # a frame beyond the result's gives 0
    assert look(r, [5, -1]).tolist() == [0.0, 0.0] and look(r, []).tolist() == []
    assert look(dict(frame_off=np.array([0]), classes=np.zeros(0, np.int32), posts=np.zeros(0)), [3]).tolist() == [0.0]


# ---- sensitivity ------------------------------------------------------------------------------------------------------------------
def fan_lattice():
    """two frames of three and two parallel arcs, every arc on a complete path"""
    return make_lattice([(0, 1, 0), (1, 2, 0), (2, 3, 1)],
                        [(0, 1, 1, 5, 0.5, 0.0), (0, 1, 2, 6, 1.0, 0.0), (0, 1, 3, 0, 1.5, 0.0), (1, 2, 4, 0, 0.25, 0.0), (1, 2, 5, 7, 0.75, 0.0)])


def test_removing_an_arc_moves_its_frames_entry_far_beyond_the_tolerance():
    for scale in (1.0, 0.1):
        L = fan_lattice()
        P = posteriors(L, scale, scale)
        r = frame_posteriors(L, scale, scale, post=P)
        for a in range(len(L.a_src)):
            f, v = int(L.st_frame[L.a_src[a]]), int(L.a_il[a])
            M = without_arc(L, a)
            q = frame_posteriors(M, scale, scale)
            assert v not in q["mass"][f] and r["mass"][f][v] > 1000.0 * tol_word(P, L, r["mass"][f][v]), (scale, a)
            # ... and the other entries of the frame by more than 1000 tolerances as well
            for u, y in q["mass"][f].items():
                assert abs(y - r["mass"][f][u]) > 1000.0 * tol_word(P, L, y), (scale, a, u)


def test_compare_rejects_what_it_must():
    L = fan_lattice()
    P = posteriors(L)
    want = frame_posteriors(L, post=P)
    good = {k: copy.deepcopy(v) for k, v in want.items() if k != "mass"}
    assert compare(copy.deepcopy(good), want, P, L) == 0.0

    def bad(change, want=want, min_post=0.0, start=good):
        g = copy.deepcopy(start)
        change(g)
        with pytest.raises(AssertionError):
            compare(g, want, P, L, min_post)

    def swap(g):
        g["classes"][[0, 1]] = g["classes"][[1, 0]]
        g["posts"][[0, 1]] = g["posts"][[1, 0]]

    def swap_classes_only(g):
        g["classes"][[0, 1]] = g["classes"][[1, 0]]

    def drop(g):
        g["classes"], g["posts"] = np.delete(g["classes"], 1), np.delete(g["posts"], 1)
        g["frame_off"][1:] -= 1

    def repeat(g):
        g["classes"], g["posts"] = np.insert(g["classes"], 1, g["classes"][0]), np.insert(g["posts"], 1, g["posts"][0])
        g["frame_off"][1:] += 1

    def distinct(g):
        g["n_distinct"][1] += 1

    def offsets(g):
        g["frame_off"][1] += 1      # frame 0 takes frame 1's first entry

    def value(g):
        g["posts"][0] += 1000.0 * tol_word(P, L, g["posts"][0])

    def mass(g):
        g["frame_mass"][1] -= 1000.0 * tol_word(P, L, 1.0)

    for change in (swap, swap_classes_only, drop, repeat, distinct, offsets, value, mass):
        bad(change)
    # an entry listed below min_post: the answer at min_post 0 held against the restatement at 0.3 (tid 3 has mass 0.186)
    assert 0.0 < want["mass"][0][3] < 0.3 and band_classes(want, P, L, 0.3) == 0
    want3 = frame_posteriors(L, min_post=0.3, post=P)
    good3 = {k: copy.deepcopy(v) for k, v in want3.items() if k != "mass"}
    assert compare(copy.deepcopy(good3), want3, P, L, 0.3) == 0.0 and len(good3["classes"]) < len(good["classes"])
    bad(lambda g: None, want3, 0.3)
    # ... and an entry missing above it
    bad(drop, want3, 0.3, good3)
    # a threshold on a class' own mass: the band holds it, and band_classes says so
    assert band_classes(want, P, L, want["mass"][0][3]) == 1
