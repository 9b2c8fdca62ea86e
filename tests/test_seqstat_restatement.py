"""CPU: the definition of wfst_decoder_sequence_stats as tests/seqstat_util.py restates it -- on hand-made lattices whose answers are
worked out by hand (in the comments), on 300 random lattices against the enumeration of every path, and invariants.  The
sensitivity tests keep the tolerance and the comparison rule from hiding a failure."""
import copy
import math

import numpy as np
import pytest

from align_util import make_lattice
from framepost_util import frame_posteriors
from posterior_util import posteriors, random_lattice
from rescale_util import all_paths
from seqstat_util import arc_acc, brute_force, compare, sequence_stats, tol_acc, tol_value

E = math.e


def close(x, y, tol=1e-14):
    return abs(float(x) - float(y)) <= tol * max(1.0, abs(float(y)))


# states (frame, graph state, final); arcs (src, dst, ilabel, olabel, graph, acoustic)
def test_a_single_path_counts_its_matching_frames_and_has_no_gradient():
    L = make_lattice([(0, 1, 0), (1, 2, 0), (2, 3, 0), (3, 4, 1)], [(0, 1, 5, 0, 0.5, 1.0), (1, 2, 6, 0, 0.25, 0.0), (2, 3, 7, 0, 0.5, 2.0)])
    r = sequence_stats(L, [5, 9, 7])
    assert r["tot_acc"] == 2.0 and r["n_frames"] == 3 and r["n_ref_frames"] == 3 and r["n_dropped"] == 0
    assert r["classes"].tolist() == [5, 6, 7] and r["posts"].tolist() == [1.0, 1.0, 1.0] and r["values"].tolist() == [0.0, 0.0, 0.0]
    m = sequence_stats(L, [5, 9, 7], "mmi")     # frame 1: the reference (9) is outside the lattice: its own entry, after class 6
    assert m["tot_acc"] == 0.0 and m["frame_off"].tolist() == [0, 1, 3, 4] and m["classes"].tolist() == [5, 6, 9, 7]
    assert m["posts"].tolist() == [1.0, 1.0, 0.0, 1.0] and m["values"].tolist() == [0.0, -1.0, 1.0, 0.0]
    d = sequence_stats(L, [5, 9, 7], "mmi", drop_frames=True)
    assert d["n_dropped"] == 1 and d["classes"].tolist() == [5, 6, 7] and d["values"].tolist() == [0.0, 0.0, 0.0]
    # drop_frames is MMI's: sMBR does not look at it
    assert sequence_stats(L, [5, 9, 7], drop_frames=True)["n_dropped"] == 0


def test_two_parallel_arcs_of_equal_cost_one_of_them_correct():
    L = make_lattice([(0, 1, 0), (1, 2, 1)], [(0, 1, 4, 5, 0.5, 0.5), (0, 1, 9, 6, 0.5, 0.5)])
    r = sequence_stats(L, [9])
    # two paths of weight 1/2; accuracies 0 and 1: tot 0.5; w = 0.5 * (acc - 0.5)
    assert r["tot_acc"] == 0.5 and r["classes"].tolist() == [4, 9] and r["posts"].tolist() == [0.5, 0.5] and r["values"].tolist() == [-0.25, 0.25]
    m = sequence_stats(L, [9], "mmi")
    assert m["classes"].tolist() == [4, 9] and m["values"].tolist() == [-0.5, 0.5]


def test_an_epsilon_chain_inside_a_frame():
    # 0 -5-> 1 -eps-> 2 -eps-> 3 -6-> 5, and 1 -7-> 4 (final); both of cost 1 after state 1: fa passes through two levels of frame 1
    L = make_lattice([(0, 1, 0), (1, 2, 0), (1, 3, 0), (1, 4, 0), (2, 5, 1), (2, 6, 1)],
                     [(0, 1, 5, 0, 0.5, 0.5), (1, 2, 0, 3, 0.25, 0.0), (2, 3, 0, 0, 0.25, 0.0), (3, 5, 6, 0, 0.25, 0.25), (1, 4, 7, 0, 0.5, 0.5)])
    r = sequence_stats(L, [5, 6])
    # paths: 5,6 (cost 2, acc 2) and 5,7 (cost 2, acc 1): tot 1.5; frame 0: one class, value 0; frame 1: +-0.25
    assert close(r["tot_acc"], 1.5) and r["classes"].tolist() == [5, 6, 7]
    assert close(r["values"][0], 0.0) and close(r["values"][1], 0.25) and close(r["values"][2], -0.25)
    assert close(r["fa"][3], 1.0) and close(r["fb"][1], 0.5) and close(r["fb"][2], 1.0)


def test_a_final_state_with_an_out_arc():
    L = make_lattice([(0, 1, 0), (1, 2, 1), (2, 3, 1)], [(0, 1, 1, 5, 1.0, 0.0), (1, 2, 2, 6, 0.5, 0.5)])
    # the paths: one arc (cost 1, acc 1), both arcs (cost 2, acc 2)
    p2 = 1.0 / (E + 1.0)
    r = sequence_stats(L, [1, 2])
    assert close(r["tot_acc"], 1.0 + p2)
    # frame 0: every path takes the arc: value = E[acc] - tot = 0; frame 1: p2 * (2 - tot)
    assert close(r["values"][0], 0.0) and close(r["values"][1], p2 * (1.0 - p2)) and close(r["posts"][1], p2)


def test_a_dead_end_and_an_infinite_arc_drop_out():
    L = make_lattice([(0, 1, 0), (1, 2, 0), (1, 3, 0), (1, 4, 0), (2, 5, 1)],
                     [(0, 1, 1, 5, 0.5, 0.5), (0, 2, 2, 5, 0.5, 0.5), (1, 4, 3, 6, 0.5, 0.5), (0, 1, 4, 5, np.inf, 0.0), (3, 4, 5, 6, 0.5, 0.5)])
    r = sequence_stats(L, [2, 3])       # the reference's class 2 sits on the dead end only
    assert r["tot_acc"] == 1.0 and r["classes"].tolist() == [1, 3] and r["values"].tolist() == [0.0, 0.0]
    m = sequence_stats(L, [2, 3], "mmi")
    assert m["classes"].tolist() == [1, 2, 3] and m["values"].tolist() == [-1.0, 1.0, 0.0] and m["posts"].tolist() == [1.0, 0.0, 1.0]
    assert sequence_stats(L, [2, 3], "mmi", drop_frames=True)["n_dropped"] == 1
    L.st_final[:] = 0       # no path at all
    z = sequence_stats(L, [2, 3])
    assert z["n_frames"] == 2 and z["frame_off"].tolist() == [0, 0, 0] and z["tot_acc"] == 0.0


def test_unlabelled_frames_and_references_longer_and_shorter_than_the_lattice():
    L = make_lattice([(0, 1, 0), (1, 2, 0), (2, 3, 1)], [(0, 1, 4, 0, 0.5, 0.5), (0, 1, 9, 0, 0.5, 0.5), (1, 2, 4, 0, 0.5, 0.5), (1, 2, 9, 0, 0.5, 0.5)])
    a = sequence_stats(L, [9, -1])
    b = sequence_stats(L, [9])
    c = sequence_stats(L, [9, -3, 4, 4, 4])
    for r in (a, b):
        assert r["n_ref_frames"] == 1 and r["tot_acc"] == 0.5 and r["values"].tolist() == [-0.25, 0.25, 0.0, 0.0]
    assert c["n_ref_frames"] == 1 and c["values"].tolist() == a["values"].tolist()
    m = sequence_stats(L, [9], "mmi")
    assert m["values"].tolist() == [-0.5, 0.5, 0.0, 0.0] and m["n_ref_frames"] == 1
    assert sequence_stats(L, [], "mmi")["n_ref_frames"] == 0 and not sequence_stats(L, [])["values"].any()
    n = sequence_stats(None, [1, 2])
    assert n["n_frames"] == 0 and compare(dict(n), n, None, None, [1, 2]) == 0.0


def test_a_silence_class_on_either_side():
    L = make_lattice([(0, 1, 0), (1, 2, 1)], [(0, 1, 4, 5, 0.5, 0.5), (0, 1, 9, 6, 0.5, 0.5)])
    assert sequence_stats(L, [9], sil_classes=[9])["tot_acc"] == 0.0       # the reference (and so the matching arc) is silence
    assert sequence_stats(L, [9], sil_classes=[4])["tot_acc"] == 0.5       # another class being silence changes nothing
    m = np.array([0, 0, 0, 0, 2, 0, 0, 0, 0, 3], np.int32)                 # tid 4 -> 2, tid 9 -> 3
    assert sequence_stats(L, [3], label_map=m, sil_classes=[3])["tot_acc"] == 0.0
    assert sequence_stats(L, [3], label_map=m, sil_classes=[2])["tot_acc"] == 0.5
    # MMI does not look at the silence list
    assert sequence_stats(L, [9], "mmi", sil_classes=[9])["values"].tolist() == [-0.5, 0.5]


# ---- random small lattices against the enumeration of every path -------------------------------------------------------------------
def cases():
    for seed in range(300):
        rs = np.random.RandomState(seed)
        L = random_lattice(rs, seed % 2 == 0)
        if L is None:
            continue
        yield seed, rs, L


def test_random_lattices_against_every_path():
    n = 0
    worst = 0.0
    for seed, rs, L in cases():
        paths = all_paths(L)
        nf = int(L.st_frame.max())
        ref = rs.randint(1, 4, size=nf + 1)
        for scale in (1.0, 0.1):
            P = posteriors(L, scale, scale)
            if not np.isfinite(P["log_z"]):
                continue
            n += 1
            r = sequence_stats(L, ref, "smbr", scale, scale, post=P)
            tot, w = brute_force(L, paths, r["acc"], scale, scale)
            assert abs(r["tot_acc"] - tot) <= 1e-12, seed
            assert np.abs(r["w"] - w).max(initial=0.0) <= 1e-12, seed
            fr = L.st_frame[L.a_src].astype(np.int64)
            for f in range(r["n_frames"]):
                for v, x in r["value"][f].items():
                    want = w[(L.a_il > 0) & (fr == f) & (L.a_il == v)].sum()
                    assert abs(x - want) <= 1e-12, (seed, f, v)
                    worst = max(worst, abs(x - want))
            # the restatement's own error is far inside the tolerance the device is held to
            assert abs(r["tot_acc"] - tot) <= 0.01 * tol_acc(P, L) + 1e-14
    assert n > 300
    print("cases", n, "worst value difference", worst)


def test_invariants_on_random_lattices():
    for seed, rs, L in cases():
        nf = int(L.st_frame.max())
        ref = rs.randint(1, 4, size=nf + 1)
        P = posteriors(L)
        if not np.isfinite(P["log_z"]):
            continue
        r = sequence_stats(L, ref, post=P)
        fp = frame_posteriors(L, post=P)
        # tot_acc is the reference's posterior mass, frame by frame
        assert abs(r["tot_acc"] - sum(fp["mass"][f].get(int(ref[f]), 0.0) for f in range(nf))) <= 1e-12
        assert np.array_equal(r["classes"], fp["classes"]) and np.array_equal(r["posts"], fp["posts"]) and np.array_equal(r["frame_off"], fp["frame_off"])
        # every complete path crosses every frame where all final states lie in the last one: the values of a frame sum to zero
        if all(int(L.st_frame[s]) == nf for s in np.nonzero(L.st_final)[0]):
            for f in range(nf):
                assert abs(sum(r["value"][f].values())) <= 1e-12
        m = sequence_stats(L, ref, "mmi", post=P)
        for f in range(nf):
            lo, hi = m["frame_off"][f], m["frame_off"][f + 1]
            for v, p, x in zip(m["classes"][lo:hi], m["posts"][lo:hi], m["values"][lo:hi]):
                assert p == fp["mass"][f].get(int(v), 0.0) and x == (1.0 if v == ref[f] else 0.0) - p     # exactly


def some_lattice():
    for seed, rs, L in cases():
        nf = int(L.st_frame.max())
        P = posteriors(L)
        if nf >= 3 and np.isfinite(P["log_z"]) and len(L.a_src) > 8:
            ref = rs.randint(1, 4, size=nf)
            r = sequence_stats(L, ref, post=P)
            if len(r["classes"]) > nf + 1 and min(abs(x) for x in r["values"]) > 1e-3:
                return L, P, ref, r
    raise AssertionError("no lattice")


def test_one_changed_reference_frame_moves_tot_acc_by_far_more_than_the_tolerance():
    L, P, ref, r = some_lattice()
    moved = 0
    for f in range(len(ref)):
        other = np.array(ref)
        other[f] = other[f] % 3 + 1
        d = abs(sequence_stats(L, other, post=P)["tot_acc"] - r["tot_acc"])
        if d > 0.0:
            assert d > 1000.0 * tol_acc(P, L)
            moved += 1
    assert moved


def test_compare_rejects_what_it_must():
    L, P, ref, r = some_lattice()
    got = lambda: {k: copy.deepcopy(v) for k, v in r.items()}
    assert compare(got(), r, P, L, ref) == 0.0
    g = got()
    g["values"][1] = -g["values"][1]                       # a flipped sign
    with pytest.raises(AssertionError):
        compare(g, r, P, L, ref)
    g = got()                                              # a dropped entry
    k = int(np.nonzero(np.diff(r["frame_off"]) > 1)[0][0])
    at = int(r["frame_off"][k])
    for key in ("classes", "posts", "values"):
        g[key] = np.delete(g[key], at)
    g["frame_off"] = g["frame_off"].copy()
    g["frame_off"][k + 1:] -= 1
    with pytest.raises(AssertionError):
        compare(g, r, P, L, ref)
    g = got()                                              # a swapped pair
    for key in ("classes", "posts", "values"):
        g[key][[at, at + 1]] = g[key][[at + 1, at]]
    with pytest.raises(AssertionError):
        compare(g, r, P, L, ref)
    g = got()
    g["n_dropped"] = 1                                     # a wrong n_dropped
    with pytest.raises(AssertionError):
        compare(g, r, P, L, ref)
    g = got()
    g["tot_acc"] += 2.0 * tol_acc(P, L)
    with pytest.raises(AssertionError):
        compare(g, r, P, L, ref)
    g = got()
    g["values"][0] += 2.0 * tol_value(P, L, g["values"][0])
    with pytest.raises(AssertionError):
        compare(g, r, P, L, ref)
    m = sequence_stats(L, ref, "mmi", post=P)
    gm = {k: copy.deepcopy(v) for k, v in m.items()}
    assert compare(gm, m, P, L, ref) == 0.0
    gm["values"][0] += 1e-6
    with pytest.raises(AssertionError):
        compare(gm, m, P, L, ref)
