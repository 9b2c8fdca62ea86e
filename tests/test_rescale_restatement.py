"""CPU: the definition of wfst_decoder_rescaled_words as tests/rescale_util.py restates it -- first on hand-made lattices whose
answers are worked out from the arcs, then against the enumeration of every path on 300 random small lattices (negative costs
included), then on the C oracle's raw lattices: at (1, 1, 0) the best path is the decoder's own where the lattice holds no near tie."""
import numpy as np
import pytest

import pyoracle
from align_util import align, make_lattice
from rescale_util import (all_paths, arc_key, bits32, bits64, candidates, cells, path_outputs, renumber, rescale, rescale_many,
                          sequential_cost)

F32, F64 = np.float32, np.float64


# states (frame, graph state, final); arcs (src, dst, ilabel, olabel, graph, acoustic)
def diamond(upper, lower, gstates=(2, 3)):
    """two paths of two arcs: the upper carries ONE word (5, on its first arc), the lower TWO (6 and 7); upper / lower = (graph,
    acoustic) of each of the path's two arcs"""
    return make_lattice([(0, 1, 0), (1, gstates[0], 0), (1, gstates[1], 0), (2, 4, 1)],
                        [(0, 1, 1, 5, upper[0], upper[1]), (1, 3, 2, 0, upper[0], upper[1]),
                         (0, 2, 3, 6, lower[0], lower[1]), (2, 3, 4, 7, lower[0], lower[1])])


def test_the_penalty_flips_the_answer_at_the_threshold_the_arcs_give():
    L = diamond((1.0, 1.0), (0.75, 1.0))
    # one word at 2 * (1 + 1) = 4.0 against two words at 2 * (0.75 + 1) = 3.5: the paths cost 4 + wip and 3.5 + 2 wip, equal at 0.5
    upper, lower = 2 * (1.0 + 1.0), 2 * (0.75 + 1.0)
    thr = upper - lower
    assert thr == 0.5
    below, above = rescale(L, 1.0, 1.0, thr - 0.25), rescale(L, 1.0, 1.0, thr + 0.25)
    assert below["words"].tolist() == [6, 7] and below["arcs"].tolist() == [2, 3] and below["scaled_cost"] == lower + 2 * (thr - 0.25)
    assert above["words"].tolist() == [5] and above["arcs"].tolist() == [0, 1] and above["scaled_cost"] == upper + (thr + 0.25)
    assert not below["tie"] and not above["tie"]
    # at the threshold itself both arrive at the end with 4.5: the tie rule takes the arc whose source token has the lower graph state
    assert rescale(L, 1.0, 1.0, thr)["arcs"].tolist() == [0, 1] and rescale(L, 1.0, 1.0, thr)["tie"]
    assert rescale(diamond((1.0, 1.0), (0.75, 1.0), (3, 2)), 1.0, 1.0, thr)["arcs"].tolist() == [2, 3]
    # a negative penalty favours the path with more words
    assert rescale(L, 1.0, 1.0, -3.0)["words"].tolist() == [6, 7] and rescale(L, 1.0, 1.0, -3.0)["scaled_cost"] == lower - 6.0
    # the scores that come with a path are its own, unscaled
    assert bits32(above["tot"]) == bits32(4.0) and bits32(above["lm"]) == bits32(2.0) and above["begin"].tolist() == [0] and above["end"].tolist() == [2]
    assert bits32(below["tot"]) == bits32(3.5) and bits32(below["lm"]) == bits32(1.5) and below["begin"].tolist() == [0, 1] and below["end"].tolist() == [1, 2]
    assert above["tids"].tolist() == [1, 2] and below["tids"].tolist() == [3, 4]


def test_a_zero_graph_scale_takes_the_acoustically_best_path_and_a_zero_acoustic_scale_the_best_by_graph():
    L = diamond((1.0, 3.0), (2.0, 1.0))     # the upper is better by graph (2 against 4), the lower acoustically (2 against 6)
    g0, a0, both = rescale(L, 0.0, 1.0, 0.0), rescale(L, 1.0, 0.0, 0.0), rescale(L, 1.0, 1.0, 0.0)
    assert g0["words"].tolist() == [6, 7] and g0["scaled_cost"] == 2.0
    assert a0["words"].tolist() == [5] and a0["scaled_cost"] == 2.0
    assert both["words"].tolist() == [6, 7] and both["scaled_cost"] == 6.0
    # in between: 2 gs + 6 as against 4 gs + 2 as
    assert rescale(L, 1.0, 0.25, 0.0)["words"].tolist() == [5] and rescale(L, 1.0, 0.25, 0.0)["scaled_cost"] == 3.5
    assert bits32(g0["tot"]) == bits32(6.0) and bits32(g0["lm"]) == bits32(4.0), "tot and lm stay unscaled"


def test_a_word_on_an_arc_inside_a_frame_pays_the_penalty():
    L = make_lattice([(0, 10, 0), (1, 11, 0), (1, 12, 0), (2, 13, 1)],
                     [(0, 1, 5, 0, 0.5, 1.0), (1, 2, 0, 7, 0.25, 0.0), (1, 2, 0, 0, 0.5, 0.0), (2, 3, 6, 0, 0.5, 2.0)])
    # through the word: 1.5 + 0.25 + 2.5 = 4.25 (+ wip); past it: 1.5 + 0.5 + 2.5 = 4.5
    r = rescale(L, 1.0, 1.0, 0.0)
    assert r["words"].tolist() == [7] and r["scaled_cost"] == 4.25 and r["begin"].tolist() == [1] and r["end"].tolist() == [2] and r["n_arcs"] == 3
    assert r["tids"].tolist() == [5, 6]
    r = rescale(L, 1.0, 1.0, 0.5)
    assert r["words"].tolist() == [] and r["scaled_cost"] == 4.5 and r["arcs"].tolist() == [0, 2, 3]
    r = rescale(L, 1.0, 1.0, 0.25)          # 4.5 either way: the same source, ilabel 0 both, the lower olabel wins
    assert r["tie"] and r["arcs"].tolist() == [0, 2, 3]


def test_an_arc_that_is_not_finite_is_no_arc():
    inf, big = float("inf"), 3e38
    # the middle state is reached over a proper arc (3.0), over an arc of infinite graph cost, and over one whose float32 graph +
    # acoustic overflows although its scaled float64 cost at (0.001, 0.001) would be the cheapest
    L = make_lattice([(0, 1, 0), (1, 2, 0), (2, 3, 1)],
                     [(0, 1, 1, 5, 1.0, 2.0), (0, 1, 2, 6, inf, 0.0), (0, 1, 3, 7, big, big), (0, 1, 4, 8, -big, -big), (1, 2, 9, 0, 1.0, 1.0)])
    for gs, as_ in ((1.0, 1.0), (0.001, 0.001), (0.0, 1.0), (0.0, 0.0)):
        r = rescale(L, gs, as_, 0.0)
        assert r["found"] and r["arcs"].tolist() == [0, 4] and r["words"].tolist() == [5], (gs, as_)
        assert r["scaled_cost"] == (gs * 1.0 + as_ * 2.0) + (gs * 1.0 + as_ * 1.0)
    # finite arcs whose scaled sum with the cell is not finite are no transition: 1.7e308 + 1.7e308
    M = make_lattice([(0, 1, 0), (1, 2, 0), (2, 3, 1)], [(0, 1, 1, 0, 1e38, 0.0), (1, 2, 2, 0, 1e38, 0.0)])
    assert np.isfinite(1.7e270 * float(F32(1e38))) and not rescale(M, 1.7e270, 1.0, 0.0)["found"]
    assert rescale(M, 1.0, 1.0, 0.0)["arcs"].tolist() == [0, 1]


def test_no_final_state_reached_and_the_least_graph_state_among_equal_finals():
    inf = float("inf")
    L = make_lattice([(0, 1, 0), (1, 2, 0), (1, 3, 1)], [(0, 1, 1, 5, 1.0, 1.0), (0, 2, 2, 6, inf, 0.0)])
    assert not rescale(L, 1.0, 1.0, 0.0)["found"], "the final state lies behind an arc that is none"
    assert not rescale(make_lattice([(0, 1, 0), (1, 2, 0)], [(0, 1, 1, 5, 1.0, 1.0)]), 1.0, 1.0, 0.0)["found"], "no final state at all"
    for gstates, want in (((7, 4), 1), ((4, 7), 0)):
        F = make_lattice([(0, 1, 0), (1, gstates[0], 1), (1, gstates[1], 1)], [(0, 1, 1, 5, 1.0, 1.0), (0, 2, 2, 6, 0.5, 1.5)])
        r = rescale(F, 1.0, 1.0, 0.0)
        assert r["tie"] and r["arcs"].tolist() == [want] and r["end_state"] == want + 1
        assert rescale(F, 1.0, 0.0, 0.0)["arcs"].tolist() == [1], "no tie: the cheaper end"


def test_a_negative_zero_sum_compares_equal_to_a_positive_one():
    nz = -0.0
    # the upper path sums 1.5 - 1.5; the lower one -0.0 arcs with a penalty of -0.0 on its words: both cells are +0.0
    L = make_lattice([(0, 1, 0), (1, 3, 0), (1, 2, 0), (2, 4, 1)],
                     [(0, 1, 1, 0, 1.5, 0.0), (1, 3, 2, 0, -1.5, 0.0), (0, 2, 3, 6, nz, nz), (2, 3, 4, 7, nz, nz)])
    r = rescale(L, 1.0, 1.0, nz)
    assert r["found"] and r["tie"] and bits64(r["scaled_cost"]) == bits64(0.0)
    assert r["arcs"].tolist() == [2, 3], "the lower path's source token has the lower graph state"
    v, c, _ = cells(L, [(1.0, 1.0, nz)])
    assert [bits64(x) for x in v[:, 0]] == [bits64(0.0), bits64(1.5), bits64(0.0), bits64(0.0)] and bits64(c[2, 0]) == bits64(nz)


def random_lattice(rs, quantised):
    """2..5 frames of 1..3 states; emitting arcs from a frame to the next, arcs inside a frame (ilabel 0) to a higher state, with and
    without words; costs from a handful of quarters (dense exact ties) or arbitrary, of either sign; now and then an arc that is none"""
    T = rs.randint(2, 6)
    frames, states = [[0]], [(0, 0, 0)]
    for f in range(1, T + 1):
        ids = []
        for _ in range(rs.randint(1, 4)):
            ids.append(len(states))
            states.append((f, rs.randint(0, 4), int((f == T and rs.rand() < 0.7) or rs.rand() < 0.05)))
        frames.append(ids)
    if not any(s[2] for s in states):
        states[-1] = (T, states[-1][1], 1)
    draw = (lambda: 0.25 * rs.randint(-2, 5)) if quantised else (lambda: float(F32(rs.normal(1.0, 2.0))))
    cost = lambda: float("inf") if rs.rand() < 0.02 else draw()
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


SETTINGS = [(1.0, 1.0, 0.0), (1.0, 0.1, 0.0), (0.1, 1.0, 0.5), (1.0, 0.0, -0.25), (0.0, 1.0, 0.25), (0.0, 0.0, 1.0), (0.0, 0.0, 0.0),
            (1.0, 1.0, -3.0), (0.7, 1.3, 0.3)]


def check_against_every_path(L, setting, r):
    """rescale()'s answer against the enumeration; returns whether the times were checked through align()"""
    costs = [(sequential_cost(L, p, setting), p) for p in all_paths(L)]
    costs = [(x, p) for x, p in costs if x is not None]
    assert r["found"] == bool(costs)
    if not costs:
        return False
    least = min(x for x, _ in costs)
    assert bits64(r["scaled_cost"]) == bits64(least), "the enumerated minimum, bit for bit"
    arcs = r["arcs"].tolist()
    # a complete path with that sequential sum
    assert (len(arcs) == 0 and L.st_final[0]) or (L.a_src[arcs[0]] == 0 and L.st_final[L.a_dst[arcs[-1]]])
    assert all(L.a_dst[a] == L.a_src[b] for a, b in zip(arcs, arcs[1:]))
    assert bits64(sequential_cost(L, arcs, setting)) == bits64(least)
    # the end: no final state with the same cell and a lower graph state; every step: no qualifying arc with a smaller key
    v, c, is_arc = cells(L, [setting])
    e = r["end_state"]
    assert e == (int(L.a_dst[arcs[-1]]) if arcs else 0)
    for s in np.nonzero(L.st_final)[0]:
        assert not (v[s, 0] < v[e, 0]) and not (v[s, 0] == v[e, 0] and L.st_gstate[s] < L.st_gstate[e])
    by_dst = np.argsort(L.a_dst, kind="stable")
    first = np.searchsorted(L.a_dst[by_dst], np.arange(L.n_states + 1))
    gb, ab = L.a_graph.astype(F32).view(np.uint32), L.a_ac.astype(F32).view(np.uint32)
    for a in arcs:
        cands = candidates(L, int(L.a_dst[a]), v[:, 0], c[:, 0], is_arc, by_dst, first)
        assert a in cands and all(arc_key(L, a, gb, ab) <= arc_key(L, b, gb, ab) for b in cands)
    # the times and sums: align()'s on the returned words where it picks the same arcs, from the arcs themselves otherwise
    al = align(L, r["words"].tolist())
    if al["found"] and al["arcs"].tolist() == arcs:
        assert np.array_equal(al["begin"], r["begin"]) and np.array_equal(al["end"], r["end"]) and al["n_arcs"] == r["n_arcs"]
        assert bits32(al["tot"]) == bits32(r["tot"]) and bits32(al["lm"]) == bits32(r["lm"])
        return True
    word_at = [i for i, a in enumerate(arcs) if L.a_ol[a] != 0]
    assert r["words"].tolist() == [int(L.a_ol[arcs[i]]) for i in word_at]
    assert r["begin"].tolist() == [int(L.st_frame[L.a_src[arcs[i]]]) for i in word_at]
    assert r["end"].tolist() == r["begin"].tolist()[1:] + [int(L.st_frame[e])] if word_at else len(r["end"]) == 0
    tot, lm = F32(0.0), F32(0.0)
    with np.errstate(all="ignore"):
        for a in arcs:
            tot = F32(tot + F32(L.a_graph[a] + L.a_ac[a]))
            lm = F32(lm + L.a_graph[a])
    assert bits32(tot + F32(0.0)) == bits32(r["tot"]) and bits32(lm) == bits32(r["lm"]) and r["n_arcs"] == len(arcs)
    assert r["tids"].tolist() == [int(L.a_il[a]) for a in arcs if L.a_il[a] != 0]
    return False


def test_random_lattices_against_every_path():
    rs = np.random.RandomState(23)
    n = n_found = n_ties = n_aligned = n_direct = n_negative = 0
    while n < 300:
        L = random_lattice(rs, quantised=n % 2 == 0)
        if L is None:
            continue
        n += 1
        picks = [SETTINGS[i] for i in rs.choice(len(SETTINGS), 3, replace=False)]
        for setting, r in zip(picks, rescale_many(L, picks)):
            via_align = check_against_every_path(L, setting, r)
            if r["found"]:
                n_found += 1
                n_ties += r["tie"]
                n_aligned += via_align
                n_direct += not via_align
                n_negative += r["scaled_cost"] < 0
    print("300 lattices, %d answers found, %d with a tie, %d negative costs; times checked through align() %d, from the arcs %d"
          % (n_found, n_ties, n_negative, n_aligned, n_direct))
    assert n_found > 600 and n_ties > 100 and n_negative > 20 and n_aligned > 100 and n_direct > 20


def test_where_every_path_ties_the_rule_alone_decides_whatever_the_numbering():
    """setting (0, 0, 0): every cell is +0.0 and every arc qualifies; the answer is the same path under a random renumbering of the
    states (a random topological order) and a random permutation of the arcs -- and so is every other setting's"""
    rs = np.random.RandomState(5)
    rng = np.random.default_rng(7)
    n = moved = 0
    while n < 60:
        L = random_lattice(rs, quantised=True)
        if L is None:
            continue
        # distinct graph states inside a frame: a tie that survives the whole key is unspecified, as on biglm lattices
        L.st_gstate = rs.permutation(L.n_states).astype(np.int32)
        n += 1
        M, new_of, perm = renumber(L, rng)
        moved += int(not np.array_equal(new_of, np.arange(L.n_states)))
        for a, b in zip(rescale_many(L, SETTINGS), rescale_many(M, SETTINGS)):
            assert a["found"] == b["found"]
            if not a["found"]:
                continue
            assert bits64(a["scaled_cost"]) == bits64(b["scaled_cost"])
            if a["ambiguous"]:
                continue    # (two parallel arcs that agree in every field of the key)
            assert perm[b["arcs"]].tolist() == a["arcs"].tolist() and new_of[a["end_state"]] == b["end_state"]
            for key in ("words", "begin", "end", "tids"):
                assert np.array_equal(a[key], b[key]), key
        z = rescale(L, 0.0, 0.0, 0.0)
        if z["found"]:
            assert bits64(z["scaled_cost"]) == bits64(0.0)
    assert moved > 30


GRAPHS = [(3000, 21), (600, 5)]
UTTS = [(40, 700), (97, 701), (150, 702)]


@pytest.fixture(scope="module")
def lattices(oracle, synth, tmp_path_factory):
    """(what, lattice, best path) of the twelve inputs test_align_restatement.py builds: two graphs, lattice_beam 4 and 8, three
    utterances (order-free mode)"""
    out = []
    tmp = tmp_path_factory.mktemp("rescale")
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


def test_oracle_lattices_at_the_search_scales(lattices):
    n = exact = 0
    for what, L, bp in lattices:
        assert L.ok and bp.ok and np.all(L.a_dst > L.a_src), what
        res = rescale_many(L, SETTINGS)
        r = res[0]
        assert r["found"], what
        # the decoder's best path is one of the lattice's paths: its float64 sequential cost at (1, 1, 0) bounds the minimum
        x = F64(0.0)
        for g, a in zip(np.asarray(bp.path_graph, F32), np.asarray(bp.path_ac, F32)):
            x = (x + ((1.0 * F64(g) + 1.0 * F64(a)) + 0.0)) + 0.0
        assert r["scaled_cost"] <= x, (what, r["scaled_cost"], x)
        paths = pyoracle.nshortest_paths(L, 2)
        if len(paths) < 2 or float(paths[1]["tot"]) - float(paths[0]["tot"]) > 1e-3:
            exact += 1
            assert r["words"].tolist() == [int(w) for w in bp.words], what
        # every setting's path is a complete path that adds up to its cell, and a penalty moves the word count the right way
        for setting, s in zip(SETTINGS, res):
            assert s["found"] and bits64(sequential_cost(L, s["arcs"], setting)) == bits64(s["scaled_cost"]), (what, setting)
            o = path_outputs(L, s["arcs"], s["end_state"])
            assert np.array_equal(o["words"], s["words"]) and len(s["tids"]) == int(L.st_frame[s["end_state"]])
        assert len(res[7]["words"]) >= len(res[0]["words"]), "a penalty of -3 never takes words away"
        n += 1
    print("%d of %d lattices have no second path within 1e-3 of the first" % (exact, n))
    assert n == 12 and 2 * exact >= n
