"""CPU: the numpy restatement of wfst_decoder_force_align (tests/force_align_util.py) against the enumeration of every path on random
small graphs, and against the oracle at a beam under which nothing is pruned.  No device."""
import os
import re

import numpy as np
import pytest

import force_align_util as U

N_SMALL = 320


def _small_cases():
    """N_SMALL graphs of <= 8 states with T <= 5: epsilon chains, epsilon weights of either sign, scores with -inf, +inf and NaN
    among them, the final state unreachable in some."""
    rng = np.random.default_rng(20261)
    cases = []
    for k in range(N_SMALL):
        g = U.random_small_graph(rng)
        T = int(rng.integers(0, 6))
        ll = rng.normal(-2.0, 1.5, size=(max(T, 1), 5)).astype(np.float32)
        if k % 4 == 0:   # non-finite scores
            bad = rng.random(ll.shape) < 0.15
            ll[bad] = rng.choice(np.array([-np.inf, np.inf, np.nan], np.float32), size=int(bad.sum()))
        cases.append((g, ll, T))
    return cases


def _header_constant():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "wfst_decoder.h")).read()
    return int(re.search(r"#define WFST_FALIGN_LDS_STATES (\d+)", hdr).group(1))


@pytest.fixture(scope="module")
def small():
    # (what is restated here is the header's section on wfst_decoder_force_align: without it there is nothing to restate)
    assert _header_constant() == U.WFST_FALIGN_LDS_STATES
    out = []
    for g, ll, T in _small_cases():
        out.append((g, ll, T, U.force_align(g, ll, T), U.enumerate_paths(g, ll, T)))
    return out


def test_the_cases_cover_what_they_should(small):
    assert len(small) >= 300
    assert all(g.n_states <= 8 and T <= 5 for g, _, T, _, _ in small)
    found = sum(1 for _, _, _, r, _ in small if r["found"])
    assert 0.2 * len(small) < found < 0.95 * len(small)               # the final state reached in many, not in all
    assert any(int(U.eps_levels(g).max()) >= 3 for g, _, _, _, _ in small)    # epsilon chains
    assert any((g.arcs["w"][g.arcs["ilabel"] == 0] < 0).any() for g, _, _, _, _ in small)
    assert any(not np.isfinite(ll).all() for _, ll, _, _, _ in small)
    assert any(T == 0 and r["found"] for _, _, T, r, _ in small)
    # a negative epsilon weight on the winning path of some case
    assert any(r["found"] and any(g.arcs["ilabel"][k] == 0 and g.arcs["w"][k] < 0 for k in r["hop_arc"]) for g, _, _, r, _ in small)


def test_cost_is_the_least_enumerated_path_cost_bit_for_bit(small):
    for i, (g, ll, T, r, paths) in enumerate(small):
        assert r["found"] == bool(paths), i
        if paths:
            best = min(c for c, _ in paths)
            assert U.bits(r["path_cost"]) == U.bits(best), (i, r["path_cost"], best)


def test_path_is_an_enumerated_path_of_that_cost_and_the_one_where_unique(small):
    unique = 0
    for i, (g, ll, T, r, paths) in enumerate(small):
        if not paths:
            continue
        best = min(c for c, _ in paths)
        at_best = [h for c, h in paths if U.bits(c) == U.bits(best)]
        mine = tuple(int(k) for k in r["hop_arc"])
        assert mine in at_best, i
        if len(at_best) == 1:
            unique += 1
            assert at_best[0] == mine, i
        # the outputs restate the hop list
        s = U.path_sums(g, ll, mine)
        assert U.bits(s["seq_cost"]) == U.bits(r["path_cost"]), i
        assert len(r["alignment"]) == T and list(r["alignment"]) == [int(g.arcs["ilabel"][k]) for k in mine if g.arcs["ilabel"][k] != 0], i
    assert unique >= 50


def test_the_tie_rule_decides_where_everything_ties():
    assert _header_constant() == U.WFST_FALIGN_LDS_STATES
    # all weights 0, all scores equal: every path costs the same, and the path is the one the rule picks cell by cell -- an emitting
    # arc before an epsilon arc, then the least arc index
    g = U.transcript_graph([3, 4, 5], seed=5, n_tid=6, weights=False)
    T = 14
    ll = np.full((T, 8), -1.0, np.float32)
    r = U.force_align(g, ll, T)
    assert r["found"]
    V, a, src = r["V"], g.arcs, U.sources(g)
    assert all(V[f, s] == f for f in range(T + 1) for s in range(g.n_states) if np.isfinite(V[f, s]))   # every arrival ties
    f, t, forks = T, g.final_state, 0
    for k in reversed(r["hop_arc"]):
        into = []
        for j in range(g.n_arcs):
            pf = f - int(a["ilabel"][j] != 0)
            if a["to"][j] == t and pf >= 0 and np.isfinite(V[pf, src[j]]):
                into.append(j)
        forks += len(into) > 1
        # the winner is the least under (epsilon last, arc index)
        assert k == min(into, key=lambda j: (a["ilabel"][j] == 0, j)), (f, t)
        f -= int(a["ilabel"][k] != 0)
        t = int(src[k])
    assert (f, t) == (0, g.start) and forks >= 5


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------
N_ORACLE = 40


def test_restatement_against_the_oracle_without_pruning(oracle, tmp_path):
    import pyoracle

    assert _header_constant() == U.WFST_FALIGN_LDS_STATES
    oracle.set_tie_rule(1)
    try:
        cfg = pyoracle.Config(beam=1.0e30, max_active=2147483647, min_active=0, lattice_beam=1.0e30)
        rng = np.random.default_rng(77)
        compared = skipped = 0
        for i in range(N_ORACLE):
            n_tid = 12
            g = U.transcript_graph([int(w) for w in rng.integers(1, 9, size=int(rng.integers(1, 4)))], seed=1000 + i, n_tid=n_tid)
            T = int(rng.integers(12, 30))
            ll = rng.normal(-2.0, 1.5, size=(T, n_tid + 1)).astype(np.float32)   # continuous costs: exact ties are rare
            r = U.force_align(g, ll, T)
            assert r["found"], i
            path = os.path.join(str(tmp_path), "g%d.flat" % i)
            g.write(path)
            h = oracle.load_graph(path)
            try:
                o = oracle.decode(h, cfg, ll, trace=True)
            finally:
                oracle.free_graph(h)
            assert o.ok, i
            # nothing was pruned: every frame's frontier holds exactly the table's reached cells
            assert list(o.frame_ntoks) == [int(np.isfinite(r["V"][f]).sum()) for f in range(T + 1)], i
            # the cost of the oracle's path in the search's own arithmetic: (cost + acoustic) + graph, hop by hop
            cost = np.float32(0)
            for il, gc, ac in zip(o.path_ilabel, o.path_graph, o.path_ac):
                cost = np.float32(np.float32(cost + ac) + gc) if il != 0 else np.float32(cost + gc)
            assert U.bits(cost) == U.bits(r["path_cost"]), (i, cost, r["path_cost"])
            compared += 1
            if o.extra["ties"] != 0:
                skipped += 1
                continue
            a = g.arcs
            mine = [(int(a["ilabel"][k]), int(a["olabel"][k]), U.bits(a["w"][k])) for k in r["hop_arc"]]
            theirs = [(int(x), int(y), U.bits(z)) for x, y, z in zip(o.path_ilabel, o.path_olabel, o.path_graph)]
            # (the oracle's list opens with the start token's own entry, which has no arc: all zero)
            assert theirs[0] == (0, 0, 0) and mine == theirs[1:], i
            assert U.bits(o.tot_score) == U.bits(r["tot_score"]) and U.bits(o.lm_score) == U.bits(r["lm_score"]), i
            assert list(o.words) == list(r["words"]) and list(o.tids) == list(r["alignment"]), i
        assert compared == N_ORACLE and skipped <= 0.1 * compared, (compared, skipped)
    finally:
        oracle.set_tie_rule(0)
