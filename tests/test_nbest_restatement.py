"""The two restatements of tests/nbest_util.py -- kbest_distinct (nbest_kernel) and kbest_paths_dp (nbest_paths_kernel) -- against
the enumeration of every path, on small random layered lattices built directly (no decoder, no GPU): frames of a few states,
emitting arcs from a frame to the next, epsilon arcs inside a frame (some with words), a few thousand paths at most.

Two families of costs.  QUANTISED: every cost a multiple of 1/8 in [-1, 1]: float32 sums are exact, exact ties are dense.
CONTINUOUS: normal draws of both signs.

What the enumeration can and cannot decide: exact ties at the K-th place of an intermediate state or at the n-th place of the
answer are broken by the history hash (kbest_distinct) or by the candidate number (kbest_paths_dp), which the enumeration does not
know.  Such cases are held to the order-free relation (totals rank by rank, every answer a true one); where the enumeration's
first n + 1 totals are bit-distinct the lists must be IDENTICAL."""
import numpy as np
import pytest

import pyoracle
from nbest_util import F32, ROOT_HASH, f2o, kbest_distinct, kbest_paths_dp, mix_word
from nearest_util import all_paths

bits = lambda x: int(np.asarray(x, F32).view(np.uint32))


def random_lattice(seed, quantised, frames=4, width=3, limit=4000):
    """a layered raw lattice (state 0 the root, ids topological) with at most `limit` paths: thinner draws until it fits"""
    rng = np.random.default_rng(seed)
    cost = (lambda: F32(rng.integers(-8, 9) / 8.0)) if quantised else (lambda: F32(rng.normal(0.0, 1.5)))
    for density in (0.8, 0.65, 0.5, 0.4, 0.3):
        layers, st_frame = [[0]], [0]
        for f in range(1, frames + 1):
            layers.append(list(range(len(st_frame), len(st_frame) + width)))
            st_frame += [f] * width
        arcs = []   # (src, dst, ilabel, olabel, graph, acoustic)
        word = lambda p: int(rng.integers(1, 6)) if rng.random() < p else 0
        for f in range(1, frames + 1):
            for t in layers[f]:
                srcs = [s for s in layers[f - 1] if rng.random() < density] or [int(rng.choice(layers[f - 1]))]
                for s in srcs:
                    for _ in range(int(rng.integers(1, 3))):      # parallel arcs too
                        arcs.append((s, t, int(rng.integers(1, 9)), word(0.6), cost(), cost()))
            for i, s in enumerate(layers[f]):                   # epsilon arcs inside the frame, to higher ids only
                for t in layers[f][i + 1:]:
                    if rng.random() < 0.5 * density:
                        arcs.append((s, t, 0, word(0.4), cost(), F32(0.0)))
        S = len(st_frame)
        fin = np.zeros(S, np.int32)
        fin[[t for t in layers[-1] if rng.random() < 0.7] or [layers[-1][0]]] = 1
        arcs.sort(key=lambda a: (a[0], a[1]))
        col = lambda j, t: np.array([a[j] for a in arcs], t)
        L = pyoracle.RawLattice(True, S, 0, fin, col(0, np.int32), col(1, np.int32), col(2, np.int32), col(3, np.int32), col(4, F32), col(5, F32),
                                np.array(st_frame, np.int32), np.arange(S, dtype=np.int32), np.zeros(S, F32))
        paths = all_paths(L, limit)
        if paths is not None:
            return L, paths
    raise AssertionError("no draw of seed %d has at most %d paths" % (seed, limit))


def path_sums(L, p):
    """(words, tot, lm) of a path: float32 sums front to back, the arc's own cost summed first"""
    tot, lm = F32(0.0), F32(0.0)
    for a in p:
        tot = F32(tot + F32(L.a_graph[a] + L.a_ac[a]))
        lm = F32(lm + L.a_graph[a])
    return tuple(int(L.a_ol[a]) for a in p if L.a_ol[a]), tot, lm


CASES = [(seed, q) for q in (True, False) for seed in range(12)]


@pytest.fixture(scope="module")
def lattices():
    out = {}
    for seed, q in CASES:
        L, paths = random_lattice(100 + seed, q)
        out[(seed, q)] = (L, paths, [path_sums(L, p) for p in paths])
    return out


def _check_distinct(L, sums, n, quantised, what):
    """-> the lists were held to the 'identical' rule"""
    per_seq = {}
    for w, tot, lm in sums:
        per_seq.setdefault(w, []).append((int(f2o(tot)), int(f2o(lm)), tot, lm))
    least = {w: min(v) for w, v in per_seq.items()}
    ranked = sorted(least.items(), key=lambda kv: kv[1][:2])
    got = kbest_distinct(L, n)
    assert len(got) == min(n, 16, len(ranked)), what
    assert [bits(g["tot"]) for g in got] == [bits(v[2]) for _, v in ranked[:len(got)]], what + ": totals rank by rank"
    seqs = [tuple(g["words"].tolist()) for g in got]
    assert len(set(seqs)) == len(seqs), what + ": a sequence twice"
    for g, w in zip(got, seqs):
        assert w in least and g["n_words"] == len(w), what + ": not a sequence of the lattice"
        assert bits(g["tot"]) == bits(least[w][2]), what + ": not the sequence's least tot"
        attaining = [v for v in per_seq[w] if v[0] == least[w][0]]
        if quantised or len(attaining) == 1:
            assert bits(g["lm"]) == bits(least[w][3]), what + ": lm of the least path"
        else:
            assert bits(g["lm"]) in {bits(v[3]) for v in attaining}, what + ": lm of no attaining path"
    head = [v[0] for _, v in ranked[:n + 1]]
    if len(set(head)) < len(head):
        return False
    assert seqs == [w for w, _ in ranked[:len(got)]], what + ": order"
    assert [bits(g["lm"]) for g in got] == [bits(v[3]) for _, v in ranked[:len(got)]], what + ": lm bits"
    return True


@pytest.mark.parametrize("quantised", [True, False], ids=["quantised", "continuous"])
def test_kbest_distinct_against_every_path(lattices, quantised):
    identical = total = truncating = 0
    for seed, q in CASES:
        if q != quantised:
            continue
        L, paths, sums = lattices[(seed, q)]
        st = {}
        kbest_distinct(L, 16, stats=st)
        truncating += int((st["distinct"] > 16).any())
        for n in (1, 2, 5, 15, 16):
            identical += _check_distinct(L, sums, n, quantised, "seed %d n %d" % (seed, n))
            total += 1
    assert truncating >= 4, "too few lattices where a state drops histories: %d" % truncating
    if not quantised:
        assert 2 * identical >= total, "only %d of %d continuous cases are free of ties" % (identical, total)


def _check_paths(L, paths, sums, n, what):
    order = sorted(range(len(paths)), key=lambda i: int(f2o(sums[i][1])))
    got = kbest_paths_dp(L, n)
    assert len(got) == min(n, len(paths)), what
    assert [bits(g["tot"]) for g in got] == [bits(sums[i][1]) for i in order[:len(got)]], what + ": totals rank by rank"
    known = {tuple(p): i for i, p in enumerate(paths)}
    seen = set()
    for g in got:
        key = tuple(g["arcs"].tolist())
        assert key in known and key not in seen, what + ": not a path of the lattice, or one twice"
        seen.add(key)
        assert bits(sums[known[key]][1]) == bits(g["tot"]), what + ": not the path's forward sum"
        assert np.array_equal(g["olabel"], L.a_ol[g["arcs"]]) and np.array_equal(g["graph"], L.a_graph[g["arcs"]]), what
    head = [int(f2o(sums[i][1])) for i in order[:n + 1]]
    if len(set(head)) < len(head):
        return False
    assert [tuple(g["arcs"].tolist()) for g in got] == [tuple(paths[i]) for i in order[:len(got)]], what + ": order"
    return True


def _as_reference_path(p):
    """a path of pyoracle.nshortest_paths in the compiled reference's shape (test_nbest_paths._strip): an epsilon arc in front, two
    free ones behind"""
    z = lambda a, k: np.concatenate([np.zeros(1, a.dtype), a, np.zeros(k, a.dtype)])
    return dict(ilabel=np.zeros(len(p["olabel"]) + 3, np.int32), olabel=z(p["olabel"], 2), graph=z(p["graph"], 2), acoustic=z(p["acoustic"], 2))


@pytest.mark.parametrize("quantised", [True, False], ids=["quantised", "continuous"])
def test_kbest_paths_dp_against_every_path_and_the_best_first_search(lattices, quantised):
    from test_nbest_paths import _same_paths

    identical = total = whole = 0
    for seed, q in CASES:
        if q != quantised:
            continue
        L, paths, sums = lattices[(seed, q)]
        for n in (1, 2, 7, 64, 5000):
            what = "seed %d n %d" % (seed, n)
            identical += _check_paths(L, paths, sums, n, what)
            total += 1
            # test_nbest_paths._same_paths, unchanged.  It compares groups of near-equal totals as sets, so a group that the n-th place
            # cuts in two is undecidable for it (both searches are right to keep any of its paths: _check_paths above has held them to
            # the enumeration): the lists are compared up to that group.
            tots = sorted(float(s[1]) for s in sums)
            k = min(n, len(tots))
            while n < len(tots) and k > 0 and abs(tots[n] - tots[k - 1]) <= 2e-5 * max(1.0, abs(tots[n])):
                k -= 1
            whole += int(k == min(n, len(tots)))
            got = [dict(p, tot=float(p["tot"])) for p in kbest_paths_dp(L, n)[:k]]
            _same_paths(got, [_as_reference_path(p) for p in pyoracle.nshortest_paths(L, n)[:k]], what + " vs nshortest_paths")
    assert 2 * whole >= total, "the n-th place cuts a tie group in %d of %d lists" % (total - whole, total)
    if not quantised:
        assert 2 * identical >= total, (identical, total)


def test_mix_word_is_the_splitmix64_finaliser():
    # splitmix64 from state 0: the first output is the finaliser of the golden-ratio increment
    assert mix_word(0, 0) == 0xE220A8397B1DCDAF
    assert mix_word(ROOT_HASH, 7) != mix_word(ROOT_HASH, 8) and mix_word(mix_word(ROOT_HASH, 7), 8) != mix_word(mix_word(ROOT_HASH, 8), 7)
    assert mix_word(ROOT_HASH, -1) == mix_word(ROOT_HASH, 0xFFFFFFFF)   # the word as 32 unsigned bits


def _hand_made():
    """root -(w5)-> 1, root -(w5)-> 2, root -(w6)-> 2 in frame 1; 1 -eps-> 2 inside frame 1 (no word); 1, 2 -> 3 in frame 2; 3 final.
    arcs: (src, dst, ilabel, olabel, graph, acoustic)"""
    from align_util import make_lattice

    return make_lattice([(0, 0, 0), (1, 1, 0), (1, 2, 0), (2, 3, 1)],
                        [(0, 1, 1, 5, 0.5, 1.0),      # 0: "5" at state 1: tot 1.5 lm 0.5
                         (0, 2, 2, 5, 1.0, 0.5),      # 1: "5" at state 2: tot 1.5 lm 1.0 -- the same history, bit-equal tot, higher lm
                         (0, 2, 3, 6, 0.25, 0.5),     # 2: "6" at state 2: tot 0.75 lm 0.25
                         (1, 2, 0, 0, 0.0, 0.0),      # 3: "5" arrives at state 2 once more: tot 1.5 lm 0.5 -- merged, the lower lm stays
                         (1, 3, 4, 7, 1.0, 1.0),      # 4: "5 7": tot 3.5 lm 1.5
                         (2, 3, 5, 0, 0.5, 0.5),      # 5: "6": 1.75 / 0.75; "5": 2.5 / 1.0
                         (2, 3, 6, 7, 2.0, 0.0)])     # 6: "6 7": 2.75 / 2.25; "5 7": 3.5 / 2.5 -- merged with arc 4's "5 7", lm 1.5 stays


def test_kbest_distinct_hand_made():
    L = _hand_made()
    st = {}
    got = kbest_distinct(L, 16, stats=st)
    assert [(g["words"].tolist(), float(g["tot"]), float(g["lm"])) for g in got] == [([6], 1.75, 0.75), ([5], 2.5, 1.0), ([6, 7], 2.75, 2.25), ([5, 7], 3.5, 1.5)]
    assert st["cands"].tolist() == [0, 1, 3, 5] and st["cnt"].tolist() == [1, 1, 2, 4] and st["merged_lm"].tolist() == [False, False, True, True]
    assert st["final_states"] == 1 and st["final_cands"] == 4 and st["final_distinct"] == 4
    assert [g["words"].tolist() for g in kbest_distinct(L, 2)] == [[6], [5]]
    # K = 1: state 2 keeps "6" alone, state 3 the cheapest of {"5 7" via state 1, "6", "6 7"}
    assert [(g["words"].tolist(), float(g["tot"])) for g in kbest_distinct(L, 3, K=1)] == [([6], 1.75)]
    # max_words cuts the words, not their count
    assert [(g["words"].tolist(), g["n_words"]) for g in kbest_distinct(L, 4, max_words=1)] == [([6], 1), ([5], 1), ([6], 2), ([5], 2)]


def test_kbest_paths_dp_hand_made():
    L = _hand_made()
    st = {}
    got = kbest_paths_dp(L, 10, stats=st)
    # state 2's candidates in q order: arc 1 (1.5), arc 2 (0.75), arc 3 (1.5): list (0.75 arc 2), (1.5 arc 1), (1.5 arc 3) -- the tie by q
    # state 3's: arc 4 (3.5) | arc 5 over state 2's list (1.75, 2.5, 2.5) | arc 6 over it (2.75, 3.5, 3.5)
    assert [(g["arcs"].tolist(), float(g["tot"])) for g in got] == [([2, 5], 1.75), ([1, 5], 2.5), ([0, 3, 5], 2.5), ([2, 6], 2.75), ([0, 4], 3.5),
                                                                    ([1, 6], 3.5), ([0, 3, 6], 3.5)]
    assert st["cands"].tolist() == [0, 1, 3, 7] and st["final_cands"] == 7 and st["level"].tolist() == [0, 1, 2, 3]
    assert [g["arcs"].tolist() for g in kbest_paths_dp(L, 3)] == [[2, 5], [1, 5], [0, 3, 5]]
    # n = 2: state 2 keeps (arc 2, arc 1); the three-arc paths are gone
    assert [g["arcs"].tolist() for g in kbest_paths_dp(L, 2)] == [[2, 5], [1, 5]]
    assert got[0]["olabel"].tolist() == [6, 0] and got[0]["graph"].tolist() == [0.25, 0.5] and got[0]["acoustic"].tolist() == [0.5, 0.5]
