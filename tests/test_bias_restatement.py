"""CPU: the definition of wfst_decoder_biased_words as tests/bias_util.py restates it -- the phrase automaton against naive occurrence
counting, the cells and the traceback against the enumeration of every path on random small lattices, the invariance under a
renumbering of states and arcs, and the J = 1 / bs = 0 cases against rescale_util."""
import numpy as np

import bias_util as B
from align_util import make_lattice
from rescale_util import all_paths, bits32, bits64, renumber, rescale

F32, F64 = np.float32, np.float64


def dyadic(rs):
    return float(rs.randint(0, 17)) / 8.0


def random_list(rs, alphabet=3, most=5, longest=4):
    seen, out = set(), []
    for _ in range(rs.randint(1, most + 1)):
        ws = tuple(int(w) for w in rs.randint(1, alphabet + 1, size=rs.randint(1, longest + 1)))
        if ws not in seen:
            seen.add(ws)
            out.append((ws, dyadic(rs)))
    return out


def check_automaton(phrases, rs, n_seq=20):
    A = B.compile_list(phrases)
    # the numbering: breadth first by (depth, parent's number, word), the root first
    keys = [(int(A.depth[j]), int(A.parent[j]), int(A.word[j])) for j in range(1, A.J)]
    assert keys == sorted(keys) and len(set(keys)) == len(keys) and A.depth[0] == 0
    assert all(A.parent[j] < j and A.fail[j] < j and A.depth[A.fail[j]] < A.depth[j] for j in range(1, A.J))
    assert all(A.fail[j] == 0 for j in range(1, A.J) if A.depth[j] == 1)
    own = {ws: b for ws, b in phrases}
    for j in range(A.J):
        s = A.strs[j]
        # beta(j) = the bonuses of every phrase that is a suffix of str(j) (dyadic: the sums are exact)
        assert A.beta[j] == sum(b for ws, b in phrases if len(ws) <= len(s) and s[len(s) - len(ws):] == ws)
        assert A.own[j] == own.get(s, 0.0) and (A.phrase[j] >= 0) == (s in own)
    alphabet = sorted({w for ws, _ in phrases for w in ws}) + [99]
    for _ in range(n_seq):
        seq = [int(rs.choice(alphabet)) for _ in range(rs.randint(0, 12))]
        nodes, hits = B.track(A, seq)
        naive = B.naive_hits(phrases, seq)
        assert hits == naive, (phrases, seq)
        assert sum(A.beta[j] for j in nodes) == sum(phrases[p][1] for p, _ in naive)
        for k, j in enumerate(nodes):   # the node is the longest suffix of what was read that is a node
            assert A.strs[j] == max((s for s in A.strs if tuple(seq[k + 1 - len(s):k + 1]) == s or not s), key=len)
    return A


def test_the_automaton_counts_every_occurrence():
    rs = np.random.RandomState(3)
    # shared prefixes; a phrase that is a suffix of another; a phrase inside another; a a in a a a; a one-word phrase
    A = check_automaton([((1, 2, 3), 1.0), ((1, 2, 4), 0.5), ((2, 3), 0.25), ((2,), 0.125), ((5, 1, 2, 4, 6), 2.0), ((1, 1), 4.0)], rs)
    assert B.track(A, [1, 2, 3])[1] == [(3, 1), (0, 2), (2, 2)], "nested: the one-word phrase, then the longest first"
    assert B.track(A, [1, 1, 1])[1] == [(5, 1), (5, 2)], "a a in a a a: twice, overlapping"
    assert B.track(A, [5, 1, 2, 4, 6])[1] == [(3, 2), (1, 3), (4, 4)], "a phrase inside another"
    assert A.beta[A.strs.index((1, 2, 3))] == 1.0 + 0.25 and A.strs[A.fail[A.strs.index((1, 2, 3))]] == (2, 3)
    one = check_automaton([((7,), 1.5)], rs)
    assert one.J == 2 and B.track(one, [7, 7, 8, 7])[1] == [(0, 0), (0, 1), (0, 3)]
    assert B.NO_LIST.J == 1 and B.track(B.NO_LIST, [1, 2])[0] == [0, 0]
    for _ in range(150):
        check_automaton(random_list(rs), rs, n_seq=6)


def random_lattice(rs, quantised, words=(0, 0, 1, 2, 3)):
    """2..5 frames of 1..3 states; emitting arcs from a frame to the next, arcs inside a frame (ilabel 0) to a higher state -- chains
    inside a frame, words on them --, final states with out-arcs, costs of either sign, now and then an arc that is none"""
    T = rs.randint(2, 6)
    frames, states = [[0]], [(0, 0, 0)]
    for f in range(1, T + 1):
        ids = []
        for _ in range(rs.randint(1, 4)):
            ids.append(len(states))
            states.append((f, rs.randint(0, 4), int((f == T and rs.rand() < 0.7) or rs.rand() < 0.08)))
        frames.append(ids)
    if not any(s[2] for s in states):
        states[-1] = (T, states[-1][1], 1)
    draw = (lambda: 0.25 * rs.randint(-2, 5)) if quantised else (lambda: float(F32(rs.normal(1.0, 2.0))))
    cost = lambda: float("inf") if rs.rand() < 0.02 else draw()
    word = lambda: int(rs.choice(words))
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


SETTINGS = [(1.0, 1.0, 0.0, 1.0), (1.0, 0.1, 0.0, 2.0), (0.1, 1.0, 0.5, 0.5), (1.0, 0.0, -0.25, 1.0), (0.0, 0.0, 0.0, 1.0), (1.0, 1.0, -3.0, 0.3),
            (0.7, 1.3, 0.3, 0.0), (1.0, 1.0, 0.0, 8.0)]


def check_against_every_path(L, A, phrases, setting, r):
    costs = [(B.sequential_cost(L, A, p, setting), p) for p in all_paths(L)]
    costs = [(x[0], p) for x, p in costs if x is not None]
    assert r["found"] == bool(costs)
    if not costs:
        return
    least = min(x for x, _ in costs)
    assert bits64(r["biased_cost"]) == bits64(least), "the enumerated minimum, bit for bit"
    arcs = r["arcs"].tolist()
    assert (len(arcs) == 0 and L.st_final[0]) or (L.a_src[arcs[0]] == 0 and L.st_final[L.a_dst[arcs[-1]]])
    assert all(L.a_dst[a] == L.a_src[b] for a, b in zip(arcs, arcs[1:]))
    x, node = B.sequential_cost(L, A, arcs, setting)
    assert bits64(x) == bits64(least) and node == r["end_node"]
    best = [p for c, p in costs if c == least]
    if not r["tie"]:
        assert best == [arcs], "without a tie the path is the enumeration's only minimum"
    else:
        assert arcs in best
    # the words, the hits and the bonus, from the arcs themselves
    seq = [int(L.a_ol[a]) for a in arcs if L.a_ol[a] != 0]
    assert r["words"].tolist() == seq and r["hits"] == B.naive_hits(phrases, seq)
    nodes = B.track(A, seq)[0]
    bonus, k = F64(0.0), 0
    for a in arcs:
        if L.a_ol[a] != 0:
            bonus = bonus + F64(setting[3]) * A.beta[nodes[k]]
            k += 1
    assert bits64(bonus) == bits64(r["bonus"])
    tot, lm = F32(0.0), F32(0.0)
    with np.errstate(all="ignore"):
        for a in arcs:
            tot = F32(tot + F32(L.a_graph[a] + L.a_ac[a]))
            lm = F32(lm + L.a_graph[a])
    assert bits32(tot + F32(0.0)) == bits32(r["tot"]) and bits32(lm) == bits32(r["lm"]) and r["n_arcs"] == len(arcs)


def test_random_lattices_against_every_path():
    rs = np.random.RandomState(29)
    n = n_found = n_ties = n_negative = n_hits = n_moved = 0
    while n < 320:
        L = random_lattice(rs, quantised=n % 2 == 0)
        if L is None:
            continue
        n += 1
        phrases = random_list(rs)
        if n % 5 == 0:   # bonuses large enough to make totals negative
            phrases = [(ws, b * 16.0) for ws, b in phrases]
        A = B.compile_list(phrases)
        picks = [SETTINGS[i] for i in rs.choice(len(SETTINGS), 3, replace=False)]
        for setting, r in zip(picks, B.bias_many(L, A, picks)):
            check_against_every_path(L, A, phrases, setting, r)
            if r["found"]:
                n_found += 1
                n_ties += r["tie"]
                n_negative += r["biased_cost"] < 0
                n_hits += len(r["hits"]) > 0
                plain = rescale(L, *setting[:3])
                n_moved += plain["arcs"].tolist() != r["arcs"].tolist()
    print("320 lattices: %d answers, %d through a tie, %d negative, %d with hits, %d on another path than without the bias"
          % (n_found, n_ties, n_negative, n_hits, n_moved))
    assert n_found > 400 and n_ties > 50 and n_negative > 50 and n_hits > 200 and n_moved > 50


def test_the_answer_does_not_depend_on_the_numbering():
    rs = np.random.RandomState(11)
    rng = np.random.default_rng(13)
    n = moved = 0
    while n < 60:
        L = random_lattice(rs, quantised=True)
        if L is None:
            continue
        L.st_gstate = rs.permutation(L.n_states).astype(np.int32)   # (a tie that survives the whole key is unspecified, as on biglm lattices)
        n += 1
        A = B.compile_list(random_list(rs))
        M, new_of, perm = renumber(L, rng)
        moved += int(not np.array_equal(new_of, np.arange(L.n_states)))
        for a, b in zip(B.bias_many(L, A, SETTINGS), B.bias_many(M, A, SETTINGS)):
            assert a["found"] == b["found"]
            if not a["found"]:
                continue
            assert bits64(a["biased_cost"]) == bits64(b["biased_cost"])
            if a["ambiguous"]:
                continue
            assert perm[b["arcs"]].tolist() == a["arcs"].tolist() and new_of[a["end_state"]] == b["end_state"] and a["end_node"] == b["end_node"]
            assert bits64(a["bonus"]) == bits64(b["bonus"]) and a["hits"] == b["hits"] and a["nodes"] == b["nodes"]
            for key in ("words", "begin", "end"):
                assert np.array_equal(a[key], b[key]), key
    assert moved > 30


def test_without_a_list_or_a_boost_the_answer_is_the_rescaled_one():
    rs = np.random.RandomState(17)
    n = n_found = 0
    while n < 120:
        L = random_lattice(rs, quantised=False)   # costs from a continuous distribution: no decision is a tie
        if L is None:
            continue
        n += 1
        A = B.compile_list(random_list(rs))
        for gs, as_, wip in ((1.0, 1.0, 0.0), (0.7, 1.3, 0.3), (1.0, 0.1, -0.5)):
            want = rescale(L, gs, as_, wip)
            for automaton, bs in ((B.NO_LIST, 1.0), (B.NO_LIST, 0.0), (A, 0.0)):
                got = B.bias(L, automaton, (gs, as_, wip, bs))
                assert got["found"] == want["found"]
                if not want["found"]:
                    continue
                n_found += 1
                assert want["tie"] is False and got["tie"] is False, "continuous costs: the comparison leaves no input out"
                assert bits64(got["biased_cost"]) == bits64(want["scaled_cost"]) and bits64(got["bonus"]) == bits64(0.0)
                assert got["arcs"].tolist() == want["arcs"].tolist() and got["end_state"] == want["end_state"]
                for key in ("words", "begin", "end", "tids"):
                    assert np.array_equal(got[key], want[key]), key
                assert bits32(got["tot"]) == bits32(want["tot"]) and bits32(got["lm"]) == bits32(want["lm"])
    assert n_found > 600
