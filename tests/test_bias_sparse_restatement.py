"""CPU: the definition of wfst_decoder_biased_words_sparse as tests/bias_sparse_util.py restates it -- the fast automaton against
bias_util.compile_list field for field, the finite support of the dense cells inside the reachable sets, the sparse restatement
against the dense one in every field (and so, through test_bias_restatement.py's chain, against the enumeration of every path), and
n_cells under a renumbering of states and arcs."""
import numpy as np

import bias_sparse_util as S
import bias_util as B
from rescale_util import bits32, bits64, renumber
from test_bias_restatement import SETTINGS, dyadic, random_lattice, random_list

F64 = np.float64


def same_automaton(A, X):
    assert A.J == X.J and A.n_phrases == X.n_phrases and A.strs == X.strs
    for key in ("parent", "word", "depth", "fail", "phrase", "words"):
        assert np.array_equal(getattr(A, key), getattr(X, key)), key
    for key in ("own", "beta"):
        assert getattr(A, key).dtype == F64 and getattr(A, key).tobytes() == getattr(X, key).tobytes(), key
    assert np.array_equal(A.table, X.table)
    for w in list(X.words[:5]) + [10 ** 6]:
        assert np.array_equal(A.column(w), X.column(w)) and all(A.delta(i, w) == X.delta(i, w) for i in range(0, A.J, max(1, A.J // 7)))
    # a node's children are consecutive numbers in ascending word order: what the device's child search relies on
    for i in range(A.J):
        kids = list(range(A.first_child[i], A.first_child[i] + A.n_child[i]))
        assert all(A.parent[j] == i for j in kids) and all(A.word[a] < A.word[b] for a, b in zip(kids, kids[1:]))
    assert int(A.n_child.sum()) == A.J - 1, "every node but the root is in its parent's range"


def big_list(rs, nodes, alphabet):
    """random phrases over a small alphabet (failure links that lead somewhere) until the trie has about `nodes` nodes"""
    out, seen, trie = [], set(), {()}
    while len(trie) < nodes:
        ws = tuple(int(w) for w in rs.randint(1, alphabet + 1, size=rs.randint(1, 7)))
        if ws in seen:
            continue
        seen.add(ws)
        out.append((ws, dyadic(rs) + (0.1 if rs.rand() < 0.3 else 0.0)))   # (not all dyadic: beta's bits depend on the order of its sums)
        trie.update(ws[:k] for k in range(1, len(ws) + 1))
    return out


def test_the_fast_automaton_is_compile_lists_field_for_field():
    rs = np.random.RandomState(41)
    same_automaton(S.compile_book([]), B.NO_LIST)
    for _ in range(120):
        phrases = random_list(rs, alphabet=rs.randint(1, 5), most=8, longest=6)
        same_automaton(S.compile_book(phrases), B.compile_list(phrases))
    sizes = []
    for nodes, alphabet in ((120, 3), (258, 4), (600, 5)):
        phrases = big_list(rs, nodes, alphabet)
        A = S.compile_book(phrases)
        same_automaton(A, B.compile_list(phrases))
        sizes.append((A.J, int(A.depth.max()), int((A.fail != 0).sum())))
    print("(nodes, depth, nodes whose failure link is not the root):", sizes)
    assert sizes[-1][0] >= 600 and all(s[2] > s[0] // 4 for s in sizes)


def test_the_finite_cells_are_reachable_and_the_sparse_answer_is_the_dense_one():
    rs = np.random.RandomState(43)
    n = n_found = n_hits = strict = 0
    dense_cells = sparse_cells = 0
    while n < 320:
        L = random_lattice(rs, quantised=n % 2 == 0)
        if L is None:
            continue
        n += 1
        phrases = random_list(rs)
        if n % 5 == 0:
            phrases = [(ws, b * 16.0) for ws, b in phrases]
        A, X = S.compile_book(phrases), B.compile_list(phrases)
        picks = [SETTINGS[i] for i in rs.choice(len(SETTINGS), 3, replace=False)]
        R = S.reach(L, A)
        v, _, _ = B.cells(L, X, picks)
        tables = S.sparse_cells(L, A, picks, R)[0]
        for q in range(len(picks)):
            finite = {(int(t), int(j)) for t, j in zip(*np.nonzero(np.isfinite(v[q])))}
            assert finite <= {(t, j) for t in range(L.n_states) for j in R[t]}, "a finite cell outside R"
            assert finite == set(tables[q]) and all(bits64(v[q][t, j]) == bits64(x) for (t, j), x in tables[q].items()), "the same cells, bit for bit"
        count = sum(len(r) for r in R)
        dense_cells += L.n_states * A.J
        sparse_cells += count
        strict += count < L.n_states * A.J
        for a, b in zip(S.bias_many_sparse(L, A, picks), B.bias_many(L, X, picks)):
            assert a["n_cells"] == count and a["found"] == b["found"]
            if not b["found"]:
                continue
            n_found += 1
            n_hits += len(b["hits"]) > 0
            assert bits64(a["biased_cost"]) == bits64(b["biased_cost"]) and bits64(a["bonus"]) == bits64(b["bonus"])
            assert a["arcs"].tolist() == b["arcs"].tolist() and a["nodes"] == b["nodes"] and a["hits"] == b["hits"]
            assert a["end_state"] == b["end_state"] and a["end_node"] == b["end_node"] and a["tie"] == b["tie"] and a["ambiguous"] == b["ambiguous"]
            for key in ("words", "begin", "end", "tids"):
                assert np.array_equal(a[key], b[key]), key
            assert bits32(a["tot"]) == bits32(b["tot"]) and bits32(a["lm"]) == bits32(b["lm"]) and a["n_arcs"] == b["n_arcs"]
    print("320 lattices: %d answers, %d with hits; %d reachable of %d dense cells, fewer on %d lattices" % (n_found, n_hits, sparse_cells, dense_cells, strict))
    assert n_found > 400 and n_hits > 200 and strict > 250


def test_an_overflowing_sum_leaves_a_reachable_cell_unreached():
    """a cell inside R may be +inf: the only way into the final state overflows float64 under a huge scale"""
    from align_util import make_lattice

    L = make_lattice([(0, 0, 0), (1, 1, 0), (2, 2, 1)], [(0, 1, 1, 5, 3.0e38, 0.0), (1, 2, 2, 0, 3.0e38, 0.0)])
    A = S.compile_book([((5,), 1.0)])
    assert S.reach(L, A) == [[0], [1], [1]]
    huge = (1.0e300, 1.0, 0.0, 1.0)
    got, want = S.bias_many_sparse(L, A, [huge, SETTINGS[0]]), B.bias_many(L, B.compile_list([((5,), 1.0)]), [huge, SETTINGS[0]])
    assert not got[0]["found"] and not want[0]["found"] and got[1]["found"] and want[1]["found"]
    assert got[0]["n_cells"] == 3 and bits64(got[1]["biased_cost"]) == bits64(want[1]["biased_cost"])


def test_n_cells_does_not_depend_on_the_numbering():
    rs = np.random.RandomState(47)
    rng = np.random.default_rng(49)
    n = moved = 0
    while n < 60:
        L = random_lattice(rs, quantised=True)
        if L is None:
            continue
        n += 1
        A = S.compile_book(random_list(rs))
        M, new_of, perm = renumber(L, rng)
        moved += int(not np.array_equal(new_of, np.arange(L.n_states)))
        R, Q = S.reach(L, A), S.reach(M, A)
        assert all(R[t] == Q[new_of[t]] for t in range(L.n_states))
        assert S.n_cells(L, A) == S.n_cells(M, A) == sum(len(r) for r in R)
    assert moved > 30
