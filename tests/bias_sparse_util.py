"""The definition of wfst_decoder_biased_words_sparse (include/wfst_decoder.h) restated on top of bias_util and rescale_util: a book's
automaton built the fast way (a trie, failure links, delta by goto / fail) in bias_util.compile_list's namespace, the reachable sets
R(t), and the cells, the end, the traceback and the outputs over a dict of the reachable cells only.

bias_util.compile_list builds the automaton straight from the definition (suffixes of strings) and its table of J x W entries, which
is what makes it the reference and what makes it slow and large beyond a thousand nodes; compile_book is checked against it field for
field (tests/test_bias_sparse_restatement.py) and then stands in for it at the sizes only a book has."""
import math

import numpy as np

import bias_util as B
import rescale_util as RU

F32, F64 = np.float32, np.float64
MAX_NODES, MAX_WORDS = 65536, 16


class Book(object):
    """compile_list's fields; table and column(w) are worked out from delta when they are asked for"""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self._columns = {}
        self._table = None

    def goto(self, i, w):
        return self.child.get((i, int(w)), -1)

    def delta(self, i, w):
        w = int(w)
        if w not in self.word_set:
            return 0
        while True:
            c = self.child.get((i, w), -1)
            if c >= 0:
                return c
            if i == 0:
                return 0
            i = int(self.fail[i])

    def column(self, w):
        w = int(w)
        if w not in self._columns:
            self._columns[w] = np.array([self.delta(i, w) for i in range(self.J)], np.int64) if w in self.word_set else np.zeros(self.J, np.int64)
        return self._columns[w]

    @property
    def table(self):
        if self._table is None:
            self._table = np.stack([self.column(w) for w in self.words], axis=1) if len(self.words) else np.zeros((self.J, 0), np.int64)
        return self._table


def compile_book(phrases):
    """the automaton of one book [(words, bonus), ...], nodes breadth first by (depth, parent's number, word id)"""
    phrases = [(tuple(int(w) for w in ws), float(b)) for ws, b in phrases]
    assert len({ws for ws, _ in phrases}) == len(phrases), "no two phrases of a book are equal"
    kids = [{}]   # the trie in the order the phrases came
    for ws, _ in phrases:
        assert 1 <= len(ws) <= MAX_WORDS and all(w > 0 for w in ws)
        x = 0
        for w in ws:
            if w not in kids[x]:
                kids[x][w] = len(kids)
                kids.append({})
            x = kids[x][w]
    # breadth first: a node's children, by word, behind the children of the nodes numbered before it
    order, parent, word, depth = [0], [-1], [0], [0]
    at = 0
    while at < len(order):
        for w in sorted(kids[order[at]]):
            order.append(kids[order[at]][w])
            parent.append(at)
            word.append(w)
            depth.append(depth[at] + 1)
        at += 1
    J = len(order)
    assert J <= MAX_NODES
    number = {x: j for j, x in enumerate(order)}
    child = {(parent[j], word[j]): j for j in range(1, J)}
    first_child, n_child = np.zeros(J, np.int32), np.zeros(J, np.int32)
    for j in range(J - 1, 0, -1):
        first_child[parent[j]] = j
        n_child[parent[j]] += 1
    strs = [()]
    for j in range(1, J):
        strs.append(strs[parent[j]] + (word[j],))
    A = Book(J=J, parent=np.array(parent, np.int32), word=np.array(word, np.int32), depth=np.array(depth, np.int32), fail=np.zeros(J, np.int32),
             phrase=np.full(J, -1, np.int32), own=np.zeros(J, F64), beta=np.zeros(J, F64), words=np.array(sorted(set(word[1:])), np.int64),
             strs=strs, n_phrases=len(phrases), child=child, word_set=set(word[1:]), first_child=first_child, n_child=n_child)
    for p, (ws, b) in enumerate(phrases):
        x = 0
        for w in ws:
            x = kids[x][w]
        A.phrase[number[x]], A.own[number[x]] = p, b
    for j in range(1, J):   # a failure link is shallower than its node: numbered, and finished, before it
        A.fail[j] = 0 if parent[j] == 0 else A.delta(int(A.fail[parent[j]]), word[j])
        A.beta[j] = A.own[j] + A.beta[A.fail[j]]
    return A


def reach(L, A):
    """R(t) per lattice state, ascending lists: R(0) = {0}; over an arc that is an arc, R(t) takes R(s) (no word) or delta(R(s), word)"""
    R = [set() for _ in range(L.n_states)]
    if L.n_states:
        R[0].add(0)
    if len(L.a_src):
        _, is_arc = RU.arc_costs(L, [(1.0, 1.0, 0.0)])
        groups, _ = RU._levels(L)
        for grp in groups:
            for a in grp[is_arc[grp]]:
                s, t, w = int(L.a_src[a]), int(L.a_dst[a]), int(L.a_ol[a])
                R[t].update(R[s] if w == 0 else {A.delta(i, w) for i in R[s]})
    return [sorted(r) for r in R]


def n_cells(L, A):
    return sum(len(r) for r in reach(L, A))


def sparse_cells(L, A, settings, R=None):
    """per setting a dict {(state, node): v} of the reachable cells that are finite; c[arcs][settings], is_arc, R"""
    st, st3, bs = B._split(settings)
    c, is_arc = RU.arc_costs(L, st3)
    R = reach(L, A) if R is None else R
    tables = []
    groups = RU._levels(L)[0] if len(L.a_src) else []
    for q in range(len(st)):
        v = {(0, 0): 0.0}
        for grp in groups:
            for a in grp[is_arc[grp]]:
                s, t, w = int(L.a_src[a]), int(L.a_dst[a]), int(L.a_ol[a])
                ca = float(c[a, q])
                for i in R[s]:
                    x = v.get((s, i))
                    if x is None:
                        continue
                    j = A.delta(i, w) if w else i
                    r = float(bs[q]) * float(A.beta[j]) if w else 0.0
                    d = ca - r
                    y = (x + d) + 0.0
                    if not math.isfinite(y):
                        continue
                    assert j in R[t]
                    if y < v.get((t, j), math.inf):
                        v[(t, j)] = y
        tables.append(v)
    return tables, c, is_arc, R


def bias_many_sparse(L, A, settings, sil_tids=None):
    """bias_util.bias_many's dicts (and n_cells in each) from the reachable cells alone"""
    st, st3, bs = B._split(settings)
    if L is None or L.n_states == 0:
        return [dict(found=False, n_cells=0) for _ in st]
    tables, c, is_arc, R = sparse_cells(L, A, st)
    count = sum(len(r) for r in R)
    by_dst = np.argsort(L.a_dst, kind="stable")
    first = np.searchsorted(L.a_dst[by_dst], np.arange(L.n_states + 1))
    gb, ab = L.a_graph.astype(F32).view(np.uint32), L.a_ac.astype(F32).view(np.uint32)
    fin_all = np.nonzero(L.st_final)[0]
    out = []
    for q in range(len(st)):
        v = tables[q]
        ends = [(v[(int(e), j)], int(L.st_gstate[e]), j, int(e)) for e in fin_all for j in R[int(e)] if (int(e), j) in v]
        if not ends:
            out.append(dict(found=False, n_cells=count))
            continue
        best = min(ends)
        tie = sum(1 for x in ends if x[0] == best[0]) > 1
        ambiguous = sum(1 for x in ends if x[:3] == best[:3]) > 1
        t, j = best[3], best[2]
        end_state, end_node, arcs, nodes = t, j, [], []
        while t != 0:
            cands = []
            for a in by_dst[first[t]:first[t + 1]]:
                if not is_arc[a]:
                    continue
                w, s = int(L.a_ol[a]), int(L.a_src[a])
                d = float(c[a, q]) - (float(bs[q]) * float(A.beta[j]) if w else 0.0)
                for i in R[s]:
                    if (A.delta(i, w) if w else i) != j or (s, i) not in v:
                        continue
                    x = (v[(s, i)] + d) + 0.0
                    if math.isfinite(x) and x == v[(t, j)]:
                        cands.append((RU.arc_key(L, a, gb, ab), int(i), int(a)))
            assert cands, "a reached cell without the arrival that made it"
            k = min(cands)
            tie = tie or len(cands) > 1
            ambiguous = ambiguous or len({x[2] for x in cands if x[0] == k[0]}) > 1
            arcs.append(k[2])
            nodes.append(j)
            t, j = int(L.a_src[k[2]]), k[1]
        assert j == 0
        arcs.reverse()
        nodes.reverse()
        r = RU.path_outputs(L, arcs, end_state, sil_tids)
        seq = r["words"].tolist()
        word_nodes, hits = B.track(A, seq)
        assert word_nodes == [n for a, n in zip(arcs, nodes) if L.a_ol[a] != 0]
        bonus = F64(0.0)
        with np.errstate(all="ignore"):
            for a, n in zip(arcs, nodes):
                bonus = bonus + (bs[q] * A.beta[n] if L.a_ol[a] != 0 else F64(0.0))
        r.update(found=True, arcs=np.array(arcs, np.int64), end_state=end_state, end_node=end_node, nodes=nodes, biased_cost=F64(best[0]),
                 bonus=F64(bonus), hits=hits, tie=bool(tie), ambiguous=bool(ambiguous), n_cells=count)
        out.append(r)
    return out
