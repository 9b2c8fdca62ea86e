"""The definition of wfst_decoder_biased_words (include/wfst_decoder.h) restated in numpy on top of rescale_util: the phrase automaton
of a bias list straight from its definition (suffixes of strings, no failure-link construction), the cells over (lattice state, node),
the end, the traceback with its tie rule, the words and their times, the sums and the hits.

A bias list is [(words, bonus), ...].  The nodes are the distinct prefixes of the phrases, numbered breadth first: root 0, then by
(depth, parent's number, word id).  fail(j) = the node of the longest proper suffix of str(j) that is a node, delta(i, w) = the node
of the longest suffix of str(i) . w that is a node, own(j) = the bonus of the phrase str(j) is (else 0.0), beta(j) = own(j) +
beta(fail(j)) in node order.  An arc costs d = c_q(a) - r with r = bs * beta(j_k) on a word arc and 0.0 otherwise, the product and the
difference rounded one by one; v[t][j] = min (v[s][i] + d) + 0.0."""
from types import SimpleNamespace

import numpy as np

import rescale_util as RU

F32, F64 = np.float32, np.float64
MAX_NODES, MAX_WORDS = 256, 16


def compile_list(phrases):
    """the automaton of one list: J, parent, word, depth, fail, phrase (index or -1), own, beta, words (the distinct word ids,
    ascending), table [J][len(words)] = delta(i, words[k]), strs (the nodes' strings) and delta(i, w)"""
    phrases = [(tuple(int(w) for w in ws), float(b)) for ws, b in phrases]
    assert len({ws for ws, _ in phrases}) == len(phrases), "no two phrases of a list are equal"
    prefixes = {()}
    for ws, _ in phrases:
        assert 1 <= len(ws) <= MAX_WORDS and all(w > 0 for w in ws)
        for k in range(1, len(ws) + 1):
            prefixes.add(ws[:k])
    # breadth first: by depth, then the parent's number, then the word
    number, strs = {(): 0}, [()]
    for depth in range(1, MAX_WORDS + 1):
        level = sorted((s for s in prefixes if len(s) == depth), key=lambda s: (number[s[:-1]], s[-1]))
        for s in level:
            number[s] = len(strs)
            strs.append(s)
    J = len(strs)
    longest = lambda s: next(number[s[k:]] for k in range(len(s) + 1) if s[k:] in number)   # (the empty suffix is the root)
    parent = np.array([-1] + [number[s[:-1]] for s in strs[1:]], np.int32)
    word = np.array([0] + [s[-1] for s in strs[1:]], np.int32)
    depth = np.array([len(s) for s in strs], np.int32)
    fail = np.array([0] + [longest(s[1:]) for s in strs[1:]], np.int32)
    phrase, own = np.full(J, -1, np.int32), np.zeros(J, F64)
    for p, (ws, b) in enumerate(phrases):
        phrase[number[ws]], own[number[ws]] = p, b
    beta = np.zeros(J, F64)
    for j in range(1, J):
        beta[j] = own[j] + beta[fail[j]]
    words = np.array(sorted({w for s in strs for w in s}), np.int64)
    table = np.zeros((J, len(words)), np.int64)
    for i in range(J):
        for k, w in enumerate(words):
            table[i, k] = longest(strs[i] + (int(w),))
    col = {int(w): k for k, w in enumerate(words)}
    A = SimpleNamespace(J=J, parent=parent, word=word, depth=depth, fail=fail, phrase=phrase, own=own, beta=beta, words=words, table=table,
                        strs=strs, n_phrases=len(phrases))
    A.delta = lambda i, w: int(table[i, col[int(w)]]) if int(w) in col else 0
    A.column = lambda w: table[:, col[int(w)]] if int(w) in col else np.zeros(J, np.int64)
    return A


NO_LIST = compile_list([])


def naive_hits(phrases, seq):
    """every occurrence of every phrase as a contiguous run of seq: [(phrase, index of its last word)], by last word ascending, the
    longest phrase first"""
    out = []
    for k in range(len(seq)):
        here = [(len(ws), p) for p, (ws, _) in enumerate(phrases) if len(ws) <= k + 1 and tuple(seq[k + 1 - len(ws):k + 1]) == tuple(ws)]
        out += [(p, k) for _, p in sorted(here, reverse=True)]
    return out


def track(A, seq):
    """the node after every word of seq, and the hits along the chains j, fail(j), ..."""
    j, nodes, hits = 0, [], []
    for k, w in enumerate(seq):
        j = A.delta(j, w)
        nodes.append(j)
        x = j
        while x != 0:
            if A.phrase[x] >= 0:
                hits.append((int(A.phrase[x]), k))
            x = int(A.fail[x])
    return nodes, hits


def _split(settings):
    st = np.asarray(settings, F64).reshape(-1, 4)
    return st, st[:, :3], st[:, 3]


def cells(L, A, settings):
    """v[settings][states][J] (inf: not reached), c[arcs][settings], is_arc"""
    st, st3, bs = _split(settings)
    c, is_arc = RU.arc_costs(L, st3)
    Q, J = len(st), A.J
    v = np.full((Q, L.n_states, J), np.inf, F64)
    v[:, 0, 0] = 0.0
    if len(L.a_src):
        groups, _ = RU._levels(L)
        nodes = np.arange(J)
        for grp in groups:
            for a in grp[is_arc[grp]]:
                s, t, w = int(L.a_src[a]), int(L.a_dst[a]), int(L.a_ol[a])
                to = A.column(w) if w else nodes
                for q in range(Q):
                    with np.errstate(all="ignore"):
                        r = bs[q] * A.beta[to] if w else np.zeros(J, F64)
                        d = c[a, q] - r
                        x = (v[q, s] + d) + 0.0
                    x[~np.isfinite(x)] = np.inf
                    np.minimum.at(v[q, t], to, x)
    return v, c, is_arc


def sequential_cost(L, A, arcs, setting):
    """(the float64 sequential sum of d along a path with its node track, the end node), None where a partial sum is not finite or
    an arc is none"""
    st, st3, bs = _split([setting])
    c, is_arc = RU.arc_costs(L, st3)
    x, j = F64(0.0), 0
    with np.errstate(all="ignore"):
        for a in arcs:
            if not is_arc[a]:
                return None
            w = int(L.a_ol[a])
            if w:
                j = A.delta(j, w)
            r = bs[0] * A.beta[j] if w else F64(0.0)
            d = c[a, 0] - r
            x = (x + d) + 0.0
            if not np.isfinite(x):
                return None
    return F64(x), j


def bias_many(L, A, settings, sil_tids=None):
    """one dict per setting (gs, as, wip, bs): found, arcs, end_state, end_node, nodes (the node after every arc), words, begin, end,
    n_arcs, biased_cost, bonus (float64), tot, lm (float32), hits [(phrase, word index)], tie, ambiguous"""
    st, st3, bs = _split(settings)
    if L is None or L.n_states == 0:
        return [dict(found=False) for _ in st]
    v, c, is_arc = cells(L, A, st)
    by_dst = np.argsort(L.a_dst, kind="stable")
    first = np.searchsorted(L.a_dst[by_dst], np.arange(L.n_states + 1))
    gb, ab = L.a_graph.astype(F32).view(np.uint32), L.a_ac.astype(F32).view(np.uint32)
    fin_all = np.nonzero(L.st_final)[0]
    out = []
    for q in range(len(st)):
        vq = v[q]
        ends = [(vq[e, j], int(L.st_gstate[e]), j, int(e)) for e in fin_all for j in range(A.J) if np.isfinite(vq[e, j])]
        if not ends:
            out.append(dict(found=False))
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
                with np.errstate(all="ignore"):
                    d = c[a, q] - (bs[q] * A.beta[j] if w else F64(0.0))
                    for i in (np.nonzero(A.column(w) == j)[0] if w else [j]):
                        x = (vq[s, i] + d) + 0.0
                        if np.isfinite(x) and x == vq[t, j]:
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
        word_nodes, hits = track(A, seq)
        assert word_nodes == [n for a, n in zip(arcs, nodes) if L.a_ol[a] != 0]
        bonus = F64(0.0)
        with np.errstate(all="ignore"):
            for a, n in zip(arcs, nodes):
                bonus = bonus + (bs[q] * A.beta[n] if L.a_ol[a] != 0 else F64(0.0))
        r.update(found=True, arcs=np.array(arcs, np.int64), end_state=end_state, end_node=end_node, nodes=nodes, biased_cost=F64(best[0]),
                 bonus=F64(bonus), hits=hits, tie=bool(tie), ambiguous=bool(ambiguous))
        out.append(r)
    return out


def bias(L, A, setting, sil_tids=None):
    return bias_many(L, A, [setting], sil_tids)[0]


def same_answer(got, want, tag=""):
    """a BatchDecoder.biased_words dict against bias()'s, bit for bit"""
    assert bool(got["found"]) == bool(want["found"]), tag
    if not want["found"]:
        assert got["n_arcs"] == 0 and got["n_hyp"] == 0 and len(got["hyp_words"]) == 0 and got["n_hits"] == 0, tag
        assert got["biased_cost"] == 0.0 and got["bonus"] == 0.0 and RU.bits32(got["tot"]) == 0 and RU.bits32(got["lm"]) == 0, tag
        return
    assert RU.bits64(got["biased_cost"]) == RU.bits64(want["biased_cost"]), (tag, got["biased_cost"], want["biased_cost"])
    assert RU.bits64(got["bonus"]) == RU.bits64(want["bonus"]), (tag, got["bonus"], want["bonus"])
    assert got["n_arcs"] == want["n_arcs"], tag
    assert got["n_hyp"] == len(want["words"]) and np.array_equal(got["hyp_words"], want["words"]), tag
    assert np.array_equal(got["begin"], want["begin"]) and np.array_equal(got["end"], want["end"]), tag
    assert RU.bits32(got["tot"]) == RU.bits32(want["tot"]) and RU.bits32(got["lm"]) == RU.bits32(want["lm"]), tag
    assert got["n_hits"] == len(want["hits"]), tag
    assert list(zip(got["hit_phrase"].tolist(), got["hit_word"].tolist())) == want["hits"], tag
