"""The definition of wfst_decoder_rescaled_words (include/wfst_decoder.h) restated in numpy over a raw lattice: the arc costs under a
setting (graph_scale, acoustic_scale, word_penalty), the min-plus cells, the end, the traceback with its tie rule, the words' begin and
end frames (silence-trimmed where a silence list is given), the alignment and the three scores.

A lattice is what align_util takes (n_states, st_final, st_frame, st_gstate, a_src, a_dst, a_il, a_ol, a_graph, a_ac; every arc goes
to a higher state id).  The cells are float64, numpy's arithmetic: every product and every sum is rounded on its own,
    c_q(a) = (gs * float64(graph) + as * float64(acoustic)) + (olabel != 0 ? wip : 0.0),   v[t] = min (v[s] + c_q(a)) + 0.0,
a sum that is not finite being no transition and an arc whose float32 graph + acoustic is not finite no arc.  tot and lm are the
float32 sequential sums LatticeToVector takes, unscaled."""
import numpy as np

F32, F64 = np.float32, np.float64


def arc_costs(L, settings):
    """(c[arcs][settings] in float64, is_arc[arcs]): the cost of every arc under every setting; an arc that is none has is_arc False"""
    st = np.asarray(settings, F64).reshape(-1, 3)
    g32, a32 = L.a_graph.astype(F32), L.a_ac.astype(F32)
    with np.errstate(all="ignore"):
        is_arc = np.isfinite((g32 + a32).astype(F32))
        g = st[None, :, 0] * g32.astype(F64)[:, None]
        a = st[None, :, 1] * a32.astype(F64)[:, None]
        scaled = g + a
        c = scaled + np.where((L.a_ol != 0)[:, None], st[None, :, 2], 0.0)
    return c, is_arc


def _levels(L):
    """arc groups such that every arc into a group's states leaves a finished state: a level = the states of one frame at one depth
    along the arcs inside the frame (ilabel 0)"""
    S = L.n_states
    src, dst = L.a_src.astype(np.int64), L.a_dst.astype(np.int64)
    assert len(src) == 0 or np.all(dst > src), "arcs must go to higher state ids"
    depth = np.zeros(S, np.int64)
    eps = np.nonzero(L.a_il == 0)[0]
    for a in eps[np.argsort(src[eps], kind="stable")]:
        depth[dst[a]] = max(depth[dst[a]], depth[src[a]] + 1)
    level = L.st_frame.astype(np.int64) * (int(depth.max()) + 1 if S else 1) + depth
    assert len(src) == 0 or np.all(level[dst] > level[src])
    order = np.argsort(level[dst], kind="stable")
    cuts = np.nonzero(np.diff(level[dst][order]))[0] + 1
    return np.split(order, cuts), depth


def cells(L, settings):
    """v[states][settings] (inf: not reached) and the arc costs"""
    c, is_arc = arc_costs(L, settings)
    Q = c.shape[1]
    v = np.full((L.n_states, Q), np.inf, F64)
    v[0, :] = 0.0
    if len(L.a_src):
        groups, _ = _levels(L)
        src, dst = L.a_src.astype(np.int64), L.a_dst.astype(np.int64)
        for grp in groups:
            grp = grp[is_arc[grp]]
            if len(grp) == 0:
                continue
            with np.errstate(all="ignore"):
                arrive = (v[src[grp]] + c[grp]) + 0.0
            arrive[~np.isfinite(arrive)] = np.inf
            np.minimum.at(v, dst[grp], arrive)
    return v, c, is_arc


def arc_key(L, a, gb, ab):
    """the traceback's key of arc a: ilabel == 0 last, graph state of the source token, ilabel, olabel, bits of graph, bits of acoustic"""
    return (int(L.a_il[a] == 0), int(L.st_gstate[L.a_src[a]]), int(L.a_il[a]), int(L.a_ol[a]), int(gb[a]), int(ab[a]))


def candidates(L, t, vq, cq, is_arc, by_dst, first):
    """the in-arcs of t that qualify: (v[s] + c(a)) + 0.0 == v[t], exactly"""
    out = []
    for a in by_dst[first[t]:first[t + 1]]:
        if not is_arc[a]:
            continue
        with np.errstate(all="ignore"):
            x = (vq[L.a_src[a]] + cq[a]) + 0.0
        if np.isfinite(x) and x == vq[t]:
            out.append(int(a))
    return out


def path_outputs(L, arcs, end_state, sil_tids=None):
    """words, begin, end, tids, tot, lm of a path (arc indices front to back), by align_words' definitions"""
    arcs = np.asarray(arcs, np.int64)
    lm, tot = F32(0.0), F32(0.0)
    with np.errstate(all="ignore"):
        for a in arcs:
            lm = F32(lm + L.a_graph[a])
            tot = F32(F32(tot + F32(F32(L.a_graph[a]) + F32(L.a_ac[a]))) + F32(0.0))
    fr = L.st_frame[L.a_src[arcs]].astype(np.int64) if len(arcs) else np.zeros(0, np.int64)
    il = L.a_il[arcs].astype(np.int64) if len(arcs) else np.zeros(0, np.int64)
    ol = L.a_ol[arcs].astype(np.int64) if len(arcs) else np.zeros(0, np.int64)
    j = np.nonzero(ol)[0]
    begin = fr[j]
    end = np.zeros(len(j), np.int64)
    for i in range(len(j)):
        hi = j[i + 1] if i + 1 < len(j) else len(arcs)
        if sil_tids is None:
            end[i] = begin[i + 1] if i + 1 < len(j) else int(L.st_frame[end_state])
        else:
            span = np.arange(j[i], hi)
            keep = span[(il[span] != 0) & ~np.isin(il[span], sil_tids)]
            end[i] = 1 + fr[keep].max() if len(keep) else begin[i]
    return dict(words=ol[j].astype(np.int32), begin=begin.astype(np.int32), end=end.astype(np.int32), tids=il[il != 0].astype(np.int32),
                tot=tot, lm=lm, n_arcs=len(arcs))


def rescale_many(L, settings, sil_tids=None):
    """one dict per setting: found, arcs, end_state, words, begin, end, tids, n_arcs, scaled_cost (float64), tot, lm (float32),
    tie (some decision had more than one exact candidate), ambiguous (two candidates of one decision had the same key: on biglm
    lattices the winner is unspecified)"""
    st = np.asarray(settings, F64).reshape(-1, 3)
    if L is None or L.n_states == 0:
        return [dict(found=False) for _ in st]
    v, c, is_arc = cells(L, st)
    by_dst = np.argsort(L.a_dst, kind="stable")
    first = np.searchsorted(L.a_dst[by_dst], np.arange(L.n_states + 1))
    gb, ab = L.a_graph.astype(F32).view(np.uint32), L.a_ac.astype(F32).view(np.uint32)
    fin_all = np.nonzero(L.st_final)[0]
    out = []
    for q in range(len(st)):
        vq, cq = v[:, q], c[:, q]
        fin = fin_all[np.isfinite(vq[fin_all])]
        if len(fin) == 0:
            out.append(dict(found=False))
            continue
        best = vq[fin].min()
        ends = fin[vq[fin] == best]
        tie = len(ends) > 1
        gmin = L.st_gstate[ends].min()
        ambiguous = int((L.st_gstate[ends] == gmin).sum()) > 1
        t = int(ends[np.argmin(L.st_gstate[ends])])
        end_state, arcs = t, []
        while t != 0:
            cands = candidates(L, t, vq, cq, is_arc, by_dst, first)
            assert cands, "a reached state without the arrival that made it"
            keys = [arc_key(L, a, gb, ab) for a in cands]
            k = min(keys)
            tie = tie or len(cands) > 1
            ambiguous = ambiguous or keys.count(k) > 1
            a = cands[keys.index(k)]
            arcs.append(a)
            t = int(L.a_src[a])
        arcs.reverse()
        r = path_outputs(L, arcs, end_state, sil_tids)
        r.update(found=True, arcs=np.array(arcs, np.int64), end_state=end_state, scaled_cost=F64(best), tie=bool(tie), ambiguous=bool(ambiguous))
        out.append(r)
    return out


def rescale(L, gs, as_, wip, sil_tids=None):
    return rescale_many(L, [(gs, as_, wip)], sil_tids)[0]


def sequential_cost(L, arcs, setting):
    """the float64 sequential sum of c_q along a path: ((0 + c) + 0.0 ...), None where a partial sum is not finite or an arc is none"""
    c, is_arc = arc_costs(L, [setting])
    x = F64(0.0)
    with np.errstate(all="ignore"):
        for a in arcs:
            if not is_arc[a]:
                return None
            x = (x + c[a, 0]) + 0.0
            if not np.isfinite(x):
                return None
    return F64(x)


def all_paths(L, limit=200000):
    """every complete path of a SMALL lattice, as lists of arc indices: from state 0 to a final state (a final state may have
    out-arcs: the path that stops there counts, and so do those that go on)"""
    out_arcs = [[] for _ in range(L.n_states)]
    for a in range(len(L.a_src)):
        out_arcs[int(L.a_src[a])].append(a)
    paths, stack = [], [(0, [])]
    while stack:
        s, p = stack.pop()
        if L.st_final[s]:
            paths.append(p)
            assert len(paths) <= limit
        for a in out_arcs[s]:
            stack.append((int(L.a_dst[a]), p + [a]))
    return paths


def renumber(L, rng):
    """the same lattice under a random renumbering of its states that keeps state 0 and "every arc goes to a higher id" (a random
    topological order) and a random permutation of its arcs: (lattice, new id of every old state, old index of every new arc)"""
    from types import SimpleNamespace
    S, A = L.n_states, len(L.a_src)
    indeg = np.zeros(S, np.int64)
    np.add.at(indeg, L.a_dst, 1)
    outs = [[] for _ in range(S)]
    for a in range(A):
        outs[int(L.a_src[a])].append(int(L.a_dst[a]))
    # state 0 first; then any state all of whose predecessors are placed, at random (states that no arc reaches are free at once)
    ready, order = [s for s in range(1, S) if indeg[s] == 0], [0]
    for d in outs[0]:
        indeg[d] -= 1
        if indeg[d] == 0:
            ready.append(d)
    while ready:
        s = ready.pop(int(rng.integers(len(ready))))
        order.append(s)
        for d in outs[s]:
            indeg[d] -= 1
            if indeg[d] == 0:
                ready.append(d)
    assert len(order) == S
    new_of = np.zeros(S, np.int64)
    new_of[np.array(order)] = np.arange(S)
    perm = rng.permutation(A)
    old = np.array(order)
    M = SimpleNamespace(n_states=S, start=0, st_final=L.st_final[old], st_frame=L.st_frame[old], st_gstate=L.st_gstate[old],
                        a_src=new_of[L.a_src[perm]].astype(np.int32), a_dst=new_of[L.a_dst[perm]].astype(np.int32), a_il=L.a_il[perm],
                        a_ol=L.a_ol[perm], a_graph=L.a_graph[perm], a_ac=L.a_ac[perm])
    return M, new_of, perm


def bits64(x):
    return int(np.asarray(x, F64).reshape(1).view(np.uint64)[0])


def bits32(x):
    return int(np.asarray(x, F32).reshape(1).view(np.uint32)[0])


def same_answer(got, want, tag="", tids=False):
    """a BatchDecoder.rescaled_words dict against rescale()'s, bit for bit"""
    assert bool(got["found"]) == bool(want["found"]), tag
    if not want["found"]:
        assert got["n_arcs"] == 0 and got["n_hyp"] == 0 and len(got["hyp_words"]) == 0 and got["scaled_cost"] == 0.0, tag
        assert bits32(got["tot"]) == 0 and bits32(got["lm"]) == 0, tag
        return
    assert bits64(got["scaled_cost"]) == bits64(want["scaled_cost"]), (tag, got["scaled_cost"], want["scaled_cost"])
    assert got["n_arcs"] == want["n_arcs"], tag
    assert got["n_hyp"] == len(want["words"]) and np.array_equal(got["hyp_words"], want["words"]), tag
    assert np.array_equal(got["begin"], want["begin"]) and np.array_equal(got["end"], want["end"]), tag
    assert bits32(got["tot"]) == bits32(want["tot"]) and bits32(got["lm"]) == bits32(want["lm"]), tag
    if tids:
        assert got["n_tids"] == len(want["tids"]) and np.array_equal(got["tids"], want["tids"]), tag
