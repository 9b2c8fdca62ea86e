"""The definition of wfst_decoder_align_words (include/wfst_decoder.h) restated in numpy over a raw lattice: the recurrence, the
traceback with its tie rule, the words' begin and end frames (silence-trimmed where a silence list is given).

A lattice here is anything with n_states, st_final, st_frame, st_gstate, a_src, a_dst, a_il, a_ol, a_graph, a_ac (pyoracle.RawLattice;
from_gpu() turns BatchDecoder.raw_lattice()'s dict into one) whose arcs all go to a higher state id.  All sums are float32:
d[t][k'] = min(d[t][k'], (d[s][k] + (graph + acoustic)) + 0.0), a total that is not finite being no path."""
from types import SimpleNamespace

import numpy as np

F32 = np.float32


def from_gpu(d):
    """BatchDecoder.raw_lattice()'s dict (None: no lattice) as the lattice align() takes"""
    if d is None:
        return None
    return SimpleNamespace(n_states=int(d["n_states"]), start=0, st_final=d["st_final"], st_frame=d["st_frame"], st_gstate=d["st_state"],
                           a_src=d["a_src"], a_dst=d["a_dst"], a_il=d["a_ilabel"], a_ol=d["a_olabel"], a_graph=d["a_graph"], a_ac=d["a_acoustic"])


def make_lattice(states, arcs):
    """states: [(frame, graph state, final)], arcs: [(src, dst, ilabel, olabel, graph, acoustic)] -- hand-made lattices"""
    st, ar = np.array(states, np.int64).reshape(-1, 3), np.array(arcs, np.float64).reshape(-1, 6)
    return SimpleNamespace(n_states=len(st), start=0, st_final=st[:, 2].astype(np.int32), st_frame=st[:, 0].astype(np.int32),
                           st_gstate=st[:, 1].astype(np.int32), a_src=ar[:, 0].astype(np.int32), a_dst=ar[:, 1].astype(np.int32),
                           a_il=ar[:, 2].astype(np.int32), a_ol=ar[:, 3].astype(np.int32), a_graph=ar[:, 4].astype(F32), a_ac=ar[:, 5].astype(F32))


def _finite_or_inf(x):
    x = (x + F32(0.0)).astype(F32)
    x[~np.isfinite(x)] = np.inf
    return x


def _tables(L, seqs):
    """d[state][sequence][k] for all the sequences at once (columns beyond a sequence's own stay inf), level by level: a level =
    the states of one frame at one depth along the epsilon arcs, so that every arc into a level leaves a finished one"""
    S, A, Q = L.n_states, len(L.a_src), len(seqs)
    W = 1 + max([len(s) for s in seqs] + [0])
    words = np.full((Q, W), -1, np.int64)   # words[q][k]: the word that takes column k to k + 1
    for q, s in enumerate(seqs):
        words[q, :len(s)] = s
    src, dst = L.a_src.astype(np.int64), L.a_dst.astype(np.int64)
    assert A == 0 or np.all(dst > src), "arcs must go to higher state ids"
    depth = np.zeros(S, np.int64)
    eps = np.nonzero(L.a_il == 0)[0]
    for a in eps[np.argsort(src[eps], kind="stable")]:   # (sources ascending: a state's depth is final before its arcs are looked at)
        depth[dst[a]] = max(depth[dst[a]], depth[src[a]] + 1)
    level = L.st_frame.astype(np.int64) * (int(depth.max()) + 1 if S else 1) + depth
    assert A == 0 or np.all(level[dst] > level[src])
    val = (L.a_graph.astype(F32) + L.a_ac.astype(F32)).astype(F32)
    d = np.full((S, Q, W), np.inf, F32)
    d[L.start, :, 0] = 0.0
    order = np.argsort(level[dst], kind="stable")
    cuts = np.nonzero(np.diff(level[dst][order]))[0] + 1
    for grp in np.split(order, cuts):
        s, o = src[grp], L.a_ol[grp].astype(np.int64)
        arrive = _finite_or_inf((d[s] + val[grp][:, None, None]).astype(F32))   # [arcs][Q][W]: over this arc from (s, k)
        cand = np.full(arrive.shape, np.inf, F32)
        e = o == 0
        cand[e] = arrive[e]
        w = ~e
        if w.any():
            hit = words[None, :, :-1] == o[w][:, None, None]    # column k -> k + 1
            cand[w, :, 1:] = np.where(hit, arrive[w][:, :, :-1], F32(np.inf))
        np.minimum.at(d, dst[grp], cand)
    return d, val


def align_many(L, seqs, sil_tids=None):
    """align() of every sequence of `seqs` over one lattice (the tables are computed together); None entries are skipped"""
    out = [None] * len(seqs)
    live = [q for q, s in enumerate(seqs) if s is not None]
    if L is None or L.n_states == 0:
        return [None if s is None else dict(found=False) for s in seqs]
    todo = [[int(x) for x in seqs[q]] for q in live]
    d, val = _tables(L, todo)
    by_dst = np.argsort(L.a_dst, kind="stable")
    first = np.searchsorted(L.a_dst[by_dst], np.arange(L.n_states + 1))
    gb, ab = L.a_graph.astype(F32).view(np.uint32), L.a_ac.astype(F32).view(np.uint32)
    for j, q in enumerate(live):
        out[q] = _trace(L, todo[j], d[:, j, :], val, by_dst, first, gb, ab, sil_tids)
    return out


def align(L, words, sil_tids=None):
    """dict(found, begin, end, tot, lm, n_arcs, arcs, tie): the cheapest path of L that spells `words`; arcs = its arc indices front
    to back; tie = some decision on it (the end state or an in-arc) had more than one exact candidate"""
    return align_many(L, [words], sil_tids)[0]


def _trace(L, w, d, val, by_dst, first, gb, ab, sil_tids):
    n = len(w)
    fin = np.nonzero(L.st_final)[0]
    fin = fin[np.isfinite(d[fin, n])]
    if len(fin) == 0:
        return dict(found=False)
    best = d[fin, n].min()
    ends = fin[d[fin, n] == best]
    tie = len(ends) > 1
    t = int(ends[np.argmin(L.st_gstate[ends])])
    end_state, k, arcs = t, n, []
    while t != L.start:
        cands = []
        for a in by_dst[first[t]:first[t + 1]]:
            o = int(L.a_ol[a])
            if o == 0:
                kk = k
            elif k > 0 and o == w[k - 1]:
                kk = k - 1
            else:
                continue
            s = int(L.a_src[a])
            v = F32(F32(d[s, kk] + val[a]) + F32(0.0))
            if np.isfinite(v) and v == d[t, k]:
                cands.append(((int(L.a_il[a] == 0), int(L.st_gstate[s]), int(L.a_il[a]), o, int(gb[a]), int(ab[a])), int(a), s, kk))
        assert cands, "a reached cell without the arrival that made it"
        tie = tie or len(cands) > 1
        _, a, t, k = min(cands)
        arcs.append(a)
    assert k == 0
    arcs.reverse()
    arcs = np.array(arcs, np.int64)
    lm = F32(0.0)
    for a in arcs:
        lm = F32(lm + L.a_graph[a])
    fr = L.st_frame[L.a_src[arcs]].astype(np.int64) if len(arcs) else np.zeros(0, np.int64)
    il = L.a_il[arcs] if len(arcs) else np.zeros(0, np.int64)
    j = np.nonzero(L.a_ol[arcs])[0] if len(arcs) else np.zeros(0, np.int64)
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
    return dict(found=True, begin=begin, end=end, tot=F32(d[end_state, n]), lm=lm, n_arcs=len(arcs), arcs=arcs, tie=bool(tie))
