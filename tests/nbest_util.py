"""The service's n-best on top of a raw lattice (SURVEY.md 8(f) rank 2 is not rebuilt; the reference's
own host functions run on the lattice this decoder returns).  Helper shared by the CPU and GPU
tests: write a lattice in the reference's on-disk format, run the reference pipeline
(oracle/_ref: Lattice::Read, LatticeCheckFormat, DeterminizeLatticeWrapper, NShortestPath,
ConvertNbestToVector, LatticeToVector) and compare with tests/golden/nbest_hclg600.npz, which holds
what the same pipeline gives on the REFERENCE decoder's own lattice."""
import os

import numpy as np

import pyoracle
from golden_util import GOLDEN_DIR


def golden_nbest(ci, ui):
    z = np.load(os.path.join(GOLDEN_DIR, "nbest_hclg600.npz"))
    key = "c%d_u%d_" % (ci, ui)
    lens = z[key + "lens"]
    words = np.split(z[key + "words"], np.cumsum(lens)[:-1]) if len(lens) else []
    return [(w, float(s[0]), float(s[1])) for w, s in zip(words, z[key + "scores"])], int(z["n"])


def check_nbest_of_lattice_bytes(ref, blob, ci, ui, tmp_path, what=""):
    want, n = golden_nbest(ci, ui)
    p = str(tmp_path / ("nbest_%d_%d.lat" % (ci, ui)))
    with open(p, "wb") as f:
        f.write(blob)
    got = pyoracle.ref_nbest_from_lattice_file(ref, p, 0, n)
    assert got is not None, what + " lattice rejected by the reference's LatticeCheckFormat / determinizer"
    paths = got[0]
    assert len(paths) == len(want), what + " number of paths"
    for k, (a, b) in enumerate(zip(paths, want)):
        assert np.array_equal(a[0], b[0]), "%s path %d words" % (what, k)
        assert abs(a[1] - b[1]) <= 1e-4 * abs(b[1]) and abs(a[2] - b[2]) <= 1e-4 * max(1.0, abs(b[2])), "%s path %d scores" % (what, k)


# ---- the two n-best kernels' own definitions, restated (asr-decoder_amd/csrc/wfst_nbest.hip) -------------------------------------
# Both are exact: np.float32 sums in the kernels' operation order, orders by the floats' orderable bits (nb_f2o: -0.0 sorts below
# +0.0), 64-bit history hashes as the device computes them.  A lattice is a pyoracle.RawLattice, align_util.from_gpu()'s object or
# the dict the decoder's getters return.
F32 = np.float32
U64 = np.uint64
ROOT_HASH = 0x243F6A8885A308D3
_M64 = (1 << 64) - 1


def mix_word(h, word):
    """the kernel's history hash step (splitmix64 finaliser), on Python integers"""
    z = ((h ^ (int(word) & 0xFFFFFFFF)) + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def _mix_words(h, word):
    """mix_word over arrays (uint64 arithmetic wraps as the device's does)"""
    z = (h ^ (word.astype(np.int64) & 0xFFFFFFFF).astype(U64)) + U64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def f2o(x):
    """float32 -> uint32 whose unsigned order is the floats' order (nb_f2o)"""
    u = np.asarray(x, F32).view(np.uint32)
    return np.where(u >> np.uint32(31), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _arrays(L):
    if isinstance(L, dict):
        L = dict(L)
        g = lambda k, alt: L[k] if k in L else L.get(alt)
        return (int(L["n_states"]), np.asarray(L["st_final"]), g("st_frame", "st_frame"), np.asarray(L["a_src"], np.int64), np.asarray(L["a_dst"], np.int64),
                np.asarray(g("a_olabel", "a_ol"), np.int64), np.asarray(g("a_graph", "a_graph"), F32), np.asarray(g("a_acoustic", "a_ac"), F32))
    return (int(L.n_states), np.asarray(L.st_final), getattr(L, "st_frame", None), np.asarray(L.a_src, np.int64), np.asarray(L.a_dst, np.int64),
            np.asarray(L.a_ol, np.int64), np.asarray(L.a_graph, F32), np.asarray(L.a_ac, F32))


def _select(tot, lm, hsh, K):
    """select_distinct over all candidates at once: per hash its least (tot, lm), then the K first by (tot, hash).  Indices into the
    candidates, and the number of distinct hashes.  (Entries of one list have distinct hashes, so lm never orders two of them.)"""
    to, lo = f2o(tot), f2o(lm)
    by_hash = np.lexsort((lo, to, hsh))
    first = by_hash[np.concatenate(([True], hsh[by_hash][1:] != hsh[by_hash][:-1]))] if len(by_hash) else by_hash
    keep = first[np.lexsort((hsh[first], to[first]))]
    return keep[:K], len(first)


def kbest_distinct(L, n, K=16, max_words=None, stats=None):
    """nbest_kernel restated: the min(n, K) cheapest DISTINCT word sequences of a raw lattice (state 0 the root, every arc to a
    higher state id: a topological order of the whole lattice, which is what the kernel's per-frame epsilon rounds converge to).
    Per state the up to K candidates with distinct history hashes that come first by (tot, hash, lm), equal hashes merged to their
    least (tot, lm); a candidate over an arc is tot = E.tot + (graph + acoustic), lm = E.lm + graph, hash = mix_word(E.hash, word)
    where the arc has a word.  The final states of the last frame are merged the same way.  Returns dicts(words, n_words, tot,
    lm), words cut to the first max_words where that is given.  stats (a dict) receives, per state, the candidate count `cands`,
    the distinct histories among them `distinct`, the list length `cnt`, `indeg`, `tie_at_K` (the K-th and K+1-th distinct
    candidates bit-equal in tot) and `merged_lm` (a history arriving twice with bit-equal tot and different lm), and for the final
    merge `final_states`, `final_cands`, `final_distinct` and `final_tots` (every distinct history's tot, in order)."""
    S, fin, frame, src, dst, ol, gr, ac = _arrays(L)
    assert len(src) == 0 or np.all(dst > src), "arcs must go to higher state ids"
    val = (gr + ac).astype(F32)
    by_dst = np.argsort(dst, kind="stable")
    first = np.searchsorted(dst[by_dst], np.arange(S + 1))
    tot, lm, hsh = [None] * S, [None] * S, [None] * S
    prev, word = [None] * S, [None] * S     # per entry: (source state, entry of its list) and the arc's word
    empty = lambda t: np.zeros(0, t)
    st = dict(cands=np.zeros(S, np.int64), distinct=np.zeros(S, np.int64), cnt=np.zeros(S, np.int64), indeg=np.diff(first),
              tie_at_K=np.zeros(S, bool), merged_lm=np.zeros(S, bool))

    def tie_and_merge(t, c_tot, c_lm, c_hsh, keep, distinct):
        if distinct > K:
            o = np.sort(np.array([int(f2o(c_tot[c_hsh == h]).min()) for h in np.unique(c_hsh)]))
            st["tie_at_K"][t] = o[K - 1] == o[K]
        for i in keep:
            same = (c_hsh == c_hsh[i]) & (f2o(c_tot) == f2o(c_tot[i]))
            if len(np.unique(f2o(c_lm[same]))) > 1:
                st["merged_lm"][t] = True

    for t in range(S):
        if t == 0:
            tot[t], lm[t], hsh[t] = np.zeros(1, F32), np.zeros(1, F32), np.array([ROOT_HASH], U64)
            prev[t], word[t] = np.array([[-1, -1]], np.int64), np.zeros(1, np.int64)
            st["cnt"][t] = 1
            continue
        arcs = by_dst[first[t]:first[t + 1]]
        arcs = arcs[[len(tot[s]) > 0 for s in src[arcs]]] if len(arcs) else arcs
        if len(arcs) == 0:
            tot[t], lm[t], hsh[t], prev[t], word[t] = empty(F32), empty(F32), empty(U64), np.zeros((0, 2), np.int64), empty(np.int64)
            continue
        c_tot = np.concatenate([(tot[src[a]] + val[a]).astype(F32) for a in arcs])
        c_lm = np.concatenate([(lm[src[a]] + gr[a]).astype(F32) for a in arcs])
        c_hsh = np.concatenate([_mix_words(hsh[src[a]], np.full(len(hsh[src[a]]), ol[a])) if ol[a] else hsh[src[a]] for a in arcs])
        c_prev = np.concatenate([np.stack([np.full(len(tot[src[a]]), src[a]), np.arange(len(tot[src[a]]))], 1) for a in arcs])
        c_word = np.concatenate([np.full(len(tot[src[a]]), ol[a]) for a in arcs])
        keep, distinct = _select(c_tot, c_lm, c_hsh, K)
        tot[t], lm[t], hsh[t], prev[t], word[t] = c_tot[keep], c_lm[keep], c_hsh[keep], c_prev[keep], c_word[keep]
        st["cands"][t], st["distinct"][t], st["cnt"][t] = len(c_tot), distinct, len(keep)
        if stats is not None:
            tie_and_merge(t, c_tot, c_lm, c_hsh, keep, distinct)
    nd = int(np.max(frame)) if S else 0
    ends = [t for t in range(S) if fin[t] and frame[t] == nd and len(tot[t])] if nd > 0 else []
    if stats is not None:
        stats.update(st)
        stats.update(final_states=len(ends), final_cands=int(sum(len(tot[t]) for t in ends)), final_distinct=0, final_tots=empty(F32))
    if not ends:
        return []
    c_tot, c_lm, c_hsh = (np.concatenate([x[t] for t in ends]) for x in (tot, lm, hsh))
    c_prev = np.concatenate([np.stack([np.full(len(tot[t]), t), np.arange(len(tot[t]))], 1) for t in ends])
    keep_all, distinct = _select(c_tot, c_lm, c_hsh, len(c_tot))
    if stats is not None:
        stats.update(final_distinct=distinct, final_tots=c_tot[keep_all])
    out = []
    for i in keep_all[:min(n, K)]:
        words = []
        s, e = c_prev[i]
        while s >= 0:
            if word[s][e]:
                words.append(int(word[s][e]))
            s, e = prev[s][e]
        words.reverse()
        out.append(dict(words=np.array(words[:max_words] if max_words else words, np.int32), n_words=len(words), tot=F32(c_tot[i]), lm=F32(c_lm[i])))
    return out


def kbest_paths_dp(D, n, stats=None):
    """nbest_paths_kernel restated: the n cheapest PATHS of a determinized or rescored lattice (state 0 the start).  Levels = the
    longest distance from state 0; level by level, a state's candidates are numbered q = 0, 1, ... over its in-arcs in ascending
    arc index and within an arc over the source's list in rank order, cost = E.cost + (graph + acoustic), and its list is the n
    first by (cost bits, q); the super-final state takes the final states in state order at cost + 0.  Returns dicts(arcs: arc
    indices front to back, olabel, graph, acoustic, tot).  stats receives `cands` per state and `final_cands`, and for the state
    of most candidates its candidates' costs in q order, `widest_costs`."""
    S, fin, _, src, dst, ol, gr, ac = _arrays(D)
    val = (gr + ac).astype(F32)
    level = np.full(S, -1, np.int64)
    if S:
        level[0] = 0
    for _ in range(S + 1):
        ok = level[src] >= 0
        new = level.copy()
        np.maximum.at(new, dst[ok], level[src[ok]] + 1)
        if np.array_equal(new, level):
            break
        level = new
    else:
        raise ValueError("a cycle: not a lattice")
    by_dst = np.argsort(dst, kind="stable")      # (stable: a state's in-arcs in ascending arc index)
    first = np.searchsorted(dst[by_dst], np.arange(S + 1))
    cost, back = [np.zeros(0, F32)] * S, [np.zeros((0, 2), np.int64)] * S   # back: (arc, rank in the source's list)
    cands = np.zeros(S, np.int64)
    widest = np.zeros(0, F32)

    def merge(c_cost, c_back):
        keep = np.argsort(f2o(c_cost), kind="stable")[:n]    # (stable: equal costs in candidate order)
        return c_cost[keep], c_back[keep]

    for t in sorted((t for t in range(S) if level[t] >= 0), key=lambda t: (level[t], t)):
        if t == 0:
            cost[t], back[t] = np.zeros(1, F32), np.array([[-1, 0]], np.int64)
            continue
        arcs = by_dst[first[t]:first[t + 1]]
        c_cost = np.concatenate([(cost[src[a]] + val[a]).astype(F32) for a in arcs])
        c_back = np.concatenate([np.stack([np.full(len(cost[src[a]]), a), np.arange(len(cost[src[a]]))], 1) for a in arcs])
        cands[t] = len(c_cost)
        if len(c_cost) > len(widest):
            widest = c_cost
        cost[t], back[t] = merge(c_cost, c_back)
    ends = [s for s in range(S) if fin[s] and level[s] >= 0 and len(cost[s])]
    if stats is not None:
        stats.update(cands=cands, final_cands=int(sum(len(cost[s]) for s in ends)), widest_costs=widest, level=level)
    if not ends:
        return []
    c_cost = np.concatenate([(cost[s] + F32(0.0)).astype(F32) for s in ends])
    c_back = np.concatenate([np.stack([np.full(len(cost[s]), s), np.arange(len(cost[s]))], 1) for s in ends])
    f_cost, f_back = merge(c_cost, c_back)
    out = []
    for c, (s, r) in zip(f_cost, f_back):
        arcs = []
        while True:
            a, r2 = back[s][r]
            if a < 0:
                break
            arcs.append(int(a))
            s, r = int(src[a]), int(r2)
        arcs.reverse()
        a = np.array(arcs, np.int64)
        out.append(dict(arcs=a, olabel=ol[a].astype(np.int32), graph=gr[a], acoustic=ac[a], tot=F32(c)))
    return out


# ---- the device's answers against the restatements': no tolerance anywhere -----------------------------------------------------
_bits = lambda x: int(np.asarray(x, F32).view(np.uint32))


def same_nbest(got, want, what):
    """BatchDecoder.nbest()'s list of one channel against kbest_distinct's: words, their order, n_words, the bits of both scores"""
    assert len(got) == len(want), "%s: %d sequences, the restatement has %d" % (what, len(got), len(want))
    for k, (a, b) in enumerate(zip(got, want)):
        assert a["words"].tolist() == b["words"].tolist() and a["n_words"] == b["n_words"], "%s rank %d: words %s / %s" % (what, k, a["words"].tolist(), b["words"].tolist())
        assert _bits(a["tot_score"]) == _bits(b["tot"]), "%s rank %d: tot_score %r / %r" % (what, k, a["tot_score"], float(b["tot"]))
        assert _bits(a["lm_score"]) == _bits(b["lm"]), "%s rank %d: lm_score %r / %r" % (what, k, a["lm_score"], float(b["lm"]))


def same_paths(got, want, what):
    """BatchDecoder.nbest_paths()'s list against kbest_paths_dp's: per-arc olabel and the bits of graph, acoustic and tot, in order"""
    assert len(got) == len(want), "%s: %d paths, the restatement has %d" % (what, len(got), len(want))
    for k, (a, b) in enumerate(zip(got, want)):
        assert a["olabel"].tolist() == b["olabel"].tolist(), "%s path %d: olabels" % (what, k)
        for key in ("graph", "acoustic"):
            assert np.array_equal(np.asarray(a[key], F32).view(np.uint32), np.asarray(b[key], F32).view(np.uint32)), "%s path %d: %s" % (what, k, key)
        assert _bits(a["tot"]) == _bits(b["tot"]), "%s path %d: tot %r / %r" % (what, k, a["tot"], float(b["tot"]))
