"""The definition of wfst_decoder_nearest_words (include/wfst_decoder.h) restated in numpy over a raw lattice: the tables of
(errors, cost) cells, the traceback with its kind order and tie rule, the edit counts, the hypothesis words and their begin and end
frames (silence-trimmed where a silence list is given), ref_hyp.

A lattice is what tests/align_util.py takes (pyoracle.RawLattice, from_gpu(), make_lattice()): every arc goes to a higher state id.
A cell is one unsigned 64-bit word, errors in the high half and the cost's orderable float32 bits in the low half, so that the
lexicographic order of (errors, cost) is the order of the words; UNREACHED is greater than every cell.  All sums are float32:
d' = (d + (graph + acoustic)) + 0.0, a d' that is not finite being no transition."""
import numpy as np

from align_util import from_gpu, make_lattice  # noqa: F401  (re-exported: the lattice objects are align_util's)

F32 = np.float32
U64 = np.uint64
UNREACHED = U64(0xFFFFFFFFFFFFFFFF)
ONE = U64(1 << 32)   # one error
KINDS = ("match/sub", "free", "ins", "del")


def f2o(x):
    """float32 -> uint32 whose unsigned order is the floats' order"""
    u = np.asarray(x, F32).view(np.uint32)
    return np.where(u >> np.uint32(31), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def o2f(o):
    o = np.asarray(o, np.uint32)
    return np.where(o >> np.uint32(31), o ^ np.uint32(0x80000000), ~o).astype(np.uint32).view(F32)


def pack(e, d):
    return (np.asarray(e).astype(U64) << U64(32)) | f2o(d).astype(U64)


def unpack(p):
    """(errors, cost) of a reached cell"""
    p = U64(p)
    return int(p >> U64(32)), F32(o2f(np.uint32(p & U64(0xFFFFFFFF))))


def _levels(L):
    """a level = the states of one frame at one depth along the arcs inside the frame (ilabel 0): every arc into a level leaves a
    finished one"""
    S = L.n_states
    src, dst = L.a_src.astype(np.int64), L.a_dst.astype(np.int64)
    assert len(src) == 0 or np.all(dst > src), "arcs must go to higher state ids"
    depth = np.zeros(S, np.int64)
    eps = np.nonzero(L.a_il == 0)[0]
    for a in eps[np.argsort(src[eps], kind="stable")]:
        depth[dst[a]] = max(depth[dst[a]], depth[src[a]] + 1)
    level = L.st_frame.astype(np.int64) * (int(depth.max()) + 1 if S else 1) + depth
    assert len(src) == 0 or np.all(level[dst] > level[src])
    return level


def _scan(rows):
    """the deletion step along the last axis: rows[..., k] = min_j<=k (rows[..., j] + (k - j) errors)"""
    for k in range(1, rows.shape[-1]):
        prev = rows[..., k - 1]
        step = np.where(prev == UNREACHED, UNREACHED, prev + ONE)
        rows[..., k] = np.minimum(rows[..., k], step)
    return rows


def tables(L, refs):
    """v[state][reference][k] (packed cells) for all the references at once, and the arcs' costs.  Columns beyond a reference's own
    length hold cells of no meaning (nothing at k <= its length depends on them)."""
    S, Q = L.n_states, len(refs)
    W = 1 + max([len(r) for r in refs] + [0])
    words = np.full((Q, W), -1, np.int64)   # words[q][k]: the reference word between column k and k + 1
    for q, r in enumerate(refs):
        words[q, :len(r)] = r
    src, dst = L.a_src.astype(np.int64), L.a_dst.astype(np.int64)
    level = _levels(L)
    val = (L.a_graph.astype(F32) + L.a_ac.astype(F32)).astype(F32)
    v = np.full((S, Q, W), UNREACHED, U64)
    v[L.start, :, 0] = pack(0, F32(0.0))
    _scan(v[L.start])
    order = np.argsort(level[dst], kind="stable")
    cuts = np.nonzero(np.diff(level[dst][order]))[0] + 1
    with np.errstate(over="ignore", invalid="ignore"):
        for grp in (np.split(order, cuts) if len(order) else []):
            ps = v[src[grp]]                                        # [arcs][Q][W]
            e = ps >> U64(32)
            d = o2f((ps & U64(0xFFFFFFFF)).astype(np.uint32))
            dn = ((d + val[grp][:, None, None]).astype(F32) + F32(0.0)).astype(F32)
            ok = (ps != UNREACHED) & np.isfinite(dn)
            lo = f2o(dn).astype(U64)
            o = L.a_ol[grp].astype(np.int64)
            word = (o != 0)[:, None, None]
            same_k = np.where(ok, ((e + word.astype(U64)) << U64(32)) | lo, UNREACHED)   # free arc, or insertion
            cand = same_k
            miss = (words[None, :, :-1] != o[:, None, None]).astype(U64)
            diag = np.where(ok[:, :, :-1] & word, ((e[:, :, :-1] + miss) << U64(32)) | lo[:, :, :-1], UNREACHED)   # match / substitution
            cand[:, :, 1:] = np.minimum(cand[:, :, 1:], diag)
            np.minimum.at(v, dst[grp], cand)
            t = np.unique(dst[grp])
            v[t] = _scan(v[t])
    return v, val


def nearest_many(L, refs, sil_tids=None):
    """nearest() of every reference of `refs` over one lattice (the tables are computed together); None entries are skipped"""
    if L is None or L.n_states == 0:
        return [None if r is None else dict(found=False) for r in refs]
    out = [None] * len(refs)
    live = [q for q, r in enumerate(refs) if r is not None]
    if not live:
        return out
    todo = [[int(x) for x in refs[q]] for q in live]
    v, val = tables(L, todo)
    by_dst = np.argsort(L.a_dst, kind="stable")
    first = np.searchsorted(L.a_dst[by_dst], np.arange(L.n_states + 1))
    gb, ab = L.a_graph.astype(F32).view(np.uint32), L.a_ac.astype(F32).view(np.uint32)
    for j, q in enumerate(live):
        out[q] = _trace(L, todo[j], v[:, j, :], val, by_dst, first, gb, ab, sil_tids)
    return out


def nearest(L, ref, sil_tids=None):
    """dict(found, n_err, n_cor, n_sub, n_ins, n_del, n_arcs, n_hyp, hyp_words, begin, end, ref_hyp, tot, lm, arcs, ops, tie): the
    lattice path nearest `ref`.  arcs = its arc indices front to back; ops = the traceback's steps front to back as (kind, arc or
    -1); tie = some decision (the end state or a predecessor) had more than one exact candidate"""
    return nearest_many(L, [ref], sil_tids)[0]


def _extend(cell, c):
    """the cell's cost over an arc of cost c: (errors, orderable bits of d') or None where that is no transition"""
    if cell == UNREACHED:
        return None
    e, d = unpack(cell)
    with np.errstate(over="ignore", invalid="ignore"):
        dn = F32(F32(d + c) + F32(0.0))
    if not np.isfinite(dn):
        return None
    return e, int(f2o(dn))


def _trace(L, r, v, val, by_dst, first, gb, ab, sil_tids):
    n = len(r)
    fin = np.nonzero(L.st_final)[0]
    fin = fin[v[fin, n] != UNREACHED]
    if len(fin) == 0:
        return dict(found=False)
    best = v[fin, n].min()
    ends = fin[v[fin, n] == best]
    tie = len(ends) > 1
    t = int(ends[np.argmin(L.st_gstate[ends])])
    end_state, k, ops = t, n, []
    n_err, tot = unpack(best)
    while (t, k) != (L.start, 0):
        here = int(v[t, k])
        cands = []
        for a in by_dst[first[t]:first[t + 1]]:
            a = int(a)
            o, s = int(L.a_ol[a]), int(L.a_src[a])
            tup = (int(L.a_il[a] == 0), int(L.st_gstate[s]), int(L.a_il[a]), o, int(gb[a]), int(ab[a]))
            if o != 0 and k > 0:
                x = _extend(v[s, k - 1], val[a])
                if x is not None and ((x[0] + (o != r[k - 1])) << 32) | x[1] == here:
                    cands.append(((0,) + tup, a, s, k - 1))
            x = _extend(v[s, k], val[a])
            if x is not None and ((x[0] + (o != 0)) << 32) | x[1] == here:
                cands.append(((1 if o == 0 else 2,) + tup, a, s, k))
        if k > 0 and v[t, k - 1] != UNREACHED and int(v[t, k - 1]) + (1 << 32) == here:
            cands.append(((3,), -1, t, k - 1))
        assert cands, "a reached cell without the arrival that made it"
        tie = tie or len(cands) > 1
        key, a, t, k = min(cands)
        ops.append((key[0], a))
    ops.reverse()
    arcs = np.array([a for _, a in ops if a >= 0], np.int64)
    cnt = dict(cor=0, sub=0, ins=0, dele=0)
    hyp, ref_hyp, kk = [], [], 0
    lm = F32(0.0)
    check = F32(0.0)
    for kind, a in ops:
        if kind == 3:
            cnt["dele"] += 1
            ref_hyp.append(-1)
            kk += 1
            continue
        lm = F32(lm + L.a_graph[a])
        check = F32(F32(check + val[a]) + F32(0.0))
        if kind == 0:
            ok = int(L.a_ol[a]) == r[kk]
            cnt["cor" if ok else "sub"] += 1
            ref_hyp.append(len(hyp))
            kk += 1
        elif kind == 2:
            cnt["ins"] += 1
        if L.a_ol[a] != 0:
            hyp.append(int(L.a_ol[a]))
    assert kk == n and check.view(np.uint32) == tot.view(np.uint32) and cnt["sub"] + cnt["ins"] + cnt["dele"] == n_err
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
    return dict(found=True, n_err=n_err, n_cor=cnt["cor"], n_sub=cnt["sub"], n_ins=cnt["ins"], n_del=cnt["dele"], n_arcs=len(arcs),
                n_hyp=len(hyp), hyp_words=np.array(hyp, np.int64), begin=begin, end=end, ref_hyp=np.array(ref_hyp, np.int64), tot=tot, lm=lm,
                arcs=arcs, ops=ops, tie=bool(tie))


def levenshtein(a, b):
    a, b = list(a), list(b)
    row = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        new = [i]
        for j, y in enumerate(b, 1):
            new.append(min(row[j] + 1, new[j - 1] + 1, row[j - 1] + (x != y)))
        row = new
    return row[-1]


def all_paths(L, limit=20000):
    """every path from the start to a final state as a list of arc indices (None if there are more than `limit`)"""
    out_arcs = [[] for _ in range(L.n_states)]
    for a in range(len(L.a_src)):
        out_arcs[int(L.a_src[a])].append(a)
    paths, stack = [], [(L.start, [])]
    while stack:
        s, p = stack.pop()
        if L.st_final[s]:
            paths.append(p)
            if len(paths) > limit:
                return None
        for a in out_arcs[s]:
            stack.append((int(L.a_dst[a]), p + [a]))
    return paths


def brute_force(L, ref, limit=20000):
    """the least (Levenshtein(words(p), ref), sequential float32 sum of the arcs' costs) over all paths p, or None: no path.  Returns
    the string 'too many' beyond `limit` paths."""
    paths = all_paths(L, limit)
    if paths is None:
        return "too many"
    val = (L.a_graph.astype(F32) + L.a_ac.astype(F32)).astype(F32)
    best = None
    with np.errstate(over="ignore", invalid="ignore"):
        for p in paths:
            d = F32(0.0)
            for a in p:
                d = F32(F32(d + val[a]) + F32(0.0))
                if not np.isfinite(d):
                    break
            else:
                key = (levenshtein([int(L.a_ol[a]) for a in p if L.a_ol[a]], ref), int(f2o(d)))
                if best is None or key < best:
                    best = key
    return None if best is None else (best[0], F32(o2f(np.uint32(best[1]))))
