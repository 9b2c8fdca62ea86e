"""Graph posteriors (wfst_decoder_graph_posteriors): the numpy restatement of the header's recursion, level by level, the enumeration
of every path in float64, the tolerance and compare().  Pure numpy on top of force_align_util (graphs, sources, eps_levels): no
device, no library."""
import numpy as np

import force_align_util as FU
from force_align_util import *   # noqa: F401,F403  (the graph makers, for the tests that import this module as U)

# the header's constant (tests/test_graph_post_surface.py holds the two to each other)
WFST_GPOST_LDS_STATES = 2048

F32, F64 = np.float32, np.float64
EPS = 2.0 ** -52


def out_levels(g):
    """Per state the longest epsilon path OUT of it (0: no epsilon out-arc)."""
    src, a = FU.sources(g), g.arcs
    e = np.nonzero(a["ilabel"] == 0)[0]
    level = np.zeros(g.n_states, np.int64)
    for _ in range(g.n_states + 1):
        new = level.copy()
        if len(e):
            np.maximum.at(new, src[e], level[a["to"][e].astype(np.int64)] + 1)
        if (new == level).all():
            return level
        level = new
    raise AssertionError("an epsilon cycle")


def _logsum_by(key, x, n):
    """Per key -log sum exp(-x) over its finite terms, m - log(sum exp(-(x - m))) with m the least; +inf without one."""
    ok = np.isfinite(x)
    key, x = key[ok], x[ok]
    m = np.full(n, np.inf)
    np.minimum.at(m, key, x)
    s = np.zeros(n)
    np.add.at(s, key, np.exp(-(x - m[key])))
    out = np.full(n, np.inf)
    has = np.isfinite(m)
    out[has] = m[has] - np.log(s[has])
    return out


def arc_costs(g, ll, T, tid2pdf=None, gs=1.0, as_=1.0):
    """c(f, a) as float64 [T][A] (+inf: no arc at that frame; the columns of epsilon arcs unused) and c(a) as float64 [A]."""
    a = g.arcs
    il, wt = a["ilabel"].astype(np.int64), a["w"].astype(F32)
    col = il if tid2pdf is None else np.asarray(tid2pdf, np.int64)[il]
    emit = il != 0
    with np.errstate(all="ignore"):
        wok = np.isfinite(wt)
        gc = F64(gs) * wt.astype(F64)
        c_eps = np.where(wok & ~emit, gc, np.inf)
        c_emit = np.full((T, len(a)), np.inf)
        if T > 0 and emit.any():
            x = (-np.asarray(ll, F32)[:T][:, col[emit]]).astype(F32)
            c = F64(as_) * x.astype(F64) + gc[emit][None, :]
            c_emit[:, emit] = np.where(np.isfinite(x) & wok[emit][None, :], c, np.inf)
    return c_emit, c_eps


def graph_posteriors(g, ll, T=None, tid2pdf=None, label_map=None, gs=1.0, as_=1.0, min_post=0.0):
    """The header's forward-backward in numpy float64.  Returns a dict: found, n_frames, log_like, post ([T][n_class] dense), frame_off,
    classes, posts, n_distinct, frame_mass, arc_occ, alpha, beta, the per-class arc counts k_class and tol_log."""
    ll = np.asarray(ll, dtype=F32)
    T = int(ll.shape[0]) if T is None else int(T)
    S, a = g.n_states, g.arcs
    A = len(a)
    src, dst = FU.sources(g), a["to"].astype(np.int64)
    il = a["ilabel"].astype(np.int64)
    emit, eps = np.nonzero(il != 0)[0], np.nonzero(il == 0)[0]
    cls = il if label_map is None else np.asarray(label_map, np.int64)[il]
    n_class = int(cls[emit].max()) + 1 if len(emit) else 1
    level, blevel = FU.eps_levels(g), out_levels(g)
    assert level is not None, "an epsilon cycle"
    c_emit, c_eps = arc_costs(g, ll, T, tid2pdf, gs, as_)
    alpha, beta = np.full((T + 1, S), np.inf), np.full((T + 1, S), np.inf)
    with np.errstate(all="ignore"):
        for f in range(T + 1):
            for L in range(int(level.max()) + 1):
                keys, xs = [], []
                if f == 0 and level[g.start] == L:
                    keys.append(np.array([g.start])); xs.append(np.array([0.0]))
                if f > 0:
                    e = emit[level[dst[emit]] == L]
                    keys.append(dst[e]); xs.append(alpha[f - 1, src[e]] + c_emit[f - 1, e])
                e = eps[level[dst[eps]] == L]
                keys.append(dst[e]); xs.append(alpha[f, src[e]] + c_eps[e])
                v = _logsum_by(np.concatenate(keys), np.concatenate(xs), S)
                at = level == L
                alpha[f, at] = v[at]
        tot = alpha[T, g.final_state]
        found = bool(np.isfinite(tot))
        for f in range(T, -1, -1):
            for L in range(int(blevel.max()) + 1):
                keys, xs = [], []
                if f == T and blevel[g.final_state] == L:
                    keys.append(np.array([g.final_state])); xs.append(np.array([0.0]))
                if f < T:
                    e = emit[blevel[src[emit]] == L]
                    keys.append(src[e]); xs.append(c_emit[f, e] + beta[f + 1, dst[e]])
                e = eps[blevel[src[eps]] == L]
                keys.append(src[e]); xs.append(c_eps[e] + beta[f, dst[e]])
                v = _logsum_by(np.concatenate(keys), np.concatenate(xs), S)
                at = blevel == L
                beta[f, at] = v[at]
    k_class = np.bincount(cls[emit], minlength=n_class) if len(emit) else np.zeros(n_class, np.int64)
    fin = np.concatenate([alpha[np.isfinite(alpha)], beta[np.isfinite(beta)], [0.0]])
    n_levels = (T + 1) * (int(level.max()) + 1)
    tol_log = 8.0 * (n_levels + 2) * EPS * max(1.0, float(np.abs(fin).max()))
    out = dict(found=found, n_frames=0, log_like=0.0, post=np.zeros((T, n_class)), frame_off=np.zeros(1, np.int32),
               classes=np.zeros(0, np.int32), posts=np.zeros(0), n_distinct=np.zeros(0, np.int32), frame_mass=np.zeros(0),
               arc_occ=np.zeros(A), alpha=alpha, beta=beta, k_class=k_class, tol_log=tol_log, eps_depth=int(level.max()))
    if not found:
        return out
    post, occ = np.zeros((T, n_class)), np.zeros(A)
    with np.errstate(all="ignore"):
        for f in range(T + 1):
            if f < T:
                x = ((alpha[f, src[emit]] + c_emit[f, emit]) + beta[f + 1, dst[emit]]) - tot
                gam = np.where(np.isfinite(x), np.exp(-x), 0.0)
                np.add.at(post[f], cls[emit], gam)
                occ[emit] += gam
            x = ((alpha[f, src[eps]] + c_eps[eps]) + beta[f, dst[eps]]) - tot
            occ[eps] += np.where(np.isfinite(x), np.exp(-x), 0.0)
    off, cl, po = [0], [], []
    for f in range(T):
        keep = np.nonzero((post[f] > 0) & (post[f] >= min_post))[0]
        cl.extend(keep.tolist()); po.extend(post[f, keep].tolist()); off.append(len(cl))
    out.update(n_frames=T, log_like=float(-tot), post=post, frame_off=np.array(off, np.int32), classes=np.array(cl, np.int32),
               posts=np.array(po, F64), n_distinct=(post > 0).sum(axis=1).astype(np.int32), frame_mass=post.sum(axis=1), arc_occ=occ)
    return out


def enumerate_posteriors(g, ll, T, tid2pdf=None, label_map=None, gs=1.0, as_=1.0):
    """Every path of exactly T emitting arcs from start to final_state over the arcs that are arcs, its cost the float64 sum of its
    arcs' costs: found, n_paths, log_like, post [T][n_class], arc_occ."""
    a = g.arcs
    off = g.row_offsets()
    il = a["ilabel"].astype(np.int64)
    cls = il if label_map is None else np.asarray(label_map, np.int64)[il]
    n_class = int(cls[il != 0].max()) + 1 if (il != 0).any() else 1
    c_emit, c_eps = arc_costs(g, ll, T, tid2pdf, gs, as_)
    paths = []

    def walk(s, f, cost, hops):
        if f == T and s == g.final_state:
            paths.append((cost, tuple(hops)))
        for k in range(int(off[s]), int(off[s + 1])):
            if il[k] != 0:
                if f == T:
                    continue
                c = c_emit[f, k]
            else:
                c = c_eps[k]
            if not np.isfinite(c):
                continue
            hops.append((f, k))
            walk(int(a["to"][k]), f + (il[k] != 0), cost + c, hops)
            hops.pop()
    walk(g.start, 0, 0.0, [])
    out = dict(found=bool(paths), n_paths=len(paths), log_like=0.0, post=np.zeros((T, n_class)), arc_occ=np.zeros(len(a)))
    if not paths:
        return out
    costs = np.array([p[0] for p in paths])
    m = costs.min()
    tot = m - np.log(np.exp(-(costs - m)).sum())
    for cost, hops in paths:
        p = np.exp(-(cost - tot))
        for f, k in hops:
            out["arc_occ"][k] += p
            if il[k] != 0:
                out["post"][f, cls[k]] += p
    out["log_like"] = float(-tot)
    return out


def hop_cost(g, ll, hops, tid2pdf=None, gs=1.0, as_=1.0):
    """The float64 cost of a hop list (force_align's hop_arc) under the header's arc costs."""
    il = g.arcs["ilabel"].astype(np.int64)
    T = int((il[np.asarray(hops, np.int64)] != 0).sum()) if len(hops) else 0
    c_emit, c_eps = arc_costs(g, ll, T, tid2pdf, gs, as_)
    cost, f = 0.0, 0
    for k in hops:
        if il[k] != 0:
            cost += c_emit[f, k]
            f += 1
        else:
            cost += c_eps[k]
    return cost


def post_tol(want, v, k):
    return 4.0 * want["tol_log"] * np.maximum(1.0, np.abs(v)) + k * EPS


def compare_dense(post, occ, log_like, found, want, what=""):
    """(found, log_like, post [T][n_class], arc_occ or None) against the restatement's dict; the largest difference / tolerance."""
    assert found == want["found"], (what, found, want["found"])
    if not want["found"]:
        assert log_like == 0.0 and not np.any(post) and (occ is None or not np.any(occ)), what
        return 0.0
    T = want["post"].shape[0]
    worst = abs(log_like - want["log_like"]) / want["tol_log"]
    assert worst <= 1.0, (what, "log_like", log_like, want["log_like"], worst)
    if T:
        n = max(post.shape[1], want["post"].shape[1])
        a, b = np.zeros((T, n)), np.zeros((T, n))
        a[:, :post.shape[1]] = post
        b[:, :want["post"].shape[1]] = want["post"]
        k = np.zeros(n)
        k[:len(want["k_class"])] = want["k_class"]
        r = np.abs(a - b) / post_tol(want, b, k[None, :])
        assert r.max() <= 1.0, (what, "post", np.unravel_index(r.argmax(), r.shape), r.max())
        worst = max(worst, float(r.max()))
    if occ is not None:
        r = np.abs(occ - want["arc_occ"]) / ((T + 1) * post_tol(want, want["arc_occ"], 1))
        assert r.max(initial=0.0) <= 1.0, (what, "arc_occ", int(r.argmax()), r.max())
        worst = max(worst, float(r.max(initial=0.0)))
    return worst


def dense_of(r, n_class):
    """The lists of a GraphPosteriors (or the restatement's dict) as post [n_frames][n_class]."""
    off, cl, po = np.asarray(r["frame_off"], np.int64), np.asarray(r["classes"], np.int64), np.asarray(r["posts"], F64)
    T = len(off) - 1
    out = np.zeros((T, max(n_class, int(cl.max()) + 1 if len(cl) else 1)))
    out[np.repeat(np.arange(T), np.diff(off)), cl] = po
    return out


def compare(got, want, what="", min_post=0.0):
    """A GraphPosteriors of the binding against the restatement's dict: found, n_frames, log_like, the lists (membership through the
    tolerance at the threshold), n_distinct, frame_mass and arc_occ where there is one.  Returns the largest difference / tolerance."""
    assert got.status == 0, (what, got.status)
    assert got.found == want["found"], (what, got.found, want["found"])
    if not want["found"]:
        assert got.n_frames == 0 and got.log_like == 0.0 and got.n_entries == 0, what
        assert len(got.classes) == 0 and len(got.posts) == 0 and len(got.frame_mass) == 0 and len(got.n_distinct) == 0, what
        assert got.arc_occ is None or not np.any(got.arc_occ), what
        return 0.0
    T = want["n_frames"]
    assert got.n_frames == T and len(got.frame_off) == T + 1 and got.n_entries == len(got.classes) == int(got.frame_off[-1]), what
    assert all(np.all(np.diff(got.classes[got.frame_off[f]:got.frame_off[f + 1]]) > 0) for f in range(T)), (what, "class order")
    assert np.all(got.posts > 0) and np.all(got.posts >= min_post), what
    n = want["post"].shape[1]
    have = dense_of(got, n)
    ref = want["post"].copy()
    if min_post > 0:   # an entry may fall on either side of the threshold by its tolerance
        k = want["k_class"][None, :]
        near = np.abs(ref - min_post) <= post_tol(want, ref, k)
        sure_out = (ref < min_post) & ~near
        assert not np.any(have[:, :n][sure_out]), (what, "listed below min_post")
        ref[sure_out] = 0.0
        ref[near & (have[:, :n] == 0)] = 0.0
    w2 = dict(want, post=ref)
    worst = compare_dense(have, got.arc_occ, got.log_like, got.found, w2, what)
    if min_post == 0:
        assert np.array_equal(got.n_distinct, np.diff(got.frame_off)), (what, "n_distinct against the lists")
    exact = (want["post"] > 4 * want["tol_log"]).sum(axis=1)
    assert np.all(got.n_distinct >= exact) and np.all(got.n_distinct <= (want["k_class"] > 0).sum()), (what, "n_distinct")
    r = np.abs(got.frame_mass - want["frame_mass"]) / post_tol(want, want["frame_mass"], want["k_class"].sum())
    assert r.max(initial=0.0) <= 1.0, (what, "frame_mass", r.max())
    return max(worst, float(r.max(initial=0.0)))
