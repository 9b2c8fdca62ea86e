"""The definition of wfst_decoder_word_confidence (include/wfst_decoder.h) restated in numpy over a raw lattice: the forward and
backward costs in the log semiring, the arcs' posteriors, the cells cut at the midpoints of the aligned words' begin frames, the
words' posterior mass, the aligned path's own log posterior -- and the tolerance the device's answer is held to, derived from the
lattice at hand.

A lattice is what tests/align_util.py takes (pyoracle.RawLattice, from_gpu(), make_lattice()): every arc goes to a higher state id.
All arithmetic is float64: c(a) = graph_scale * graph + acoustic_scale * acoustic; an arc whose float32 graph + acoustic is not
finite is no arc; every sum is m - log(sum exp(-(x - m))) with m the least term; a state without a finite term is +inf and its arcs
have posterior 0."""
import math

import numpy as np

from align_util import align_many, make_lattice

F32 = np.float32
EPS = 2.0 ** -52


def levels_of(L):
    """a level = the states of one frame at one depth along the arcs inside the frame (ilabel 0): every arc into a level leaves a
    finished one (align_util._tables' levels)"""
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


def arc_costs(L, graph_scale, acoustic_scale):
    """(c(a) in float64, "is an arc")"""
    with np.errstate(over="ignore", invalid="ignore"):
        ok = np.isfinite((L.a_graph.astype(F32) + L.a_ac.astype(F32)).astype(F32))
        c = float(graph_scale) * L.a_graph.astype(np.float64) + float(acoustic_scale) * L.a_ac.astype(np.float64)
    return c, ok


def _logsum_into(val, key, x, use):
    """val[j] = m - log(sum exp(-(x - m))) over the entries with key == j that are in use and finite, for every j that has one
    (x may already hold a term per j: pass it in val as a finite number)"""
    use = use & np.isfinite(x)
    k, x = key[use], x[use]
    m = np.full(len(val), np.inf)
    have = np.isfinite(val)
    m[have] = val[have]
    np.minimum.at(m, k, x)
    s = np.zeros(len(val))
    s[have] = np.exp(-(val[have] - m[have]))
    np.add.at(s, k, np.exp(-(x - m[k])))
    out = np.full(len(val), np.inf)
    got = s > 0
    out[got] = m[got] - np.log(s[got])
    return out


def posteriors(L, graph_scale=1.0, acoustic_scale=1.0):
    """dict(alpha, beta, log_z, gamma, c, ok, n_levels, A, tol_log)"""
    S = L.n_states
    src, dst = L.a_src.astype(np.int64), L.a_dst.astype(np.int64)
    level = levels_of(L)
    c, ok = arc_costs(L, graph_scale, acoustic_scale)
    alpha = np.full(S, np.inf)
    alpha[L.start] = 0.0
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        order = np.argsort(level[dst], kind="stable")
        cuts = np.nonzero(np.diff(level[dst][order]))[0] + 1
        for grp in (np.split(order, cuts) if len(order) else []):
            t = np.unique(dst[grp])
            idx = np.searchsorted(t, dst[grp])
            alpha[t] = _logsum_into(np.full(len(t), np.inf), idx, alpha[src[grp]] + c[grp], ok[grp])
        alpha[L.start] = 0.0
        # beta: [s final] is a term of cost 0; the states level by level from the last
        beta = np.where(np.asarray(L.st_final) != 0, 0.0, np.inf)
        order = np.argsort(-level[src], kind="stable")
        cuts = np.nonzero(np.diff(level[src][order]))[0] + 1
        for grp in (np.split(order, cuts) if len(order) else []):
            s = np.unique(src[grp])
            idx = np.searchsorted(s, src[grp])
            beta[s] = _logsum_into(beta[s], idx, c[grp] + beta[dst[grp]], ok[grp])
        log_z = -beta[L.start]
        x = alpha[src] + c + beta[dst] + log_z
        gamma = np.where(ok & np.isfinite(x), np.exp(-np.where(np.isfinite(x), x, 0.0)), 0.0)
    fin = np.concatenate([alpha[np.isfinite(alpha)], beta[np.isfinite(beta)]])
    A = float(np.abs(fin).max()) if len(fin) else 0.0
    n_levels = len(np.unique(level))
    return dict(alpha=alpha, beta=beta, log_z=float(log_z), gamma=gamma, c=c, ok=ok, n_levels=n_levels, A=A,
                tol_log=8.0 * (n_levels + 2) * EPS * max(1.0, A))


def tol_word(P, L, value):
    """the tolerance of one word_post value: alpha, beta and log_z each enter gamma's exponent, and up to every arc is added"""
    return 4.0 * P["tol_log"] * max(1.0, abs(float(value))) + len(L.a_src) * EPS


def cuts_of(begin):
    """m[0..L]: m[0] = 0, m[k] = (b[k - 1] + b[k] + 1) >> 1, m[L] = +inf (here: the largest int64)"""
    b = [int(x) for x in begin]
    return [0] + [(b[k - 1] + b[k] + 1) >> 1 for k in range(1, len(b))] + [np.iinfo(np.int64).max]


def confidence_many(L, seqs, graph_scale=1.0, acoustic_scale=1.0, sil_tids=None, post=None, aligned=None):
    """word_confidence() of every sequence of `seqs` over one lattice; None entries are skipped.  Per sequence align_util's dict plus
    word_post (float64 array), conf = min(1, word_post), path_logpost, log_z; found = False: word_post empty, path_logpost 0.
    post / aligned: posteriors() at these scales / align_many() of these sequences, where the caller has them already."""
    al = [None if r is None else dict(r) for r in aligned] if aligned is not None else align_many(L, seqs, sil_tids)
    if L is None or L.n_states == 0:
        return al
    P = post if post is not None else posteriors(L, graph_scale, acoustic_scale)
    fr = L.st_frame[L.a_src].astype(np.int64)
    ol = L.a_ol.astype(np.int64)
    for w, r in zip(seqs, al):
        if r is None:
            continue
        r["log_z"] = P["log_z"]
        if not r["found"]:
            r.update(word_post=np.zeros(0), conf=np.zeros(0), path_logpost=0.0)
            continue
        m = cuts_of(r["begin"])
        wp = np.zeros(len(w))
        for k, word in enumerate(w):
            wp[k] = P["gamma"][(ol == int(word)) & (fr >= m[k]) & (fr < m[k + 1])].sum()
        cost = 0.0
        for a in r["arcs"]:
            cost += float(P["c"][a])
        r.update(word_post=wp, conf=np.minimum(1.0, wp), path_logpost=-P["log_z"] - cost)
    return al


def confidence(L, words, graph_scale=1.0, acoustic_scale=1.0, sil_tids=None):
    return confidence_many(L, [words], graph_scale, acoustic_scale, sil_tids)[0]


# ---- the enumeration of every path ---------------------------------------------------------------------------------------------
def brute_force(L, paths, graph_scale, acoustic_scale):
    """(log_z, gamma per arc) from the paths themselves: weights math.fsum of exp(-(cost - min)); (-inf, zeros) without a path"""
    c, ok = arc_costs(L, graph_scale, acoustic_scale)
    good = [p for p in paths if all(ok[a] for a in p)]
    if not good:
        return -math.inf, np.zeros(len(L.a_src))
    cost = [math.fsum(float(c[a]) for a in p) for p in good]
    lo = min(cost)
    w = [math.exp(-(x - lo)) for x in cost]
    z = math.fsum(w)
    parts = [[] for _ in range(len(L.a_src))]
    for p, x in zip(good, w):
        for a in p:
            parts[a].append(x)
    return -lo + math.log(z), np.array([math.fsum(x) / z for x in parts])


def random_lattice(rs, quantised):
    """tests/test_nearest_restatement.py's recipe: 2..5 frames of 1..3 states; emitting arcs from a frame to the next, arcs inside a
    frame (ilabel 0) to a higher state, with and without words; costs from a handful of quarters or arbitrary"""
    T = rs.randint(2, 6)
    frames = [[0]]
    states = [(0, 0, 0)]
    for f in range(1, T + 1):
        ids = []
        for _ in range(rs.randint(1, 4)):
            ids.append(len(states))
            states.append((f, rs.randint(0, 4), int(f == T and rs.rand() < 0.7)))
        frames.append(ids)
    if not any(s[2] for s in states):
        states[-1] = (T, states[-1][1], 1)
    cost = (lambda: 0.25 * rs.randint(-2, 5)) if quantised else (lambda: float(F32(rs.normal(1.0, 2.0))))
    word = lambda: int(rs.choice([0, 0, 1, 2, 3]))
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


def without_arc(L, a):
    """L with arc a removed"""
    from types import SimpleNamespace
    keep = np.arange(len(L.a_src)) != a
    d = dict(vars(L))
    for k in ("a_src", "a_dst", "a_il", "a_ol", "a_graph", "a_ac"):
        d[k] = np.asarray(d[k])[keep]
    return SimpleNamespace(**d)


# ---- a device answer against the restatement -------------------------------------------------------------------------------------
def compare(got, want, P, L, what=""):
    """one (channel, sequence) dict of BatchDecoder.word_confidences against confidence_many's; returns the largest
    difference / tolerance seen.  Integer outputs and align's float32 scores are compared exactly."""
    if want is None:
        want = dict(found=False)
    assert got["found"] == bool(want["found"]), what + " found"
    if not want["found"]:
        assert got["n_arcs"] == 0 and not got["begin"].any() and not got["end"].any() and float(got["tot"]) == 0 and float(got["lm"]) == 0, what
        assert not np.asarray(got["word_post"]).any() and got["path_logpost"] == 0.0, what
        return 0.0
    assert got["n_arcs"] == want["n_arcs"], what + " n_arcs"
    assert np.array_equal(got["begin"], want["begin"]) and np.array_equal(got["end"], want["end"]), what + " frames"
    assert np.asarray([got["tot"], got["lm"]], F32).tobytes() == np.asarray([want["tot"], want["lm"]], F32).tobytes(), what + " scores"
    worst = abs(got["path_logpost"] - want["path_logpost"]) / P["tol_log"]
    assert len(got["word_post"]) == len(want["word_post"]), what
    for k, (x, y) in enumerate(zip(got["word_post"], want["word_post"])):
        assert np.isfinite(x), what
        worst = max(worst, abs(float(x) - float(y)) / tol_word(P, L, y))
    assert np.array_equal(got["conf"], np.minimum(1.0, got["word_post"])), what + " clamp"
    return float(worst)
