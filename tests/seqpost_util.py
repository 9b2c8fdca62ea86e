"""The definition of wfst_decoder_sequence_posterior (include/wfst_decoder.h) restated in numpy over a raw lattice: the table of
states x (L + 1) cells in the log semiring, the sentence posterior read from its last column (mode 0), the phrase's occurrences, their
count and hit_mass (mode 1) -- the enumeration of every path that the restatement itself is checked against, and the tolerance the
device's answer is held to, derived from the lattice at hand.

A lattice is what tests/posterior_util.py takes; alpha, beta, log_z, the arc costs, the "no arc" rule and the way a sum is taken are
posterior_util's.  All arithmetic is float64."""
import math

import numpy as np

from posterior_util import EPS, _logsum_into, levels_of, posteriors


def n_frames_of(L):
    """the state frames 0 .. frames decoded: the room a hit_mass row needs"""
    return int(np.asarray(L.st_frame).max()) + 1 if L.n_states else 0


def table(L, w, mode, P):
    """S[state][L + 1] (mode 0) or P[state][L] (mode 1), level by level: a cell is summed from finished cells only"""
    S, n = L.n_states, len(w)
    W = n if mode else n + 1
    w = np.asarray(w, np.int64).reshape(-1)
    src, dst, ol = L.a_src.astype(np.int64), L.a_dst.astype(np.int64), L.a_ol.astype(np.int64)
    c, ok = P["c"], P["ok"]
    T = np.full((S, max(W, 1)), np.inf)
    if mode:
        T[:, 0] = P["alpha"]
    else:
        T[L.start, 0] = 0.0
    level = levels_of(L)
    k0 = 1 if mode else 0       # the columns the recurrence fills
    order = np.argsort(level[dst], kind="stable")
    cuts = np.nonzero(np.diff(level[dst][order]))[0] + 1
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for grp in (np.split(order, cuts) if len(order) else []):
            grp = grp[ok[grp]]
            if not len(grp) or W <= k0:
                continue
            t = np.unique(dst[grp])
            row = np.searchsorted(t, dst[grp])
            free = np.nonzero(ol[grp] == 0)[0]                                # k -> k, every column
            cols = np.arange(k0, W)
            key = [(row[free][:, None] * W + cols[None, :]).ravel()]
            x = [(T[src[grp[free]]][:, k0:W] + c[grp[free]][:, None]).ravel()]
            ai, kk = np.nonzero(ol[grp][:, None] == w[None, :W - 1])          # k - 1 -> k over an arc that says w[k - 1]
            key.append(row[ai] * W + kk + 1)
            x.append(T[src[grp[ai]], kk] + c[grp[ai]])
            key, x = np.concatenate(key), np.concatenate(x)
            val = _logsum_into(np.full(len(t) * W, np.inf), key, x, np.ones(len(x), bool)).reshape(len(t), W)
            T[t, k0:] = val[:, k0:]
    return T[:, :W] if W else T[:, :0]


def _tol(L, P, T):
    """tol_log with A taken over the table's finite cells as well as alpha and beta"""
    fin = T[np.isfinite(T)]
    A = max(P["A"], float(np.abs(fin).max()) if len(fin) else 0.0)
    return 8.0 * (P["n_levels"] + 2) * EPS * max(1.0, A)


def sentence(L, w, P):
    """dict(found, logpost, tol): mode 0 for one sequence over posteriors() P"""
    T = table(L, w, 0, P)
    fin = T[np.asarray(L.st_final) != 0, len(w)]
    fin = fin[np.isfinite(fin)]
    tol = _tol(L, P, T) + P["tol_log"]     # the table's own levels, and log_z's
    if not len(fin) or not np.isfinite(P["log_z"]):
        return dict(found=False, logpost=0.0, tol=tol)
    m = fin.min()
    cost = m - math.log(np.exp(-(fin - m)).sum())
    return dict(found=True, logpost=-P["log_z"] - cost, tol=tol)


def phrase(L, w, P):
    """dict(found, count, conf, hit_mass [n_frames], tol_log): mode 1 for one phrase (at least one word) over posteriors() P"""
    assert len(w) >= 1
    T = table(L, w, 1, P)
    src, dst = L.a_src.astype(np.int64), L.a_dst.astype(np.int64)
    sel = np.nonzero((L.a_ol.astype(np.int64) == int(w[-1])) & P["ok"])[0]
    with np.errstate(over="ignore", invalid="ignore"):
        x = T[src[sel], len(w) - 1] + P["c"][sel] + P["beta"][dst[sel]] + P["log_z"]
        good = np.isfinite(x)
        occ = np.exp(-x[good])
    hit = np.bincount(np.asarray(L.st_frame).astype(np.int64)[src[sel[good]]], weights=occ, minlength=n_frames_of(L))
    count = float(occ.sum())
    return dict(found=count > 0.0, count=count, conf=min(1.0, count), hit_mass=hit, tol_log=_tol(L, P, T), arcs=sel[good], occ=occ)


def tol_count(r, L, value):
    """the tolerance of a count or a hit_mass entry: posterior_util.tol_word's form over the phrase's own tol_log"""
    return 4.0 * r["tol_log"] * max(1.0, abs(float(value))) + len(L.a_src) * EPS


def sentence_many(L, seqs, graph_scale=1.0, acoustic_scale=1.0, post=None):
    P = post if post is not None else posteriors(L, graph_scale, acoustic_scale)
    return [None if w is None else sentence(L, w, P) for w in seqs]


def phrase_many(L, phrases, graph_scale=1.0, acoustic_scale=1.0, post=None):
    P = post if post is not None else posteriors(L, graph_scale, acoustic_scale)
    return [None if w is None else phrase(L, w, P) for w in phrases]


# ---- the enumeration of every path ---------------------------------------------------------------------------------------------
def brute_force(L, paths, graph_scale, acoustic_scale):
    """From the paths themselves, weights by math.fsum: (sentences, spot) -- sentences = {word tuple: posterior}; spot(phrase) =
    (count, hit_mass [n_frames]): per path every position at which its words say the phrase (overlapping ones too), at the frame of
    the source state of the arc that carries the phrase's last word."""
    from posterior_util import arc_costs
    c, ok = arc_costs(L, graph_scale, acoustic_scale)
    good = [p for p in paths if all(ok[a] for a in p)]
    cost = [math.fsum(float(c[a]) for a in p) for p in good]
    lo = min(cost) if cost else 0.0
    wt = [math.exp(-(x - lo)) for x in cost]
    z = math.fsum(wt)
    word_arcs = [[a for a in p if L.a_ol[a]] for p in good]
    by_seq = {}
    for arcs, x in zip(word_arcs, wt):
        by_seq.setdefault(tuple(int(L.a_ol[a]) for a in arcs), []).append(x)
    sentences = {k: math.fsum(v) / z for k, v in by_seq.items()}

    def spot(ph):
        ph = [int(x) for x in ph]
        parts = [[] for _ in range(n_frames_of(L))]
        for arcs, x in zip(word_arcs, wt):
            said = [int(L.a_ol[a]) for a in arcs]
            for i in range(len(said) - len(ph) + 1):
                if said[i:i + len(ph)] == ph:
                    parts[int(L.st_frame[L.a_src[arcs[i + len(ph) - 1]]])].append(x)
        hit = np.array([math.fsum(v) / z for v in parts]) if z else np.zeros(len(parts))
        return math.fsum(x for v in parts for x in v) / z if z else 0.0, hit

    return sentences, spot


# ---- a device answer against the restatement -------------------------------------------------------------------------------------
def compare_sentence(got, want, what=""):
    """one (channel, sequence) dict of BatchDecoder.sentence_posteriors against sentence(); returns difference / tolerance"""
    assert got["found"] == want["found"], what + " found"
    if not want["found"]:
        assert got["logpost"] == 0.0, what
        return 0.0
    assert np.isfinite(got["logpost"]), what
    return abs(got["logpost"] - want["logpost"]) / want["tol"]


def compare_phrase(got, want, L, what="", rows=True):
    """one (channel, phrase) dict of BatchDecoder.phrase_posteriors against phrase(); returns the largest difference / tolerance"""
    assert got["found"] == want["found"], what + " found"
    assert got["conf"] == min(1.0, got["count"]), what + " clamp"
    worst = abs(got["count"] - want["count"]) / tol_count(want, L, want["count"])
    if rows:
        assert got["n_frames"] == len(want["hit_mass"]) == len(got["hit_mass"]), what + " n_frames"
        assert np.all(np.isfinite(got["hit_mass"])), what
        for x, y in zip(got["hit_mass"], want["hit_mass"]):
            worst = max(worst, abs(float(x) - float(y)) / tol_count(want, L, y))
    return float(worst)
