"""The definition of wfst_decoder_word_alternatives (include/wfst_decoder.h) restated in numpy over a raw lattice: the mass of every
word in every cell of an aligned sequence's time axis, the ordered alternatives, n_distinct, and the mass of the paths that say
nothing in a cell (the restricted forward pass A_k) -- the enumeration of every path the restatement itself is checked against, the
tolerance the device's answer is held to, and the rule by which a device's lists are compared.

A lattice is what tests/posterior_util.py takes; alpha, beta, log_z, gamma, the arc costs, the "no arc" rule, the cells and the way
a sum is taken are posterior_util's.  All arithmetic is float64.

The tolerance (stated before any GPU run): alt_post, word_post and none_post are held at posterior_util.tol_word(P, L, value).
A mass is a sum of arc posteriors over a subset of the arcs, as word_post is.  A_k passes through no more levels than alpha and
starts from alpha's own values, so its error is within tol_log as alpha's is; a term of none_post has A_k (or alpha), beta and log_z
in its exponent, three of the four tol_log that tol_word grants, and none_post adds at most one term per arc and final state, where
tol_word grants len(arcs) * EPS for the additions -- the final states add at most n_states more, which `tol_none` grants on top."""
import math

import numpy as np

from align_util import align_many
from posterior_util import EPS, _logsum_into, arc_costs, confidence_many, cuts_of, levels_of, posteriors, tol_word

LDS_KEYS = 1024      # WFST_ALTERN_LDS_KEYS (tests/test_altern_surface.py holds the header to it)
MAX_ALTS = 16
TINY = 2.0 ** -970   # below this exp() may flush on one side only


def assert_frames(L):
    """an arc with ilabel 0 stays inside its frame, every other arc goes from frame f to f + 1"""
    fs, fd = L.st_frame[L.a_src].astype(np.int64), L.st_frame[L.a_dst].astype(np.int64)
    assert np.all(fd == fs + (np.asarray(L.a_il) != 0)), "an arc neither stays in its frame nor goes to the next"


def tol_none(P, L, value):
    return tol_word(P, L, value) + L.n_states * EPS


def masses(L, P, m):
    """per cell {word: mass(k, word)} of the words with mass > 0; m = cuts_of(begin).  The sum of a (cell, word) is taken exactly as
    posterior_util.confidence_many takes word_post's."""
    fr = L.st_frame[L.a_src].astype(np.int64)
    ol = L.a_ol.astype(np.int64)
    out = []
    for k in range(len(m) - 1):
        cell = (fr >= m[k]) & (fr < m[k + 1])
        d = {}
        for v in np.unique(ol[cell & (ol > 0)]):
            x = float(P["gamma"][(ol == int(v)) & (fr >= m[k]) & (fr < m[k + 1])].sum())
            if x > 0.0:
                d[int(v)] = x
        out.append(d)
    return out


def ordered(d):
    """a cell's alternatives: (word, mass) by mass descending, then word ascending"""
    return sorted(d.items(), key=lambda e: (-e[1], e[0]))


def none_posts(L, P, m):
    """none_post[k] of every cell: the restricted forward pass A_k over the cell's frames, then the leaving arcs, the final states in
    the cell and the final states before it"""
    assert_frames(L)
    S = L.n_states
    src, dst, ol = L.a_src.astype(np.int64), L.a_dst.astype(np.int64), L.a_ol.astype(np.int64)
    fr = L.st_frame.astype(np.int64)
    c, ok, alpha, beta, log_z = P["c"], P["ok"], P["alpha"], P["beta"], P["log_z"]
    final = np.asarray(L.st_final) != 0
    if "_altern_groups" not in P:   # (the levels are the lattice's: kept beside its posteriors for the next sequence)
        level = levels_of(L)
        order = np.argsort(level[dst], kind="stable")
        cuts = np.nonzero(np.diff(level[dst][order]))[0] + 1
        groups = np.split(order, cuts) if len(order) else []
        P["_altern_groups"] = (groups, np.array([fr[dst[g[0]]] for g in groups], np.int64))
    groups, gframe = P["_altern_groups"]
    out = np.zeros(len(m) - 1)
    if not np.isfinite(log_z):
        return out
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for k in range(len(m) - 1):
            lo, hi = m[k], m[k + 1]
            if lo >= hi:
                out[k] = 1.0
                continue
            A = np.full(S, np.inf)
            if lo == 0:
                A[L.start] = 0.0
            for gi in np.nonzero((gframe >= lo) & (gframe < hi))[0]:
                g = groups[gi]
                s = src[g]
                enters = fr[s] < lo
                x = np.where(enters, alpha[s], A[s]) + c[g]
                use = ok[g] & (enters | (ol[g] == 0))
                t = np.unique(dst[g])
                A[t] = _logsum_into(np.full(len(t), np.inf), np.searchsorted(t, dst[g]), x, use)
            in_cell = (fr >= lo) & (fr < hi)
            leave = ok & in_cell[src] & (fr[dst] >= hi) & (ol == 0)
            terms = [A[src[leave]] + c[leave] + beta[dst[leave]] + log_z, A[final & in_cell] + log_z, alpha[final & (fr < lo)] + log_z]
            x = np.concatenate(terms)
            out[k] = math.fsum(np.exp(-x[np.isfinite(x)]))
    return out


def alternatives_many(L, seqs, graph_scale=1.0, acoustic_scale=1.0, sil_tids=None, post=None, aligned=None):
    """word_alternatives() of every sequence of `seqs` over one lattice; None entries are skipped.  Per sequence confidence_many's dict
    plus mass (per cell {word: mass}), alts (per cell the whole ordered list of (word, mass)), n_distinct, none_post; found = False:
    all of them empty."""
    if L is None or L.n_states == 0:
        return align_many(L, seqs, sil_tids)
    P = post if post is not None else posteriors(L, graph_scale, acoustic_scale)
    res = confidence_many(L, seqs, graph_scale, acoustic_scale, sil_tids, post=P, aligned=aligned)
    for w, r in zip(seqs, res):
        if r is None:
            continue
        if not r["found"] or len(w) == 0:
            r.update(mass=[], alts=[], n_distinct=np.zeros(0, np.int64), none_post=np.zeros(0))
            continue
        m = cuts_of(r["begin"])
        ms = masses(L, P, m)
        r.update(mass=ms, alts=[ordered(d) for d in ms], n_distinct=np.array([len(d) for d in ms], np.int64), none_post=none_posts(L, P, m))
    return res


def alternatives(L, words, graph_scale=1.0, acoustic_scale=1.0, sil_tids=None):
    return alternatives_many(L, [words], graph_scale, acoustic_scale, sil_tids)[0]


# ---- the enumeration of every path ---------------------------------------------------------------------------------------------
def brute_force(L, paths, graph_scale, acoustic_scale, m):
    """From the paths themselves, weights by math.fsum: (none [cells], mass [cells] {word: mass}, some [cells]) -- the share of the
    weight on the paths without a word-carrying arc whose source frame lies in the cell, the expected number of times a path says
    the word there, and the share on the paths that say some word there."""
    c, ok = arc_costs(L, graph_scale, acoustic_scale)
    good = [p for p in paths if all(ok[a] for a in p)]
    cost = [math.fsum(float(c[a]) for a in p) for p in good]
    lo = min(cost) if cost else 0.0
    wt = [math.exp(-(x - lo)) for x in cost]
    z = math.fsum(wt)
    fr = L.st_frame[L.a_src].astype(np.int64)
    none, mass, some = [], [], []
    for k in range(len(m) - 1):
        quiet, loud, by_word = [], [], {}
        for p, x in zip(good, wt):
            said = [int(L.a_ol[a]) for a in p if L.a_ol[a] and m[k] <= fr[a] < m[k + 1]]
            (loud if said else quiet).append(x)
            for v in said:
                by_word.setdefault(v, []).append(x)
        none.append(math.fsum(quiet) / z)
        some.append(math.fsum(loud) / z)
        mass.append({v: math.fsum(xs) / z for v, xs in by_word.items()})
    return none, mass, some


# ---- a device answer against the restatement -------------------------------------------------------------------------------------
def compare_lists(got_alts, got_distinct, want_mass, n_alts, tol, what=""):
    """The device's list of ONE slot (got_alts: [(word, post)] without the zero padding) against the restatement's {word: mass};
    tol(value) is the tolerance of a mass.  Returns the largest difference / tolerance seen.  Near ties are real, so no position is
    compared: the rules are the issue's six."""
    worst = 0.0
    words = [w for w, _ in got_alts]
    assert len(got_alts) <= n_alts, what + " a list longer than n_alts"
    # 1. strictly ordered on its own values, no word twice, every post finite and > 0
    assert len(set(words)) == len(words), what + " a word twice"
    for w, x in got_alts:
        assert w > 0 and np.isfinite(x) and x > 0.0, what + " a listed post that is not a positive number"
    for (w0, x0), (w1, x1) in zip(got_alts, got_alts[1:]):
        assert x0 > x1 or (x0 == x1 and w0 < w1), what + " not ordered by (post descending, word ascending)"
    # 2. every listed entry is the restatement's, within tolerance
    for w, x in got_alts:
        assert w in want_mass or x < TINY, what + " word %d is not in the cell" % w
        y = want_mass.get(w, 0.0)
        assert abs(x - y) <= tol(y), what + " word %d: %r against %r" % (w, x, y)
        worst = max(worst, abs(x - y) / tol(y))
    # 6. a word whose mass is below 2^-970 may be counted and listed, or not
    sure = {w: y for w, y in want_mass.items() if y >= TINY}
    listed = set(words)
    if len(got_alts) == n_alts:
        # 3. every word above the last listed post by more than twice the tolerance is listed
        last = got_alts[-1][1]
        for w, y in sure.items():
            assert w in listed or y <= last + 2.0 * tol(y), what + " word %d of mass %r is missing above the list's end %r" % (w, y, last)
    else:
        # 4. a list shorter than n_alts holds every word of the cell
        for w in sure:
            assert w in listed, what + " word %d is missing from a list with room" % w
    # 5. n_distinct is exact
    assert len(sure) <= got_distinct <= len(want_mass), what + " n_distinct %d, the cell has %d words" % (got_distinct, len(want_mass))
    assert len(got_alts) == min(n_alts, got_distinct), what + " the list's length against n_distinct"
    return worst


def compare(got, want, P, L, n_alts, what=""):
    """one (channel, sequence) dict of BatchDecoder.word_alternatives against alternatives_many's; returns the largest
    difference / tolerance seen.  Integer outputs and align's float32 scores are compared exactly (posterior_util.compare)."""
    from posterior_util import compare as compare_conf
    worst = compare_conf(got, want, P, L, what)
    if want is None or not want["found"]:
        assert len(got["alts"]) == 0 or not any(got["alts"]), what + " alternatives of a sequence that is not found"
        assert not np.asarray(got["none_post"]).any() and not np.asarray(got["n_distinct"]).any(), what
        return worst
    n = len(want["word_post"])
    assert len(got["alts"]) == len(got["none_post"]) == len(got["n_distinct"]) == n, what + " slots"
    for k in range(n):
        x, y = float(got["none_post"][k]), float(want["none_post"][k])
        assert np.isfinite(x), what
        if n > 1 and cuts_of(want["begin"])[k] >= cuts_of(want["begin"])[k + 1]:
            assert x == 1.0, what + " an empty cell"
        worst = max(worst, abs(x - y) / tol_none(P, L, y))
        worst = max(worst, compare_lists(got["alts"][k], int(got["n_distinct"][k]), want["mass"][k], n_alts,
                                         lambda v: tol_word(P, L, v), "%s slot %d" % (what, k)))
    return float(worst)
