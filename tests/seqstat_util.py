"""The definition of wfst_decoder_sequence_stats (include/wfst_decoder.h) restated in numpy over a raw lattice: the arcs' accuracies
against a reference alignment, the expectation-semiring recurrences fa / fb in the probability domain, tot_acc, the arcs' signed
weights w(a), and per frame the list of (class, post, value) under the sMBR and the MMI criterion -- Kaldi's
LatticeForwardBackwardMpeVariants ("smbr") and LatticeForwardBackwardMmi -- with the enumeration of every path the restatement itself
is checked against, the tolerance the device's answer is held to, and the rule by which a device's lists are compared.

A lattice is what tests/posterior_util.py takes; alpha, beta, log_z, gamma, the arc costs, the "no arc" rule and the levels are
posterior_util's, the classes and the membership of a frame's list framepost_util's at min_post = 0.  All arithmetic is float64.

The tolerance (stated before any GPU run, derived, not tuned).  log_z is held at tol_log, post at posterior_util.tol_word.
fa[t] and fb[s] are convex combinations (the weights p_in / p_out of a state sum to at most 1) of values that are at most n_frames.
A weight's exponent carries three forward (backward) costs, each off by at most tol_log, so a weight is off by a factor within
4 * tol_log of 1 (exp's own rounding included); that error enters once per level and is carried through the levels above it, each
time scaled by a value <= n_frames: (n_levels + 2) * 4 * tol_log * n_frames.  The sums themselves add one rounding per arc of a
value <= n_frames: n_arcs * n_frames * EPS.
    tol_acc = 4 * (n_levels + 2) * n_frames * tol_log + n_arcs * n_frames * EPS          (fa, fb, tot_acc)
w(a) = gamma(a) * (fa + acc + fb - tot_acc): three terms off by tol_acc each, times a gamma whose own relative error (4 * tol_log)
scales a bracket <= n_frames and is therefore below tol_acc; a value(f, v) adds w over arcs whose gammas sum to at most 1:
    tol_value(x) = 4 * tol_acc * max(1, |x|)                                               (sMBR)
Under MMI value = [v == ref] - post is held at post's own tolerance.  Integers -- n_frames, n_ref_frames, n_dropped, frame_off, the
classes and their order -- are exact, except that a class whose restatement mass lies below altern_util.TINY is free (exp() may
flush on one side only); a frame whose reference class is such a class is free to be dropped or not, and the GPU tests assert from
the restatement alone that they hold no such frame before they look at the device."""
import math

import numpy as np

from altern_util import TINY, assert_frames
from framepost_util import class_of, n_frames_of
from posterior_util import EPS, arc_costs, levels_of, posteriors, tol_word

LDS_RECS = 1024          # WFST_SEQSTAT_LDS_RECS (tests/test_seqstat_surface.py holds the header to it)
SEQ_MMI, SEQ_SMBR = 0, 1   # WFST_SEQ_MMI, WFST_SEQ_SMBR
MAX_SIL = 64             # WFST_SEQSTAT_MAX_SIL
CRITERIA = {"mmi": SEQ_MMI, "smbr": SEQ_SMBR}


def ref_of(ref, nf):
    """ref[f] for f < nf: -1 where the frame is unlabelled (ref[f] < 0, or f beyond the reference)"""
    r = np.full(nf, -1, np.int64)
    ref = np.asarray(ref, np.int64).reshape(-1)
    k = min(nf, len(ref))
    r[:k] = np.where(ref[:k] >= 0, ref[:k], -1)
    return r


def arc_acc(L, ref, label_map=None, sil_classes=()):
    """acc(a) per arc: 1 where an emitting arc's class is its frame's reference class and no silence class, 0 otherwise"""
    nf = n_frames_of(L)
    il = np.asarray(L.a_il).astype(np.int64)
    fr = np.asarray(L.st_frame)[np.asarray(L.a_src)].astype(np.int64)
    cls = class_of(L, label_map)
    r = ref_of(ref, nf + 1)   # (no emitting arc leaves frame nf; the entry is never a match)
    r[nf] = -1
    want = r[np.minimum(fr, nf)]
    sil = np.isin(cls, np.asarray(list(sil_classes), np.int64))
    return ((il > 0) & (want >= 0) & (cls == want) & ~sil).astype(np.float64)


def expect(L, P, acc):
    """(fa, fb): the expected accuracy of the partial paths into and out of every state, level by level, probability domain"""
    S = L.n_states
    src, dst = np.asarray(L.a_src).astype(np.int64), np.asarray(L.a_dst).astype(np.int64)
    alpha, beta, c, ok = P["alpha"], P["beta"], P["c"], P["ok"]
    level = levels_of(L)
    fa, fb = np.zeros(S), np.zeros(S)
    with np.errstate(over="ignore", invalid="ignore"):
        x = alpha[src] + c - alpha[dst]
        pin = np.where(ok & np.isfinite(x), np.exp(-np.where(np.isfinite(x), x, 0.0)), 0.0)
        y = c + beta[dst] - beta[src]
        pout = np.where(ok & np.isfinite(y), np.exp(-np.where(np.isfinite(y), y, 0.0)), 0.0)
    order = np.argsort(level[dst], kind="stable")
    cuts = np.nonzero(np.diff(level[dst][order]))[0] + 1
    for grp in (np.split(order, cuts) if len(order) else []):
        add = np.zeros(S)
        np.add.at(add, dst[grp], pin[grp] * (fa[src[grp]] + acc[grp]))
        t = np.unique(dst[grp])
        fa[t] = add[t]
    order = np.argsort(-level[src], kind="stable")
    cuts = np.nonzero(np.diff(level[src][order]))[0] + 1
    for grp in (np.split(order, cuts) if len(order) else []):
        add = np.zeros(S)
        np.add.at(add, src[grp], pout[grp] * (fb[dst[grp]] + acc[grp]))
        s = np.unique(src[grp])
        fb[s] = add[s]
    return fa, fb


def tol_acc(P, L):
    nf = max(n_frames_of(L), 1)
    return 4.0 * (P["n_levels"] + 2) * nf * P["tol_log"] + len(L.a_src) * nf * EPS


def tol_value(P, L, value):
    return 4.0 * tol_acc(P, L) * max(1.0, abs(float(value)))


def _per_frame(L, cls, weights):
    """per frame {class: sum of weights over the frame's emitting arcs of the class}, every class of an emitting arc present"""
    nf = n_frames_of(L)
    il = np.asarray(L.a_il)
    fr = np.asarray(L.st_frame)[np.asarray(L.a_src)].astype(np.int64)
    out = [dict() for _ in range(nf)]
    sel = np.nonzero(il > 0)[0]
    if len(sel) == 0:
        return out
    span = int(cls[sel].max()) + 1
    key, inv = np.unique(fr[sel] * span + cls[sel], return_inverse=True)
    sums = np.bincount(inv.reshape(-1), weights=weights[sel], minlength=len(key))
    for k, x in zip(key.tolist(), sums.tolist()):
        out[k // span][k % span] = x
    return out


def lists_of(post, value, ref, criterion, drop_frames):
    """the frames' lists from {class: post} and {class: w-sum} per frame: (frame_off, classes, posts, values, n_ref_frames, n_dropped,
    dropped flags)"""
    nf = len(post)
    r = ref_of(ref, nf)
    off, classes, posts, values, dropped = [0], [], [], [], []
    for f in range(nf):
        d = post[f]
        ent = [(v, d[v], value[f][v] if criterion == SEQ_SMBR else (1.0 if v == r[f] else 0.0) - d[v]) for v in sorted(d) if d[v] > 0.0]
        drop = False
        if criterion == SEQ_MMI:
            if r[f] < 0:
                ent = [(v, p, 0.0) for v, p, _ in ent]
            elif not any(v == r[f] for v, _, _ in ent):
                if drop_frames:
                    drop = True
                    ent = [(v, p, 0.0) for v, p, _ in ent]
                else:
                    ent = sorted(ent + [(int(r[f]), 0.0, 1.0)])
        dropped.append(drop)
        for v, p, x in ent:
            classes.append(v)
            posts.append(p)
            values.append(x)
        off.append(len(classes))
    return (np.array(off, np.int32), np.array(classes, np.int32), np.array(posts, np.float64), np.array(values, np.float64),
            int((r >= 0).sum()), int(sum(dropped)), dropped)


def sequence_stats(L, ref, criterion="smbr", graph_scale=1.0, acoustic_scale=1.0, label_map=None, sil_classes=(), drop_frames=False,
                   post=None):
    """dict(log_z, tot_acc, n_frames, n_ref_frames, n_dropped, frame_off, classes, posts, values) as BatchDecoder.sequence_stats names
    them, plus post / value (per frame {class: number} over EVERY class of an emitting arc), dropped, fa, fb, w, acc.  No lattice:
    n_frames 0, everything 0."""
    crit = CRITERIA[criterion] if isinstance(criterion, str) else int(criterion)
    if L is None or L.n_states == 0:
        return dict(log_z=0.0, tot_acc=0.0, n_frames=0, n_ref_frames=0, n_dropped=0, frame_off=np.zeros(1, np.int32),
                    classes=np.zeros(0, np.int32), posts=np.zeros(0), values=np.zeros(0), post=[], value=[], dropped=[])
    assert_frames(L)
    P = post if post is not None else posteriors(L, graph_scale, acoustic_scale)
    cls = class_of(L, label_map)
    acc = arc_acc(L, ref, label_map, sil_classes)
    fa, fb = expect(L, P, acc)
    tot = float(fb[L.start])
    src, dst = np.asarray(L.a_src).astype(np.int64), np.asarray(L.a_dst).astype(np.int64)
    w = P["gamma"] * (fa[src] + acc + fb[dst] - tot)
    mass = _per_frame(L, cls, P["gamma"])
    value = _per_frame(L, cls, w)
    off, classes, posts, values, n_ref, n_drop, dropped = lists_of(mass, value, ref, crit, drop_frames)
    return dict(log_z=P["log_z"], tot_acc=tot if crit == SEQ_SMBR else 0.0, n_frames=len(mass), n_ref_frames=n_ref, n_dropped=n_drop,
                frame_off=off, classes=classes, posts=posts, values=values, post=mass, value=value, dropped=dropped, fa=fa, fb=fb, w=w,
                acc=acc, criterion=crit)


def free_frames(want, ref):
    """the labelled frames whose reference class has a mass in (0, TINY): the device may see the class or not"""
    r = ref_of(ref, want["n_frames"])
    return [f for f in range(want["n_frames"]) if r[f] >= 0 and 0.0 < want["post"][f].get(int(r[f]), 0.0) < TINY]


# ---- the enumeration of every path ---------------------------------------------------------------------------------------------
def brute_force(L, paths, acc, graph_scale, acoustic_scale):
    """(tot_acc, w per arc) from the paths themselves, weights by math.fsum; (0, zeros) without a path"""
    c, ok = arc_costs(L, graph_scale, acoustic_scale)
    good = [p for p in paths if all(ok[a] for a in p)]
    if not good:
        return 0.0, np.zeros(len(L.a_src))
    cost = [math.fsum(float(c[a]) for a in p) for p in good]
    lo = min(cost)
    wt = [math.exp(-(x - lo)) for x in cost]
    z = math.fsum(wt)
    pa = [sum(acc[a] for a in p) for p in good]
    tot = math.fsum(w * a for w, a in zip(wt, pa)) / z
    out = np.zeros(len(L.a_src))
    for a in range(len(L.a_src)):
        out[a] = math.fsum(w * (x - tot) for p, w, x in zip(good, wt, pa) if a in p) / z
    return tot, out


# ---- a device answer against the restatement -------------------------------------------------------------------------------------
def compare(got, want, P, L, ref, what=""):
    """one channel's dict of BatchDecoder.sequence_stats against sequence_stats(); returns the largest difference / tolerance seen.
    P, L: the lattice and its posteriors (None, None: no lattice)."""
    assert got["n_frames"] == want["n_frames"], what + " n_frames"
    nf = want["n_frames"]
    off = np.asarray(got["frame_off"])
    assert len(off) == nf + 1 and off[0] == 0 and np.all(np.diff(off) >= 0), what + " frame_off"
    assert len(got["classes"]) == len(got["posts"]) == len(got["values"]) == int(off[-1]), what + " frame_off against the entries"
    if nf == 0:
        assert got["log_z"] == 0.0 and got["tot_acc"] == 0.0 and got["n_ref_frames"] == 0 and got["n_dropped"] == 0, what + " no lattice"
        return 0.0
    crit = want["criterion"]
    assert got["n_ref_frames"] == want["n_ref_frames"], what + " n_ref_frames"
    r = ref_of(ref, nf)
    worst = 0.0
    if np.isfinite(P["log_z"]):
        worst = abs(got["log_z"] - P["log_z"]) / P["tol_log"]
        assert worst <= 1.0, what + " log_z"
    else:
        assert got["log_z"] == P["log_z"], what + " log_z"
    ta = tol_acc(P, L)
    x, y = float(got["tot_acc"]), float(want["tot_acc"])
    assert np.isfinite(x) and abs(x - y) <= ta, what + " tot_acc %r against %r" % (x, y)
    worst = max(worst, abs(x - y) / ta)
    exact = True
    for f in range(nf):
        tag = "%s frame %d" % (what, f)
        d, dv = want["post"][f], want["value"][f]
        cls = [int(v) for v in got["classes"][off[f]:off[f + 1]]]
        pst = [float(v) for v in got["posts"][off[f]:off[f + 1]]]
        val = [float(v) for v in got["values"][off[f]:off[f + 1]]]
        assert all(a < b for a, b in zip(cls, cls[1:])), tag + " classes not strictly ascending (a swapped pair or a repeated class)"
        ref_free = r[f] >= 0 and 0.0 < d.get(int(r[f]), 0.0) < TINY
        dropped = want["dropped"][f]
        for v, p, x in zip(cls, pst, val):
            assert np.isfinite(p) and np.isfinite(x), tag
            if p == 0.0:   # only MMI's extra entry has no mass
                assert crit == SEQ_MMI and v == r[f] and x == 1.0 and not dropped, tag + " class %d listed without mass" % v
                assert d.get(v, 0.0) < TINY, tag + " the extra entry stands for a class of mass %r" % d.get(v)
                continue
            assert p > 0.0 and v in d, tag + " class %d is not in the frame" % v
            y = d[v]
            assert abs(p - y) <= tol_word(P, L, y), tag + " class %d post: %r against %r" % (v, p, y)
            worst = max(worst, abs(p - y) / tol_word(P, L, y))
            if crit == SEQ_SMBR:
                yv, tv = dv[v], tol_value(P, L, dv[v])
            elif r[f] < 0 or (dropped and not ref_free):
                yv, tv = 0.0, 0.0
            else:
                yv, tv = (1.0 if v == r[f] else 0.0) - y, tol_word(P, L, y)
            if crit == SEQ_MMI and ref_free and x == 0.0:
                continue   # (the device dropped a frame that was free to be dropped)
            assert abs(x - yv) <= tv, tag + " class %d value: %r against %r" % (v, x, yv)
            if tv > 0.0:
                worst = max(worst, abs(x - yv) / tv)
        listed = set(cls)
        for v, y in d.items():
            if y < TINY:
                exact = exact and not (y > 0.0 or (crit == SEQ_MMI and v == r[f]))
                continue
            assert v in listed, tag + " class %d of mass %r is missing" % (v, y)
        if crit == SEQ_MMI and r[f] >= 0 and d.get(int(r[f]), 0.0) == 0.0:   # the reference is outside the frame's lattice
            assert (int(r[f]) in listed) == (not dropped), tag + " the reference's own entry"
        exact = exact and not ref_free
    if exact:
        assert np.array_equal(off, want["frame_off"]), what + " frame_off"
        assert np.array_equal(got["classes"], want["classes"]), what + " classes"
        assert got["n_dropped"] == want["n_dropped"], what + " n_dropped %d against %d" % (got["n_dropped"], want["n_dropped"])
    return float(worst)
