"""The definition of wfst_decoder_frame_posteriors (include/wfst_decoder.h) restated in numpy over a raw lattice: per frame the
posterior mass of every class of the frame's emitting arcs, n_distinct, frame_mass and the packed lists -- the enumeration of every
path the restatement itself is checked against, the tolerance the device's answer is held to, and the rule by which a device's
lists are compared.

A lattice is what tests/posterior_util.py takes; alpha, beta, log_z, gamma, the arc costs, the "no arc" rule and the way a sum is
taken are posterior_util's.  All arithmetic is float64.

The tolerance (stated before any GPU run, derived, not tuned): entry_post and frame_mass are held at
posterior_util.tol_word(P, L, value) -- a mass is a sum of arc posteriors over a subset of the arcs, as word_post is: alpha, beta
and log_z each enter gamma's exponent, and up to every arc is added.  log_z is held at tol_log.  frame_off, n_frames, the classes
and their order are exact.  n_distinct is exact, except that a class whose restatement mass is below 2^-970 (altern_util.TINY) is
free: exp() may flush on one side only.  Under min_post > 0 a class is free only if its restatement mass lies within the tolerance
of the threshold (the band); every class above the band must be listed, every class below it must be absent, and every listed
value is >= min_post on the device's own number.  The GPU tests allow ZERO classes in the band: each asserts that from the
restatement alone (band_classes) before it looks at the device's answer."""
import math

import numpy as np

from altern_util import TINY, assert_frames
from posterior_util import arc_costs, posteriors, tol_word

LDS_RECS = 1024   # WFST_FRAMEPOST_LDS_RECS (tests/test_framepost_surface.py holds the header to it)


def n_frames_of(L):
    """the frames the lattice spans: state frames 0 .. n_frames, emitting arcs out of frames 0 .. n_frames - 1"""
    return int(np.asarray(L.st_frame).max()) if L is not None and L.n_states else 0


def class_of(L, label_map=None):
    """class(a) of every arc (meaningless where ilabel == 0)"""
    il = np.asarray(L.a_il).astype(np.int64)
    if label_map is None:
        return il
    m = np.asarray(label_map).astype(np.int64)
    assert il.max(initial=0) < len(m), "label_map is shorter than the lattice's largest ilabel"
    return m[il]


def frame_posts(L, P, label_map=None):
    """per frame {class: post(f, class)} over EVERY class of an emitting arc out of the frame (a mass may be 0), n_frames entries"""
    assert_frames(L)
    nf = n_frames_of(L)
    il = np.asarray(L.a_il)
    fr = np.asarray(L.st_frame)[np.asarray(L.a_src)].astype(np.int64)
    cls = class_of(L, label_map)
    out = [dict() for _ in range(nf)]
    sel = np.nonzero(il > 0)[0]
    if len(sel) == 0:
        return out
    span = int(cls[sel].max()) + 1
    key, inv = np.unique(fr[sel] * span + cls[sel], return_inverse=True)
    sums = np.bincount(inv.reshape(-1), weights=P["gamma"][sel], minlength=len(key))   # (every sum in arc order)
    for k, x in zip(key.tolist(), sums.tolist()):
        out[k // span][k % span] = x
    return out


def frame_posteriors(L, graph_scale=1.0, acoustic_scale=1.0, label_map=None, min_post=0.0, post=None):
    """dict(log_z, n_frames, frame_off, classes, posts, n_distinct, frame_mass, mass): the call's outputs as
    BatchDecoder.frame_posteriors names them, plus mass = frame_posts().  No lattice: n_frames 0, log_z 0, no entries."""
    if L is None or L.n_states == 0:
        return dict(log_z=0.0, n_frames=0, frame_off=np.zeros(1, np.int32), classes=np.zeros(0, np.int32), posts=np.zeros(0),
                    n_distinct=np.zeros(0, np.int32), frame_mass=np.zeros(0), mass=[])
    P = post if post is not None else posteriors(L, graph_scale, acoustic_scale)
    mass = frame_posts(L, P, label_map)
    off, classes, posts, nd, fm = [0], [], [], [], []
    for d in mass:
        nd.append(sum(1 for x in d.values() if x > 0.0))
        fm.append(float(np.sum([d[v] for v in sorted(d)])) if d else 0.0)
        for v in sorted(d):
            if d[v] > 0.0 and d[v] >= min_post:
                classes.append(v)
                posts.append(d[v])
        off.append(len(classes))
    return dict(log_z=P["log_z"], n_frames=len(mass), frame_off=np.array(off, np.int32), classes=np.array(classes, np.int32),
                posts=np.array(posts, np.float64), n_distinct=np.array(nd, np.int32), frame_mass=np.array(fm, np.float64), mass=mass)


def band_classes(want, P, L, min_post):
    """how many (frame, class) of the restatement lie within the tolerance of the threshold: the device may list them or not"""
    if min_post <= 0.0:
        return 0
    return sum(1 for d in want["mass"] for y in d.values() if y > 0.0 and abs(y - min_post) <= tol_word(P, L, y))


# ---- the enumeration of every path ---------------------------------------------------------------------------------------------
def brute_force(L, paths, graph_scale, acoustic_scale, label_map=None):
    """per frame {class: mass} from the paths themselves, weights by math.fsum: the share of the weight on the paths that cross the
    frame over an arc of the class (a path crosses a frame once, so shares add)"""
    c, ok = arc_costs(L, graph_scale, acoustic_scale)
    good = [p for p in paths if all(ok[a] for a in p)]
    cost = [math.fsum(float(c[a]) for a in p) for p in good]
    lo = min(cost) if cost else 0.0
    wt = [math.exp(-(x - lo)) for x in cost]
    z = math.fsum(wt)
    cls = class_of(L, label_map)
    fr = np.asarray(L.st_frame)[np.asarray(L.a_src)].astype(np.int64)
    parts = [dict() for _ in range(n_frames_of(L))]
    for p, x in zip(good, wt):
        for a in p:
            if L.a_il[a] > 0:
                parts[int(fr[a])].setdefault(int(cls[a]), []).append(x)
    return [{v: math.fsum(xs) / z for v, xs in d.items()} for d in parts]


# ---- a device answer against the restatement -------------------------------------------------------------------------------------
def compare(got, want, P, L, min_post=0.0, what=""):
    """one channel's dict of BatchDecoder.frame_posteriors against frame_posteriors(); returns the largest difference / tolerance
    seen.  P, L: the lattice and its posteriors (None, None: no lattice)."""
    assert got["n_frames"] == want["n_frames"], what + " n_frames"
    nf = want["n_frames"]
    off = np.asarray(got["frame_off"])
    assert len(off) == nf + 1 and off[0] == 0 and np.all(np.diff(off) >= 0), what + " frame_off"
    assert len(got["classes"]) == len(got["posts"]) == int(off[-1]), what + " frame_off against the entries"
    assert len(got["n_distinct"]) == nf and len(got["frame_mass"]) == nf, what + " rows"
    if nf == 0:
        assert got["log_z"] == 0.0, what + " log_z without a lattice"
        return 0.0
    tol = lambda v: tol_word(P, L, v)
    worst = 0.0
    if np.isfinite(P["log_z"]):
        worst = abs(got["log_z"] - P["log_z"]) / P["tol_log"]
    else:
        assert got["log_z"] == P["log_z"], what + " log_z"
    exact_off = True
    for f in range(nf):
        tag = "%s frame %d" % (what, f)
        d = want["mass"][f]
        cls = [int(v) for v in got["classes"][off[f]:off[f + 1]]]
        val = [float(x) for x in got["posts"][off[f]:off[f + 1]]]
        assert all(a < b for a, b in zip(cls, cls[1:])), tag + " classes not strictly ascending (a swapped pair or a repeated class)"
        for v, x in zip(cls, val):
            assert np.isfinite(x) and x > 0.0 and x >= min_post, tag + " class %d listed at %r below min_post %r" % (v, x, min_post)
            assert v in d, tag + " class %d is not in the frame" % v
            y = d[v]
            assert abs(x - y) <= tol(y), tag + " class %d: %r against %r" % (v, x, y)
            worst = max(worst, abs(x - y) / tol(y))
        listed = set(cls)
        for v, y in d.items():
            free = y < TINY or (min_post > 0.0 and abs(y - min_post) <= tol(y))
            exact_off = exact_off and not free
            if free:
                continue
            if y >= min_post:
                assert v in listed, tag + " class %d of mass %r is missing" % (v, y)
            else:
                assert v not in listed, tag + " class %d of mass %r is listed below min_post" % (v, y)
        sure = sum(1 for y in d.values() if y >= TINY)
        some = sum(1 for y in d.values() if y > 0.0)
        assert sure <= int(got["n_distinct"][f]) <= some, tag + " n_distinct %d, the frame has %d classes" % (got["n_distinct"][f], some)
        x, y = float(got["frame_mass"][f]), float(want["frame_mass"][f])
        assert np.isfinite(x) and abs(x - y) <= tol(y), tag + " frame_mass %r against %r" % (x, y)
        worst = max(worst, abs(x - y) / tol(y))
    if exact_off:
        assert np.array_equal(off, want["frame_off"]), what + " frame_off"
    return float(worst)
