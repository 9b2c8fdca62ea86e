"""-m gpu: wfst_decoder_frame_posteriors (frame_post_kernel / frame_pack_kernel behind align_index_kernel and posterior_kernel) --
per frame of a channel's raw lattice the posterior mass of every transition-id, pdf or phone.

The reference of every comparison is the definition restated in numpy (tests/framepost_util.py) over dec.raw_lattice(channel,
use_final_probs) fetched at the same moment.  frame_off, n_frames, the classes, their order and n_distinct are compared exactly;
entry_post, frame_mass and log_z at the restatement's tolerances, derived from the lattice at hand; under a threshold no class may
lie within the tolerance of it, which every test asserts from the restatement before it looks at the device's answer.  Every test
prints the largest difference / tolerance it saw; a ratio above 1 is a bug."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from align_util import from_gpu
from framepost_util import LDS_RECS, band_classes, compare, frame_posteriors
from golden_util import GOLDEN_DIR, Golden, bits
from posterior_util import posteriors

pytestmark = pytest.mark.gpu

E_ARG, E_CAPACITY, E_STATE = -1, -4, -5
N_TID = 600
LIM = dict(max_frames=192, max_tokens_per_frame=32768, arena_tokens=1 << 20, lattice_links=1 << 21)
SCALES = [(1.0, 1.0), (0.1, 0.1), (1.0, 0.0)]
WIDE = dict(beam=200.0, max_active=1000000, min_active=0, lattice_beam=100.0, prune_interval=10)


def cfg(lattice_beam):
    return dict(beam=12.0, max_active=1000000, min_active=0, lattice_beam=lattice_beam, prune_interval=10)


def phone_map(n_tid, per=12):
    """tid -> phone: `per` consecutive transition-ids per phone, phones from 1"""
    m = (np.arange(n_tid + 1, dtype=np.int32) - 1) // per + 1
    m[0] = 0
    return m


@pytest.fixture(scope="module")
def world(synth, tmp_path_factory):
    import gpu_util as G

    W = G.wfstdec
    g = synth.make_hclg_like(3000, seed=21, n_tid=N_TID, n_words=500)
    m = synth.default_tid2pdf(N_TID)
    path = str(tmp_path_factory.mktemp("framepost") / "g.bin")
    g.write(path)
    graph = W.Graph.load(path)
    graph.set_tid2pdf(m)
    mats = [synth.make_loglikes(g, T, N_TID // 2, m, seed=s, mu=-2.2)[0] for T, s in ((40, 700), (97, 701), (150, 702))]
    dev = G.upload(mats)
    maps = dict(tid=None, pdf=np.asarray(m, np.int32), phone=phone_map(N_TID))
    yield dict(G=G, W=W, graph=graph, mats=mats, dev=dev, ptrs=[t.data_ptr() for t in dev], T=[x.shape[0] for x in mats], maps=maps)
    graph.free()


def decoder(world, lattice_beam, n=3, **kw):
    lim = dict(LIM)
    lim.update(kw)
    return world["W"].BatchDecoder(world["graph"], world["G"].gpu_config(cfg(lattice_beam)), n, **lim)


def decode_all(world, dec):
    dec.init()
    dec.advance(world["ptrs"], world["T"], N_TID // 2)
    dec.finalize()


def check(dec, channels, ufp=True, scales=(1.0, 1.0), label_map=None, min_post=0.0, what="", lattices=None, posts=None, max_cells=0):
    """frame_posteriors of the list against the restatement on each channel's raw lattice now; returns (got, want, worst ratio).
    lattices / posts: the channels' lattices / their posteriors() at these scales, where the caller has them at this moment"""
    lat = lattices if lattices is not None else [from_gpu(dec.raw_lattice(int(c), ufp)) for c in channels]
    want, Ps = [], []
    for i, L in enumerate(lat):
        none = L is None or L.n_states == 0
        P = None if none else (posts[i] if posts is not None else posteriors(L, scales[0], scales[1]))
        w = frame_posteriors(None if none else L, scales[0], scales[1], label_map, min_post, post=P)
        # decided on the restatement alone, before the device's answer is looked at: no class within the tolerance of the threshold
        assert none or band_classes(w, P, L, min_post) == 0, "%s: min_post %r lies within the tolerance of a class' mass" % (what, min_post)
        want.append(w)
        Ps.append(P)
    got = dec.frame_posteriors(channels, use_final_probs=ufp, graph_scale=scales[0], acoustic_scale=scales[1], label_map=label_map,
                               min_post=min_post, max_cells=max_cells)
    assert len(got) == len(channels)
    worst = 0.0
    for i, c in enumerate(channels):
        tag = "%s channel %d scales %s min_post %g" % (what, c, scales, min_post)
        assert got[i]["status"] == 0, tag
        worst = max(worst, compare(got[i], want[i], Ps[i], None if Ps[i] is None else lat[i], min_post, tag))
    assert worst <= 1.0, "%s: difference / tolerance = %g" % (what, worst)
    return got, want, worst


def raw_call(W, dec, channels, capf, cape, ufp=True, label_map=None, n_tid=0, min_post=0.0, max_cells=0, gs=1.0, as_=1.0):
    """the C entry point itself, with rows of the caller's size: dict of the raw output arrays and the return code"""
    I, D = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    ch = np.ascontiguousarray(channels, np.int32)
    n = len(ch)
    o = dict(status=np.full(n, 99, np.int32), log_z=np.full(n, 9.0), n_frames=np.full(n, 99, np.int32), n_entries=np.full(n, 99, np.int32),
             frame_off=np.full((n, capf + 1), 99, np.int32), n_distinct=np.full((n, capf), 99, np.int32), frame_mass=np.full((n, capf), 9.0),
             entry_class=np.full((n, cape), 99, np.int32), entry_post=np.full((n, cape), 9.0))
    p = lambda a: a.ctypes.data_as(I if a.dtype == np.int32 else D)
    m = None if label_map is None else np.ascontiguousarray(label_map, np.int32)
    o["rc"] = W.lib().wfst_decoder_frame_posteriors(dec.h, p(ch), n, int(ufp), C.c_double(gs), C.c_double(as_), None if m is None else p(m), n_tid,
                                                    C.c_double(min_post), C.c_int64(max_cells), capf, cape, p(o["status"]), p(o["log_z"]),
                                                    p(o["n_frames"]), p(o["n_entries"]), p(o["frame_off"]), p(o["n_distinct"]), p(o["frame_mass"]),
                                                    p(o["entry_class"]), p(o["entry_post"]))
    return o


def canonical_states(L):
    k = np.stack([L.st_frame, L.st_gstate, L.st_final], axis=1)
    return k[np.lexsort(k.T[::-1])]


def canonical_arcs(L):
    f, g = L.st_frame, L.st_gstate
    k = np.stack([f[L.a_src], g[L.a_src], f[L.a_dst], g[L.a_dst], L.a_il, L.a_ol, bits(L.a_graph), bits(L.a_ac)], axis=1)
    return k[np.lexsort(k.T[::-1])]


def small_decoder(synth, tmp_path, name, n_states, arcs, finals, n_pdf, T, tid2pdf=None):
    """a hand-made graph decoded over T frames of equal scores with nothing pruned: (graph, decoder), both to be freed"""
    import gpu_util as G

    g = synth.graph_from_arc_lists(n_states, 0, arcs, finals)
    path = str(tmp_path / (name + ".bin"))
    g.write(path)
    graph = G.wfstdec.Graph.load(path)
    graph.set_tid2pdf(tid2pdf if tid2pdf is not None else synth.default_tid2pdf(n_pdf * 2))
    x = np.full((T, n_pdf), -0.5, np.float32)
    dec = G.wfstdec.BatchDecoder(graph, G.gpu_config(WIDE), 1, max_frames=96, max_tokens_per_frame=4096, arena_tokens=1 << 16, lattice_links=1 << 16)
    dev = G.upload([x])
    dec.init()
    dec.advance([dev[0].data_ptr()], [T], n_pdf)
    dec.finalize()
    return graph, dec


def one_to_one(n_tid):
    """tid2pdf: transition-id t reads column t - 1"""
    m = np.arange(n_tid + 1, dtype=np.int32) - 1
    m[0] = 0
    return m


def most_records(L):
    """the most emitting arcs of one frame: what the kernel holds against WFST_FRAMEPOST_LDS_RECS"""
    return int(np.bincount(L.st_frame[L.a_src][L.a_il > 0]).max())


# ---- 1. finalized channels ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lattice_beam", [4.0, 8.0])
def test_finalized_channels(world, lattice_beam):
    """T = 40 / 97 / 150 at the three pairs of scales, each with the identity, the tid -> pdf and the tid -> phone map"""
    dec = decoder(world, lattice_beam)
    try:
        decode_all(world, dec)
        ch = [2, 0, 1]
        lat = [from_gpu(dec.raw_lattice(c, True)) for c in ch]
        worst, most, entries = 0.0, 0, []
        for sc in SCALES:
            Ps = [posteriors(L, sc[0], sc[1]) for L in lat]
            for name, m in world["maps"].items():
                got, want, r = check(dec, ch, True, sc, m, 0.0, "lattice_beam %g %s" % (lattice_beam, name), lattices=lat, posts=Ps)
                worst = max(worst, r)
                for i, c in enumerate(ch):
                    assert got[i]["n_frames"] == world["T"][c]
                    assert np.all(np.abs(got[i]["frame_mass"] - 1.0) < 1e-9), "every path of a finalized lattice runs to the end"
                if name == "tid" and sc == SCALES[0]:
                    most = max(int(g["n_distinct"].max()) for g in got)
                    entries = [int(g["n_entries"]) for g in got]
        print("finalized, lattice_beam %g: largest difference / tolerance %.3g; entries per lattice %s, most distinct transition-ids in a "
              "frame %d, most emitting arcs of a frame %d" % (lattice_beam, worst, entries, most, max(most_records(L) for L in lat)))
    finally:
        dec.free()


# ---- 2. live channels, read-only ----------------------------------------------------------------------------------------------
def test_live_channels_and_the_call_is_read_only(world):
    """the 150-frame utterance at lattice_beam 8, at frames 40 and 75; both use_final_probs, both live-prune modes.  Channel 0 is
    queried, channel 1 is its twin that never is."""
    dec = decoder(world, 8.0, 2)
    try:
        p, stride = world["ptrs"][2], N_TID // 2
        maps = list(world["maps"].items())
        dec.init()
        worst, k, sizes = 0.0, 0, []
        for upto in (40, 75):
            dec.advance([p, p], [upto, upto], stride)
            for mode in (0, 1):
                dec.set_live_lattice_prune(mode)
                for ufp in (False, True):
                    L = from_gpu(dec.raw_lattice(0, ufp))
                    name, m = maps[k % 3]
                    sc = SCALES[(k // 3 + k) % 3]
                    k += 1
                    got, _, r = check(dec, [0], ufp, sc, m, 0.0, "frame %d mode %d ufp %d %s" % (upto, mode, ufp, name), lattices=[L])
                    worst = max(worst, r)
                    assert got[0]["n_frames"] == upto
                    sizes.append((upto, mode, int(ufp), L.n_states, most_records(L), int(got[0]["n_entries"])))
            dec.set_live_lattice_prune(0)
        print("(frame, mode, ufp, states, most emitting arcs of a frame, entries):", sizes)
        print("live: largest difference / tolerance %.3g" % worst)
        assert any(s[4] > LDS_RECS for s in sizes), "frames beyond the LDS capacity: the workspace path is taken (frame 0 never is one)"
        dec.advance([p, p], [150, 150], stride)
        dec.finalize()
        a, b = dec.best_paths([0, 1])
        for key in ("ilabel", "olabel"):
            assert np.array_equal(a[key], b[key]), key
        for key in ("graph", "ac"):
            assert np.array_equal(bits(a[key]), bits(b[key])), key
        La, Lb = from_gpu(dec.raw_lattice(0)), from_gpu(dec.raw_lattice(1))
        assert La.n_states == Lb.n_states and len(La.a_src) == len(Lb.a_src)
        assert np.array_equal(canonical_states(La), canonical_states(Lb)) and np.array_equal(canonical_arcs(La), canonical_arcs(Lb))
        # the hypothesis' frame-level confidence trace: the best path's transition-ids are in the lattice at every frame
        res = dec.frame_posteriors([0])[0]
        trace = world["W"].frame_post_lookup(res, a["tids"])
        assert len(a["tids"]) == 150 == res["n_frames"] and np.all(trace > 0.0) and np.all(trace <= 1.0 + 1e-9)
    finally:
        dec.free()


# ---- 3. the goldens: epsilon chains, dead ends, negative costs --------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lattice_eps_chains", "dead_end", "neg_hclg600"])
def test_golden_fixtures(name, tmp_path):
    import gpu_util as G

    g = Golden(name)
    graph = G.wfstdec.Graph.load(g.write_graph(str(tmp_path / "g.bin")))
    if g.tid2pdf is not None:
        graph.set_tid2pdf(g.tid2pdf)
    cd = dict(g.meta["cfgs"][g.meta["cases"][0]["cfg"]])
    mats = list(g.utts)
    dec = G.wfstdec.BatchDecoder(graph, G.gpu_config(cd), len(mats), max_frames=64, max_tokens_per_frame=32768, arena_tokens=1 << 20, lattice_links=1 << 21)
    try:
        dev = G.upload(mats)
        dec.init()
        dec.advance([t.data_ptr() for t in dev], [x.shape[0] for x in mats], mats[0].shape[1])
        dec.finalize()
        ch = list(range(len(mats)))
        lat = [from_gpu(dec.raw_lattice(c, True)) for c in ch]
        thirds = np.arange((1 << 16) + 1, dtype=np.int32) % 3     # (longer than any fixture's transition-ids)
        worst, n_eps, n_zero = 0.0, 0, 0
        for sc in SCALES[:2]:
            for m in (None, thirds):
                got, want, r = check(dec, ch, True, sc, m, 0.0, name, lattices=lat)
                worst = max(worst, r)
                for i in ch:
                    assert (got[i]["n_frames"] > 0) == (lat[i] is not None)
                    n_zero += sum(1 for d in want[i]["mass"] for y in d.values() if y == 0.0)
        n_eps = sum(int((L.a_il == 0).sum()) for L in lat if L is not None)
        print("%s: largest difference / tolerance %.3g; arcs inside a frame %d, (frame, class) pairs of mass 0 that stay out %d" % (name, worst, n_eps, n_zero))
        if name == "lattice_eps_chains":
            assert n_eps > 0
    finally:
        dec.free()
        graph.free()


# ---- 4. a fan around the LDS capacity -------------------------------------------------------------------------------------------
LEAD = 5
_LEAD_SEEN = {}   # (fan, map) -> the answer of the frames before the fan


@pytest.mark.parametrize("fan", [LDS_RECS - 1, LDS_RECS, LDS_RECS + 1], ids=["one_below", "capacity", "one_above"])
def test_a_fan_around_the_lds_capacity(fan, synth, tmp_path):
    """five steps of two arcs each, then a fan of `fan` emitting arcs with distinct transition-ids into as many final states: the last
    frame has WFST_FRAMEPOST_LDS_RECS - 1 emitting arcs, exactly as many, and one more, where the workspace takes over.  Under the identity
    every record is a run of its own; under tid % 3 there are three runs of about 341 records.  The frames before the fan give the
    same answer in all three to rounding."""
    T = LEAD
    arcs = {s: [(2 * s + 1, s + 1, 0.5, s + 1), (2 * s + 2, 0, 0.25, s + 1)] for s in range(T)}
    arcs[T] = [(2 * T + 1 + i, 1000 + i, (i % 97) / 64.0, T + 1 + i) for i in range(fan)]
    finals = {T + 1 + i: 0.0 for i in range(fan)}
    n_pdf = 2 * T + fan
    graph, dec = small_decoder(synth, tmp_path, "fan", T + 1 + fan, arcs, finals, n_pdf, T + 1, one_to_one(n_pdf))
    try:
        L = from_gpu(dec.raw_lattice(0, True))
        assert most_records(L) == fan and int((L.st_frame[L.a_src] == T).sum()) == fan
        thirds = np.arange(n_pdf + 1, dtype=np.int32) % 3
        for name, m in (("tid", None), ("thirds", thirds)):
            got, want, worst = check(dec, [0], True, (1.0, 1.0), m, 0.0, "fan %d %s" % (fan, name), lattices=[L])
            g = got[0]
            assert g["n_frames"] == T + 1 and g["n_distinct"].tolist() == [2 if m is None else (2 if len({int(m[2 * s + 1]), int(m[2 * s + 2])}) == 2 else 1)
                                                                          for s in range(T)] + [fan if m is None else 3]
            assert abs(g["frame_mass"][-1] - 1.0) < 1e-9
            if m is None:
                assert g["classes"][g["frame_off"][T]:].tolist() == list(range(2 * T + 1, 2 * T + 1 + fan))
            lead = np.concatenate([g["posts"][:g["frame_off"][T]], g["frame_mass"][:T]])
            for (other, oname), seen in _LEAD_SEEN.items():
                if oname == name:
                    assert np.allclose(lead, seen, rtol=0, atol=1e-9), (fan, other, name)
            _LEAD_SEEN[(fan, name)] = lead
            print("fan %d %s: largest difference / tolerance %.3g" % (fan, name, worst))
    finally:
        dec.free()
        graph.free()


# ---- 5. fans of many sizes in one lattice -------------------------------------------------------------------------------------------
FANS = [1, 2, 63, 64, 65, 255, 256, 257]


def test_fans_around_the_wave_and_the_block(synth, tmp_path):
    """eight fans in a row, one per frame: hub f --N emitting arcs, N distinct transition-ids--> N middle states --arcs inside the
    frame--> hub f + 1: a frame's range of records holds N emitting arcs and N arcs that are none, which the load skips, around the
    wave's 64 lanes and the block's 256.  A frame with one arc has a post of exactly 1."""
    arcs, state, tid = {}, 0, 0
    first = []
    for f, N in enumerate(FANS):
        hub, nxt = state, state + N + 1
        arcs[hub] = []
        first.append(tid + 1)
        for i in range(N):
            tid += 1
            arcs[hub].append((tid, 100 * (f + 1) + i, 0.125 * (i % 13), hub + 1 + i))
            arcs[hub + 1 + i] = [(0, 0, 0.25, nxt)]
        state = nxt
    graph, dec = small_decoder(synth, tmp_path, "fans", state + 1, arcs, {state: 0.0}, tid, len(FANS), one_to_one(tid))
    try:
        L = from_gpu(dec.raw_lattice(0, True))
        worst = 0.0
        for name, m in (("tid", None), ("sevenths", np.arange(tid + 1, dtype=np.int32) % 7)):
            got, want, r = check(dec, [0], True, (1.0, 1.0), m, 0.0, "fans " + name, lattices=[L])
            worst = max(worst, r)
            g = got[0]
            assert g["n_distinct"].tolist() == (FANS if m is None else [min(N, 7) for N in FANS])
            assert np.all(np.abs(g["frame_mass"] - 1.0) < 1e-12)
            assert g["posts"][0] == 1.0 and g["frame_mass"][0] == 1.0, "a frame with a single arc"
            if m is None:
                assert g["classes"].tolist() == list(range(1, tid + 1)) and g["frame_off"].tolist() == [0] + list(np.cumsum(FANS))
        print("fans: largest difference / tolerance %.3g" % worst)
    finally:
        dec.free()
        graph.free()


# ---- 6. two chains that share transition-ids -----------------------------------------------------------------------------------------
def test_two_chains_that_share_tids(synth, tmp_path):
    """0 --tid 1--> 1, then two chains 1 -> 2 -> 4 -> 6 and 1 -> 3 -> 5 -> 6 over the same transition-ids at different costs: from
    frame 2 on a class sums arcs that leave different states"""
    arcs = {0: [(1, 9, 0.0, 1)], 1: [(2, 1, 0.25, 2), (3, 2, 1.0, 3)], 2: [(4, 0, 0.5, 4), (5, 0, 0.75, 4)], 3: [(4, 0, 0.125, 5), (5, 0, 2.0, 5)],
            4: [(6, 3, 0.0, 6)], 5: [(6, 4, 1.5, 6), (7, 5, 0.25, 6)]}
    graph, dec = small_decoder(synth, tmp_path, "chains", 7, arcs, {6: 0.0}, 7, 4, one_to_one(7))
    try:
        L = from_gpu(dec.raw_lattice(0, True))
        worst = 0.0
        for sc in SCALES:
            got, want, r = check(dec, [0], True, sc, None, 0.0, "chains", lattices=[L])
            worst = max(worst, r)
            g = got[0]
            assert g["n_frames"] == 4 and g["frame_off"].tolist() == [0, 1, 3, 5, 7] and g["classes"].tolist() == [1, 2, 3, 4, 5, 6, 7]
            assert g["posts"][0] == 1.0 and g["n_distinct"].tolist() == [1, 2, 2, 2], "a frame with a single arc: exactly 1"
            for t in (4, 5, 6):
                assert len(set(L.a_src[L.a_il == t].tolist())) == 2, "transition-id %d leaves two states" % t
        print("chains: largest difference / tolerance %.3g" % worst)
    finally:
        dec.free()
        graph.free()


# ---- 7. thresholds -----------------------------------------------------------------------------------------------------------------
def test_min_post(world):
    dec = decoder(world, 8.0, 1)
    try:
        dec.init()
        dec.advance(world["ptrs"][1:2], [97], N_TID // 2)
        dec.finalize()
        L = from_gpu(dec.raw_lattice(0, True))
        P = posteriors(L)
        worst, counts = 0.0, []
        for name, m in (("tid", None), ("phone", world["maps"]["phone"])):
            for mp in (0.0, 0.01, 0.5):
                got, want, r = check(dec, [0], True, (1.0, 1.0), m, mp, "min_post %s" % name, lattices=[L], posts=[P])
                worst = max(worst, r)
                counts.append(int(got[0]["n_entries"]))
                assert np.all(got[0]["posts"] >= mp) and np.all(np.diff(got[0]["frame_off"]) <= got[0]["n_distinct"])
                assert np.all(np.abs(got[0]["frame_mass"] - 1.0) < 1e-9), "frame_mass is from before the threshold"
        assert counts[0] > counts[1] > counts[2] > 0 and counts[3] > counts[4] > counts[5] > 0
        print("min_post: entries %s; largest difference / tolerance %.3g" % (counts, worst))
    finally:
        dec.free()


# ---- 8. mixed lists, a channel over max_cells, rows too short ---------------------------------------------------------------------------
def test_mixed_list_and_capacities(world, monkeypatch):
    W = world["W"]
    dec = decoder(world, 8.0)
    try:
        dec.init()
        dec.advance(world["ptrs"], [40, 60, 150], N_TID // 2)
        dec.finalize(channels=[0, 2])          # channel 1 stays live at frame 60
        dec.set_live_lattice_prune(1)
        ch = [1, 2, 0]
        got, want, worst = check(dec, ch, True, (1.0, 1.0), world["maps"]["pdf"], 0.0, "mixed")
        assert [g["n_frames"] for g in got] == [60, 150, 40]
        lat = [from_gpu(dec.raw_lattice(c, True)) for c in ch]
        states = [L.n_states for L in lat]
        big = int(np.argmax(states))
        assert sorted(states)[-1] > sorted(states)[-2]
        # a channel over max_cells: its lists zero, the others' answers stand
        tight = dec.frame_posteriors(ch, max_cells=states[big] - 1)
        assert [g["status"] for g in tight] == [E_CAPACITY if i == big else 0 for i in range(3)]
        t = tight[big]
        assert t["n_frames"] == 0 and t["log_z"] == 0.0 and len(t["classes"]) == 0 and len(t["frame_mass"]) == 0
        for i in set(range(3)) - {big}:
            P = posteriors(lat[i])
            worst = max(worst, compare(tight[i], frame_posteriors(lat[i], post=P), P, lat[i], 0.0, "beside the channel over max_cells"))
        # at max_cells = its states the channel fits
        assert [g["status"] for g in dec.frame_posteriors(ch, max_cells=states[big])] == [0, 0, 0]
        # rows too short for ONE channel: the room needed comes back, the lists are zero, the others stand
        full = dec.frame_posteriors(ch)
        need = [int(g["n_entries"]) for g in full]
        most = int(np.argmax(need))
        cape = sorted(need)[-2]
        assert need[most] > cape >= 1
        o = raw_call(W, dec, ch, 150, cape)
        assert o["rc"] == 0 and o["status"].tolist() == [E_CAPACITY if i == most else 0 for i in range(3)]
        assert o["n_entries"].tolist() == need and o["n_frames"].tolist() == [60, 150, 40]
        assert not o["frame_off"][most].any() and not o["entry_class"][most].any() and not o["entry_post"][most].any() and not o["frame_mass"][most].any()
        for i in set(range(3)) - {most}:
            k, e = full[i]["n_frames"], need[i]
            assert np.array_equal(o["frame_off"][i, :k + 1], full[i]["frame_off"]) and np.array_equal(o["entry_class"][i, :e], full[i]["classes"])
            assert np.allclose(o["entry_post"][i, :e], full[i]["posts"], rtol=0, atol=1e-9)
            assert not o["entry_class"][i, e:].any() and not o["entry_post"][i, e:].any() and not o["frame_off"][i, k + 1:].any()
        # frames too short: likewise
        o = raw_call(W, dec, ch, 60, max(need))
        assert o["rc"] == 0 and o["status"].tolist() == [0, E_CAPACITY, 0] and o["n_frames"].tolist() == [60, 150, 40] and o["n_entries"].tolist() == need
        # the binding takes its first room from the frames decoded: with one entry per frame that is too little, and its repeat runs
        monkeypatch.setattr(W, "FRAME_POST_ENTRIES_PER_FRAME", 1)
        first = raw_call(W, dec, ch, 150, 150)
        assert first["status"].tolist() == [E_CAPACITY] * 3
        again = dec.frame_posteriors(ch)
        monkeypatch.undo()
        for a, b in zip(again, full):
            assert a["status"] == 0 and np.array_equal(a["frame_off"], b["frame_off"]) and np.array_equal(a["classes"], b["classes"])
            assert np.allclose(a["posts"], b["posts"], rtol=0, atol=1e-9)
        # use_final_probs = 0: the finalized channels have no lattice (status OK, n_frames 0, log_z 0), the live one answers
        live_only = dec.frame_posteriors(ch, use_final_probs=False)
        assert [g["status"] for g in live_only] == [0, 0, 0] and [g["n_frames"] for g in live_only] == [60, 0, 0]
        assert live_only[1]["log_z"] == 0.0 and len(live_only[1]["classes"]) == 0 and live_only[1]["frame_off"].tolist() == [0]
        assert worst <= 1.0
        print("mixed: largest difference / tolerance %.3g; entries needed %s" % (worst, need))
    finally:
        dec.free()


# ---- 9. a biglm lattice decoder -----------------------------------------------------------------------------------------------
def test_biglm_lattice_decoder(tmp_path):
    import gpu_util as G

    W = G.wfstdec
    z = np.load(os.path.join(GOLDEN_DIR, "biglm_hclg600.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    with open(tmp_path / "g.bin", "wb") as f:
        f.write(bytes(z["graph"]))
    graph = W.Graph.load(str(tmp_path / "g.bin"))
    graph.set_tid2pdf(z["tid2pdf"])
    pname = [p for p in meta["pairs"] if p != "unigram"][0]
    lms = []
    for tag, scale in (("old", -1.0), ("new", 1.0)):
        p = str(tmp_path / ("lm_%s.bin" % tag))
        with open(p, "wb") as f:
            f.write(bytes(z["lm_%s_%s" % (pname, tag)]))
        lms.append(W.Lm.load(p, scale))
    cd = dict(beam=13.0, max_active=1000000, min_active=0, lattice_beam=25.0, prune_interval=7)
    mats = [z["ll_%d" % i] for i in range(int(z["n_utt"]))]
    dec = W.BatchDecoder(graph, G.gpu_config(cd), len(mats), old_lm=lms[0], new_lm=lms[1], max_frames=64, max_tokens_per_frame=32768,
                         arena_tokens=1 << 20, lattice_links=1 << 21)
    try:
        dev = G.upload(mats)
        dec.init()
        dec.advance([t.data_ptr() for t in dev], [x.shape[0] for x in mats], int(mats[0].shape[1]))
        dec.finalize()
        have = [c for c in range(len(mats)) if dec.raw_lattice(c, True) is not None]
        assert have, "no utterance kept its lattice"
        m = np.asarray(z["tid2pdf"], np.int32)
        got, _, worst = check(dec, have, True, (1.0, 0.1), None, 0.0, "biglm tid")
        _, _, r = check(dec, have, True, (1.0, 0.1), m, 0.0, "biglm pdf")
        assert all(g["n_frames"] > 0 and g["n_entries"] > 0 for g in got)
        print("biglm: %d lattices, largest difference / tolerance %.3g" % (len(have), max(worst, r)))
    finally:
        dec.free()
        for lm in lms:
            lm.free()
        graph.free()


# ---- 10. the error surface -------------------------------------------------------------------------------------------------------
def test_error_surface(world):
    W = world["W"]
    plain = decoder(world, 4.0, 2, lattice_links=0)
    try:
        plain.init()
        plain.advance(world["ptrs"][:2], [10, 10], N_TID // 2)
        with pytest.raises(W.WfstError) as e:
            plain.frame_posteriors()
        assert e.value.code == E_STATE
    finally:
        plain.free()
    dec = decoder(world, 4.0, 3)
    try:
        dec.init(channels=[0, 1])
        dec.advance(world["ptrs"][:2], [20, 20], N_TID // 2, channels=[0, 1])
        ok = dec.frame_posteriors([0], use_final_probs=False)
        assert ok[0]["status"] == 0 and ok[0]["n_frames"] == 20
        for ch, code in (([0, 0], E_ARG), ([0, 3], E_ARG), ([0, 2], E_STATE)):
            with pytest.raises(W.WfstError) as e:
                dec.frame_posteriors(ch, use_final_probs=False)
            assert e.value.code == code, ch
        for gs, as_ in ((-1.0, 1.0), (1.0, -0.5), (float("nan"), 1.0), (1.0, float("inf")), (float("-inf"), 1.0)):
            with pytest.raises(W.WfstError) as e:
                dec.frame_posteriors([0], use_final_probs=False, graph_scale=gs, acoustic_scale=as_)
            assert e.value.code == E_ARG and "scale" in str(e.value), (gs, as_)
        for mp in (-0.1, 1.5, float("nan")):
            with pytest.raises(W.WfstError) as e:
                dec.frame_posteriors([0], use_final_probs=False, min_post=mp)
            assert e.value.code == E_ARG and "min_post" in str(e.value), mp
        # a label map shorter than the graph's largest transition-id; a negative class
        short = np.zeros(N_TID // 2, np.int32)
        with pytest.raises(W.WfstError) as e:
            dec.frame_posteriors([0], use_final_probs=False, label_map=short)
        assert e.value.code == E_ARG and "label_map" in str(e.value)
        neg = np.zeros(N_TID + 1, np.int32)
        neg[17] = -1
        with pytest.raises(W.WfstError) as e:
            dec.frame_posteriors([0], use_final_probs=False, label_map=neg)
        assert e.value.code == E_ARG and "label_map" in str(e.value)
        with pytest.raises(W.WfstError):
            dec.frame_posteriors([0], use_final_probs=False, max_cells=-1)
        # through the C ABI: rows of no room, and NULL outputs are fine
        assert raw_call(W, dec, [0], 0, 10, ufp=False)["rc"] == E_ARG and raw_call(W, dec, [0], 10, 0, ufp=False)["rc"] == E_ARG
        one = np.array([0], np.int32)
        rc = W.lib().wfst_decoder_frame_posteriors(dec.h, one.ctypes.data_as(C.POINTER(C.c_int32)), 1, 0, C.c_double(1.0), C.c_double(1.0), None, 0,
                                                   C.c_double(0.0), C.c_int64(0), 32, 4096, *([None] * 9))
        assert rc == 0
    finally:
        dec.free()
