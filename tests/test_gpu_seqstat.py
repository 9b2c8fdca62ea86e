"""-m gpu: wfst_decoder_sequence_stats (acc_kernel / seqstat_frame_kernel / seqstat_pack_kernel / seqstat_dense_kernel behind
align_index_kernel and posterior_kernel) -- the sMBR and MMI statistics of a channel's raw lattice against a reference alignment.

The reference of every comparison is the definition restated in numpy (tests/seqstat_util.py) over dec.raw_lattice(channel,
use_final_probs) fetched at the same moment.  The integers, the classes and their order are compared exactly; log_z, post, tot_acc
and value at the restatement's tolerances, derived from the lattice at hand before any run.  No test may hold a labelled frame whose
reference class has a mass below altern_util.TINY: each asserts that from the restatement before it looks at the device's answer.
Every test prints the largest difference / tolerance it saw; a ratio above 1 is a bug.  The lattices are built as
tests/test_gpu_framepost.py builds its own."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from align_util import from_gpu
from golden_util import GOLDEN_DIR, Golden, bits
from posterior_util import posteriors
from seqstat_util import LDS_RECS, compare, free_frames, sequence_stats
from test_gpu_framepost import (FANS, LEAD, N_TID, SCALES, canonical_arcs, canonical_states, decode_all, decoder, most_records, one_to_one,  # noqa: F401
                                small_decoder, world)

pytestmark = pytest.mark.gpu

E_ARG, E_CAPACITY, E_STATE = -1, -4, -5
CRITERIA = ["smbr", "mmi"]
SEQ_SCALES = [(1.0, 1.0), (0.1, 0.1), (1.0, 0.1)]


def best_ref(dec, c, label_map=None, ufp=True):
    """the 1-best's alignment through the map: one class per frame"""
    tids = np.asarray(dec.best_paths([int(c)], use_final_probs=ufp)[0]["tids"], np.int64)
    return tids if label_map is None else np.asarray(label_map, np.int64)[tids]


def every_fifth_changed(ref):
    r = np.array(ref, np.int64)
    r[::5] += 1
    return r


def check(dec, channels, refs, criterion, ufp=True, scales=(1.0, 1.0), label_map=None, sil=(), drop=False, what="", lattices=None, posts=None,
          **kw):
    """sequence_stats of the list against the restatement on each channel's raw lattice now; returns (got, want, worst ratio)"""
    lat = lattices if lattices is not None else [from_gpu(dec.raw_lattice(int(c), ufp)) for c in channels]
    want, Ps = [], []
    for i, L in enumerate(lat):
        none = L is None or L.n_states == 0
        P = None if none else (posts[i] if posts is not None else posteriors(L, scales[0], scales[1]))
        w = sequence_stats(None if none else L, refs[i], criterion, scales[0], scales[1], label_map, sil, drop, post=P)
        # decided on the restatement alone, before the device's answer is looked at
        assert none or not free_frames(w, refs[i]), "%s: a reference class with a mass below TINY" % what
        want.append(w)
        Ps.append(P)
    got = dec.sequence_stats(refs, channels, criterion=criterion, use_final_probs=ufp, graph_scale=scales[0], acoustic_scale=scales[1],
                             label_map=label_map, sil_classes=sil, drop_frames=drop, **kw)
    assert len(got) == len(channels)
    worst = 0.0
    for i, c in enumerate(channels):
        tag = "%s channel %d %s scales %s" % (what, c, criterion, scales)
        assert got[i]["status"] == 0, tag
        worst = max(worst, compare(got[i], want[i], Ps[i], None if Ps[i] is None else lat[i], refs[i], tag))
    assert worst <= 1.0, "%s: difference / tolerance = %g" % (what, worst)
    return got, want, worst


# ---- 1. finalized channels ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lattice_beam", [4.0, 8.0])
def test_finalized_channels(world, lattice_beam):
    """T = 40 / 97 / 150: both criteria, the three maps, the three pairs of scales; ref = the 1-best's alignment, and the same with
    every fifth frame changed"""
    dec = decoder(world, lattice_beam)
    try:
        decode_all(world, dec)
        ch = [2, 0, 1]
        lat = [from_gpu(dec.raw_lattice(c, True)) for c in ch]
        worst, tots = 0.0, []
        for sc in SEQ_SCALES:
            Ps = [posteriors(L, sc[0], sc[1]) for L in lat]
            for name, m in world["maps"].items():
                best = [best_ref(dec, c, m) for c in ch]
                for refs, rname in ((best, "1-best"), ([every_fifth_changed(r) for r in best], "changed")):
                    for crit in CRITERIA:
                        got, want, r = check(dec, ch, refs, crit, True, sc, m, what="lattice_beam %g %s %s" % (lattice_beam, name, rname),
                                             lattices=lat, posts=Ps)
                        worst = max(worst, r)
                        for i, c in enumerate(ch):
                            assert got[i]["n_frames"] == got[i]["n_ref_frames"] == world["T"][c]
                            if crit == "smbr" and rname == "1-best":
                                assert 0.0 < got[i]["tot_acc"] <= world["T"][c] + 1e-9
                        if crit == "smbr" and name == "pdf" and sc == (1.0, 1.0):
                            tots.append([round(g["tot_acc"], 3) for g in got])
        print("finalized, lattice_beam %g: largest difference / tolerance %.3g; tot_acc (1-best, changed) %s" % (lattice_beam, worst, tots))
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
                    sc = SEQ_SCALES[(k // 3 + k) % 3]
                    ref = every_fifth_changed(best_ref(dec, 0, m, ufp))
                    for crit in CRITERIA:
                        got, _, r = check(dec, [0], [ref], crit, ufp, sc, m, what="frame %d mode %d ufp %d %s" % (upto, mode, ufp, name), lattices=[L])
                        worst = max(worst, r)
                        assert got[0]["n_frames"] == upto
                    k += 1
                    sizes.append((upto, mode, int(ufp), L.n_states, int(np.bincount(L.st_frame).max()), most_records(L)))
            dec.set_live_lattice_prune(0)
        print("(frame, mode, ufp, states, most states of a frame, most emitting arcs of a frame):", sizes)
        print("live: largest difference / tolerance %.3g" % worst)
        assert any(s[4] > 1024 for s in sizes), "frames of more than 1 024 states: acc_kernel's lanes stride"
        assert any(s[5] > LDS_RECS for s in sizes), "frames beyond the LDS capacity: the workspace path is taken"
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
        worst = 0.0
        for sc in SCALES[:2]:
            for m in (None, thirds):
                refs = [every_fifth_changed(best_ref(dec, c, m)) if lat[c] is not None else np.zeros(0, np.int64) for c in ch]
                for crit in CRITERIA:
                    got, want, r = check(dec, ch, refs, crit, True, sc, m, what=name, lattices=lat)
                    worst = max(worst, r)
                    for i in ch:
                        assert (got[i]["n_frames"] > 0) == (lat[i] is not None)
        n_eps = sum(int((L.a_il == 0).sum()) for L in lat if L is not None)
        print("%s: largest difference / tolerance %.3g; arcs inside a frame %d" % (name, worst, n_eps))
        if name == "lattice_eps_chains":
            assert n_eps > 0
    finally:
        dec.free()
        graph.free()


# ---- 4. a fan around the LDS capacity -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fan", [LDS_RECS - 1, LDS_RECS, LDS_RECS + 1], ids=["one_below", "capacity", "one_above"])
def test_a_fan_around_the_lds_capacity(fan, synth, tmp_path):
    """test_gpu_framepost.py's fan: five steps of two arcs each, then `fan` emitting arcs with distinct transition-ids into as many
    final states: WFST_SEQSTAT_LDS_RECS - 1 triples, exactly as many, and one more, where the workspace takes over.  Under the identity
    every record is a run of its own; under tid % 3 there are three runs of about 341 records."""
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
            # the reference: the dearer arc of every step, then an arc from the middle of the fan
            tids = np.array([2 * s + 1 for s in range(T)] + [2 * T + 1 + fan // 2], np.int64)
            ref = tids if m is None else m[tids].astype(np.int64)
            for crit in CRITERIA:
                got, want, worst = check(dec, [0], [ref], crit, True, (1.0, 1.0), m, what="fan %d %s" % (fan, name), lattices=[L])
                g = got[0]
                assert g["n_frames"] == T + 1 and int(np.diff(g["frame_off"])[-1]) == (fan if m is None else 3)
                if m is None:
                    assert g["classes"][g["frame_off"][T]:].tolist() == list(range(2 * T + 1, 2 * T + 1 + fan))
                if crit == "smbr":
                    assert abs(g["values"][g["frame_off"][T]:].sum()) < 1e-9 and 0.0 < g["tot_acc"] < T + 1
                print("fan %d %s %s: largest difference / tolerance %.3g" % (fan, name, crit, worst))
    finally:
        dec.free()
        graph.free()


# ---- 5. fans of many sizes in one lattice -------------------------------------------------------------------------------------------
def test_fans_around_the_wave_and_the_block(synth, tmp_path):
    """test_gpu_framepost.py's eight fans in a row, one per frame (1, 2, 63, 64, 65, 255, 256, 257 emitting arcs and as many arcs
    inside the frame, which the load skips): the wave's 64 lanes and the block's 256 in the sort and both scans"""
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
        sevenths = np.arange(tid + 1, dtype=np.int32) % 7
        for name, m in (("tid", None), ("sevenths", sevenths)):
            tids = np.array([a + N // 2 for a, N in zip(first, FANS)], np.int64)      # an arc from the middle of every fan
            ref = tids if m is None else m[tids].astype(np.int64)
            ref[3] = -1                                                               # one unlabelled frame
            for crit in CRITERIA:
                got, want, r = check(dec, [0], [ref], crit, True, (1.0, 1.0), m, what="fans " + name, lattices=[L])
                worst = max(worst, r)
                g = got[0]
                assert g["n_ref_frames"] == len(FANS) - 1
                assert np.diff(g["frame_off"]).tolist() == (FANS if m is None else [min(N, 7) for N in FANS])
                if crit == "smbr":
                    assert g["values"][0] == 0.0, "a frame with a single arc has no gradient"
                    for f in range(len(FANS)):
                        assert abs(g["values"][g["frame_off"][f]:g["frame_off"][f + 1]].sum()) < 1e-9
        print("fans: largest difference / tolerance %.3g" % worst)
    finally:
        dec.free()
        graph.free()


# ---- 6. two chains that share transition-ids, under a phone map -----------------------------------------------------------------------
def test_two_chains_that_share_tids_under_a_phone_map(synth, tmp_path):
    """0 --tid 1--> 1, then two chains of 300-arc fans over the SAME transition-ids at different costs, 1 -> {a_i} and 1 -> {b_i}, which
    one phone map sends to two phones: a frame's class sums records that leave different states, in runs of hundreds"""
    N = 300
    arcs = {0: [(1, 9, 0.0, 1)], 1: [(2, 1, 0.25, 2), (3, 2, 1.0, 3)]}
    arcs[2] = [(4 + i, 0, 0.01 * (i % 17), 4) for i in range(N)]
    arcs[3] = [(4 + i, 0, 0.02 * (i % 13), 5) for i in range(N)]
    arcs[4] = [(4 + N, 3, 0.0, 6)]
    arcs[5] = [(4 + N, 4, 1.5, 6), (5 + N, 5, 0.25, 6)]
    n_tid = 5 + N
    graph, dec = small_decoder(synth, tmp_path, "chains", 7, arcs, {6: 0.0}, n_tid, 4, one_to_one(n_tid))
    try:
        L = from_gpu(dec.raw_lattice(0, True))
        phone = np.ones(n_tid + 1, np.int32)
        phone[4:4 + N] = 2 + (np.arange(N) >= N // 2)      # the shared transition-ids: phones 2 and 3, 150 tids and 300 records each
        phone[4 + N:] = 4
        phone[0] = 0
        worst = 0.0
        for sc in SEQ_SCALES:
            for m, ref in ((phone, [1, 1, 3, 4]), (None, [1, 2, 4 + 7, 4 + N])):
                for crit in CRITERIA:
                    got, want, r = check(dec, [0], [np.array(ref)], crit, True, sc, m, what="chains", lattices=[L])
                    worst = max(worst, r)
                    g = got[0]
                    assert g["n_frames"] == 4
                    if m is not None:
                        assert g["frame_off"].tolist() == [0, 1, 2, 4, 5] and g["classes"].tolist() == [1, 1, 2, 3, 4]
        assert int(((L.st_frame[L.a_src] == 2) & (L.a_il > 0)).sum()) == 2 * N
        print("chains: largest difference / tolerance %.3g" % worst)
    finally:
        dec.free()
        graph.free()


# ---- 7. a long epsilon chain inside a frame -----------------------------------------------------------------------------------------------
def test_a_seventy_step_epsilon_chain_inside_a_frame(synth, tmp_path):
    """0 --tid 1--> s1, s1 -eps-> s2 -eps-> ... -eps-> s71 inside frame 1, every s_k --tid 2 + k % 3--> F --tid 5--> the final state:
    acc_kernel walks 71 levels of frame 1 forward and backward, and fa / fb differ along the chain"""
    K = 70
    arcs = {0: [(1, 7, 0.0, 1)]}
    F = K + 2
    for k in range(1, K + 2):
        arcs[k] = [(2 + k % 3, 0, 0.03 * (k % 5), F)]
        if k <= K:
            arcs[k].append((0, 0, 0.02, k + 1))
    arcs[F] = [(5, 8, 0.0, F + 1)]
    graph, dec = small_decoder(synth, tmp_path, "epschain", F + 2, arcs, {F + 1: 0.0}, 5, 3, one_to_one(5))
    try:
        L = from_gpu(dec.raw_lattice(0, True))
        assert int((L.a_il == 0).sum()) >= K and posteriors(L)["n_levels"] >= K + 3
        worst = 0.0
        for sc in [(1.0, 1.0), (0.1, 0.1)]:
            for ref in ([1, 3, 5], [1, 2, 9]):
                for crit in CRITERIA:
                    got, want, r = check(dec, [0], [np.array(ref)], crit, True, sc, None, what="eps chain", lattices=[L])
                    worst = max(worst, r)
                    assert got[0]["classes"].tolist()[:4] == [1, 2, 3, 4]
        print("eps chain: largest difference / tolerance %.3g" % worst)
    finally:
        dec.free()
        graph.free()


# ---- 8. silence classes and drop_frames --------------------------------------------------------------------------------------------------
def test_silence_classes_and_drop_frames(world):
    dec = decoder(world, 8.0, 1)
    try:
        dec.init()
        dec.advance(world["ptrs"][1:2], [97], N_TID // 2)
        dec.finalize()
        L = from_gpu(dec.raw_lattice(0, True))
        P = posteriors(L)
        m = world["maps"]["phone"]
        best = best_ref(dec, 0, m)
        changed = every_fifth_changed(best)
        worst = 0.0
        plain, _, r = check(dec, [0], [best], "smbr", label_map=m, what="no silence", lattices=[L], posts=[P])
        sil = sorted(set(int(x) for x in best[:30]))[:64]
        quiet, _, r2 = check(dec, [0], [best], "smbr", label_map=m, sil=sil, what="silence", lattices=[L], posts=[P])
        assert quiet[0]["tot_acc"] < plain[0]["tot_acc"] - 1.0, "the reference's silence frames count no more"
        # 64 classes, most of them in no frame
        many = sorted(set(sil) | set(range(1000, 1000 + 64 - len(sil))))
        assert len(many) == 64
        full, _, r3 = check(dec, [0], [best], "smbr", label_map=m, sil=many, what="64 silence classes", lattices=[L], posts=[P])
        assert abs(full[0]["tot_acc"] - quiet[0]["tot_acc"]) < 1e-9
        worst = max(r, r2, r3)
        for drop in (False, True):
            got, want, r = check(dec, [0], [changed], "mmi", label_map=m, drop=drop, what="drop %d" % drop, lattices=[L], posts=[P])
            worst = max(worst, r)
            assert got[0]["n_dropped"] == want[0]["n_dropped"] and (want[0]["n_dropped"] > 0) == drop
            if not drop:
                extra = int((got[0]["posts"] == 0.0).sum())
                assert extra > 0 and np.all(got[0]["values"][got[0]["posts"] == 0.0] == 1.0)
            else:
                assert extra == want[0]["n_dropped"] and np.all(got[0]["posts"] > 0.0)
        print("silence and drop_frames: largest difference / tolerance %.3g; frames dropped %d of %d" % (worst, want[0]["n_dropped"], want[0]["n_ref_frames"]))
    finally:
        dec.free()


# ---- 9. mixed lists, a channel over max_cells, rows too short ---------------------------------------------------------------------------
def test_mixed_list_and_capacities(world, monkeypatch):
    W = world["W"]
    dec = decoder(world, 8.0)
    try:
        dec.init()
        dec.advance(world["ptrs"], [40, 60, 150], N_TID // 2)
        dec.finalize(channels=[0, 2])          # channel 1 stays live at frame 60
        dec.set_live_lattice_prune(1)
        ch = [1, 2, 0]
        m = world["maps"]["pdf"]
        refs = [every_fifth_changed(best_ref(dec, c, m)) for c in ch]
        lat = [from_gpu(dec.raw_lattice(c, True)) for c in ch]
        got, want, worst = check(dec, ch, refs, "smbr", label_map=m, what="mixed", lattices=lat)
        assert [g["n_frames"] for g in got] == [60, 150, 40]
        states = [L.n_states for L in lat]
        big = int(np.argmax(states))
        tight = dec.sequence_stats(refs, ch, label_map=m, max_cells=states[big] - 1)
        assert [g["status"] for g in tight] == [E_CAPACITY if i == big else 0 for i in range(3)]
        t = tight[big]
        assert t["n_frames"] == 0 and t["log_z"] == 0.0 and t["tot_acc"] == 0.0 and len(t["classes"]) == 0 and t["n_ref_frames"] == 0
        for i in set(range(3)) - {big}:
            P = posteriors(lat[i])
            worst = max(worst, compare(tight[i], sequence_stats(lat[i], refs[i], "smbr", label_map=m, post=P), P, lat[i], refs[i], "beside the channel over max_cells"))
        assert [g["status"] for g in dec.sequence_stats(refs, ch, label_map=m, max_cells=states[big])] == [0, 0, 0]
        # the binding takes its first room from the frames decoded: with one entry per frame that is too little, and its repeat runs
        monkeypatch.setattr(W, "FRAME_POST_ENTRIES_PER_FRAME", 1)
        again = dec.sequence_stats(refs, ch, label_map=m)
        monkeypatch.undo()
        for a, b in zip(again, got):
            assert a["status"] == 0 and a["n_entries"] > 150 and np.array_equal(a["frame_off"], b["frame_off"]) and np.array_equal(a["classes"], b["classes"])
            assert np.allclose(a["values"], b["values"], rtol=0, atol=1e-9) and np.allclose(a["posts"], b["posts"], rtol=0, atol=1e-9)
        # rows too short through the C ABI: the room needed comes back, the channel's lists stay zero
        o = raw_call(W, dec, ch, refs, 150, 150, label_map=m)
        assert o["rc"] == 0 and o["status"].tolist() == [E_CAPACITY] * 3 and o["n_entries"].tolist() == [g["n_entries"] for g in got]
        assert o["n_frames"].tolist() == [60, 150, 40] and not o["entry_class"].any() and not o["entry_value"].any() and not o["frame_off"].any()
        # use_final_probs = 0: the finalized channels have no lattice, the live one answers
        live_only = dec.sequence_stats(refs, ch, label_map=m, use_final_probs=False)
        assert [g["status"] for g in live_only] == [0, 0, 0] and [g["n_frames"] for g in live_only] == [60, 0, 0]
        assert live_only[1]["log_z"] == 0.0 and live_only[1]["tot_acc"] == 0.0 and live_only[1]["frame_off"].tolist() == [0]
        assert worst <= 1.0
        print("mixed: largest difference / tolerance %.3g" % worst)
    finally:
        dec.free()


def raw_call(W, dec, channels, refs, capf, cape, crit=1, ufp=True, label_map=None, sil=(), max_cells=0, gs=1.0, as_=1.0, grad=None,
             n_cols=0, grad_scale=1.0, n_ref=None):
    """the C entry point itself, with rows of the caller's size: dict of the raw output arrays and the return code"""
    I, D = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    ch = np.ascontiguousarray(channels, np.int32)
    n = len(ch)
    cap_ref = max([len(r) for r in refs] + [1])
    ref = np.full((n, cap_ref), -1, np.int32)
    for i, r in enumerate(refs):
        ref[i, :len(r)] = r
    nr = np.array([len(r) for r in refs] if n_ref is None else n_ref, np.int32)
    o = dict(status=np.full(n, 99, np.int32), log_z=np.full(n, 9.0), tot_acc=np.full(n, 9.0), n_frames=np.full(n, 99, np.int32),
             n_ref_frames=np.full(n, 99, np.int32), n_dropped=np.full(n, 99, np.int32), n_entries=np.full(n, 99, np.int32),
             frame_off=np.full((n, capf + 1), 99, np.int32), entry_class=np.full((n, cape), 99, np.int32), entry_post=np.full((n, cape), 9.0),
             entry_value=np.full((n, cape), 9.0))
    p = lambda a: a.ctypes.data_as(I if a.dtype == np.int32 else D)
    m = None if label_map is None else np.ascontiguousarray(label_map, np.int32)
    s = np.ascontiguousarray(list(sil), np.int32)
    g_ptr = g_pitch = g_rows = None
    if grad is not None:
        g_ptr = (C.c_void_p * n)(*[int(x[0]) for x in grad])
        g_pitch = np.array([x[1] for x in grad], np.int64)
        g_rows = np.array([x[2] for x in grad], np.int32)
    o["rc"] = W.lib().wfst_decoder_sequence_stats(
        dec.h, p(ch), n, int(crit), int(ufp), C.c_double(gs), C.c_double(as_), None if m is None else p(m), 0 if m is None else len(m) - 1, p(ref),
        p(nr), cap_ref, p(s) if len(s) else None, len(s), 0, C.c_int64(max_cells), capf, cape, g_ptr,
        None if grad is None else g_pitch.ctypes.data_as(C.POINTER(C.c_int64)), None if grad is None else p(g_rows), n_cols, C.c_double(grad_scale),
        C.c_void_p(W.WFST_STREAM_NONE), p(o["status"]), p(o["log_z"]), p(o["tot_acc"]), p(o["n_frames"]), p(o["n_ref_frames"]), p(o["n_dropped"]),
        p(o["n_entries"]), p(o["frame_off"]), p(o["entry_class"]), p(o["entry_post"]), p(o["entry_value"]))
    o["msg"] = W.lib().wfst_last_error().decode()
    return o


# ---- 10. a biglm lattice decoder -----------------------------------------------------------------------------------------------
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
        refs = [every_fifth_changed(best_ref(dec, c, m)) for c in have]
        worst = 0.0
        for crit in CRITERIA:
            got, _, r = check(dec, have, refs, crit, True, (1.0, 0.1), m, what="biglm pdf")
            worst = max(worst, r)
            assert all(g["n_frames"] > 0 and g["n_entries"] > 0 for g in got)
        print("biglm: %d lattices, largest difference / tolerance %.3g" % (len(have), worst))
    finally:
        dec.free()
        for lm in lms:
            lm.free()
        graph.free()


# ---- 11. the dense output -------------------------------------------------------------------------------------------------------------
def test_dense_rows(world):
    """grad[f][v] is bit for bit float32(grad_scale * value) of the SAME call's list and zero in the other columns; a sentinel in the
    padding beyond n_cols and in the rows past n_frames survives; a channel without a tensor is left alone; the lists do not depend
    on grad"""
    import torch

    dec = decoder(world, 4.0)
    try:
        decode_all(world, dec)
        m = world["maps"]["pdf"]
        n_cols, pitch = N_TID // 2, N_TID // 2 + 20
        ch = [1, 0, 2]
        refs = [every_fifth_changed(best_ref(dec, c, m)) % n_cols for c in ch]
        SENT = 777.0
        side = torch.cuda.Stream()
        for crit, scale in (("smbr", -0.5), ("mmi", 3.0)):
            # channel 1 (97 frames): more rows than frames, pitched; channel 0 (40 frames): none; channel 2 (150 frames): fewer rows, dense
            # on a stream of torch's own that is not the default one: the fills are enqueued on it and NOT waited for, the call's writes
            # come behind them, and the reads enqueued on it right behind the call see the rows because that stream waits for them
            with torch.cuda.stream(side):
                a = torch.full((110, pitch), SENT, dtype=torch.float32, device="cuda")
                b = torch.full((100, n_cols), SENT, dtype=torch.float32, device="cuda")
                got = dec.sequence_stats(refs, ch, criterion=crit, label_map=m, grad=[a[:, :n_cols], None, b], grad_scale=scale, stream="current")
                ha, hb = a.cpu().numpy(), b.cpu().numpy()
            for g, h, rows, T in ((got[0], ha, 110, 97), (got[2], hb, 100, 150)):
                assert g["status"] == 0 and g["n_frames"] == T
                k = min(rows, T)
                want = np.zeros((k, n_cols), np.float32)
                for f in range(k):
                    lo, hi = g["frame_off"][f], g["frame_off"][f + 1]
                    want[f, g["classes"][lo:hi]] = (scale * g["values"][lo:hi]).astype(np.float32)
                assert want.any() and np.array_equal(bits(h[:k, :n_cols]), bits(want)), crit
                assert np.all(h[k:] == SENT), "the rows past n_frames"
            assert np.all(ha[:, n_cols:] == SENT), "the padding beyond n_cols"
            # the lists without grad: the same, to the rounding of a sum whose order the index decides
            bare = dec.sequence_stats(refs, ch, criterion=crit, label_map=m)
            for x, y in zip(bare, got):
                assert np.array_equal(x["frame_off"], y["frame_off"]) and np.array_equal(x["classes"], y["classes"]) and x["n_dropped"] == y["n_dropped"]
                assert np.allclose(x["values"], y["values"], rtol=0, atol=1e-9) and np.allclose(x["posts"], y["posts"], rtol=0, atol=1e-9)
            # the dense rows alone (no lists fetched) hold the same numbers, to that rounding
            c = torch.full((150, n_cols), SENT, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()     # stream=None: the rows are free when the call is made
            only = dec.sequence_stats(refs[2:], ch[2:], criterion=crit, label_map=m, grad=[c], grad_scale=scale, stream=None, lists=False)
            assert only[0]["status"] == 0 and only[0]["n_frames"] == 150 and len(only[0]["classes"]) == 0
            assert abs(only[0]["tot_acc"] - got[2]["tot_acc"]) < 1e-9
            assert np.allclose(c.cpu().numpy()[:100], hb, rtol=0, atol=1e-6)
    finally:
        dec.free()


# ---- 12. the error surface -------------------------------------------------------------------------------------------------------
def test_error_surface(world):
    import torch

    W = world["W"]
    plain = decoder(world, 4.0, 2, lattice_links=0)
    try:
        plain.init()
        plain.advance(world["ptrs"][:2], [10, 10], N_TID // 2)
        with pytest.raises(W.WfstError) as e:
            plain.sequence_stats([[1], [1]])
        assert e.value.code == E_STATE
    finally:
        plain.free()
    dec = decoder(world, 4.0, 3)
    try:
        dec.init(channels=[0, 1])
        dec.advance(world["ptrs"][:2], [20, 20], N_TID // 2, channels=[0, 1])
        ref = [best_ref(dec, 0, None, False)]
        ok = dec.sequence_stats(ref, [0], use_final_probs=False)
        assert ok[0]["status"] == 0 and ok[0]["n_frames"] == 20 and ok[0]["n_ref_frames"] == 20
        for ch, code in (([0, 0], E_ARG), ([0, 3], E_ARG), ([0, 2], E_STATE)):
            with pytest.raises(W.WfstError) as e:
                dec.sequence_stats(ref * 2, ch, use_final_probs=False)
            assert e.value.code == code, ch
        for kw, word in ((dict(graph_scale=-1.0), "scale"), (dict(acoustic_scale=float("nan")), "scale"), (dict(criterion=7), "criterion"),
                         (dict(sil_classes=[3, 2]), "sil_classes"), (dict(sil_classes=[-1]), "sil_classes"), (dict(sil_classes=list(range(65))), "sil_classes"),
                         (dict(max_cells=-1), "max_cells"), (dict(label_map=np.zeros(N_TID // 2, np.int32)), "label_map")):
            with pytest.raises(W.WfstError) as e:
                dec.sequence_stats(ref, [0], use_final_probs=False, **kw)
            assert e.value.code == E_ARG and word in str(e.value), kw
        # the dense rules: a width that does not exceed the largest transition-id, a map entry beyond it, a reference class beyond it, a
        # misaligned pointer, a pitch below the width, a grad_scale that is not finite
        g = torch.zeros((20, N_TID + 1), dtype=torch.float32, device="cuda")
        assert dec.sequence_stats(ref, [0], use_final_probs=False, grad=[g])[0]["status"] == 0
        with pytest.raises(W.WfstError) as e:
            dec.sequence_stats(ref, [0], use_final_probs=False, grad=[g[:, :10]])
        assert e.value.code == E_ARG and "n_cols" in str(e.value)
        with pytest.raises(W.WfstError) as e:
            dec.sequence_stats([[5, 5]], [0], use_final_probs=False, label_map=world["maps"]["pdf"], grad=[g[:, :100]])
        assert e.value.code == E_ARG and "label_map class" in str(e.value)
        with pytest.raises(W.WfstError) as e:
            dec.sequence_stats([[5, N_TID + 1]], [0], use_final_probs=False, grad=[g])
        assert e.value.code == E_ARG and "ref class" in str(e.value)
        with pytest.raises(W.WfstError) as e:
            dec.sequence_stats(ref, [0], use_final_probs=False, grad=[g], grad_scale=float("inf"))
        assert e.value.code == E_ARG and "grad_scale" in str(e.value)
        o = raw_call(W, dec, [0], ref, 32, 4096, ufp=False, grad=[(g.data_ptr() + 2, N_TID + 1, 20)], n_cols=N_TID + 1)
        assert o["rc"] == E_ARG and "aligned" in o["msg"]
        o = raw_call(W, dec, [0], ref, 32, 4096, ufp=False, grad=[(g.data_ptr(), N_TID, 20)], n_cols=N_TID + 1)
        assert o["rc"] == E_ARG and "pitch" in o["msg"]
        # through the C ABI: rows of no room (one of the two), a negative n_ref, and NULL outputs are fine
        assert raw_call(W, dec, [0], ref, 0, 10, ufp=False)["rc"] == E_ARG and raw_call(W, dec, [0], ref, 10, 0, ufp=False)["rc"] == E_ARG
        assert raw_call(W, dec, [0], ref, 32, 4096, ufp=False, n_ref=[-1])["rc"] == E_ARG
        none = raw_call(W, dec, [0], ref, 0, 0, ufp=False)
        assert none["rc"] == 0 and none["status"].tolist() == [0] and none["n_frames"].tolist() == [20] and none["n_entries"][0] > 0
        one = np.array([0], np.int32)
        rc = W.lib().wfst_decoder_sequence_stats(dec.h, one.ctypes.data_as(C.POINTER(C.c_int32)), 1, 1, 0, C.c_double(1.0), C.c_double(1.0), None, 0,
                                                 None, None, 0, None, 0, 0, C.c_int64(0), 32, 4096, None, None, None, 0, C.c_double(1.0),
                                                 C.c_void_p(W.WFST_STREAM_NONE), *([None] * 11))
        assert rc == 0
    finally:
        dec.free()
