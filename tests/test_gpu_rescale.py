"""-m gpu: wfst_decoder_rescaled_words (rescale_kernel behind align_index_kernel) -- the best path of a channel's raw lattice picked
again under another graph scale, acoustic scale and word penalty.

The reference of every comparison is the definition restated in numpy (tests/rescale_util.py) over dec.raw_lattice(channel,
use_final_probs) fetched at the same moment, and everything is compared BIT FOR BIT: found, the words, their times, n_arcs, the
transition-ids, and the bits of scaled_cost, tot_score and lm_score."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import pyoracle
import signed_util as S
from align_util import from_gpu
from golden_util import GOLDEN_DIR, bits
from posterior_util import posteriors
from rescale_util import _levels, bits32, bits64, rescale_many, same_answer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_CAPACITY, E_STATE = -1, -4, -5
N_TID = 600
LIM = dict(max_frames=192, max_tokens_per_frame=32768, arena_tokens=1 << 20, lattice_links=1 << 21)
WIDE = dict(beam=200.0, max_active=1000000, min_active=0, lattice_beam=100.0, prune_interval=10)
# the search's own scales, the usual sweep's corners, one scale off, both off (every path ties, with and without a penalty that then
# decides alone), a negative and a large penalty
SETTINGS = [(1.0, 1.0, 0.0), (1.0, 0.1, 0.0), (0.1, 1.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, 0.0),
            (1.0, 1.0, -3.0), (1.0, 1.0, 5.0)]


def cfg(lattice_beam):
    return dict(beam=12.0, max_active=1000000, min_active=0, lattice_beam=lattice_beam, prune_interval=10)


def kernel_lanes():
    text = open(os.path.join(ROOT, "asr-decoder_amd", "csrc", "wfst_rescale.hip")).read()
    return int(re.search(r"constexpr int kRsThreads = (\d+);", text).group(1))


@pytest.fixture(scope="module")
def world(synth, tmp_path_factory):
    import gpu_util as G

    W = G.wfstdec
    g = synth.make_hclg_like(3000, seed=21, n_tid=N_TID, n_words=500)
    m = synth.default_tid2pdf(N_TID)
    path = str(tmp_path_factory.mktemp("rescale") / "g.bin")
    g.write(path)
    graph = W.Graph.load(path)
    graph.set_tid2pdf(m)
    mats = [synth.make_loglikes(g, T, N_TID // 2, m, seed=s, mu=-2.2)[0] for T, s in ((40, 700), (97, 701), (150, 702))]
    dev = G.upload(mats)
    yield dict(G=G, W=W, graph=graph, mats=mats, dev=dev, ptrs=[t.data_ptr() for t in dev], T=[x.shape[0] for x in mats])
    graph.free()


def decoder(world, cd, n=3, **kw):
    lim = dict(LIM)
    lim.update(kw)
    return world["W"].BatchDecoder(world["graph"], world["G"].gpu_config(cd), n, **lim)


def decode_all(world, dec):
    dec.init()
    dec.advance(world["ptrs"], world["T"], N_TID // 2)
    dec.finalize()


def check(dec, channels, settings=SETTINGS, ufp=True, what="", lattices=None, exact_path=True):
    """rescaled_words of the list against the restatement on each channel's raw lattice now; returns (got, want, lattices).
    exact_path=False (biglm): where a decision of the restatement was ambiguous only the costs are held bit for bit"""
    lat = lattices if lattices is not None else [from_gpu(dec.raw_lattice(int(c), ufp)) for c in channels]
    want = [rescale_many(L, settings) for L in lat]
    got = dec.rescaled_words(settings, channels, use_final_probs=ufp, cap_tids=LIM["max_frames"])
    assert len(got) == len(channels)
    for i, c in enumerate(channels):
        assert len(got[i]) == len(settings)
        for q, s in enumerate(settings):
            tag = "%s channel %d setting %s" % (what, c, s)
            assert got[i][q]["status"] == 0, tag
            if not exact_path and want[i][q]["found"] and want[i][q]["ambiguous"]:
                assert got[i][q]["found"] and bits64(got[i][q]["scaled_cost"]) == bits64(want[i][q]["scaled_cost"]), tag
                continue
            same_answer(got[i][q], want[i][q], tag, tids=True)
    return got, want, lat


def raw_call(W, dec, channels, settings, cap_words, cap_tids=0, ufp=True, max_cells=0, with_tids=False):
    """the C entry point itself, with rows of the caller's size: dict of the raw output arrays and the return code"""
    I, D, F = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_float)
    ch = np.ascontiguousarray(channels, np.int32)
    st = np.ascontiguousarray(settings, np.float64).reshape(-1, 3)
    n, ns = len(ch), len(st)
    pair = lambda t, fill: np.full((n, ns), fill, t)
    o = dict(status=np.full(n, 99, np.int32), found=pair(np.int32, 99), n_arcs=pair(np.int32, 99), n_hyp=pair(np.int32, 99), n_tids=pair(np.int32, 99),
             hyp_words=np.full((n, ns, cap_words), 99, np.int32), begin=np.full((n, ns, cap_words), 99, np.int32),
             end=np.full((n, ns, cap_words), 99, np.int32), tids=np.full((n, ns, max(cap_tids, 1)), 99, np.int32),
             scaled_cost=pair(np.float64, 9.0), tot=pair(np.float32, 9.0), lm=pair(np.float32, 9.0))
    p = lambda a: a.ctypes.data_as({np.dtype(np.int32): I, np.dtype(np.float64): D, np.dtype(np.float32): F}[a.dtype])
    o["rc"] = W.lib().wfst_decoder_rescaled_words(dec.h, p(ch), n, int(ufp), ns, p(st), cap_words, cap_tids, C.c_int64(max_cells), p(o["status"]),
                                                  p(o["found"]), p(o["n_arcs"]), p(o["n_hyp"]), p(o["n_tids"]), p(o["hyp_words"]), p(o["begin"]),
                                                  p(o["end"]), p(o["tids"]) if with_tids else None, p(o["scaled_cost"]), p(o["tot"]), p(o["lm"]))
    return o


# ---- 1. finalized channels --------------------------------------------------------------------------------------------------------
def test_finalized_channels(world):
    """T = 40 / 97 / 150 at lattice_beam 6 under the nine settings; the all-tie and near-all-tie settings are the ones that catch a
    traceback that depends on the order of the device's arc index"""
    dec = decoder(world, cfg(6.0))
    try:
        decode_all(world, dec)
        ch = [2, 0, 1]
        got, want, lat = check(dec, ch, what="finalized")
        n_own = 0
        for i, c in enumerate(ch):
            assert all(g["found"] for g in got[i])
            assert all(g["n_tids"] == world["T"][c] for g in got[i]), "one transition-id per frame"
            # (1, 1, 0) is the search's own best path where the lattice has no second path within 1e-3 of the first (the search
            # compares float32 sums); its float64 cost bounds the minimum in any case
            bp = dec.best_paths([c])[0]
            x = np.float64(0.0)
            for gr, ac in zip(bp["graph"], bp["ac"]):
                x = (x + ((1.0 * np.float64(gr) + 1.0 * np.float64(ac)) + 0.0)) + 0.0
            assert got[i][0]["scaled_cost"] <= x
            two = pyoracle.nshortest_paths(lat[i], 2)
            if len(two) < 2 or float(two[1]["tot"]) - float(two[0]["tot"]) > 1e-3:
                n_own += 1
                assert np.array_equal(got[i][0]["hyp_words"], bp["words"]) and np.array_equal(got[i][0]["tids"], bp["tids"])
                assert bits32(got[i][0]["tot"]) == bits32(bp["tot_score"]) and bits32(got[i][0]["lm"]) == bits32(bp["lm_score"])
            assert got[i][7]["n_hyp"] >= got[i][0]["n_hyp"] >= got[i][8]["n_hyp"], "a penalty moves the word count its way"
        ties = sum(w["tie"] for ws in want for w in ws)
        differ = sum(not np.array_equal(ws[0]["words"], w["words"]) for ws in want for w in ws[1:])
        print("finalized: states %s; %d of %d answers went through a tie; %d of %d settings' words differ from (1, 1, 0)'s; words per setting %s"
              % ([L.n_states for L in lat], ties, 3 * len(SETTINGS), differ, 3 * (len(SETTINGS) - 1), [[g["n_hyp"] for g in row] for row in got]))
        assert ties >= 6 and differ >= 6 and n_own >= 2
    finally:
        dec.free()


# ---- 2. one setting, sixty-four settings ----------------------------------------------------------------------------------------------
def test_one_setting_and_sixty_four(world):
    dec = decoder(world, cfg(6.0))
    try:
        decode_all(world, dec)
        lat = [from_gpu(dec.raw_lattice(c, True)) for c in (0, 1, 2)]
        check(dec, [0, 1, 2], [(1.0, 0.07, 0.5)], what="one setting", lattices=lat)
        sweep = [(1.0, 1.0 / lmwt, wip) for lmwt in (1, 2, 4, 7, 9, 11, 13, 17) for wip in (-2.0, -1.0, -0.5, 0.0, 0.25, 0.5, 1.0, 2.0)]
        assert len(sweep) == 64
        got, want, _ = check(dec, [1, 2, 0], sweep, what="64 settings", lattices=[lat[1], lat[2], lat[0]])
        distinct = [len({tuple(g["hyp_words"].tolist()) for g in row}) for row in got]
        print("64 settings: distinct word sequences per channel %s" % distinct)
        assert max(distinct) >= 3
    finally:
        dec.free()


# ---- 3. frames wider than the workgroup, chains of arcs inside a frame -----------------------------------------------------------------
def test_wide_lattice_strided_frames_and_epsilon_chains(world):
    dec = decoder(world, WIDE, 1)
    try:
        dec.init()
        dec.advance(world["ptrs"][:1], [40], N_TID // 2)
        dec.finalize()
        L = from_gpu(dec.raw_lattice(0, True))
        # asserted from the lattice, before the device's answer is looked at
        most = int(np.bincount(L.st_frame).max())
        assert most > kernel_lanes(), "some frame has more states than the workgroup has lanes: the strided path"
        _, depth = _levels(L)
        assert int(depth.max()) >= 2, "some frame has a chain of arcs inside it at least two arcs deep: the relaxation runs more than once"
        got, want, _ = check(dec, [0], what="wide", lattices=[L])
        print("wide: %d states, %d arcs, most states of a frame %d (lanes %d), deepest chain inside a frame %d; words %s"
              % (L.n_states, len(L.a_src), most, kernel_lanes(), int(depth.max()), [g["n_hyp"] for g in got[0]]))
    finally:
        dec.free()


# ---- 4. live channels mixed with finalized ones, read-only ------------------------------------------------------------------------------
def test_live_channels_mixed_with_finalized_and_the_call_is_read_only(world):
    """channels 0 and 1 decode the 150-frame utterance, channel 2 the 40-frame one and is finalized; at frames 25 and 97 channels 0 and
    2 are queried under both live-prune modes and both use_final_probs; channel 1 is channel 0's twin that is never queried"""
    dec = decoder(world, cfg(6.0))
    try:
        p, q, stride = world["ptrs"][2], world["ptrs"][0], N_TID // 2
        dec.init()
        dec.advance([p, p, q], [25, 25, 40], stride)
        dec.finalize(channels=[2])
        sizes = []
        for upto in (25, 97):
            if upto > 25:
                dec.advance([p, p], [upto, upto], stride, channels=[0, 1])
            for mode in (0, 1):
                dec.set_live_lattice_prune(mode)
                for ufp in (False, True):
                    got, want, lat = check(dec, [0, 2], ufp=ufp, what="frame %d mode %d ufp %d" % (upto, mode, ufp))
                    assert all(g["found"] and g["n_tids"] == upto for g in got[0])
                    if ufp:
                        assert all(g["found"] and g["n_tids"] == 40 for g in got[1])
                    else:   # a finalized channel asked without final-probs has no lattice: all zero, status OK
                        assert lat[1] is None
                        for g in got[1]:
                            assert not g["found"] and g["status"] == 0 and g["n_arcs"] == 0 and g["n_hyp"] == 0 and g["n_tids"] == 0
                            assert g["scaled_cost"] == 0.0 and bits32(g["tot"]) == 0 and bits32(g["lm"]) == 0 and len(g["tids"]) == 0
                    sizes.append((upto, mode, int(ufp), lat[0].n_states))
            dec.set_live_lattice_prune(0)
        print("(frame, mode, ufp, states of the live lattice):", sizes)
        assert min(s[3] for s in sizes if s[1] == 1) < min(s[3] for s in sizes if s[1] == 0), "mode 1 serves a pruned lattice"
        dec.advance([p, p], [150, 150], stride, channels=[0, 1])
        dec.finalize(channels=[0, 1])
        a, b = dec.best_paths([0, 1])
        for key in ("ilabel", "olabel"):
            assert np.array_equal(a[key], b[key]), key
        for key in ("graph", "ac"):
            assert np.array_equal(bits(a[key]), bits(b[key])), key
        assert bits32(a["tot_score"]) == bits32(b["tot_score"]) and bits32(a["lm_score"]) == bits32(b["lm_score"])
    finally:
        dec.free()


# ---- 5. negative and zero-crossing costs ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", ["crossing", "negative"])
def test_signed_costs(shift, synth, tmp_path):
    import gpu_util as G

    g, m, mats = S.workloads(synth)
    path = str(tmp_path / "g.bin")
    g.write(path)
    graph = G.wfstdec.Graph.load(path)
    graph.set_tid2pdf(m)
    x = mats[shift]
    dec = G.wfstdec.BatchDecoder(graph, G.gpu_config(S.BEAM_ONLY), len(x), max_frames=64, max_tokens_per_frame=32768, arena_tokens=1 << 20,
                                 lattice_links=1 << 21)
    try:
        dev = G.upload(x)
        dec.init()
        dec.advance([t.data_ptr() for t in dev], [a.shape[0] for a in x], S.N_PDF)
        dec.finalize()
        got, want, lat = check(dec, list(range(len(x))), what=shift)
        costs = np.array([[g["scaled_cost"] for g in row] for row in got])
        print("%s: scaled_cost at (1, 1, 0) %s, at (1, 0.1, 0) %s" % (shift, costs[:, 0].tolist(), costs[:, 1].tolist()))
        assert np.all(costs[:, 0] < 0.0) if shift == "negative" else np.any(costs < 0.0)
        # arcs of both signs on the winning paths
        L, arcs = lat[0], want[0][0]["arcs"]
        tot = L.a_graph[arcs] + L.a_ac[arcs]
        assert np.any(tot < 0) and (shift == "negative" or np.any(tot > 0))
    finally:
        dec.free()
        graph.free()


# ---- 6. a biglm lattice decoder ---------------------------------------------------------------------------------------------------------
def test_biglm_lattice_decoder(tmp_path):
    """costs bit for bit; the path in full where no decision was ambiguous (two tokens of a frame may share a graph state here, so the
    order among the survivors of the tie rule is unspecified), and otherwise as a valid minimal path: the lattice restricted to the
    arcs that carry the device's transition-ids at their frames has a path of exactly the device's cost"""
    import gpu_util as G
    from types import SimpleNamespace

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
        got, want, lat = check(dec, have, what="biglm", exact_path=False)
        n_exact = n_valid = 0
        for i, L in enumerate(lat):
            for q, s in enumerate(SETTINGS):
                g, w = got[i][q], want[i][q]
                assert g["found"] and w["found"]
                if not w["ambiguous"]:
                    n_exact += 1
                    continue
                # a complete path: one transition-id per frame, and the lattice that keeps only the arcs with those transition-ids
                # holds a path of the same cost, bit for bit
                assert g["n_tids"] == int(L.st_frame.max())
                keep = (L.a_il == 0) | (L.a_il == g["tids"][np.minimum(L.st_frame[L.a_src], len(g["tids"]) - 1)])
                R = SimpleNamespace(n_states=L.n_states, start=0, st_final=L.st_final, st_frame=L.st_frame, st_gstate=L.st_gstate,
                                    a_src=L.a_src[keep], a_dst=L.a_dst[keep], a_il=L.a_il[keep], a_ol=L.a_ol[keep], a_graph=L.a_graph[keep],
                                    a_ac=L.a_ac[keep])
                r = rescale_many(R, [s])[0]
                assert r["found"] and bits64(r["scaled_cost"]) == bits64(g["scaled_cost"]), (i, s)
                n_valid += 1
        print("biglm: %d lattices; %d answers equal in full, %d through an ambiguous tie (cost bit for bit, a valid minimal path)"
              % (len(have), n_exact, n_valid))
        assert n_exact >= len(have)
    finally:
        dec.free()
        for lm in lms:
            lm.free()
        graph.free()


# ---- 7. rows too short, a lattice over max_cells ------------------------------------------------------------------------------------------
def test_capacities_of_one_channel(world, monkeypatch):
    W = world["W"]
    dec = decoder(world, cfg(6.0))
    try:
        decode_all(world, dec)
        ch = [1, 2, 0]
        settings = [(1.0, 1.0, -3.0), (1.0, 1.0, 0.0)]
        full, want, lat = check(dec, ch, settings, what="full")
        need = np.array([[g["n_hyp"] for g in row] for row in full])
        most = int(np.argmax(need.max(axis=1)))
        cap = int(need.max()) - 1
        short = need.max(axis=1) > cap
        assert cap >= 1 and short[most] and not short.all(), "the longest path is one word longer than the rows; another channel's fit"
        o = raw_call(W, dec, ch, settings, cap)
        assert o["rc"] == 0 and o["status"].tolist() == [E_CAPACITY if short[i] else 0 for i in range(3)]
        assert o["n_hyp"].tolist() == need.tolist(), "the room needed"
        for i in range(3):
            for q in range(2):
                g, k = full[i][q], min(int(need[i, q]), cap)
                assert o["found"][i, q] == 1 and o["n_arcs"][i, q] == g["n_arcs"] and bits64(o["scaled_cost"][i, q]) == bits64(g["scaled_cost"])
                assert bits32(o["tot"][i, q]) == bits32(g["tot"]) and bits32(o["lm"][i, q]) == bits32(g["lm"])
                assert np.array_equal(o["hyp_words"][i, q, :k], g["hyp_words"][:k]) and np.array_equal(o["begin"][i, q, :k], g["begin"][:k])
                assert np.array_equal(o["end"][i, q, :k], g["end"][:k]) and not o["hyp_words"][i, q, k:].any()
        # the transition-ids likewise: 150 of them against rows of 149
        o = raw_call(W, dec, ch, settings, 256, cap_tids=149, with_tids=True)
        assert o["rc"] == 0 and o["status"].tolist() == [0, E_CAPACITY, 0] and o["n_tids"].tolist() == [[97, 97], [150, 150], [40, 40]]
        for i in range(3):
            for q in range(2):
                k = min(len(full[i][q]["tids"]), 149)
                assert np.array_equal(o["tids"][i, q, :k], full[i][q]["tids"][:k]) and np.array_equal(o["hyp_words"][i, q, :need[i, q]], full[i][q]["hyp_words"])
        # with tids NULL the alignment is skipped: no count is held against cap_tids
        o = raw_call(W, dec, ch, settings, 256, cap_tids=0)
        assert o["rc"] == 0 and o["status"].tolist() == [0, 0, 0] and o["n_tids"].tolist() == [[97, 97], [150, 150], [40, 40]]
        # the binding repeats the call once with the room needed
        again = dec.rescaled_words(settings, ch, cap_words=1, cap_tids=1)
        for i in range(3):
            for q in range(2):
                same_answer(again[i][q], want[i][q], "the binding's repeat", tids=True)
                assert again[i][q]["status"] == 0
        # a lattice over max_cells: its answers zero, the others' stand; at max_cells = its states it fits
        states = [L.n_states for L in lat]
        big = int(np.argmax(states))
        assert sorted(states)[-1] > sorted(states)[-2]
        tight = dec.rescaled_words(settings, ch, max_cells=states[big] - 1)
        assert [row[0]["status"] for row in tight] == [E_CAPACITY if i == big else 0 for i in range(3)]
        for i in range(3):
            for q in range(2):
                if i == big:
                    assert not tight[i][q]["found"] and tight[i][q]["n_hyp"] == 0 and tight[i][q]["scaled_cost"] == 0.0
                else:
                    same_answer(tight[i][q], want[i][q], "beside the channel over max_cells")
        assert [row[0]["status"] for row in dec.rescaled_words(settings, ch, max_cells=states[big])] == [0, 0, 0]
        print("capacities: words needed %s, states %s" % (need.tolist(), states))
    finally:
        dec.free()


# ---- 8. the best path's cost bounds the lattice's log-sum ---------------------------------------------------------------------------------
def test_the_best_cost_is_at_least_minus_log_z(world):
    """at every setting scaled_cost >= -log_z of word_confidences at the same (gs, as) with wip = 0: the best path is one of the paths
    the sum runs over -- within the tolerance posterior_util derives for log_z on that lattice"""
    dec = decoder(world, cfg(6.0))
    try:
        decode_all(world, dec)
        ch = [0, 1, 2]
        lat = [from_gpu(dec.raw_lattice(c, True)) for c in ch]
        scales = sorted({(gs, as_) for gs, as_, _ in SETTINGS})
        got = dec.rescaled_words([(gs, as_, 0.0) for gs, as_ in scales], ch)
        closest = np.inf
        for q, (gs, as_) in enumerate(scales):
            conf = dec.word_confidences([[[]] for _ in ch], ch, graph_scale=gs, acoustic_scale=as_)
            for i in range(3):
                tol = posteriors(lat[i], gs, as_)["tol_log"]
                gap = got[i][q]["scaled_cost"] + conf[i][0]["log_z"]
                assert gap >= -tol, (scales[q], i, gap, tol)
                closest = min(closest, gap)
        print("scaled_cost + log_z: the smallest over %d scale pairs and 3 lattices is %.6g" % (len(scales), closest))
    finally:
        dec.free()


# ---- 9. the error surface -----------------------------------------------------------------------------------------------------------------
def test_error_surface(world):
    W = world["W"]
    plain = decoder(world, cfg(4.0), 2, lattice_links=0)
    try:
        plain.init()
        plain.advance(world["ptrs"][:2], [10, 10], N_TID // 2)
        with pytest.raises(W.WfstError) as e:
            plain.rescaled_words([(1.0, 1.0, 0.0)])
        assert e.value.code == E_STATE
    finally:
        plain.free()
    dec = decoder(world, cfg(4.0), 3)
    try:
        dec.init(channels=[0, 1])
        dec.advance(world["ptrs"][:2], [20, 20], N_TID // 2, channels=[0, 1])
        ok = dec.rescaled_words([(1.0, 1.0, 0.0)], [0], use_final_probs=False)
        assert ok[0][0]["status"] == 0 and ok[0][0]["found"]
        for ch, code in (([0, 0], E_ARG), ([0, 3], E_ARG), ([0, 2], E_STATE)):
            with pytest.raises(W.WfstError) as e:
                dec.rescaled_words([(1.0, 1.0, 0.0)], ch, use_final_probs=False)
            assert e.value.code == code, ch
        for bad in ([(-1.0, 1.0, 0.0)], [(1.0, float("nan"), 0.0)], [(1.0, 1.0, float("inf"))], [(1.0, 1.0, 0.0)] * 65, []):
            with pytest.raises(W.WfstError) as e:
                dec.rescaled_words(bad, [0], use_final_probs=False)
            assert e.value.code == E_ARG, bad
        for kw in (dict(cap_words=0), dict(cap_tids=-1), dict(max_cells=-1)):
            with pytest.raises(W.WfstError) as e:
                dec.rescaled_words([(1.0, 1.0, 0.0)], [0], use_final_probs=False, **kw)
            assert e.value.code == E_ARG, kw
        # through the C ABI: NULL outputs are fine
        one, st = np.array([0], np.int32), np.array([1.0, 1.0, 0.0])
        rc = W.lib().wfst_decoder_rescaled_words(dec.h, one.ctypes.data_as(C.POINTER(C.c_int32)), 1, 0, 1, st.ctypes.data_as(C.POINTER(C.c_double)), 16, 0,
                                                 C.c_int64(0), *([None] * 12))
        assert rc == 0
    finally:
        dec.free()
