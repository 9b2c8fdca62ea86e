"""-m gpu: pruned live lattices (wfst_decoder_set_live_lattice_prune): with mode 1 the live getters serve the SNAPSHOT lattice
S(channel, use_final_probs) -- FinalizeDecoding's pruning (my-decoder/online-decoder-base-inl.h:725-847) priced on a snapshot of a
live channel, the channel itself left bit for bit as it was.

The yardsticks: a TWIN channel fed the same frames and finalized (use_final_probs = 1: S is exactly its raw lattice), the order-free
oracle's finalized lattice of the prefix, and, where no twin exists (use_final_probs = 0: every token of the newest frame final at
cost 0), the numpy restatement that tests/test_live_prune_restatement.py proves against the oracle.  Graphs are small synthetic ones
with real-valued weights (no ties), max_active 1000000, min_active 0: the regime in which lattices are bit-exact against the oracle.

Every form of the walk is reached at the smallest shape that reaches it, and each such case asserts that it got there from the
per-frame state counts of the mode-0 live lattice (the raw frames the walk has to price)."""
import numpy as np
import pytest

import pyoracle
from golden_util import Golden, bits
from live_prune_util import (LENGTHS, LIM, PREFIXES, advance_in_two_chunks, advance_to, as_raw, config, frame_counts, restate,
                             same_lattice, small_graph, utterances)

pytestmark = pytest.mark.gpu
E_CAPACITY = -4


@pytest.fixture(scope="module")
def world(synth, oracle, tmp_path_factory):
    import gpu_util as G

    g, m, path = small_graph(synth, tmp_path_factory.mktemp("lp"))
    mats = utterances(synth, g, m)
    graph = G.wfstdec.Graph.load(path)
    graph.set_tid2pdf(m)
    h = oracle.load_graph(path)
    yield dict(G=G, W=G.wfstdec, g=g, m=m, path=path, graph=graph, mats=mats, dev=G.upload(mats), h=h)
    oracle.free_graph(h)
    graph.free()


def _decoder(world, cd, n=None, mode=0, **kw):
    lim = dict(LIM)
    lim.update(kw)
    dec = world["W"].BatchDecoder(world["graph"], world["G"].gpu_config(cd), n or len(world["mats"]), **lim)
    if mode:
        dec.set_live_lattice_prune(True)
    dec.init()
    return dec


def _twin_lattices(world, B, upto, lengths=LENGTHS, dev=None, frm=0):
    """twin B: InitDecoding, the same frames in the same two chunks, FinalizeDecoding; its raw lattices"""
    B.init()
    advance_in_two_chunks(B, dev or world["dev"], lengths, frm, upto)
    B.finalize()
    return [B.raw_lattice(c, True) for c in range(B.n)]


def _eq_dict(x, y):
    if x is None or y is None:
        return x is None and y is None
    return all(np.array_equal(np.asarray(x[k]).view(np.int32), np.asarray(y[k]).view(np.int32)) if k != "n_states" else x[k] == y[k] for k in x)


# ---- 1. twin equality, 2. the channel is untouched ---------------------------------------------------------------------------------
@pytest.mark.parametrize("lattice_beam", [0.5, 7.0])
def test_snapshot_equals_the_finalized_twin_and_the_oracle_and_leaves_the_channel_alone(lattice_beam, world, oracle):
    """A (mode 1) is asked at every T' in {1, 24, 25, 26, 53} (prune_interval 25: before, at and behind a running pass, and behind the
    second); B is fed the same frames and finalized; the order-free oracle finalizes the prefix.  C is fed like A and never asked.
    At T' = 26 A is switched to mode 0 and back: its live lattice there is what a decoder that never knew the mode (B, asked before
    its FinalizeDecoding) holds.  At the end A's final lattice, best path and lattice_stats are C's."""
    cd = config(lattice_beam)
    cfg = pyoracle.Config(**cd)
    mats, dev, m, h = world["mats"], world["dev"], world["m"], world["h"]
    A, B, C = _decoder(world, cd, mode=1), _decoder(world, cd), _decoder(world, cd)
    assert A.live_lattice_prune()[0] == 1 and A.live_lattice_prune()[1] >= 8 * A.n * LIM["arena_tokens"]
    assert B.live_lattice_prune() == (0, 0)
    n = 0
    try:
        oracle.set_order_free(True)
        frm = 0
        for upto in PREFIXES:
            for d in (A, C):
                advance_in_two_chunks(d, dev, LENGTHS, frm, upto)
            got = [A.raw_lattice(c, True) for c in range(A.n)]
            if upto == 26:   # mode 0 again: everything alive, as a decoder without the feature lists it
                B.init()
                advance_in_two_chunks(B, dev, LENGTHS, 0, upto)
                A.set_live_lattice_prune(False)
                for c in range(A.n):
                    L0, LB = as_raw(A.raw_lattice(c, True)), as_raw(B.raw_lattice(c, True))
                    same_lattice(L0, LB, "mode 0 again, channel %d" % c)
                    # the small form of the walk: every frame it prices, raw ones included, holds at most 4096 tokens
                    assert L0.n_states > as_raw(got[c]).n_states and 1 < frame_counts(L0).max() <= 4096, frame_counts(L0).max()
                A.set_live_lattice_prune(True)
                B.finalize()
                twin = [B.raw_lattice(c, True) for c in range(B.n)]
            else:
                twin = _twin_lattices(world, B, upto)
            for c in range(A.n):
                k = min(upto, LENGTHS[c])
                what = "lattice_beam %g frames %d channel %d" % (lattice_beam, k, c)
                O = pyoracle.oracle_raw_lattice(oracle, h, cfg, mats[c][:k], m, finalize=True)
                assert got[c] is not None and twin[c] is not None and O.ok, what
                L = as_raw(got[c])
                same_lattice(L, as_raw(twin[c]), what + " (twin)")
                same_lattice(L, O, what + " (oracle)")
                assert L.st_frame[0] == 0 and L.st_frame.max() == k and np.all(L.a_dst > L.a_src) and np.all(np.diff(L.st_frame) >= 0), what
                n += 1
            frm = upto
        # ---- the channel is untouched: on to the end
        for d in (A, C):
            advance_in_two_chunks(d, dev, LENGTHS, frm, max(LENGTHS))
            d.finalize()
        bA, bC = A.best_paths(), C.best_paths()
        for c in range(A.n):
            what = "after the queries, channel %d" % c
            same_lattice(as_raw(A.raw_lattice(c, True)), as_raw(C.raw_lattice(c, True)), what)
            for k in ("tids", "words", "ilabel", "olabel"):
                assert np.array_equal(bA[c][k], bC[c][k]), what + " " + k
            for k in ("graph", "ac"):
                assert np.array_equal(bits(bA[c][k]), bits(bC[c][k])), what + " " + k
            assert A.lattice_stats(c) == C.lattice_stats(c), (what, A.lattice_stats(c), C.lattice_stats(c))
            O = pyoracle.oracle_raw_lattice(oracle, h, cfg, mats[c], m, finalize=True)
            same_lattice(as_raw(A.raw_lattice(c, True)), O, what + " (oracle)")
    finally:
        oracle.set_order_free(False)
        for d in (A, B, C):
            d.free()
    assert n == len(PREFIXES) * len(LENGTHS)


def test_twin_equality_on_a_biglm_lattice_decoder(tmp_path):
    """the same on the biglm lattice decoder (the golden graph and LM pairs of tests/test_gpu_biglm.py; utterances of 40, 33, ... frames,
    prune_interval 25 and 7): ComputeFinalCosts with the LMs' final costs, the graph cost of a word arc = arc weight + LM step"""
    import json
    import os

    import gpu_util as G
    from golden_util import GOLDEN_DIR

    W = G.wfstdec
    z = np.load(os.path.join(GOLDEN_DIR, "biglm_hclg600.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    with open(tmp_path / "g.bin", "wb") as f:
        f.write(bytes(z["graph"]))
    graph = W.Graph.load(str(tmp_path / "g.bin"))
    graph.set_tid2pdf(z["tid2pdf"])
    pname = meta["pairs"][0]
    lms = []
    for tag, scale in (("old", -1.0), ("new", 1.0)):
        p = str(tmp_path / ("lm_%s.bin" % tag))
        with open(p, "wb") as f:
            f.write(bytes(z["lm_%s_%s" % (pname, tag)]))
        lms.append(W.Lm.load(p, scale))
    mats = [z["ll_%d" % i][: 40 - 7 * i] for i in range(int(z["n_utt"]))]
    lengths = [int(x.shape[0]) for x in mats]
    dev = G.upload(mats)
    stride = int(mats[0].shape[1])

    def adv(d, upto):
        d.advance([t.data_ptr() for t in dev], [min(upto, t) for t in lengths], stride)

    n = n_pruned = 0
    for interval in (25, 7):
        cd = dict(beam=13.0, max_active=1000000, min_active=0, lattice_beam=25.0 if interval == 25 else 7.0, prune_interval=interval)
        mk = lambda: W.BatchDecoder(graph, G.gpu_config(cd), len(mats), old_lm=lms[0], new_lm=lms[1], max_frames=64, max_tokens_per_frame=32768,
                                    arena_tokens=1 << 20, lattice_links=1 << 21)
        A, B = mk(), mk()
        A.set_live_lattice_prune(True)
        A.init()
        for upto in (1, 24, 25, 26, 40):
            adv(A, upto)
            B.init()
            adv(B, upto)
            live = [B.raw_lattice(c, True) for c in range(B.n)]
            B.finalize()
            for c in range(A.n):
                what = "prune_interval %d frames %d channel %d" % (interval, min(upto, lengths[c]), c)
                got, twin = A.raw_lattice(c, True), B.raw_lattice(c, True)
                assert (got is None) == (twin is None), what   # (the reference's final pruning may leave a biglm utterance no lattice)
                if got is None:
                    continue
                same_lattice(as_raw(got), as_raw(twin), what)
                n += 1
                n_pruned += live[c] is not None and live[c]["n_states"] > got["n_states"]
        A.free()
        B.free()
    for L in lms:
        L.free()
    graph.free()
    assert n >= 20 and n_pruned >= 1, (n, n_pruned)


# ---- 3. use_final_probs = 0 --------------------------------------------------------------------------------------------------------
def test_without_final_probs_on_a_frontier_without_final_tokens_both_modes_of_the_seed_agree(tmp_path):
    """3a: the graph of tests/golden/no_final.npz has no reachable final state: ComputeFinalCosts makes every frontier token final at
    cost 0, which is what use_final_probs = 0 asks for -- the two snapshot lattices are identical"""
    import gpu_util as G

    gn = Golden("no_final")
    graph = G.wfstdec.Graph.load(gn.write_graph(str(tmp_path / "nf.bin")))
    cd = dict(gn.meta["cfgs"][0], max_active=1000000, min_active=0)
    x = gn.utts[1]
    dev = G.upload([x])
    A = G.wfstdec.BatchDecoder(graph, G.gpu_config(cd), 1, **LIM)
    A.set_live_lattice_prune(True)
    A.init()
    for upto in range(1, x.shape[0] + 1):
        A.advance([dev[0].data_ptr()], [upto], int(x.shape[1]))
        L1, L0 = as_raw(A.raw_lattice(0, True)), as_raw(A.raw_lattice(0, False))
        newest = L1.st_frame == upto
        assert newest.any() and np.all(L1.st_final[newest] == 1) and L1.st_final.sum() == newest.sum()   # no token of the frontier is final in the graph
        same_lattice(L0, L1, "frames %d" % upto)
    A.free()
    graph.free()


@pytest.mark.parametrize("lattice_beam", [0.5, 7.0])
def test_without_final_probs_equals_the_restatement_of_the_live_lattice(lattice_beam, world):
    """3b: on the ordinary graph S(c, 0) is the restatement, seeded with every frontier token final at cost 0, of the mode-0 live
    lattice of the same channel at the same frame; S(c, 1) the restatement with ComputeFinalCosts' seed"""
    cd = config(lattice_beam)
    A = _decoder(world, cd)
    n = n_differ = 0
    frm = 0
    for upto in PREFIXES:
        advance_in_two_chunks(A, world["dev"], LENGTHS, frm, upto)
        frm = upto
        A.set_live_lattice_prune(False)
        live = [[as_raw(A.raw_lattice(c, ufp)) for c in range(A.n)] for ufp in (False, True)]
        A.set_live_lattice_prune(True)
        for c in range(A.n):
            what = "lattice_beam %g frames %d channel %d" % (lattice_beam, min(upto, LENGTHS[c]), c)
            S0, S1 = as_raw(A.raw_lattice(c, False)), as_raw(A.raw_lattice(c, True))
            same_lattice(S0, restate(live[1][c], lattice_beam, all_final=True), what + " use_final_probs 0")
            same_lattice(S0, restate(live[0][c], lattice_beam, all_final=True), what + " use_final_probs 0 (from the live lattice without final-probs)")
            same_lattice(S1, restate(live[1][c], lattice_beam), what + " use_final_probs 1")
            newest = S0.st_frame == S0.st_frame.max()
            assert np.all(S0.st_final[newest] == 1) and S0.st_final.sum() == newest.sum(), what
            n += 1
            n_differ += S0.n_states != S1.n_states or not np.array_equal(S0.st_final, S1.st_final)
    A.free()
    assert n == len(PREFIXES) * len(LENGTHS) and n_differ >= 1   # (somewhere the frontier holds a graph-final token: the two seeds differ)


# ---- 4. every form of the walk -----------------------------------------------------------------------------------------------------
def _twin_case(G, graph, cd, mats, prefixes, lim, options=None, want_counts=None, oracle=None, h=None, m=None, strict=True):
    """A (mode 1) against twin B at every prefix; want_counts(counts of the mode-0 live lattice's frames, prefix): the case's own
    assertion that the walk met the frames it is about.  Returns the number of lattices compared."""
    W = G.wfstdec
    mk = lambda: W.BatchDecoder(graph, G.gpu_config(cd), len(mats), options=options, **lim)
    lengths = [int(x.shape[0]) for x in mats]
    dev = G.upload(mats)
    stride = int(mats[0].shape[1])
    A, B = mk(), mk()
    A.set_live_lattice_prune(True)
    A.init()
    n = 0
    try:
        for upto in prefixes:
            A.advance([t.data_ptr() for t in dev], [min(upto, t) for t in lengths], stride)
            B.init()
            B.advance([t.data_ptr() for t in dev], [min(upto, t) for t in lengths], stride)
            live = [as_raw(B.raw_lattice(c, True)) for c in range(B.n)]   # mode 0: what the walk has to price
            B.finalize()
            if want_counts is not None:
                want_counts([frame_counts(L) for L in live], upto)
            for c in range(A.n):
                k = min(upto, lengths[c])
                what = "frames %d channel %d" % (k, c)
                S = as_raw(A.raw_lattice(c, True))
                same_lattice(S, as_raw(B.raw_lattice(c, True)), what + " (twin)")
                assert S.n_states <= live[c].n_states and (S.n_states < live[c].n_states or not strict), what
                if oracle is not None:
                    same_lattice(S, pyoracle.oracle_raw_lattice(oracle, h, pyoracle.Config(**cd), mats[c][:k], m, finalize=True), what + " (oracle)")
                n += 1
    finally:
        A.free()
        B.free()
    return n


@pytest.mark.parametrize("pair_form", [False, True])
def test_walk_over_frames_between_4096_and_32768_tokens(pair_form, synth, tmp_path):
    """raw frames of 4096 .. 32768 tokens (a 20 000-state graph at beam 40, prune_interval 10, as
    test_closure_launch_workgroups_per_channel_give_one_lattice builds): the streamed form and, above 16384, the extras-only form
    of the frame in LDS; pair_form (wfst_options.debug 0x1000: links carry their cost, DecoderDev::link_delta 0) the WIDE form, whose
    costs come from the tokens"""
    import gpu_util as G

    g = synth.make_hclg_like(20000, seed=11, n_tid=2000, n_words=3000)
    m = synth.default_tid2pdf(2000)
    path = str(tmp_path / "g.bin")
    g.write(path)
    graph = G.wfstdec.Graph.load(path)
    graph.set_tid2pdf(m)
    cd = dict(beam=40.0, max_active=1000000, min_active=0, lattice_beam=6.0, prune_interval=10)
    mats = [synth.make_loglikes_multi(g, T, 1000, m, seed=70 + i)[0] for i, T in enumerate((34, 21))]
    lim = dict(max_frames=64, max_tokens_per_frame=65536, arena_tokens=1 << 22, lattice_links=1 << 23)
    seen = []

    def counts(per_channel, upto):
        seen.extend(int(x) for fc in per_channel for x in fc)
        assert max(int(fc.max()) for fc in per_channel) <= 32768

    n = _twin_case(G, graph, cd, mats, (27, 34), lim, options=G.wfstdec.Options(debug=0x1000) if pair_form else None, want_counts=counts)
    graph.free()
    assert n == 4
    assert any(4096 < x <= 16384 for x in seen) and any(16384 < x <= 32768 for x in seen), sorted(seen)[-8:]


def test_walk_over_frames_beyond_32768_tokens(synth, oracle, tmp_path):
    """raw frames of more than 32768 tokens -- beyond the LDS buffers: the walk's HBM path, priced with atomics through L2 -- on a
    60 000-state graph at beam 40, 18 frames (the oracle's token counts say so on the CPU before the device is asked)"""
    import gpu_util as G

    g = synth.make_hclg_like(60000, seed=11, n_tid=2000, n_words=3000)
    m = synth.default_tid2pdf(2000)
    path = str(tmp_path / "g.bin")
    g.write(path)
    cd = dict(beam=40.0, max_active=1000000, min_active=0, lattice_beam=6.0, prune_interval=10)
    mats = [synth.make_loglikes_multi(g, 18, 1000, m, seed=71)[0]]
    h = oracle.load_graph(path)
    try:
        oracle.set_order_free(True)
        O = pyoracle.oracle_raw_lattice(oracle, h, pyoracle.Config(**cd), mats[0], m, finalize=False, max_states=1 << 23, max_arcs=1 << 25)
        assert 32768 < frame_counts(O).max() <= 65536, frame_counts(O)
        graph = G.wfstdec.Graph.load(path)
        graph.set_tid2pdf(m)
        lim = dict(max_frames=32, max_tokens_per_frame=65536, arena_tokens=1 << 22, lattice_links=1 << 23)
        seen = []
        n = _twin_case(G, graph, cd, mats, (15, 18), lim, want_counts=lambda per, upto: seen.append(int(per[0].max())), oracle=oracle, h=h, m=m)
        graph.free()
    finally:
        oracle.set_order_free(False)
        oracle.free_graph(h)
    assert n == 2 and max(seen) > 32768, seen


@pytest.mark.parametrize("lattice_beam", [0.5, 7.0])
def test_walk_in_the_pair_form(lattice_beam, world, oracle):
    """the pair form of the frame in LDS: a decoder whose links carry their cost (wfst_options.debug 0x1000: the iterated closure pass,
    DecoderDev::link_delta 0), the small graph"""
    cd = config(lattice_beam)
    try:
        oracle.set_order_free(True)
        n = _twin_case(world["G"], world["graph"], cd, world["mats"], PREFIXES, LIM, options=world["W"].Options(debug=0x1000),
                       oracle=oracle, h=world["h"], m=world["m"], strict=False)
    finally:
        oracle.set_order_free(False)
    assert n == len(PREFIXES) * len(LENGTHS)


@pytest.mark.parametrize("cfg_index", [0, 1])
def test_walk_to_the_epsilon_fixpoint(cfg_index, oracle, tmp_path):
    """epsilon links inside a frame to their fixpoint: the graph of tests/golden/lattice_eps_chains.npz (chains of epsilon arcs)"""
    import gpu_util as G

    gl = Golden("lattice_eps_chains")
    path = gl.write_graph(str(tmp_path / "g.bin"))
    graph = G.wfstdec.Graph.load(path)
    cd = dict(dict(prune_interval=25), **gl.meta["cfgs"][cfg_index])
    cd.update(max_active=1000000, min_active=0)
    h = oracle.load_graph(path)
    try:
        oracle.set_order_free(True)
        n = _twin_case(G, graph, cd, [gl.utts[3], gl.utts[2]], (1, 3, 4, 17, 30), LIM, oracle=oracle, h=h, m=None, strict=False)
    finally:
        oracle.set_order_free(False)
        oracle.free_graph(h)
    graph.free()
    assert n == 10


# ---- 5. what the feature is for ----------------------------------------------------------------------------------------------------
def _same_nbest_words(got, want, what):
    assert got[0] == want[0] == 0, (what, got[0], want[0])
    assert len(got[1]) == len(want[1]) >= 1, what
    for k, (p, q) in enumerate(zip(got[1], want[1])):
        assert np.array_equal(p["words"], q["words"]) and p["n_words"] == q["n_words"], "%s path %d words" % (what, k)
        for name in ("tot", "lm", "path_tot"):
            assert np.float32(p[name]).tobytes() == np.float32(q[name]).tobytes(), "%s path %d %s" % (what, k, name)


def _same_paths(x, y):
    return len(x) == len(y) and all(np.array_equal(np.asarray(p[k]).view(np.int32), np.asarray(q[k]).view(np.int32)) for p, q in zip(x, y)
                                    for k in ("olabel", "graph", "acoustic")) and all(np.float32(p["tot"]).tobytes() == np.float32(q["tot"]).tobytes() for p, q in zip(x, y))


def test_live_nbest_answers_where_the_unpruned_lattice_is_beyond_the_determinizers_bounds(world):
    """At frame 49 a live raw lattice holds tens of thousands of states, the finalized twin's a thousand or two.  With the
    determinizer's raw-lattice bounds halfway between, mode 0 refuses every channel (WFST_E_CAPACITY in status) and mode 1 answers,
    bit for bit what the finalized twin answers: nbest_words, nbest_paths, determinized_lattice.  A mixed list in mode 1 (live,
    finalized, one channel with no frame decoded): the finalized channels' entries are mode 0's."""
    W = world["W"]
    cd = config(7.0)
    dev, T = world["dev"], 49
    n_ch = 3   # (the fourth utterance ends at frame 26: its live lattice is no larger than the others' finalized ones)
    A, B = _decoder(world, cd), _decoder(world, cd)
    for d in (A, B):
        advance_in_two_chunks(d, dev, LENGTHS, 0, T)
    B.finalize()
    live = [A.raw_lattice(c, True) for c in range(n_ch)]
    fin = [B.raw_lattice(c, True) for c in range(n_ch)]
    A.free()
    B.free()
    s_lo, s_hi = max(x["n_states"] for x in fin), min(x["n_states"] for x in live)
    a_lo, a_hi = max(len(x["a_src"]) for x in fin), min(len(x["a_src"]) for x in live)
    print("frame %d: finalized at most %d states / %d arcs, live at least %d / %d" % (T, s_lo, a_lo, s_hi, a_hi))
    assert 2 * s_lo < s_hi and 2 * a_lo < a_hi
    caps = dict(det_raw_states=(s_lo + s_hi) // 2, det_raw_arcs=(a_lo + a_hi) // 2)
    A = _decoder(world, cd, n=n_ch + 2, **caps)   # + a channel finalized early, + one with no frame decoded
    B = _decoder(world, cd, n=n_ch + 2, **caps)
    ptrs = [t.data_ptr() for t in dev][:n_ch]
    for d in (A, B):
        for r in (T // 2, T):
            d.advance(ptrs + [ptrs[1]], [min(r, t) for t in LENGTHS[:n_ch]] + [min(r, 20)], 1000, channels=list(range(n_ch + 1)))
        d.finalize(channels=[n_ch])
    B.finalize(channels=list(range(n_ch)))
    chans = list(range(n_ch))
    try:
        want = B.nbest_words(5, channels=chans, use_final_probs=True)
        got0 = A.nbest_words(5, channels=chans, use_final_probs=True)
        for c in chans:
            assert got0[c][0] == E_CAPACITY and got0[c][1] == [], (c, got0[c][0])
            with pytest.raises(W.WfstError) as e:
                A.nbest_paths(c, 5, use_final_probs=True)
            assert e.value.code == E_CAPACITY
            with pytest.raises(W.WfstError) as e:
                A.determinized_lattice(c, True)
            assert e.value.code == E_CAPACITY
        mixed = [n_ch + 1, 2, n_ch, 0]   # no frame decoded, live, finalized, live
        mixed0 = A.nbest_words(5, channels=mixed, use_final_probs=True)
        A.set_live_lattice_prune(True)
        got1 = A.nbest_words(5, channels=chans, use_final_probs=True)
        for c in chans:
            what = "channel %d" % c
            _same_nbest_words(got1[c], want[c], what)
            assert _same_paths(A.nbest_paths(c, 5, use_final_probs=True), B.nbest_paths(c, 5, use_final_probs=True)), what
            assert _eq_dict(A.determinized_lattice(c, True), B.determinized_lattice(c, True)), what
        mixed1 = A.nbest_words(5, channels=mixed, use_final_probs=True)
        assert mixed1[0] == mixed0[0] == (0, [])                  # no frame decoded: no lattice, in either mode
        _same_nbest_words(mixed1[2], mixed0[2], "the finalized channel of the mixed list")
        _same_nbest_words(mixed1[2], B.nbest_words(5, channels=[n_ch], use_final_probs=True)[0], "the finalized channel against B's")
        assert mixed0[1][0] == mixed0[3][0] == E_CAPACITY
        _same_nbest_words(mixed1[1], want[2], "live channel 2 of the mixed list")
        _same_nbest_words(mixed1[3], want[0], "live channel 0 of the mixed list")
        # ... and the short list over the raw lattice (wfst_decoder_get_nbest) works from S too
        nbA, nbB = A.nbest(3, channels=chans), B.nbest(3, channels=chans)
        for c in chans:
            assert len(nbA[c]) == len(nbB[c]) >= 1
            for p, q in zip(nbA[c], nbB[c]):
                assert np.array_equal(p["words"], q["words"]) and np.float32(p["tot_score"]).tobytes() == np.float32(q["tot_score"]).tobytes(), c
    finally:
        A.free()
        B.free()


def test_where_both_modes_answer_the_cheapest_path_agrees_and_a_mode_change_drops_what_is_kept(world):
    """Early in the utterance (8 frames) the unpruned lattice is within the default bounds and both modes answer: the cheapest
    path's words are the same (the pruning never removes the best path).  6: determinized_lattice live in mode 0, the mode switched
    to 1, the same call without advancing -- the answer is the snapshot's (the finalized twin's) lattice, not the kept one; and back."""
    cd = config(7.0)
    dev, T = world["dev"], 8
    A, B = _decoder(world, cd), _decoder(world, cd)
    try:
        for d in (A, B):
            advance_to(d, dev, LENGTHS, T)
        B.finalize()
        w0 = A.nbest_words(5, use_final_probs=True)
        det0 = [A.determinized_lattice(c, True) for c in range(A.n)]
        nbp0 = [A.nbest_paths(c, 3, use_final_probs=True) for c in range(A.n)]
        A.set_live_lattice_prune(True)
        det1 = [A.determinized_lattice(c, True) for c in range(A.n)]
        nbp1 = [A.nbest_paths(c, 3, use_final_probs=True) for c in range(A.n)]
        w1 = A.nbest_words(5, use_final_probs=True)
        both = 0
        for c in range(A.n):
            if w0[c][0] == 0 and w1[c][0] == 0:
                assert np.array_equal(w0[c][1][0]["words"], w1[c][1][0]["words"]), c
                assert np.float32(w0[c][1][0]["path_tot"]).tobytes() == np.float32(w1[c][1][0]["path_tot"]).tobytes(), c
                both += 1
            assert _eq_dict(det1[c], B.determinized_lattice(c, True)), "channel %d: the snapshot's lattice after the mode change" % c
            assert _same_paths(nbp1[c], B.nbest_paths(c, 3, use_final_probs=True)), c
        assert both == A.n
        assert any(not _eq_dict(det0[c], det1[c]) for c in range(A.n))   # (the case can tell the two apart)
        assert all(len(nbp0[c]) >= 1 for c in range(A.n))
        A.set_live_lattice_prune(False)
        for c in range(A.n):
            assert _eq_dict(A.determinized_lattice(c, True), det0[c]), "channel %d: mode 0 again" % c
    finally:
        A.free()
        B.free()


def test_errors(world):
    """WFST_E_STATE on a decoder without lattice_links, WFST_E_ARG on a mode outside {0, 1}"""
    W, G = world["W"], world["G"]
    cd = config(7.0)
    best = W.BatchDecoder(world["graph"], G.gpu_config(cd), 1, max_frames=32, max_tokens_per_frame=8192, arena_tokens=1 << 16)
    assert W.lib().wfst_decoder_set_live_lattice_prune(best.h, 1) == -5
    assert W.lib().wfst_decoder_get_live_lattice_prune(best.h, None, None) == -5
    best.free()
    lat = W.BatchDecoder(world["graph"], G.gpu_config(cd), 1, max_frames=32, max_tokens_per_frame=8192, arena_tokens=1 << 16, lattice_links=1 << 17)
    assert W.lib().wfst_decoder_set_live_lattice_prune(lat.h, 2) == -1 and W.lib().wfst_decoder_set_live_lattice_prune(lat.h, -1) == -1
    assert lat.live_lattice_prune() == (0, 0)
    lat.set_live_lattice_prune(True)
    mode, scratch = lat.live_lattice_prune()
    assert mode == 1 and scratch >= 8 * (1 << 16)   # 8 bytes per arena entry of every channel
    lat.set_live_lattice_prune(False)
    assert lat.live_lattice_prune() == (0, scratch)   # the scratch stays until the decoder goes
    lat.free()
