"""-m gpu: how an insert item of the fused best-path decoder leaves its frame -- the count-out on {new_count, items_left}, the
workgroup that learns it was the channel's last item closing the frame (frame_boundary_fused) -- and how its token stores are
issued (insert_body, asr-decoder_amd/csrc/wfst_kernels.hip).  Written for an item that counts itself out right behind its token
allocation, so that the last workgroup may close the frame while siblings still store; that order was measured and not kept
(NOTES.md, round 9), the cases stay as the yardstick for any change to the order of these steps.

What could go wrong, and the case that would show it:
  * the boundary sees a token count that misses an item           -> many items per channel (per-frame token counts, 1 and 3 channels)
  * a risky frame is closed before its tokens have landed          -> risky and calm frames in one utterance
  * an item of several allocations counts out behind the first    -> sub-pass items beside one-sweep items
  * a failed allocation's frame error does not reach the boundary  -> an arena too small; a hard per-frame limit (lattice decoder)
  * boundary 1 / 2, with and without the next frame's preparation  -> every case runs as one call, in chunks of 7, frame by frame
  * equal costs                                                    -> the dense 50-state graph with quantised costs, tie-mode oracle

Bar: bit for bit against the CPU oracle in its order-free mode (each frame's FINAL cutoff applied to every arc: what the device
computes) -- words, transition-ids, per-hop labels and float costs, total and LM score -- and the per-frame token counts of the
frame-by-frame run against the oracle's trace; the three advance granularities agree on the decoder's token and peak
counters as well (the record counter is no such figure: the expansion writes a candidate while the frame's cutoff still falls, so
it differs from run to run; the tests use it per frame, as a bound)."""
import numpy as np
import pytest

import pyoracle
import signed_util as S
import tie_util
from test_gpu_insert_single_probe import dense_graph

pytestmark = pytest.mark.gpu

FRAMES = 40
LIMITS = dict(max_frames=64, max_tokens_per_frame=32768, arena_tokens=1 << 20)
BEAM_ONLY = dict(beam=11.0, max_active=1000000, min_active=0, lattice_beam=6.0)
SEEDS = [12, 24, 31]   # make_loglikes seeds over the 3000-state graph; seed 12 grows to 2000 tokens a frame


class World:
    def __init__(self, synth, oracle, d):
        import gpu_util as G

        self.G, self.W, self.oracle = G, G.wfstdec, oracle
        self.g = synth.make_hclg_like(S.GRAPH["n_states"], seed=S.GRAPH["seed"], n_tid=S.GRAPH["n_tid"], n_words=S.GRAPH["n_words"])
        self.m = synth.default_tid2pdf(S.GRAPH["n_tid"])
        self.mats = [synth.make_loglikes(self.g, FRAMES, S.N_PDF, self.m, seed=s)[0] for s in SEEDS]
        self.path = str(d / "g3000.bin")
        self.g.write(self.path)
        self.graph = self.W.Graph.load(self.path)
        self.graph.set_tid2pdf(self.m)
        self.h = oracle.load_graph(self.path)
        # the dense 50-state graph with costs quantised to 0.5: exact ties abound
        self.gd = tie_util.quantised_graph(synth, dense_graph(synth))
        self.dpath = str(d / "dense50q.bin")
        self.gd.write(self.dpath)
        self.dgraph = self.W.Graph.load(self.dpath)
        self.hd = oracle.load_graph(self.dpath)
        rng = np.random.default_rng(5)
        self.dmats = [tie_util.quantise(rng.normal(-1.5, 1.0, size=(FRAMES, 41))) for _ in range(3)]
        self.cache = {}

    def want(self, key, h, cd, x, m, tie=False):
        """the oracle's trace (order-free; tie mode on request) of utterance x, computed once"""
        k = (key, tuple(sorted(cd.items())), tie)
        if k not in self.cache:
            try:
                self.oracle.set_order_free(True)
                self.oracle.set_tie_rule(tie)
                self.cache[k] = self.oracle.decode(h, pyoracle.Config(**cd), x, m, trace=True)
            finally:
                self.oracle.set_order_free(False)
                self.oracle.set_tie_rule(False)
        return self.cache[k]

    def close(self):
        self.graph.free()
        self.dgraph.free()
        self.oracle.free_graph(self.h)
        self.oracle.free_graph(self.hd)


@pytest.fixture(scope="module")
def world(synth, oracle, tmp_path_factory):
    w = World(synth, oracle, tmp_path_factory.mktemp("early_countout"))
    yield w
    w.close()


def run_all_granularities(G, dec, graph, cd, mats, want, what, ties_allowed=False):
    """one call, chunks of 7, frame by frame: each against the oracle; the frame-by-frame run's frontier sizes against the oracle's
    trace; the counters of the three runs against each other.  Returns (per-frame records, per-frame tokens) of the last run, per
    channel."""
    T = [int(x.shape[0]) for x in mats]
    counters = []
    for chunk in (0, 7):
        res = G.decode_batch(graph, cd, mats, chunk=chunk, dec=dec)
        for i, (r, o) in enumerate(zip(res, want)):
            assert ties_allowed or o.extra["ties"] == 0, "%s utt %d: an exact tie on the best path" % (what, i)
            G.assert_same_as_oracle(r, o, "%s utt %d chunk %d" % (what, i, chunk))
        counters.append([(r.stats["tokens"], r.stats["peak_tokens"], r.stats["frames"]) for r in res])
    # frame by frame, the counters read after every call
    dev = G.upload(mats)
    ptrs = [t.data_ptr() for t in dev]
    dec.init()
    rec = [np.zeros(t + 1, np.int64) for t in T]
    ntok = [np.zeros(t + 1, np.int64) for t in T]
    for c in range(len(mats)):
        ntok[c][0] = len(dec.frontier(c)[0])
    for f in range(1, max(T) + 1):
        dec.advance(ptrs, [min(f, t) for t in T], int(mats[0].shape[1]))
        for c in range(len(mats)):
            if f <= T[c]:
                rec[c][f] = dec.stats(c)["records"]
                ntok[c][f] = len(dec.frontier(c)[0])
    dec.finalize()
    res = [G.GpuResult(d) for d in dec.best_paths()]
    for c, (r, o) in enumerate(zip(res, want)):
        G.assert_same_as_oracle(r, o, "%s utt %d frame by frame" % (what, c))
        assert np.array_equal(ntok[c], o.frame_ntoks), "%s utt %d tokens per frame" % (what, c)
        s = dec.stats(c)
        assert (s["tokens"], s["peak_tokens"], s["frames"]) == counters[0][c] == counters[1][c], "%s utt %d counters" % (what, c)
        assert s["peak_tokens"] == int(o.frame_ntoks[1:].max()) and s["frames"] == T[c], "%s utt %d peak / frames" % (what, c)
        assert dec.degraded_frames(c) >= 0
    return [np.diff(r) for r in rec], [n[1:] for n in ntok]


@pytest.mark.parametrize("n_chan", [1, 3])
def test_many_items_per_channel(world, n_chan):
    """64 partitions, joint_max 16: a group of partitions is one item only while it holds 16 records or fewer, so a frame of more
    than 8 x 16 records is at least 8 items, each with a workgroup of its own -- whichever counts out last closes the frame and
    must see every item's tokens in the count"""
    G = world.G
    mats = world.mats[:n_chan]
    want = [world.want(("g", i), world.h, BEAM_ONLY, x, world.m) for i, x in enumerate(mats)]
    dec = world.W.BatchDecoder(world.graph, G.gpu_config(BEAM_ONLY), n_chan, options=world.W.Options(log2_partitions=6, joint_max=16), **LIMITS)
    try:
        pf = dec.path_flags()
        assert pf["two_launch"] == 1 and pf["best_exp"] == 1, pf
        rec, _ = run_all_granularities(G, dec, world.graph, BEAM_ONLY, mats, want, "many items, %d channels" % n_chan)
    finally:
        dec.free()
    for c in range(n_chan):
        assert (rec[c] > 8 * 16).sum() >= 10, "channel %d: %s records per frame" % (c, rec[c].tolist())


def test_risky_and_calm_frames_in_one_utterance(world):
    """max_active 300 over a per-frame limit of 256 (the limit acts as the max_active: soft_limit) and min_active 20: the limit
    binds on the later frames (risky: the boundary selects over the frame's tokens, written through and counted out of stores_left,
    the drain) and the frame after a cut is risky through min_active; the frames before are calm (plain stores, no drain).
    Both in one hipGraph replay when the utterance is one call.

    Risky frames occurred: degraded_frames() counts the frames on which the limit bound.  Calm frames occurred: by plan_channel's
    test a frame is calm when it has no more candidate records than the limit and the frame before left the plain beam -- which a
    frame does that holds more than min_active and no more than the limit's tokens, behind another such frame; the record and
    token counts are read from the decoder frame by frame."""
    G = world.G
    cd = dict(beam=11.0, max_active=300, min_active=20, lattice_beam=6.0)
    ocd = dict(cd, max_active=256)
    limit = 256
    mats = world.mats[:1]
    want = [world.want(("g", 0), world.h, ocd, mats[0], world.m)]
    dec = world.W.BatchDecoder(world.graph, G.gpu_config(cd), 1, max_frames=64, max_tokens_per_frame=limit, arena_tokens=1 << 20)
    try:
        pf = dec.path_flags()
        assert pf["two_launch"] == 1 and pf["soft_limit"] == 1 and pf["best_exp"] == 1, pf
        rec, ntok = run_all_granularities(G, dec, world.graph, cd, mats, want, "risky and calm")
        degraded = dec.degraded_frames(0)
    finally:
        dec.free()
    rec, ntok = rec[0], ntok[0]   # (index f - 1: frame f)
    ok = (ntok > cd["min_active"]) & (ntok <= limit)
    calm = [f for f in range(3, FRAMES) if rec[f] <= limit and ok[f - 1] and ok[f - 2] and rec[f - 1] <= limit]
    assert degraded >= 5, "the limit bound on %d frames only" % degraded
    assert len(calm) >= 3, "calm frames %s (records %s, tokens %s)" % (calm, rec.tolist(), ntok.tolist())
    assert (ntok > limit).sum() >= 5


def test_subpass_items_beside_one_sweep_items(world):
    """256-slot tables (3/4 = 192 records) under the default joint_max of 1536, 8 partitions: a partition of more than 192 records
    is an item of several sub-passes -- one allocation per sub-pass, the count-out behind the last -- and the
    lighter partitions of the same frame are one-sweep items, one allocation each.  Frames of more than 8 x 192 records hold a
    sub-pass item for certain, frames of 192 records or fewer none; the frames between mix the two."""
    G = world.G
    mats = world.mats[:2]
    want = [world.want(("g", i), world.h, BEAM_ONLY, x, world.m) for i, x in enumerate(mats)]
    dec = world.W.BatchDecoder(world.graph, G.gpu_config(BEAM_ONLY), 2, options=world.W.Options(log2_lds_slots=8, log2_partitions=3, joint_max=1536), **LIMITS)
    try:
        rec, _ = run_all_granularities(G, dec, world.graph, BEAM_ONLY, mats, want, "sub-passes")
    finally:
        dec.free()
    r = rec[0]
    assert (r > 8 * 192).sum() >= 3 and (r <= 192).sum() >= 3 and ((r > 2 * 192) & (r < 6 * 192)).sum() >= 3, r.tolist()


def test_an_arena_too_small_for_the_utterance(world):
    """two channels, 64 partitions and joint_max 16 (many items per frame); an arena of 1024 tokens under a per-frame limit of 256
    still gives a two-launch decoder (the collection's reserve holds two frames at the limit), but the limit is soft: channel 0's
    raw frames reach 650 tokens, and two of them with the history they point back to do not fit.  The items whose allocation does not fit write nothing and
    raise the frame error bit before they count out; the boundary -- run by whichever workgroup is last, possibly while siblings
    that did fit are still storing -- closes the frame without tokens.  The channel's error is WFST_E_CAPACITY and stays it, at
    every advance granularity; the channel behind it (its arena is the memory right behind) decodes its three frames as the
    oracle does."""
    G, W = world.G, world.W
    x = world.mats[0]
    short = world.mats[1][:3]
    o_short = world.want(("short", 1), world.h, BEAM_ONLY, short, world.m)
    dev = G.upload([x, short])
    ptrs = [t.data_ptr() for t in dev]
    for chunk in (0, 7, 1):
        dec = W.BatchDecoder(world.graph, G.gpu_config(BEAM_ONLY), 2, options=W.Options(log2_partitions=6, joint_max=16),
                             max_frames=64, max_tokens_per_frame=256, arena_tokens=1024)
        try:
            pf = dec.path_flags()
            assert pf["two_launch"] == 1 and pf["soft_limit"] == 1, pf
            dec.init()
            codes = []
            for r in ([FRAMES] if chunk == 0 else list(range(chunk, FRAMES, chunk)) + [FRAMES]):
                try:
                    dec.advance(ptrs, [r, min(r, 3)], S.N_PDF)
                    dec.sync()
                except W.WfstError as e:
                    codes.append(e.code)
            assert codes and set(codes) == {-4}, "chunk %d: %s" % (chunk, codes)
            for _ in range(2):
                with pytest.raises(W.WfstError) as e:
                    dec.sync()
                assert e.value.code == -4
            dec.finalize(channels=[1])
            G.assert_same_as_oracle(G.GpuResult(dec.best_paths(channels=[1])[0]), o_short, "the channel behind the failing one, chunk %d" % chunk)
            assert len(dec.frontier(1)[0]) == int(o_short.frame_ntoks[3])
        finally:
            dec.free()


def test_a_hard_per_frame_limit_on_the_lattice_decoder(world):
    """the per-frame limit is a capacity only for decoders without soft_limit -- the fused best-path decoder always has it, so
    this is the lattice decoder on the fused rows, whose items count nothing out: its insert code is as it was.  A limit of 256
    tokens fails the first frame beyond it with WFST_E_CAPACITY; a second channel that stays below it decodes as the oracle does."""
    G, W = world.G, world.W
    x = world.mats[0]
    short = world.mats[1][:3]
    o_short = world.want(("short", 1), world.h, BEAM_ONLY, short, world.m)
    full = world.want(("g", 0), world.h, BEAM_ONLY, x, world.m)
    assert int(full.frame_ntoks.max()) > 256 and int(o_short.frame_ntoks.max()) <= 256
    dev = G.upload([x, short])
    dec = W.BatchDecoder(world.graph, G.gpu_config(BEAM_ONLY), 2, options=W.Options(log2_partitions=6, joint_max=16),
                         max_frames=64, max_tokens_per_frame=256, arena_tokens=1 << 18, lattice_links=1 << 20)
    try:
        assert dec.path_flags()["soft_limit"] == 0
        dec.init()
        dec.advance([t.data_ptr() for t in dev], [FRAMES, 3], S.N_PDF)
        for _ in range(2):
            with pytest.raises(W.WfstError) as e:
                dec.sync()
            assert e.value.code == -4
        dec.finalize(channels=[1])
        G.assert_same_as_oracle(G.GpuResult(dec.best_paths(channels=[1])[0]), o_short, "the channel behind the failing one")
    finally:
        dec.free()


def test_dense_ties(world):
    """the 50-state graph, 24 arcs a state, weights and scores quantised to 0.5: a frame's 1200 records land on 50 states and equal
    costs abound; against the oracle in tie mode (deviation 3), three channels"""
    G = world.G
    cd = dict(beam=12.0, max_active=1000000, min_active=0, lattice_beam=6.0)
    want = [world.want(("d", i), world.hd, cd, x, None, tie=True) for i, x in enumerate(world.dmats)]
    assert sum(o.extra["ties"] for o in want) > 0, "no exact tie on any best path: the workload is not tie-dense"
    dec = world.W.BatchDecoder(world.dgraph, G.gpu_config(cd), len(world.dmats), options=world.W.Options(log2_partitions=6, joint_max=16), **LIMITS)
    try:
        assert dec.path_flags()["two_launch"] == 1
        rec, _ = run_all_granularities(G, dec, world.dgraph, cd, world.dmats, want, "dense ties", ties_allowed=True)
    finally:
        dec.free()
    assert all((r[5:] > 8 * 16).all() for r in rec), [r.tolist() for r in rec]   # (eight items a frame and more, as above)
