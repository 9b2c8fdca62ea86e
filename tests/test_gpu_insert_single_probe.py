"""-m gpu: the insert item that probes its LDS table once.  Pass 1 leaves every record with the slot it ended on, pass 2 claims
that slot without hashing or walking again, and a thread claims for all its records before it stores a token (insert_body,
asr-decoder_amd/csrc/wfst_kernels.hip).  The shapes are the smallest at which a carried slot can go wrong: 64-slot tables whose
probe chains run over the table's end, many records per state, records above the final cutoff among live ones, sub-passes by hash
class, the items of more than one sweep that still probe twice, an arena that does not take the item's tokens -- each for the
best-path decoder, the first two also for a lattice and a biglm decoder.

Bar: words, transition-ids, per-hop labels and float costs, tot_score bit-identical to the CPU oracle; every workload is checked
to have no exact cost tie on its best paths (continuous random scores), so no tie rule is involved."""
import importlib

import numpy as np
import pytest

import pyoracle

pytestmark = pytest.mark.gpu
lmsynth = importlib.import_module("asr-decoder_amd.lmsynth")

FRAMES = 40
LIMITS = dict(max_frames=64, max_tokens_per_frame=32768, arena_tokens=1 << 20)


def dense_graph(synth, n_states=50, fan=24, n_labels=40, seed=3):
    """every state has `fan` emitting arcs to distinct random states (in-degree = fan on average) and a self-loop: a frame's
    candidates are many times its states, most records lose their state's minimum"""
    rng = np.random.default_rng(seed)
    rows = {}
    for s in range(n_states):
        to = rng.choice(n_states, size=fan, replace=False)
        rows[s] = [(int(rng.integers(1, n_labels + 1)), int(rng.integers(0, 30)), float(np.float32(rng.uniform(0.0, 4.0))), int(t)) for t in to]
    return synth.graph_from_arc_lists(n_states, 0, rows, {s: float(np.float32(rng.uniform(0.0, 2.0))) for s in range(0, n_states, 7)})


def hclg(synth, n_states, seed):
    return synth.make_hclg_like(n_states, seed=seed, n_tid=600, n_words=29), synth.default_tid2pdf(600)


def workload(synth, name):
    """(graph, tid2pdf or None, [loglikes], config, wfst_options) of a case"""
    cfg = lambda beam: dict(beam=beam, max_active=1000000, min_active=0, lattice_beam=6.0)
    if name == "wrap64":       # items of <= 16 records: 64-slot tables, a chain that starts near slot 63 runs on at slot 0
        g, m = hclg(synth, 300, 11)
        return g, m, [synth.make_loglikes(g, FRAMES, 300, m, seed=100 + i, mu=-2.0)[0] for i in range(6)], cfg(7.0), dict(log2_partitions=6, joint_max=16)
    if name == "dense":        # ~1200 records on <= 50 states per frame, in the smallest table (sub-passes of a heavy item)
        g = dense_graph(synth)
        rng = np.random.default_rng(5)
        return g, None, [rng.normal(-1.5, 1.0, size=(FRAMES, 41)).astype(np.float32) for _ in range(4)], cfg(12.0), dict(log2_lds_slots=8, log2_partitions=1)
    if name == "cutoff":       # a wide score spread under a beam of 4: of a frame's ~1200 records most are at or above the final cutoff,
        g = dense_graph(synth)  # in every wave, among live ones (20 to 30 of the 50 states keep a token)
        rng = np.random.default_rng(9)
        return g, None, [rng.normal(-1.5, 3.0, size=(FRAMES, 41)).astype(np.float32) for _ in range(6)], cfg(4.0), dict()
    if name == "subpass":      # one-sweep items (<= 1536 records) beyond 3/4 of a 256-slot table: sub-passes by hash class
        g, m = hclg(synth, 6000, 17)
        return g, m, [synth.make_loglikes(g, FRAMES, 300, m, seed=300 + i, mu=-2.0)[0] for i in range(4)], cfg(14.0), dict(log2_lds_slots=8, log2_partitions=3, joint_max=64)
    if name == "multisweep":   # ONE bucket per channel: frames of more than 512 x 3 records are items of several sweeps (the re-probing path)
        g, m = hclg(synth, 6000, 17)
        return g, m, [synth.make_loglikes(g, FRAMES, 300, m, seed=300 + i, mu=-2.0)[0] for i in range(4)], cfg(14.0), dict(log2_partitions=0, joint_max=64)
    raise KeyError(name)


CASES = ["wrap64", "dense", "cutoff", "subpass", "multisweep"]


class Case:
    def __init__(self, synth, oracle, tmp, name):
        import gpu_util as G

        self.G, self.name = G, name
        self.g, self.m, self.mats, self.cd, self.opt = workload(synth, name)
        self.path = str(tmp / (name + ".bin"))
        self.g.write(self.path)
        self.graph = G.wfstdec.Graph.load(self.path)
        if self.m is not None:
            self.graph.set_tid2pdf(self.m)
        self.h = oracle.load_graph(self.path)
        self.want = [oracle.decode(self.h, pyoracle.Config(**self.cd), x, self.m) for x in self.mats]

    def options(self):
        return self.G.wfstdec.Options(**self.opt)

    def close(self, oracle):
        self.graph.free()
        oracle.free_graph(self.h)


@pytest.fixture(scope="module")
def cases(tmp_path_factory, synth, oracle):
    """every case's graph on the device and its oracle results, computed once"""
    tmp = tmp_path_factory.mktemp("single_probe")
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(synth, oracle, tmp, name)
        return made[name]
    yield get
    for c in made.values():
        c.close(oracle)


@pytest.mark.parametrize("name", CASES)
def test_best_path_equals_the_oracle(cases, name):
    c = cases(name)
    G = c.G
    assert all(o.ok and o.extra["ties"] == 0 for o in c.want), "the workload must have no exact tie on a best path"
    per_frame = min(o.extra["tokens_created"] for o in c.want) / FRAMES
    if name == "multisweep":   # (records >= tokens: a mean above one sweep's 512 x 3 records means frames of several sweeps)
        assert per_frame > 512 * 3, per_frame
    if name == "subpass":      # (eight buckets, each beyond 3/4 of its 256 slots)
        assert per_frame > 8 * 192, per_frame
    dec = G.wfstdec.BatchDecoder(c.graph, G.gpu_config(c.cd), len(c.mats), options=c.options(), **LIMITS)
    try:
        for chunk in (0, 7):
            for i, (r, o) in enumerate(zip(G.decode_batch(c.graph, c.cd, c.mats, chunk=chunk, dec=dec), c.want)):
                G.assert_same_as_oracle(r, o, "%s utt %d chunk %d" % (name, i, chunk))
    finally:
        dec.free()


def test_an_item_that_does_not_fit_the_arena_writes_nothing_and_is_loud(cases, oracle):
    """arena_tokens too small for the utterance: WFST_E_CAPACITY as before, and it stays the channel's error (the error word does
    not move when it is read again); a neighbouring channel's arena -- the memory right behind the failing one's -- still holds
    ITS utterance's tokens: its best path is the oracle's."""
    c = cases("multisweep")
    G, W = c.G, c.G.wfstdec
    big = G.decode_batch(c.graph, c.cd, c.mats[:1])[0]
    need = int(big.stats["tokens"])
    assert need > 2048
    # both channels get arena_tokens; channel 0 decodes the utterance in full and fails, channel 1 decodes its first 3 frames and fits
    short = c.mats[1][:3]
    dec = W.BatchDecoder(c.graph, G.gpu_config(c.cd), 2, max_frames=64, max_tokens_per_frame=32768, arena_tokens=2048)
    try:
        dev = G.upload([c.mats[0], short])
        dec.init()
        dec.advance([t.data_ptr() for t in dev], [FRAMES, 3], int(short.shape[1]))
        codes = []
        for _ in range(2):
            with pytest.raises(W.WfstError) as e:
                dec.sync()
            codes.append(e.value.code)
        assert codes == [-4, -4]
        dec.finalize(channels=[1])
        r = G.GpuResult(dec.best_paths(channels=[1])[0])
    finally:
        dec.free()
    G.assert_same_as_oracle(r, oracle.decode(c.h, pyoracle.Config(**c.cd), short, c.m), "the channel behind the failing one")


@pytest.mark.parametrize("name", ["wrap64", "dense"])
def test_lattice_decoder_equals_the_oracle(cases, oracle, name):
    """the lattice instantiation takes the carried slot too (its links' destination slots): best path and the raw lattice, arc for arc"""
    c = cases(name)
    G = c.G
    dec = G.wfstdec.BatchDecoder(c.graph, G.gpu_config(c.cd), len(c.mats), options=c.options(), lattice_links=1 << 20, **LIMITS)
    try:
        res = G.decode_batch(c.graph, c.cd, c.mats, dec=dec)
        for i, (r, o) in enumerate(zip(res, c.want)):
            G.assert_same_as_oracle(r, o, "%s lattice decoder utt %d" % (name, i))
        try:
            oracle.set_order_free(True)   # (the order-independent part of the reference's lattice: DESIGN.md section 4, deviation 6)
            for i, x in enumerate(c.mats):
                O = pyoracle.oracle_raw_lattice(oracle, c.h, pyoracle.Config(**c.cd), x, c.m)
                d = dec.raw_lattice(i)
                L = pyoracle.RawLattice(True, d["n_states"], 0, d["st_final"], d["a_src"], d["a_dst"], d["a_ilabel"], d["a_olabel"],
                                        d["a_graph"], d["a_acoustic"], d["st_frame"], d["st_state"], d["st_cost"])
                assert np.array_equal(L.labelled_arcs(), O.labelled_arcs()), "%s utt %d lattice" % (name, i)
        finally:
            oracle.set_order_free(False)
    finally:
        dec.free()


@pytest.mark.parametrize("name", ["wrap64", "dense"])
def test_biglm_decoder_equals_the_fixed_mode_oracle(cases, oracle, tmp_path, name):
    """the biglm instantiation: pass 1b (the lowest source pair key among the holders of a slot's minimum) goes to the carried slot"""
    c = cases(name)
    G = c.G
    old, new = lmsynth.make_lm(30, 2, 12, 3, 0, 0, seed=11), lmsynth.make_lm(30, 3, 15, 3, 12, 2, seed=12)
    p1, p2 = str(tmp_path / "old.bin"), str(tmp_path / "new.bin")
    old.to_fsa().write(p1)
    new.to_fsa().write(p2)
    L1, L2 = G.wfstdec.Lm.load(p1, -1.0), G.wfstdec.Lm.load(p2, 1.0)
    o1, o2 = pyoracle.Lm(oracle, p1, -1.0), pyoracle.Lm(oracle, p2, 1.0)
    cd = dict(c.cd, lattice_beam=25.0)
    try:
        oracle.set_order_free(True)
        want = [pyoracle.biglm_decode(oracle, c.h, pyoracle.Config(**cd), o1, o2, x, c.m, fixed=True) for x in c.mats]
    finally:
        oracle.set_order_free(False)
    assert all(o.extra["ties"] == 0 and o.extra["lm_oob"] == 0 for o in want)
    dec = G.wfstdec.BatchDecoder(c.graph, G.gpu_config(cd), len(c.mats), old_lm=L1, new_lm=L2, options=c.options(), **LIMITS)
    try:
        for i, (r, o) in enumerate(zip(G.decode_batch(c.graph, cd, c.mats, dec=dec), want)):
            G.assert_same_as_oracle(r, o, "%s biglm utt %d" % (name, i))
    finally:
        dec.free()
        L1.free()
        L2.free()
