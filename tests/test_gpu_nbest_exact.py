"""-m gpu: the n-best kernels held BIT FOR BIT to their restatements (tests/nbest_util.py, proven against the enumeration of every
path by tests/test_nbest_restatement.py) on the lattices of tests/nbest_geometry_util.py, each aimed at a constant the kernels are
cut along (tests/test_nbest_geometry.py holds the oracle's lattices to the same shape checks as are applied here to the device's).

nbest_kernel: dec.nbest(n, max_words=...) against kbest_distinct on dec.raw_lattice(c) fetched at the same moment -- words, their
order, n_words, and the bits of tot_score and lm_score -- on a live channel mid-utterance and on the finalized one.

nbest_paths_kernel: dec.nbest_paths(...) against kbest_paths_dp on dec.determinized_lattice(c) / dec.rescored_lattice(c, L1, L2):
per-arc olabel and the bits of graph, acoustic and tot, in order.  The dicts those getters return keep the device's arc order
(copy_lattice copies the determinizer's and the composition's output as it lies, det_pack_kernel packs it in order), so the
comparison is exact INCLUDING the order of paths with bit-equal totals: nothing here is compared as a set.  Both variants of the
kernel are asked: the per-channel call launches the 1024-thread one, a batch (or the text call) of at most 64 paths the one-wave one.

There are no tolerances in this file.

What it is for, tried with in-bounds mutants of wfst_nbest.hip built aside (none committed); beside each the cases that fail:
  nbest_kernel adds (E.tot + graph) + acoustic            every continuous nbest case, the call surface, max_words, the golden
  select_distinct without its lm step                     merge, widths (quantised)
  the candidate of lane 63 dropped before a pass          fan (both families)
  the backpointers left out of the rounds' comparison     eps_chains (both families), the epsilon-chains golden
  the max_words overflow branch as an in-buffer reversal  test_nbest_max_words
  nbest_paths_kernel's key with ~q for q                  small, sortbuf, chain14 (quantised), the text on chain14
  the second chunk's candidates numbered from 0 again     chain14
Of these the n-best tests as they stood caught the lane-63 one alone (the backpointer one was not tried on them)."""
import numpy as np
import pytest

import nbest_geometry_util as U
from align_util import from_gpu
from golden_util import Golden
from nbest_util import F32, kbest_distinct, kbest_paths_dp, same_nbest, same_paths

pytestmark = pytest.mark.gpu
E_ARG = -1


class Decoded:
    def __init__(self, synth, tmp_path, build, quantised, limits=None):
        import gpu_util as G

        self.G, self.W = G, G.wfstdec
        self.g, self.mats = build(synth, quantised)
        path = str(tmp_path / "g.bin")
        self.g.write(path)
        self.graph = self.W.Graph.load(path)
        self.dec = self.W.BatchDecoder(self.graph, G.gpu_config(U.CFG), len(self.mats), **(limits or U.LIM))
        self.dev = G.upload(self.mats)
        self.T, self.stride = int(self.mats[0].shape[0]), int(self.mats[0].shape[1])
        self.dec.init()

    def advance(self, upto):
        self.dec.advance([t.data_ptr() for t in self.dev], [upto] * len(self.mats), self.stride)

    def finish(self):
        self.advance(self.T)
        self.dec.finalize()

    def free(self):
        self.dec.free()
        self.graph.free()


def check_nbest_now(dec, channels, ns, what, max_words=256):
    """the lattices of `channels` as they are now, then the calls: every answer the restatement's"""
    lats = {c: from_gpu(dec.raw_lattice(c, True)) for c in channels}
    for n in ns:
        got = dec.nbest(n, channels=channels, max_words=max_words)
        for i, c in enumerate(channels):
            want = kbest_distinct(lats[c], n, max_words=max_words) if lats[c] is not None else []
            same_nbest(got[i], want, "%s channel %d n %d" % (what, c, n))
    return lats


# ---- nbest_kernel ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,quantised", U.nbest_case_ids(), ids=lambda v: str(v))
def test_nbest_equals_kbest_distinct(name, quantised, synth, tmp_path):
    build, check, _ = U.NBEST_CASES[name]
    d = Decoded(synth, tmp_path, build, quantised)
    try:
        chans = list(range(len(d.mats)))
        for upto in sorted({1, max(1, d.T // 2), d.T - 1} - {0, d.T}):     # mid-utterance: everything alive now
            d.advance(upto)
            check_nbest_now(d.dec, chans, (1, 16), "%s live at frame %d" % (name, upto))
        d.finish()
        lats = check_nbest_now(d.dec, chans, U.NS, name)
        for c in chans:
            check(U.facts(lats[c]), quantised)
    finally:
        d.free()


def test_nbest_call_surface(synth, tmp_path):
    """a sub-list and a non-ascending list of channels (three utterances on the fan graph); n outside 1..16 is an argument error"""
    build, _, _ = U.NBEST_CASES["fan"]
    d = Decoded(synth, tmp_path, build, False)
    try:
        d.finish()
        for chans in ([1], [2, 0], [2, 1, 0], [1, 2]):
            check_nbest_now(d.dec, chans, (3, 16), "fan, channels %s" % chans)
        for n in (0, 17):
            with pytest.raises(d.W.WfstError) as e:
                d.dec.nbest(n)
            assert e.value.code == E_ARG
    finally:
        d.free()


def test_nbest_max_words(synth, tmp_path):
    """the line of 20 words (two paths, 20 words each): n_words is 20 whatever max_words is, the FIRST max_words words are returned
    (max_words below 20: the branch that walks the path a second time), and a path's words stay inside its own row"""
    build, check, _ = U.NBEST_CASES["line20"]
    d = Decoded(synth, tmp_path, build, False)
    try:
        d.finish()
        L = from_gpu(d.dec.raw_lattice(0, True))
        check(U.facts(L), False)
        full = kbest_distinct(L, 2)
        assert [p["n_words"] for p in full] == [20, 20] and full[0]["words"].tolist()[:19] == list(range(1, 20))
        for mw in (20, 19, 5, 1):
            got = d.dec.nbest(2, max_words=mw)[0]
            same_nbest(got, kbest_distinct(L, 2, max_words=mw), "line, max_words %d" % mw)
            assert [p["n_words"] for p in got] == [20, 20]
            for p, f in zip(got, full):
                assert p["words"].tolist() == f["words"].tolist()[:mw]
    finally:
        d.free()


def test_nbest_on_the_epsilon_chains_golden(tmp_path):
    """tests/golden/lattice_eps_chains.npz: epsilon chains with words, final weights, a dead-end branch"""
    import gpu_util as G

    g = Golden("lattice_eps_chains")
    graph = G.wfstdec.Graph.load(g.write_graph(str(tmp_path / "g.bin")))
    if g.tid2pdf is not None:
        graph.set_tid2pdf(g.tid2pdf)
    cd = dict(g.meta["cfgs"][g.meta["cases"][0]["cfg"]])
    mats = list(g.utts)
    dec = G.wfstdec.BatchDecoder(graph, G.gpu_config(cd), len(mats), max_frames=64, max_tokens_per_frame=4096, arena_tokens=1 << 16, lattice_links=1 << 18)
    try:
        dev = G.upload(mats)
        dec.init()
        lens = [int(x.shape[0]) for x in mats]
        dec.advance([t.data_ptr() for t in dev], [min(5, t) for t in lens], int(mats[0].shape[1]))
        live = [c for c in range(len(mats)) if lens[c] > 5]
        n_live = check_nbest_now(dec, live, (1, 16), "eps_chains golden, live")
        dec.advance([t.data_ptr() for t in dev], lens, int(mats[0].shape[1]))
        dec.finalize()
        lats = check_nbest_now(dec, list(range(len(mats))), U.NS, "eps_chains golden")
        assert len(n_live) >= 1 and sum(L is not None for L in lats.values()) >= 2
    finally:
        dec.free()
        graph.free()


# ---- nbest_paths_kernel ----------------------------------------------------------------------------------------------------------
PATHS_LIM = dict(max_frames=32, max_tokens_per_frame=4096, arena_tokens=1 << 14, lattice_links=1 << 15)


@pytest.mark.parametrize("name,quantised", U.paths_case_ids(), ids=lambda v: str(v))
def test_nbest_paths_equal_kbest_paths_dp(name, quantised, synth, tmp_path):
    """every n of NS_PATHS through the per-channel call (the 1024-thread kernel) and through a batch (the one-wave kernel up to 64
    paths): both the restatement's answer, hence each other's.  n = 4096 on the small lattices: fewer paths than asked for."""
    build, check, _ = U.PATHS_CASES[name]
    d = Decoded(synth, tmp_path, build, quantised, PATHS_LIM)
    try:
        d.advance(max(1, d.T // 2))
        D = d.dec.determinized_lattice(0, True)
        same_paths(d.dec.nbest_paths(0, 7), kbest_paths_dp(D, 7), name + " live, n 7")
        d.finish()
        D = d.dec.determinized_lattice(0)
        f = U.paths_facts(D)
        r = check(f, quantised)
        assert r is None or r, sorted(set(f["cands"].tolist()))
        assert int(np.asarray(D["st_final"]).sum()) == 1 and int(np.asarray(D["st_final"])[D["a_dst"]].sum()) == 1   # one final-weight arc, shared
        for n in U.NS_PATHS:
            want = kbest_paths_dp(D, n)
            assert len(want) == min(n, f["n_paths"])
            same_paths(d.dec.nbest_paths(0, n), want, "%s n %d, alone" % (name, n))
            d.dec.nbest_paths_batch(n)
            same_paths(d.dec.nbest_paths(0, n), want, "%s n %d, batched" % (name, n))
    finally:
        d.free()


def test_nbest_words_on_the_chunked_merge_lattice(synth, tmp_path):
    """nbest_words = nbest_paths + wfst_lattice_to_vector by its definition: the 64 cheapest of the 14-frame chain's 24576 paths
    (quantised: ties everywhere) as the restatement lists them, through LatticeToVector; bytes compared"""
    from test_gpu_nbest_words import _same, _to_vector

    build, _, _ = U.PATHS_CASES["chain14"]
    d = Decoded(synth, tmp_path, build, True, PATHS_LIM)
    try:
        d.finish()
        D = d.dec.determinized_lattice(0)
        want = [(_to_vector(d.W, p), p["tot"]) for p in kbest_paths_dp(D, 64)]
        _same(d.dec.nbest_words(64, channels=[0])[0], want, "chain14")
    finally:
        d.free()


def test_nbest_paths_on_the_rescored_lattice(synth, tmp_path):
    """the second pass: nbest_paths(c, n, L1, L2) against the restatement on rescored_lattice(c, L1, L2) (final flags per state, a
    final weight per LM state), with tests/test_compose_lattice.py's LM pair, alone and batched"""
    from test_compose_lattice import _setup

    _, _, _, p1, p2, _ = _setup(synth, tmp_path, 0)
    build, _, _ = U.PATHS_CASES["small"]
    for quantised in (False, True):
        d = Decoded(synth, tmp_path, build, quantised, PATHS_LIM)
        L1, L2 = d.W.Lm.load(p1, -1.0), d.W.Lm.load(p2, 1.0)
        try:
            d.finish()
            R = d.dec.rescored_lattice(0, L1, L2)
            assert R is not None and R["n_states"] >= d.dec.determinized_lattice(0)["n_states"]
            for n in (1, 64, 65, 4096):
                want = kbest_paths_dp(R, n)
                assert 1 <= len(want) <= n
                same_paths(d.dec.nbest_paths(0, n, L1, L2), want, "rescored, n %d, alone" % n)
                d.dec.nbest_paths_batch(n, L1, L2)
                same_paths(d.dec.nbest_paths(0, n, L1, L2), want, "rescored, n %d, batched" % n)
        finally:
            L1.free()
            L2.free()
            d.free()
