"""-m gpu: incremental partial hypotheses with a stable word prefix (wfst_decoder_get_partial and its halves; partial_kernel).

What is pinned, all through the C ABI, all under beam-only pruning (the regime in which the device equals the reference bit for
bit), each on a best-path and on a lattice decoder:
  words      after every chunk equal the oracle's partial best path at that frame count (decode(prefix, finalize=False,
             use_final_probs=False)) and the words of wfst_decoder_get_best_path(use_final_probs = 0) at the same point; exactly;
  safety     every call's words[:n_stable] is a prefix of every later call's words, of the oracle's final words, of the device's
             best path after FinalizeDecoding (use_final_probs = 1) and of its last best path with use_final_probs = 0 (asked right
             before FinalizeDecoding: the library, like the reference, refuses that call afterwards); n_stable and stable_frame
             never decrease;
  liveness   on a layered graph whose every L-th layer is a single state the commit token is known by construction.
"""
import ctypes as C

import numpy as np
import pytest

import pyoracle

pytestmark = pytest.mark.gpu

BEAM_ONLY = dict(beam=13.0, max_active=1000000, min_active=0, lattice_beam=7.0)


def make_decoder(G, graph, cd, n, lattice, max_frames=512, arena=1 << 22, max_tok=32768, links=1 << 22, **kw):
    lim = dict(max_frames=max_frames, max_tokens_per_frame=max_tok, arena_tokens=arena)
    if lattice:
        lim["lattice_links"] = links
    lim.update(kw)
    return G.wfstdec.BatchDecoder(graph, G.gpu_config(cd), n, **lim)


def is_prefix(a, b):
    return len(a) <= len(b) and np.array_equal(np.asarray(a), np.asarray(b)[: len(a)])


class History:
    """The partial results of one utterance, call after call: checks what must hold between them."""

    def __init__(self, what):
        self.what, self.calls = what, []   # (frames, words, n_stable, stable_frame)

    def add(self, frames, words, n_stable, stable_frame):
        what = "%s @%d" % (self.what, frames)
        assert 0 <= n_stable <= len(words), what
        if self.calls:
            _, _, ns0, sf0 = self.calls[-1]
            assert n_stable >= ns0 and stable_frame >= sf0, what + ": the commit point moved backwards"
        for f0, w0, ns0, _ in self.calls:
            assert is_prefix(w0[:ns0], words), "%s: the stable prefix of @%d was retracted" % (what, f0)
        self.calls.append((frames, np.array(words), int(n_stable), int(stable_frame)))

    def check_final(self, words, which):
        for f0, w0, ns0, _ in self.calls:
            assert is_prefix(w0[:ns0], words), "%s: the stable prefix of @%d is no prefix of %s" % (self.what, f0, which)


def stream(G, dec, mats, chunk, stride, check_call, cap=1024, hop_cap=2048):
    """init, then chunk after chunk: advance, get_partial, get_best_path(use_final_probs = 0); check_call(c, frames, words, n_stable,
    stable_frame) per channel and call.  Then FinalizeDecoding.  Returns (histories, the device's final words with
    use_final_probs = 1, its last words with use_final_probs = 0)."""
    T = [int(m.shape[0]) for m in mats]
    dev = G.upload(mats)
    dec.init()
    hist = [History("channel %d" % c) for c in range(len(mats))]
    last0 = None
    for r in list(range(chunk, max(T), chunk)) + [max(T)]:
        dec.advance([t.data_ptr() for t in dev], [min(r, t) for t in T], stride)
        words, ns, sf = dec.partial(cap_words=cap)
        bp = dec.best_paths(use_final_probs=False, cap=hop_cap)
        for c in range(len(mats)):
            fr = min(r, T[c])
            assert np.array_equal(words[c], bp[c]["words"]), "channel %d @%d: partial words != get_best_path's" % (c, fr)
            hist[c].add(fr, words[c], ns[c], sf[c])
            check_call(c, fr, words[c], int(ns[c]), int(sf[c]))
        last0 = [b["words"] for b in bp]
    dec.finalize()
    fin = [b["words"] for b in dec.best_paths(use_final_probs=True, cap=hop_cap)]
    for c in range(len(mats)):
        hist[c].check_final(fin[c], "the final best path (use_final_probs = 1)")
        hist[c].check_final(last0[c], "the last best path with use_final_probs = 0")
    return hist, fin, last0


# ---- 1 + 2: words and safety on the 50k-arc graph --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def setup50k(tmp_path_factory, synth, oracle):
    import gpu_util as G

    g = synth.make_hclg_like(14000, seed=7)  # ~50k arcs, as tests/test_gpu_parity.py
    path = str(tmp_path_factory.mktemp("g") / "g50k.bin")
    g.write(path)
    m = synth.default_tid2pdf(6000)
    graph = G.wfstdec.Graph.load(path)
    graph.set_tid2pdf(m)
    h = oracle.load_graph(path)
    yield dict(g=g, path=path, m=m, graph=graph, h=h, G=G)
    graph.free()
    oracle.free_graph(h)


@pytest.mark.parametrize("lattice", [False, True])
@pytest.mark.parametrize("chunk", [7, 25, 64])
def test_words_and_stable_prefix(setup50k, synth, oracle, chunk, lattice):
    s = setup50k
    G = s["G"]
    lengths = [160, 63, 100, 29, 131, 8]
    mats = [synth.make_loglikes(s["g"], T, 3000, s["m"], seed=8100 + i)[0] for i, T in enumerate(lengths)]
    cfg = pyoracle.Config(**BEAM_ONLY)
    seen = {}

    def check(c, fr, words, ns, sf):
        if (c, fr) not in seen:
            seen[(c, fr)] = oracle.decode(s["h"], cfg, mats[c][:fr], s["m"], finalize=False, use_final_probs=False).words
        assert np.array_equal(words, seen[(c, fr)]), "channel %d @%d: partial words != the oracle's" % (c, fr)
        assert sf < max(fr, 1)

    dec = make_decoder(G, s["graph"], BEAM_ONLY, len(mats), lattice)
    hist, fin, _ = stream(G, dec, mats, chunk, 3000, check)
    dec.free()
    n_committed = 0
    for c, x in enumerate(mats):
        o = oracle.decode(s["h"], cfg, x, s["m"])
        hist[c].check_final(o.words, "the oracle's final words")
        assert np.array_equal(fin[c], o.words)
        n_committed += hist[c].calls[-1][2]
    assert n_committed > 0, "nothing was ever committed: the safety checks were vacuous"


# ---- 3: liveness, exactly ----------------------------------------------------------------------------------------------------------
def layered_graph(synth, n_layers, period, width, fan, n_tid, n_words, seed):
    """Layer k is reached after exactly k emitting arcs (modulo n_layers: the layers wrap around); every period-th layer is ONE
    state; no self-loops, no epsilon arcs but the super-final ones (final states sit in the wide layers only, so that the frame of
    a single-state layer holds exactly one token); real random weights (no ties), distinct targets per state (no parallel arcs)."""
    assert n_layers % period == 0
    rng = np.random.default_rng(seed)
    layers, n = [], 0
    for k in range(n_layers):
        w = 1 if k % period == 0 else width
        layers.append(list(range(n, n + w)))
        n += w
    arcs, finals = {}, {}
    for k in range(n_layers):
        nxt = layers[(k + 1) % n_layers]
        for st in layers[k]:
            to = rng.choice(nxt, size=min(fan, len(nxt)), replace=False)
            arcs[st] = [(int(rng.integers(1, n_tid + 1)), int(rng.integers(1, n_words + 1)) if rng.random() < 0.4 else 0,
                         float(rng.uniform(0.1, 3.0)), int(t)) for t in to]
            if len(layers[k]) > 1 and rng.random() < 0.1:
                finals[st] = float(rng.uniform(0.1, 2.0))
    return synth.graph_from_arc_lists(n, layers[0][0], arcs, finals)


@pytest.mark.parametrize("lattice", [False, True])
def test_liveness_on_a_layered_graph(synth, oracle, tmp_path, lattice):
    """After the frame of a single-state layer exactly one token exists, so with b the largest such frame below
    m_last = (nd - 1) / prune_interval * prune_interval: stable_frame >= b and n_stable >= the words of the oracle's partial path
    up to its b-th emitting hop -- for every channel at every call, the last one before FinalizeDecoding included."""
    import gpu_util as G

    period, interval, chunk, n_tid = 6, 10, 25, 200
    g = layered_graph(synth, 24, period, 40, 5, n_tid, 300, seed=11)
    path = str(tmp_path / "layered.bin")
    g.write(path)
    m = synth.default_tid2pdf(n_tid)
    graph = G.wfstdec.Graph.load(path)
    graph.set_tid2pdf(m)
    h = oracle.load_graph(path)
    cd = dict(beam=9.0, max_active=1000000, min_active=0, lattice_beam=5.0, prune_interval=interval)
    cfg = pyoracle.Config(**cd)
    lengths = [300, 287, 263]   # (ragged ends; every utterance long enough for b to advance ten times)
    rng = np.random.default_rng(12)
    mats = [rng.normal(-2.0, 1.0, size=(T, n_tid // 2)).astype(np.float32) for T in lengths]
    advances = [set() for _ in lengths]
    n_checked = [0]

    def check(c, fr, words, ns, sf):
        o = oracle.decode(h, cfg, mats[c][:fr], m, finalize=False, use_final_probs=False)
        assert np.array_equal(words, o.words), (c, fr)
        m_last = ((fr - 1) // interval) * interval
        b = ((m_last - 1) // period) * period if m_last >= 1 else 0   # the largest multiple of period below m_last
        assert sf >= b, "channel %d @%d: stable_frame %d < %d" % (c, fr, sf, b)
        emitting = np.cumsum(o.path_ilabel != 0)
        want = int(np.sum((o.path_olabel != 0) & (emitting <= b) & ((o.path_ilabel != 0) | (emitting < b))))
        assert ns >= want, "channel %d @%d: n_stable %d < %d" % (c, fr, ns, want)
        advances[c].add(b)
        n_checked[0] += 1

    try:
        dec = make_decoder(G, graph, cd, len(mats), lattice, max_frames=320, arena=1 << 20, max_tok=8192, links=1 << 20)
        hist, _, _ = stream(G, dec, mats, chunk, n_tid // 2, check)
        dec.free()
        n_calls = sum(len(x.calls) for x in hist)
        assert n_checked[0] == n_calls == 3 * len(range(chunk, 300, chunk)) + 3   # no call left out of the comparison
        assert all(len(a) - 1 >= 8 for a in advances), "b advanced %s times only" % [len(a) - 1 for a in advances]   # per utterance
    finally:
        oracle.free_graph(h)
        graph.free()


# ---- 4: the parallel-arc quirk -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lattice", [False, True])
def test_parallel_arc_quirk_is_committed_only_once_frozen(synth, oracle, tmp_path, lattice):
    """Two parallel arcs 0 -> 1 with words 11 (cheaper) and 22; the dearer one survives the beam but not lattice_beam.  Until a
    PruneActiveTokens pass has met the hop GetBestPath reports word 22 (the first matching forward link), afterwards word 11:
    the partial words follow it, and the word is stable only once it is frozen (the m_last rule)."""
    import gpu_util as G

    g = synth.graph_from_arc_lists(
        3, 0,
        {0: [(1, 11, 1.0, 1), (2, 22, 1.5, 1)], 1: [(3, 0, 0.5, 1), (4, 33, 0.25, 2)], 2: [(5, 0, 0.625, 2)]},   # (staying in state 1 is cheaper than staying in 2: no ties)
        {2: 0.75},
    )
    path = str(tmp_path / "quirk.bin")
    g.write(path)
    graph = G.wfstdec.Graph.load(path)
    h = oracle.load_graph(path)
    cd = dict(beam=13.0, max_active=1000, min_active=0, lattice_beam=0.25, prune_interval=5)
    ll = np.full((14, 8), -1.0, np.float32)
    ll[:, 1] = ll[:, 2] = -2.25
    got = {}

    def check(c, fr, words, ns, sf):
        o = oracle.decode(h, pyoracle.Config(**cd), ll[:fr], None, finalize=False, use_final_probs=False)
        assert np.array_equal(words, o.words), fr
        got[fr] = (list(words), ns, sf)

    try:
        dec = make_decoder(G, graph, cd, 1, lattice, max_frames=64, arena=1 << 16, max_tok=4096, links=1 << 16)
        hist, fin, _ = stream(G, dec, [ll], 3, 8, check, cap=64, hop_cap=256)
        dec.free()
        assert got[3][0][0] == 22 and got[3][1] == 0          # before the pass: the shadowing arc, and nothing stable
        assert got[6][0][0] == 11 and got[6][1] >= 1 and got[6][2] >= 1   # behind it (m_last = 5): the winner, committed
        assert fin[0][0] == 11
    finally:
        oracle.free_graph(h)
        graph.free()


# ---- 5: token collection and compaction ------------------------------------------------------------------------------------------
def test_collections_and_compactions_do_not_show(synth, oracle, tmp_path):
    """The setup of tests/test_gpu_token_gc.py: an arena a twelfth of the tokens created, so that collections (which move tokens and
    resolve epsilon backpointers) run between the partial calls; a lattice decoder with prune_interval 5 compacts its arena every
    five frames.  Both answer call for call as a roomy best-path decoder does, n_stable and stable_frame included."""
    import gpu_util as G

    g = synth.make_hclg_like(5000, seed=17, n_tid=2000, n_words=3000)
    m = synth.default_tid2pdf(2000)
    path = str(tmp_path / "g.bin")
    g.write(path)
    graph = G.wfstdec.Graph.load(path)
    graph.set_tid2pdf(m)
    cd = dict(beam=10.0, max_active=1000000, min_active=0, lattice_beam=5.0, prune_interval=5)
    T = [1200, 777, 333]
    mats = [synth.make_loglikes(g, t, 1000, m, seed=70 + i, mu=-2.5)[0] for i, t in enumerate(T)]
    h = oracle.load_graph(path)
    try:
        created = max(oracle.decode(h, pyoracle.Config(**cd), x, m).extra["tokens_created"] for x in mats)
        runs = {}
        for name, lattice, arena in (("roomy", False, 1 << 22), ("small", False, int(created // 12)), ("lattice", True, 1 << 22)):
            rec = []
            dec = make_decoder(G, graph, cd, len(T), lattice, max_frames=1300, arena=arena, max_tok=16384)
            dev = G.upload(mats)
            dec.init()
            hist = [History("%s channel %d" % (name, c)) for c in range(len(T))]
            for r in list(range(97, max(T), 97)) + [max(T)]:
                dec.advance([t.data_ptr() for t in dev], [min(r, t) for t in T], 1000)
                words, ns, sf = dec.partial(cap_words=1300)
                for c in range(len(T)):
                    hist[c].add(min(r, T[c]), words[c], ns[c], sf[c])
                rec.append(([w.tolist() for w in words], ns.tolist(), sf.tolist()))
            dec.sync()
            if name == "small":
                assert dec.stats(0)["collections"] >= 4
            dec.finalize()
            fin = dec.best_paths(cap=4096)
            for c in range(len(T)):
                hist[c].check_final(fin[c]["words"], "the final best path")
            dec.free()
            runs[name] = rec
        assert runs["small"] == runs["roomy"] and runs["lattice"] == runs["roomy"]
        assert max(runs["roomy"][-1][1]) > 0
    finally:
        oracle.free_graph(h)
        graph.free()


# ---- 6: an utterance longer than the kernels' LDS frame table ------------------------------------------------------------------------
@pytest.mark.parametrize("lattice", [False, True])
def test_long_utterance(synth, oracle, tmp_path, lattice):
    import gpu_util as G

    g = synth.make_hclg_like(3000, seed=21, n_tid=600, n_words=500)
    m = synth.default_tid2pdf(600)
    path = str(tmp_path / "g.bin")
    g.write(path)
    graph = G.wfstdec.Graph.load(path)
    graph.set_tid2pdf(m)
    h = oracle.load_graph(path)
    cd = dict(beam=9.0, max_active=1000000, min_active=0, lattice_beam=5.0)
    cfg = pyoracle.Config(**cd)
    T = 3300   # > kBpFrames (3072)
    mats = [synth.make_loglikes(g, T, 300, m, seed=90, mu=-2.2)[0]]

    def check(c, fr, words, ns, sf):
        o = oracle.decode(h, cfg, mats[c][:fr], m, finalize=False, use_final_probs=False)
        assert np.array_equal(words, o.words), fr

    try:
        dec = make_decoder(G, graph, cd, 1, lattice, max_frames=3400, arena=1 << 22, max_tok=16384)
        hist, fin, _ = stream(G, dec, mats, 471, 300, check, cap=3400, hop_cap=8192)
        dec.free()
        o = oracle.decode(h, cfg, mats[0], m)
        hist[0].check_final(o.words, "the oracle's final words")
        assert np.array_equal(fin[0], o.words)
        assert hist[0].calls[-1][3] > 3072 - 471 and hist[0].calls[-1][2] > 0
    finally:
        oracle.free_graph(h)
        graph.free()


# ---- 7: the walk's stop token on a chunk edge ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("lattice", [False, True])
def test_stop_token_on_a_chunk_edge(synth, oracle, tmp_path, lattice):
    """A chain graph (one path, no input-epsilon arcs: one hop is one frame, one token per frame), a word on every third arc.  Every
    frame holds one token, so a call at nd frames commits on frame m_last - 1 = (nd - 1) / prune_interval * prune_interval - 1, and
    the next call walks from its frontier back to that token: nd' - stable_frame hops.  Calls spaced so that this is 63, 64, 65 and
    128 hops -- the stop token inside partial_kernel's 64-hop chunk, as its last entry, as the first of the next chunk, and at the
    end of a second full chunk."""
    import gpu_util as G

    n_states, n_tid, interval = 400, 100, 10
    rng = np.random.default_rng(3)
    arcs = {s: [(int(rng.integers(1, n_tid + 1)), 1 + s if s % 3 == 1 else 0, float(rng.uniform(0.1, 3.0)), (s + 1) % n_states)]
            for s in range(n_states)}
    g = synth.graph_from_arc_lists(n_states, 0, arcs, {n_states - 1: 0.5})
    path = str(tmp_path / "chain.bin")
    g.write(path)
    m = synth.default_tid2pdf(n_tid)
    graph = G.wfstdec.Graph.load(path)
    graph.set_tid2pdf(m)
    h = oracle.load_graph(path)
    cd = dict(beam=9.0, max_active=1000000, min_active=0, lattice_beam=5.0, prune_interval=interval)
    cfg = pyoracle.Config(**cd)
    frames = [30, 82, 143, 204, 327]
    x = rng.normal(-2.0, 1.0, size=(340, n_tid // 2)).astype(np.float32)
    try:
        dec = make_decoder(G, graph, cd, 1, lattice, max_frames=384, arena=1 << 16, max_tok=4096, links=1 << 16)
        dev = G.upload([x])
        dec.init()
        hist, walked = History("chain"), []
        for fr in frames:
            dec.advance([dev[0].data_ptr()], [fr], n_tid // 2)
            if hist.calls:
                walked.append(fr - hist.calls[-1][3])
            words, ns, sf = dec.partial(cap_words=256)
            o = oracle.decode(h, cfg, x[:fr], m, finalize=False, use_final_probs=False)
            assert np.array_equal(words[0], o.words), "@%d: partial words != the oracle's" % fr
            hist.add(fr, words[0], ns[0], sf[0])
            assert sf[0] == ((fr - 1) // interval) * interval - 1, "@%d: stable_frame" % fr
            emitting = np.cumsum(o.path_ilabel != 0)
            assert ns[0] == int(np.sum((o.path_olabel != 0) & (o.path_ilabel != 0) & (emitting <= sf[0]))), "@%d: n_stable" % fr
        assert walked == [63, 64, 65, 128]
        dec.advance([dev[0].data_ptr()], [340], n_tid // 2)
        dec.finalize()
        fin = dec.best_paths(cap=1024)[0]["words"]
        dec.free()
        o = oracle.decode(h, cfg, x, m)
        assert np.array_equal(fin, o.words)
        hist.check_final(o.words, "the oracle's final words")
    finally:
        oracle.free_graph(h)
        graph.free()


# ---- 8: the halves, and the errors -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lattice", [False, True])
def test_halves_and_errors(synth, oracle, tmp_path, lattice):
    import gpu_util as G

    wd = G.wfstdec
    L = wd.lib()
    I32 = C.POINTER(C.c_int32)
    p = lambda a: a.ctypes.data_as(I32)
    g = synth.make_hclg_like(3000, seed=21, n_tid=600, n_words=500)
    m = synth.default_tid2pdf(600)
    path = str(tmp_path / "g.bin")
    g.write(path)
    graph = wd.Graph.load(path)
    graph.set_tid2pdf(m)
    cd = dict(beam=12.0, max_active=1000000, min_active=0, lattice_beam=6.0, prune_interval=10)
    lengths = [90, 60, 75, 40, 90, 33]
    mats = [synth.make_loglikes(g, T, 300, m, seed=500 + i, mu=-2.2)[0] for i, T in enumerate(lengths)]
    dev = G.upload(mats)
    dec = make_decoder(G, graph, cd, 6, lattice, max_frames=128, arena=1 << 20, links=1 << 21)
    with pytest.raises(wd.WfstError) as ei:   # before InitDecoding
        dec.partial([0])
    assert ei.value.code == -5
    with pytest.raises(wd.WfstError) as ei:
        dec.partial([0], cap_words=0)
    assert ei.value.code == -1
    with pytest.raises(wd.WfstError) as ei:   # nothing outstanding
        dec.partial_ready()
    assert ei.value.code == -5
    dec.init()
    words, ns, sf = dec.partial()   # no frame decoded
    assert all(len(w) == 0 for w in words) and not ns.any() and not sf.any()
    dec.advance([t.data_ptr() for t in dev], lengths, 300)
    want_w, want_ns, want_sf = dec.partial()
    bp = dec.best_paths(use_final_probs=False)
    assert all(np.array_equal(a, b["words"]) for a, b in zip(want_w, bp)) and want_ns.max() > 0
    # the halves, on a list in arbitrary order with holes, beside an outstanding best-path request
    order = np.array([4, 0, 5, 2], np.int32)
    cap = 2048
    assert L.wfst_decoder_best_path_enqueue(dec.h, p(order), 4, 0, cap) == 0
    dec.partial_enqueue(order, cap_words=64)
    with pytest.raises(wd.WfstError) as ei:   # a second one
        dec.partial_enqueue([1])
    assert ei.value.code == -5
    while not dec.partial_ready():
        pass
    w2, ns2, sf2 = dec.partial_fetch()
    il, ol = np.zeros((4, cap), np.int32), np.zeros((4, cap), np.int32)
    gr, ac = np.zeros((4, cap), np.float32), np.zeros((4, cap), np.float32)
    nh = np.zeros(4, np.int32)
    F32 = C.POINTER(C.c_float)
    assert L.wfst_decoder_best_path_fetch(dec.h, p(il), p(ol), gr.ctypes.data_as(F32), ac.ctypes.data_as(F32), p(nh)) == 0
    for i, c in enumerate(order):
        assert np.array_equal(w2[i], want_w[c]) and ns2[i] == want_ns[c] and sf2[i] == want_sf[c]
        assert np.array_equal(ol[i, : nh[i]][ol[i, : nh[i]] != 0], want_w[c])
    # NULL outputs
    assert L.wfst_decoder_get_partial(dec.h, p(order), 4, 64, None, None, None, None) == 0
    # a capacity too small: the needed size comes back
    c_long = int(np.argmax([len(w) for w in want_w]))
    need = len(want_w[c_long])
    assert need >= 2
    one = np.array([c_long], np.int32)
    wbuf, nw = np.zeros(need - 1, np.int32), np.zeros(1, np.int32)
    assert L.wfst_decoder_get_partial(dec.h, p(one), 1, need - 1, p(wbuf), p(nw), None, None) == -4
    assert nw[0] == need and np.array_equal(wbuf, want_w[c_long][: need - 1])
    # init of a reused channel starts from zero; the others keep their commit state
    dec.init([c_long])
    words, ns, sf = dec.partial([c_long, (c_long + 1) % 6])
    assert len(words[0]) == 0 and ns[0] == 0 and sf[0] == 0
    assert ns[1] == want_ns[(c_long + 1) % 6] and sf[1] == want_sf[(c_long + 1) % 6]
    short = mats[c_long][:35]
    d1 = G.upload([short])
    dec.advance([d1[0].data_ptr()], [35], 300, channels=[c_long])
    words, ns, sf = dec.partial([c_long])
    assert np.array_equal(words[0], dec.best_paths([c_long], use_final_probs=False)[0]["words"]) and sf[0] < 35
    # a finalized channel
    dec.finalize([2])
    with pytest.raises(wd.WfstError) as ei:
        dec.partial([0, 2])
    assert ei.value.code == -5
    with pytest.raises(wd.WfstError) as ei:   # a duplicate, an index out of range
        dec.partial([0, 0])
    assert ei.value.code == -1
    with pytest.raises(wd.WfstError) as ei:
        dec.partial([6])
    assert ei.value.code == -1
    dec.free()
    # biglm: refused with a message
    lmsynth = __import__("importlib").import_module("asr-decoder_amd.lmsynth")
    lm = lmsynth.make_lm(500, 2, 400, 5, 0, 0, seed=3)
    lp = str(tmp_path / "lm.bin")
    lm.to_fsa().write(lp)
    L1, L2 = wd.Lm.load(lp, -1.0), wd.Lm.load(lp, 1.0)
    db = wd.BatchDecoder(graph, wd.Config(**cd), 1, max_frames=64, max_tokens_per_frame=8192, arena_tokens=1 << 18,
                         old_lm=L1, new_lm=L2, lm_pairs=1 << 14)
    db.init()
    with pytest.raises(wd.WfstError) as ei:
        db.partial([0])
    assert ei.value.code == -1 and "biglm" in str(ei.value)
    db.free()
    L1.free()
    L2.free()
    graph.free()
