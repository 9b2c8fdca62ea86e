"""GPU: wfst_decoder_get_nbest_words -- the service's per-chunk GetNbestTxt (kaldi-nnet3/kaldi-online-nnet3-my-decoder.cc:139-150)
for a LIST of channels, live and finalized ones mixed, one launch per stage, the text made on the device (nbest_words_kernel).

The definition is by the existing calls: for every listed channel what wfst_decoder_get_nbest_paths returns at that moment, its
arcs run through wfst_lattice_to_vector.  So the reference here is a second decoder fed identically and asked channel by channel;
words are compared exactly, the three floats per path by their bytes."""
import ctypes as C

import numpy as np
import pytest

from test_compose_lattice import _setup

pytestmark = pytest.mark.gpu

CD = dict(beam=11.0, max_active=7000, min_active=0, lattice_beam=6.0, prune_interval=10)
LIMITS = dict(max_frames=64, max_tokens_per_frame=32768, arena_tokens=1 << 20, lattice_links=1 << 21)
# Eight channels: (utterance, frames).  Utterances 0..2 are _setup's, 3.. its recipe under further seeds.  A LIVE lattice is unpruned
# near the frontier, and with this data most of them outgrow the determinizer's bounds from frame 20..30 on (a loud WFST_E_CAPACITY
# after seconds of subset construction, from either call); these lengths keep every lattice asked for below within bounds and
# cheap (the last two channels: utterances 0 and 1 again, ending elsewhere).
SOURCES = [(0, 22), (1, 20), (11, 17), (9, 22), (6, 12), (4, 21), (0, 14), (1, 16)]
LENGTHS = [t for _, t in SOURCES]   # ragged: channels run out of frames at different chunks
E_CAPACITY, E_STATE = -4, -5


@pytest.fixture(scope="module")
def world(synth, tmp_path_factory):
    import gpu_util as G

    W = G.wfstdec
    g, m, gp, p1, p2, lls = _setup(synth, tmp_path_factory.mktemp("nbw"), 0)
    lls = lls + [synth.make_loglikes(g, 40, 300, m, seed=2950 + u, mu=-2.2)[0] for u in range(9)]
    lls = [np.ascontiguousarray(lls[u][:t]) for u, t in SOURCES]
    graph = W.Graph.load(gp)
    graph.set_tid2pdf(m)
    L1, L2 = W.Lm.load(p1, -1.0), W.Lm.load(p2, 1.0)
    dev = G.upload(lls)
    yield dict(W=W, G=G, graph=graph, L1=L1, L2=L2, lls=lls, dev=dev, ptrs=[t.data_ptr() for t in dev])
    L1.free()
    L2.free()
    graph.free()


def _decoder(world, n=None, **kw):
    lim = dict(LIMITS)
    lim.update(kw)
    return world["W"].BatchDecoder(world["graph"], world["G"].gpu_config(CD), n or len(world["lls"]), **lim)


def _advance(world, dec, upto, channels=None):
    ch = list(range(dec.n)) if channels is None else list(channels)
    dec.advance([world["ptrs"][c] for c in ch], [min(upto, LENGTHS[c]) for c in ch], 300, channels=None if channels is None else ch)


def _to_vector(W, p):
    """wfst_lattice_to_vector over one path's arcs, front to back, ilabel = 0: (words, tot, lm)"""
    k = len(p["olabel"])
    il = np.zeros(max(k, 1), np.int32)
    ol, gr, ac = (np.ascontiguousarray(p[x]) for x in ("olabel", "graph", "acoustic"))
    words = np.zeros(max(k, 1), np.int32)
    nw, nt = C.c_int32(0), C.c_int32(0)
    tot, lm = C.c_float(0), C.c_float(0)
    I, F = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    rc = W.lib().wfst_lattice_to_vector(il.ctypes.data_as(I), ol.ctypes.data_as(I), gr.ctypes.data_as(F), ac.ctypes.data_as(F), k,
                                        words.ctypes.data_as(I), len(words), C.byref(nw), None, 0, C.byref(nt), C.byref(tot), C.byref(lm))
    assert rc == 0
    return words[: nw.value].copy(), np.float32(tot.value), np.float32(lm.value)


def _want(W, B, c, n, lms, ufp):
    """what the definition says for channel c: B's per-channel paths through LatticeToVector"""
    try:
        return [(_to_vector(W, p), np.float32(p["tot"])) for p in B.nbest_paths(c, n, *lms, use_final_probs=ufp)]
    except W.WfstError as e:   # the channel's own failure: the list call carries it in status[i], without paths
        return e.code


def _same(got, want, what):
    status, paths = got
    if not isinstance(want, list):
        assert status == want and paths == [], "%s: status %d, per channel %d" % (what, status, want)
        return
    assert status == 0, "%s: status %d" % (what, status)
    assert len(paths) == len(want), "%s: %d paths, per channel %d" % (what, len(paths), len(want))
    for k, (p, ((words, tot, lm), ptot)) in enumerate(zip(paths, want)):
        assert np.array_equal(p["words"], words) and p["n_words"] == len(words), "%s path %d words" % (what, k)
        for name, x, y in (("path_tot", p["path_tot"], ptot), ("tot", p["tot"], tot), ("lm", p["lm"], lm)):
            assert np.float32(x).tobytes() == np.float32(y).tobytes(), "%s path %d %s: %r / %r" % (what, k, name, x, y)


def _eq_lat(x, y):
    return (x is None and y is None) or (x is not None and y is not None and all(np.array_equal(np.asarray(x[k]).view(np.int32) if k != "n_states" else x[k],
                                                                                             np.asarray(y[k]).view(np.int32) if k != "n_states" else y[k]) for k in x))


def _same_paths(x, y):
    return len(x) == len(y) and all(np.array_equal(p[k].view(np.int32), q[k].view(np.int32)) for p, q in zip(x, y) for k in ("olabel", "graph", "acoustic")) \
        and all(np.float32(p["tot"]).tobytes() == np.float32(q["tot"]).tobytes() for p, q in zip(x, y))


def test_equals_the_per_channel_calls_streaming_and_asking_changes_nothing(world):
    """Two lattice decoders fed identically, prune_interval = 10 (the running back-pruning and its compactions fall between the
    calls), 10-frame chunks over ragged lengths.  After every chunk A answers wfst_decoder_get_nbest_words for all channels in a
    non-ascending list order, n_paths in {1, 5}, with and without the LM pair, use_final_probs = 0; B answers
    wfst_decoder_get_nbest_paths channel by channel.  Then half the channels are finalized and the mixed list is asked with
    use_final_probs = 1, and once more with 0 (the finalized channels give no paths, the live ones answer).

    Then nothing A was asked has changed what it answers elsewhere: after FinalizeDecoding of the rest, a prefetch and a batched
    n-best right behind a get_nbest_words, the best paths, the determinized lattices and the n-best of every channel equal B's,
    which never called the new function, arc for arc and bit for bit."""
    W, L1, L2 = world["W"], world["L1"], world["L2"]
    A, B = _decoder(world), _decoder(world)
    n_ch = A.n
    order = [5, 2, 7, 0, 3, 6, 1, 4]
    cases = []   # (paths asked, paths got, most words on a path) per (channel, call)

    def both(ufp, calls):
        for n, lms in calls:
            got = A.nbest_words(n, channels=order, old_lm=lms[0], new_lm=lms[1], use_final_probs=ufp)
            for (i, c) in enumerate(order):
                want = _want(W, B, c, n, lms, ufp)
                _same(got[i], want, "frames %d channel %d n %d lms %s ufp %d" % (A.num_frames_decoded(c), c, n, lms[0] is not None, ufp))
                want = want if isinstance(want, list) else []
                cases.append((n, len(want), max([len(w[0][0]) for w in want] or [0])))

    calls = [(n, lms) for n in (1, 5) for lms in ((None, None), (L1, L2))]
    for d in (A, B):
        d.init()
    for upto in (10, 20, 30):
        for d in (A, B):
            _advance(world, d, upto)
        both(False, calls)
    done = [0, 2, 4, 6]
    for d in (A, B):
        d.finalize(channels=done)
    both(True, calls)
    n_before = len(cases)
    both(False, [(5, (None, None))])
    for (i, c) in enumerate(order):
        assert (cases[n_before + i][1] == 0) == (c in done), "use_final_probs = 0: finalized channels have no lattice, live ones answer"
    # the conditions on the data (B alone decides them)
    two = sum(1 for (n, k, w) in cases if k >= 2)
    worded = sum(1 for (n, k, w) in cases if w >= 1)
    fewer = sum(1 for (n, k, w) in cases if k < n)
    print("cases %d: >= 2 paths %d, a path with words %d, fewer paths than asked %d" % (len(cases), two, worded, fewer))
    assert 2 * two >= len(cases) and 2 * worded >= len(cases) and fewer >= 1
    # ---- asking changed nothing
    rest = [c for c in range(n_ch) if c not in done]
    for d in (A, B):
        d.finalize(channels=rest)
    got = A.nbest_words(5, channels=order)
    for (i, c) in enumerate(order):
        _same(got[i], _want(W, B, c, 5, (None, None), True), "finalized, channel %d" % c)
    A.prefetch_determinized()   # (the slots the call above filled are the prefetch's now)
    A.nbest_paths_batch(5)
    for c in range(n_ch):
        assert _same_paths(A.nbest_paths(c, 5), B.nbest_paths(c, 5)), "batch behind get_nbest_words, channel %d" % c
    got = A.nbest_words(3, old_lm=L1, new_lm=L2)   # (ascending list: the slots hold these very lattices since the prefetch)
    for c in range(n_ch):
        _same(got[c], _want(W, B, c, 3, (L1, L2), True), "behind the batch, channel %d" % c)
    bpa, bpb = A.best_paths(), B.best_paths()
    for c in range(n_ch):
        for k in ("words", "tids", "olabel", "ilabel"):
            assert np.array_equal(bpa[c][k], bpb[c][k]), (c, k)
        for k in ("graph", "ac"):
            assert np.array_equal(bpa[c][k].view(np.int32), bpb[c][k].view(np.int32)), (c, k)
        assert _eq_lat(A.determinized_lattice(c), B.determinized_lattice(c)), "determinized lattice, channel %d" % c
        for n, lms in ((5, (None, None)), (4, (L1, L2))):
            assert _same_paths(A.nbest_paths(c, n, *lms), B.nbest_paths(c, n, *lms)), "n-best %d, channel %d" % (n, c)
    A.free()
    B.free()


def test_a_live_channels_cached_lattice_survives(world):
    """wfst_decoder_get_determinized_lattice keeps a live channel's result until the channel moves on; a get_nbest_words in between
    (which determinizes the same channel into a workspace slot) leaves the next fetch what it was."""
    A, B = _decoder(world, 3), _decoder(world, 3)
    for d in (A, B):
        d.init()
        _advance(world, d, 20)
    first = A.determinized_lattice(1, use_final_probs=False)
    assert first is not None
    A.nbest_words(5, channels=[2, 1, 0], use_final_probs=False)
    assert _eq_lat(A.determinized_lattice(1, use_final_probs=False), first)
    assert _eq_lat(first, B.determinized_lattice(1, use_final_probs=False))
    assert _same_paths(A.nbest_paths(0, 5, use_final_probs=False), B.nbest_paths(0, 5, use_final_probs=False))
    A.free()
    B.free()


def test_more_channels_than_determinizer_slots(world):
    """det_workspace_bytes that buys 2 slots, 5 channels listed: three rounds, the results those of a roomy decoder."""
    L1, L2 = world["L1"], world["L2"]
    roomy = _decoder(world, 6)
    slots, per = roomy.determinizer_slots()
    assert slots == 6
    tight = _decoder(world, 6, det_workspace_bytes=2 * per + per // 2)
    assert tight.determinizer_slots() == (2, per)
    for d in (roomy, tight):
        d.init()
        _advance(world, d, 20)
        d.finalize(channels=[3])
    listed = [4, 2, 0, 3, 1]
    n_paths = 0
    for lms in ((None, None), (L1, L2)):
        a = tight.nbest_words(5, channels=listed, old_lm=lms[0], new_lm=lms[1])
        b = roomy.nbest_words(5, channels=listed, old_lm=lms[0], new_lm=lms[1])
        for (sa, pa), (sb, pb), c in zip(a, b, listed):
            assert sa == sb == 0 and len(pa) == len(pb), c
            for p, q in zip(pa, pb):
                assert np.array_equal(p["words"], q["words"]), c
                assert all(np.float32(p[k]).tobytes() == np.float32(q[k]).tobytes() for k in ("tot", "lm", "path_tot")), c
            n_paths += len(pa)
    assert n_paths >= 2 * len(listed)
    for d in (roomy, tight):
        d.free()


def test_per_channel_status_and_whole_call_errors(world):
    W, L1 = world["W"], world["L1"]
    dec = _decoder(world, 6)
    dec.init(channels=[0, 1, 2, 3, 4])
    _advance(world, dec, 20, channels=[0, 1, 2, 3, 4])
    listed = [3, 0, 4, 1, 2]
    full = dec.nbest_words(5, channels=listed, use_final_probs=False)
    assert all(s == 0 for s, _ in full)
    longest = max(p["n_words"] for _, paths in full for p in paths)
    assert longest >= 2
    cap = longest - 1
    cut = dec.nbest_words(5, channels=listed, use_final_probs=False, cap_words=cap)   # (returns: the call itself is WFST_OK)
    n_short = 0
    for (s, paths), (_, ref), c in zip(cut, full, listed):
        over = any(p["n_words"] > cap for p in ref)
        assert s == (E_CAPACITY if over else 0), c
        n_short += not over
        assert len(paths) == len(ref)
        for p, q in zip(paths, ref):
            assert p["n_words"] == q["n_words"] and np.array_equal(p["words"], q["words"][:cap]), c
            assert p["tot"].tobytes() == q["tot"].tobytes() and p["path_tot"].tobytes() == q["path_tot"].tobytes()
    print("cap_words %d: %d of %d channels within it" % (cap, n_short, len(listed)))
    # whole-call errors: nothing is computed
    for kw, code in ((dict(n_paths=0), -1), (dict(n_paths=65), -1), (dict(n_paths=5, old_lm=L1), -1), (dict(n_paths=5, cap_words=0), -1),
                     (dict(n_paths=5, channels=[0, 0]), -1), (dict(n_paths=5, channels=[0, 6]), -1), (dict(n_paths=5, channels=[0, 5]), E_STATE)):
        with pytest.raises(W.WfstError) as e:
            dec.nbest_words(**kw)
        assert e.value.code == code, kw
    # the batched post-processing of FINALIZED channels keeps refusing a live one
    with pytest.raises(W.WfstError) as e:
        dec.nbest_paths_batch(5, channels=[0])
    assert e.value.code == E_STATE
    dec.free()
    plain = _decoder(world, 2, lattice_links=0)
    plain.init()
    _advance(world, plain, 10)
    with pytest.raises(W.WfstError) as e:
        plain.nbest_words(5)
    assert e.value.code == E_STATE
    plain.free()
