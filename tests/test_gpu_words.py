"""-m gpu: an utterance's words, word times and scores in one launch (wfst_decoder_get_words and its halves; words_kernel).

The oracle of every test is the project's older path on the same channel at the same moment: wfst_decoder_get_best_path, then
wfst_lattice_to_vector_batch / wfst_lattice_labels_batch (BatchDecoder.best_paths), then the definitions of
include/wfst_decoder.h in a few lines of numpy (expected()).  Words, begin and end frames and hop counts must be equal, the
two scores equal bit for bit; there are no tolerances."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from golden_util import GOLDEN_DIR, Golden, bits

pytestmark = pytest.mark.gpu

I32, F32 = C.POINTER(C.c_int32), C.POINTER(C.c_float)
pi = lambda a: a.ctypes.data_as(I32)
pf = lambda a: a.ctypes.data_as(F32)


def expected(bp, sil_tids=None):
    """(words, begin, end, n_hops) of one best_paths() entry; sil_tids: the silence transition-ids, None: no silence list"""
    il, ol = np.asarray(bp["ilabel"]), np.asarray(bp["olabel"])
    H = len(il)
    emit = il != 0
    F = np.cumsum(emit) - emit           # F(j): emitting hops before hop j
    E = int(emit.sum())
    j = np.nonzero(ol)[0]
    begin = F[j]
    end = np.zeros(len(j), np.int64)
    for k in range(len(j)):
        hi = j[k + 1] if k + 1 < len(j) else H
        if sil_tids is None:
            end[k] = begin[k + 1] if k + 1 < len(j) else E
        else:
            seg = np.arange(j[k], hi)
            keep = seg[emit[seg] & ~np.isin(il[seg], sil_tids)]
            end[k] = 1 + F[keep].max() if len(keep) else begin[k]
    return ol[j], begin, end, H


def check(dec, channels, use_final_probs, sil_tids=None, cap_words=1024, cap=2048, what=""):
    """words() of the listed channels against best_paths() of the same channels now; returns the oracle's (bp, expected) pairs"""
    bps = dec.best_paths(channels, use_final_probs=use_final_probs, cap=cap)
    got = dec.words(channels, use_final_probs=use_final_probs, cap_words=cap_words)
    assert len(got) == len(bps)
    out = []
    for i, (g, bp) in enumerate(zip(got, bps)):
        w, b, e, H = expected(bp, sil_tids)
        tag = "%s list entry %d" % (what, i)
        assert g[5] == H, tag + " n_hops"
        assert np.array_equal(g[0], w), tag + " words"
        assert np.array_equal(g[1], b), tag + " begin frames"
        assert np.array_equal(g[2], e), tag + " end frames"
        assert np.array_equal(bits([g[3], g[4]]), bits([bp["tot_score"], bp["lm_score"]])), tag + " scores"
        if H == 0:   # the reference's "no path"
            assert len(g[0]) == 0 and bits([g[3], g[4]]).tolist() == [0, 0], tag
        out.append((bp, (w, b, e, H)))
    return out


def two_points(T, prune_interval):
    """two chunk boundaries below T frames, one of them not a multiple of prune_interval"""
    pts = []
    for p in (prune_interval, prune_interval + 7, max(1, T // 3), max(2, T // 2), 1):
        if 0 < p < T and p not in pts:
            pts.append(p)
    pts = sorted(pts[:2])
    assert len(pts) == 2 and any(p % prune_interval for p in pts), (T, prune_interval)
    return pts


def run_workload(G, dec, mats, prune_interval, what):
    """mid-utterance at two chunk boundaries (use_final_probs = 0), then after FinalizeDecoding (use_final_probs = 1)"""
    T = [int(m.shape[0]) for m in mats]
    dev = G.upload(mats)
    ptrs = [t.data_ptr() for t in dev]
    stride = int(mats[0].shape[1])
    dec.init()
    seen = []
    for r in two_points(max(T), prune_interval):
        dec.advance(ptrs, [min(r, t) for t in T], stride)
        seen += check(dec, None, False, what="%s @%d" % (what, r))
    dec.advance(ptrs, T, stride)
    dec.finalize()
    seen += check(dec, None, True, what=what + " final")
    return seen


def wordy_graph(synth, n_states, seed, plain_every):
    """make_hclg_like's graph with a word on every emitting arc but each plain_every-th (those stay as they were)"""
    g = synth.make_hclg_like(n_states, seed=seed, n_tid=600, n_words=500)
    arcs = g.arcs
    put = (arcs["ilabel"] != 0) & ((np.arange(len(arcs)) % plain_every) != 0)
    arcs["olabel"][put] = 1 + (np.nonzero(put)[0] % 500).astype(np.int32)
    S = len(g.state_info) - 1
    src = np.repeat(np.arange(S, dtype=np.int64), g.state_info["num_arcs"][:S])
    g.state_info["noepsilons"][:S] = np.bincount(src[arcs["olabel"] == 0], minlength=S)
    return g


# ---- 1. the golden graphs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lattice", [False, True])
@pytest.mark.parametrize("name", ["hclg600", "eps_chains", "quirk_parallel_arcs", "no_final", "dead_end"])
def test_golden_workloads(name, lattice, tmp_path):
    import gpu_util as G

    g = Golden(name)
    graph = G.wfstdec.Graph.load(g.write_graph(str(tmp_path / "g.bin")))
    if g.tid2pdf is not None:
        graph.set_tid2pdf(g.tid2pdf)
    c0 = g.meta["cases"][0]
    cd = dict(g.meta["cfgs"][c0["cfg"]])
    utts = sorted(set(c["utt"] for c in g.meta["cases"] if c["cfg"] == c0["cfg"] and c["mode"] == c0["mode"]))
    mats = [g.utts[u] for u in utts]
    lim = dict(max_frames=512, max_tokens_per_frame=32768, arena_tokens=1 << 22)
    if lattice:
        lim["lattice_links"] = 1 << 21
    dec = G.wfstdec.BatchDecoder(graph, G.gpu_config(cd), len(mats), **lim)
    try:
        seen = run_workload(G, dec, mats, int(G.gpu_config(cd).prune_interval), name)
    finally:
        dec.free()
        graph.free()
    hops = [e[3] for _, e in seen]
    if name == "dead_end":
        assert 0 in hops   # (check() holds n_words = 0 and both scores 0 there)
    else:
        assert max(hops) > 0 and any(len(e[0]) > 0 for _, e in seen)
    if name == "eps_chains":   # words on epsilon hops: a word that begins where the one before it began
        assert any((np.diff(e[1]) == 0).any() for _, e in seen if len(e[1]) > 1)


def test_biglm_golden_workload(tmp_path):
    import gpu_util as G

    z = np.load(os.path.join(GOLDEN_DIR, "biglm_hclg600.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    with open(tmp_path / "g.bin", "wb") as f:
        f.write(bytes(z["graph"]))
    graph = G.wfstdec.Graph.load(str(tmp_path / "g.bin"))
    graph.set_tid2pdf(z["tid2pdf"])
    mats = [z["ll_%d" % i] for i in range(int(z["n_utt"]))]
    lms = []
    try:
        for pname in meta["pairs"]:
            pair = []
            for tag, scale in (("old", -1.0), ("new", 1.0)):
                p = str(tmp_path / ("lm_%s_%s.bin" % (pname, tag)))
                with open(p, "wb") as f:
                    f.write(bytes(z["lm_%s_%s" % (pname, tag)]))
                pair.append(G.wfstdec.Lm.load(p, scale))
            lms += pair
            cd = dict(meta["cfgs"][0])
            dec = G.wfstdec.BatchDecoder(graph, G.gpu_config(cd), len(mats), old_lm=pair[0], new_lm=pair[1], max_frames=512,
                                         max_tokens_per_frame=32768, arena_tokens=1 << 21)
            try:
                seen = run_workload(G, dec, mats, int(G.gpu_config(cd).prune_interval), "biglm " + pname)
            finally:
                dec.free()
            assert any(len(e[0]) > 0 for _, e in seen)
            # LM-carrying graph costs: a hop's graph cost is not the arc's alone, so lm_score differs from the plain decoder's
            assert any(bp["lm_score"] != 0.0 for bp, _ in seen)
    finally:
        for lm in lms:
            lm.free()
        graph.free()


# ---- 2. silence trimming ----------------------------------------------------------------------------------------------------
SIL_N_TID = 600
SIL_SEED = 41
SIL_CD = dict(beam=12.0, max_active=1000000, min_active=0, lattice_beam=6.0, prune_interval=10)


def silence_tables():
    t2p = (1 + np.arange(SIL_N_TID + 1, dtype=np.int32) % 30).astype(np.int32)   # 30 phones; 1..10 are silence: a third of the tids
    phones = np.arange(1, 11, dtype=np.int32)
    tids = np.nonzero(np.isin(t2p, phones))[0]
    return t2p, phones, tids[tids > 0]


def silence_workload(synth):
    g = wordy_graph(synth, 1000, 5, 2)   # a word on every other emitting arc: short words, some of them all silence
    m = synth.default_tid2pdf(SIL_N_TID)
    return g, m, synth.make_loglikes(g, 120, SIL_N_TID // 2, m, seed=SIL_SEED, mu=-2.2)[0]


@pytest.mark.parametrize("lattice", [False, True])
def test_silence_list_trims_word_ends(lattice, synth, tmp_path):
    import gpu_util as G

    wd = G.wfstdec
    g, m, x = silence_workload(synth)
    t2p, phones, sil_tids = silence_tables()
    path = str(tmp_path / "g.bin")
    g.write(path)
    graph = wd.Graph.load(path)
    graph.set_tid2pdf(m)
    lim = dict(max_frames=128, max_tokens_per_frame=32768, arena_tokens=1 << 20)
    if lattice:
        lim["lattice_links"] = 1 << 21
    dec = wd.BatchDecoder(graph, G.gpu_config(SIL_CD), 1, **lim)
    try:
        with pytest.raises(wd.WfstError) as ei:   # no tid2phone yet
            dec.set_silence_phones(phones)
        assert ei.value.code == -5
        graph.set_tid2phone(t2p)
        for bad in ([3, 3], [0, 2], [-1]):
            with pytest.raises(wd.WfstError) as ei:
                dec.set_silence_phones(bad)
            assert ei.value.code == -1
        dev = G.upload([x])
        dec.init()
        dec.advance([dev[0].data_ptr()], [73], x.shape[1])
        for final in (False, True):
            if final:
                dec.advance([dev[0].data_ptr()], [x.shape[0]], x.shape[1])
                dec.finalize()
            dec.set_silence_phones(phones)
            (_, trimmed), = check(dec, [0], final, sil_tids, what="silence list set")
            dec.set_silence_phones([])
            (_, plain), = check(dec, [0], final, None, what="silence list cleared")
            assert np.array_equal(trimmed[0], plain[0]) and np.array_equal(trimmed[1], plain[1])
            assert (trimmed[2] != plain[2]).any(), "no word end moved by the silence list"
            assert (trimmed[2] == trimmed[1]).any(), "no word without a non-silence frame"
        # the endpoint configuration sets the list too (plain decoders)
        dec.set_endpoint_config(wd.EndpointConfig(silence_phones=[int(p) for p in phones]))
        check(dec, [0], True, sil_tids, what="silence list of the endpoint config")
    finally:
        dec.free()
        graph.free()


# ---- 3. packing across strides ----------------------------------------------------------------------------------------------
def test_more_words_than_one_stride_and_a_small_capacity(synth, tmp_path):
    import gpu_util as G

    wd = G.wfstdec
    g = wordy_graph(synth, 300, 31, 5)          # four emitting arcs in five carry a word
    m = synth.default_tid2pdf(600)
    T = 600
    x = synth.make_loglikes(g, T, 300, m, seed=90, mu=-2.2)[0]
    path = str(tmp_path / "g.bin")
    g.write(path)
    graph = wd.Graph.load(path)
    graph.set_tid2pdf(m)
    dec = wd.BatchDecoder(graph, G.gpu_config(dict(beam=6.0, max_active=1000000, min_active=0, lattice_beam=4.0)), 1,
                          max_frames=T + 8, max_tokens_per_frame=8192, arena_tokens=1 << 20)
    try:
        dev = G.upload([x])
        dec.init()
        dec.advance([dev[0].data_ptr()], [T], x.shape[1])
        dec.finalize()
        (bp, (w, b, e, H)), = check(dec, [0], True, what="600 frames")
        assert len(w) > 256 and H > 512
        # cap_words = 100: the needed size, the first 100 words and times, the scores and the hop count
        L = wd.lib()
        one = np.array([0], np.int32)
        words, begin, end = np.zeros(100, np.int32), np.zeros(100, np.int32), np.zeros(100, np.int32)
        nw, nh = np.zeros(1, np.int32), np.zeros(1, np.int32)
        tot, lm = np.zeros(1, np.float32), np.zeros(1, np.float32)
        rc = L.wfst_decoder_get_words(dec.h, pi(one), 1, 1, 100, pi(words), pi(begin), pi(end), pi(nw), pi(nh), pf(tot), pf(lm))
        assert rc == -4
        assert nw[0] == len(w) and nh[0] == H
        assert np.array_equal(words, w[:100]) and np.array_equal(begin, b[:100]) and np.array_equal(end, e[:100])
        assert np.array_equal(bits([tot[0], lm[0]]), bits([bp["tot_score"], bp["lm_score"]]))
        # NULL outputs
        assert L.wfst_decoder_get_words(dec.h, pi(one), 1, 1, 1024, None, None, None, None, None, None, None) == 0
    finally:
        dec.free()
        graph.free()


# ---- 4. beyond both LDS tables (the workload shape of tests/test_gpu_traceback_long.py) ---------------------------------------
@pytest.mark.parametrize("lattice", [False, True])
def test_path_beyond_both_lds_tables(lattice, synth, tmp_path):
    import gpu_util as G

    wd = G.wfstdec
    n_tid, T, T_MID = 600, 4200, 4150   # > kBpFrames = 3072; T_MID > kBpChainLds = 4096 too
    cd = dict(beam=6.0, max_active=1000000, min_active=0, lattice_beam=4.0)
    g = synth.make_hclg_like(300, seed=31, n_tid=n_tid, n_words=500)
    m = synth.default_tid2pdf(n_tid)
    path = str(tmp_path / "g.bin")
    g.write(path)
    x = synth.make_loglikes(g, T, n_tid // 2, m, seed=90, mu=-2.2)[0]
    graph = wd.Graph.load(path)
    graph.set_tid2pdf(m)
    graph.set_tid2phone((1 + np.arange(n_tid + 1, dtype=np.int32) % 3).astype(np.int32))
    sil_tids = np.arange(3, n_tid + 1, 3)   # phone 1
    lim = dict(max_frames=T + 56, max_tokens_per_frame=8192, arena_tokens=1 << 20)
    if lattice:
        lim["lattice_links"] = 1 << 21
    dec = wd.BatchDecoder(graph, G.gpu_config(cd), 1, **lim)
    try:
        dev = G.upload([x])
        dec.init()
        dec.advance([dev[0].data_ptr()], [100], x.shape[1])
        check(dec, [0], False, cap=8192, what="@100 (before the walk needs scratch)")
        dec.advance([dev[0].data_ptr()], [T_MID], x.shape[1])
        (_, e), = check(dec, [0], False, cap=8192, what="@%d (the scratch grows, the list runs again)" % T_MID)
        assert e[3] > 4096
        dec.set_silence_phones([1])
        check(dec, [0], False, sil_tids, cap=8192, what="@%d with a silence list" % T_MID)
        dec.advance([dev[0].data_ptr()], [T], x.shape[1])
        dec.finalize()
        (_, e), = check(dec, [0], True, sil_tids, cap=8192, what="final")
        assert e[3] > 4096
    finally:
        dec.free()
        graph.free()


# ---- 5. a list --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lattice", [False, True])
def test_list_of_channels_in_two_halves(lattice, synth, tmp_path):
    import gpu_util as G

    wd = G.wfstdec
    L = wd.lib()
    g = synth.make_hclg_like(3000, seed=21, n_tid=600, n_words=500)
    m = synth.default_tid2pdf(600)
    path = str(tmp_path / "g.bin")
    g.write(path)
    graph = wd.Graph.load(path)
    graph.set_tid2pdf(m)
    cd = dict(beam=12.0, max_active=1000000, min_active=0, lattice_beam=6.0, prune_interval=10)
    lengths = [90, 60, 75, 33]           # channels 1..4; channel 0 decodes no frame
    mats = [synth.make_loglikes(g, T, 300, m, seed=500 + i, mu=-2.2)[0] for i, T in enumerate(lengths)]
    dev = G.upload(mats)
    lim = dict(max_frames=128, max_tokens_per_frame=32768, arena_tokens=1 << 20)
    if lattice:
        lim["lattice_links"] = 1 << 21
    dec = wd.BatchDecoder(graph, G.gpu_config(cd), 5, **lim)
    try:
        with pytest.raises(wd.WfstError) as ei:   # before InitDecoding
            dec.words([0])
        assert ei.value.code == -5
        with pytest.raises(wd.WfstError) as ei:   # nothing outstanding
            dec.words_ready()
        assert ei.value.code == -5
        dec.init()
        with pytest.raises(wd.WfstError) as ei:
            dec.words([0], cap_words=0)
        assert ei.value.code == -1
        dec.advance([t.data_ptr() for t in dev], lengths, 300, channels=[1, 2, 3, 4])
        order = np.array([3, 0, 4, 1, 2], np.int32)
        seen = check(dec, order, False, what="one-shot")
        assert seen[1][1][3] == 0 and all(e[3] > 0 for i, (_, e) in enumerate(seen) if i != 1)
        want = dec.words(order, use_final_probs=False)
        # the halves, beside an outstanding best-path request
        cap = 2048
        assert L.wfst_decoder_best_path_enqueue(dec.h, pi(order), 5, 0, cap) == 0
        dec.words_enqueue(order, use_final_probs=False)
        with pytest.raises(wd.WfstError) as ei:   # a second one
            dec.words_enqueue([1], use_final_probs=False)
        assert ei.value.code == -5
        with pytest.raises(wd.WfstError) as ei:   # the list it reads
            dec.set_silence_phones([])
        assert ei.value.code == -5
        while not dec.words_ready():
            pass
        got = dec.words_fetch()
        il, ol = np.zeros((5, cap), np.int32), np.zeros((5, cap), np.int32)
        gr, ac = np.zeros((5, cap), np.float32), np.zeros((5, cap), np.float32)
        nh = np.zeros(5, np.int32)
        assert L.wfst_decoder_best_path_fetch(dec.h, pi(il), pi(ol), pf(gr), pf(ac), pi(nh)) == 0
        for i in range(5):
            for a, b in zip(got[i][:3], want[i][:3]):
                assert np.array_equal(a, b)
            assert bits([got[i][3], got[i][4]]).tolist() == bits([want[i][3], want[i][4]]).tolist() and got[i][5] == want[i][5] == nh[i]
            assert np.array_equal(ol[i, : nh[i]][ol[i, : nh[i]] != 0], got[i][0])
        # the use_final_probs rule after FinalizeDecoding
        dec.finalize([2])
        with pytest.raises(wd.WfstError) as ei:
            dec.words([1, 2], use_final_probs=False)
        assert ei.value.code == -5
        check(dec, [2], True, what="finalized channel")
    finally:
        dec.free()
        graph.free()


# ---- 6. the host mirror -----------------------------------------------------------------------------------------------------
def test_host_mirror_prints_the_frames_of_the_python_path(tmp_path):
    """wfst-decode --word-times in the batch shape (GpuBatchDecoder::GetWords) and with --single-stream
    (GpuLatticeDecoder::GetWords), without and with silence phones, on the hclg600 workload"""
    import struct
    import subprocess

    import gpu_util as G

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cli = os.path.join(root, "asr-decoder_amd", "host", "wfst-decode")
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(cli)])
    g = Golden("hclg600")
    c0 = g.meta["cases"][0]
    cd = dict(g.meta["cfgs"][c0["cfg"]])
    mats = g.utts
    gpath = g.write_graph(str(tmp_path / "g.bin"))
    g.tid2pdf.astype("<i4").tofile(str(tmp_path / "tid2pdf.bin"))
    n_tid = len(g.tid2pdf) - 1
    t2p = (1 + np.arange(n_tid + 1, dtype=np.int32) % 30).astype("<i4")
    t2p.tofile(str(tmp_path / "tid2phone.bin"))
    phones = list(range(1, 11))
    (tmp_path / "decoder.conf").write_text("--beam=%g\n--max-active=%d\n--min-active=%d\n--lattice-beam=%g\n"
                                           % (cd["beam"], cd["max_active"], cd["min_active"], cd["lattice_beam"]))
    with open(tmp_path / "ll.bin", "wb") as f:
        for i, x in enumerate(mats):
            key = ("utt%03d" % i).encode()
            f.write(struct.pack("<i", len(key)) + key + struct.pack("<ii", x.shape[0], x.shape[1]) + np.ascontiguousarray(x, np.float32).tobytes())
    # the Python path
    graph = G.wfstdec.Graph.load(gpath)
    graph.set_tid2pdf(g.tid2pdf)
    graph.set_tid2phone(t2p)
    dec = G.wfstdec.BatchDecoder(graph, G.gpu_config(cd), len(mats), max_frames=512, max_tokens_per_frame=32768, arena_tokens=1 << 22)
    try:
        dev = G.upload(mats)
        dec.init()
        dec.advance([t.data_ptr() for t in dev], [m.shape[0] for m in mats], mats[0].shape[1])
        dec.finalize()
        want = {False: dec.words()}
        dec.set_silence_phones(phones)
        want[True] = dec.words()
    finally:
        dec.free()
        graph.free()
    assert any((a[2] != b[2]).any() for a, b in zip(want[False], want[True]))
    head = [cli, "--tid2pdf=" + str(tmp_path / "tid2pdf.bin")]
    tail = [str(tmp_path / "decoder.conf"), gpath, str(tmp_path / "ll.bin")]
    plain = subprocess.run(head + tail, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stderr[-2000:]
    for shape in ([], ["--single-stream"]):
        for sil in (False, True):
            extra = ["--word-times"] + (["--silence-phones=" + ":".join(map(str, phones)), "--tid2phone=" + str(tmp_path / "tid2phone.bin")] if sil else [])
            p = subprocess.run(head + shape + extra + tail, capture_output=True, text=True, timeout=300)
            assert p.returncode == 0, p.stderr[-2000:]
            lines = p.stdout.splitlines()
            assert [l for l in lines if "#" not in l.split()[0]] == plain.stdout.splitlines()   # the other lines are unchanged
            for i, w in enumerate(want[sil]):
                got = [[int(v) for v in l.split()[1:]] for l in lines if l.startswith("utt%03d#" % i)]
                assert got == [[int(a), int(b), int(c)] for a, b, c in zip(w[0], w[1], w[2])], (shape, sil, i)
                assert len(got) > 0
