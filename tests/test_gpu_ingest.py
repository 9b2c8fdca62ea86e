"""-m gpu: acoustic-model chunks ingested on the device (wfst_decoder_set_score_transform / _advance_chunk / _get_scores,
ingest_kernel): float16 / bfloat16 / float32 rows where the model left them, (x - log_prior) * acoustic_scale in float32, into the
decoder-owned history, then the search.

Bars: the ingested scores equal numpy's float32 arithmetic bit for bit on every bit pattern; decoding through the chunk path equals
the reference-made goldens (float32, scale 1), the oracle on the host-transformed matrix and `advance` on that matrix, bit for
bit, for every decoder kind, layout, stream ordering, restart and mix with advance_host; every error of the header leaves the
decoder usable.  Where max_active / min_active bind, the oracle runs order-free, as in tests/test_gpu_golden.py."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import pyoracle
from golden_util import GOLDEN_DIR, Golden, bits, check_result

pytestmark = pytest.mark.gpu

LIM = dict(max_frames=512, max_tokens_per_frame=32768, arena_tokens=1 << 22)
SCALE = 0.1


def _beam_only(cd):
    return cd["max_active"] >= 100000 and cd["min_active"] == 0


@pytest.fixture(scope="module")
def env(tmp_path_factory, oracle):
    import gpu_util as G
    import torch

    g = Golden("hclg600")
    path = g.write_graph(str(tmp_path_factory.mktemp("ingest") / "g.bin"))
    graph = G.wfstdec.Graph.load(path)
    graph.set_tid2pdf(g.tid2pdf)
    h = oracle.load_graph(path)
    prior = np.random.RandomState(20).normal(-5.0, 1.5, 300).astype(np.float32)
    e = dict(G=G, W=G.wfstdec, torch=torch, g=g, graph=graph, h=h, path=path, prior=prior, cache={})
    yield e
    graph.free()
    oracle.free_graph(h)


def _torch_dtype(torch, dt):
    return dict(f32=torch.float32, f16=torch.float16, bf16=torch.bfloat16)[dt]


def _raw_and_scores(env, dt, utts=None, prior=None):
    """The model's raw output y = (x / 0.1 + prior) in the half type (device tensors), and what the transform makes of it on the
    host in float32: (float32(y) - prior) * float32(0.1)."""
    torch = env["torch"]
    prior = env["prior"] if prior is None else prior
    raw, host = [], []
    for x in (env["g"].utts if utts is None else utts):
        y = torch.from_numpy((x / np.float32(SCALE) + prior).astype(np.float32)).to(_torch_dtype(torch, dt))
        raw.append(y.to("cuda:0"))
        host.append(((y.float().numpy() - prior) * np.float32(SCALE)).astype(np.float32))
    return raw, host


def _feed(dec, raw, chunk=7, stream="current", channels=None, after=None, make=None):
    """The utterances in ragged chunks: channel c gets chunk + c rows per call, one entry per call has none (None and an empty
    tensor in turn)."""
    B = len(raw)
    T = [int(t.shape[0]) for t in raw]
    have = [0] * B
    call = 0
    while any(have[c] < T[c] for c in range(B)):
        ks = [min(chunk + c, T[c] - have[c]) for c in range(B)]
        z = call % B
        if sum(1 for c in range(B) if ks[c] > 0 and c != z):
            ks[z] = 0
        chunks = []
        for c in range(B):
            rows = raw[c][have[c]:have[c] + ks[c]]
            if make is not None and ks[c]:
                rows = make(c, rows)
            chunks.append(None if (ks[c] == 0 and call % 2 == 0 and sum(ks) > 0) else rows)
            have[c] += ks[c]
        dec.advance_chunk(chunks, channels=channels, stream=stream)
        if after is not None:
            after(chunks)
        call += 1


def _chunk_decode(env, dec, raw, finalize=True, use_final_probs=True, **kw):
    dec.init()
    _feed(dec, raw, **kw)
    if finalize:
        dec.finalize()
    return [env["G"].GpuResult(d) for d in dec.best_paths(use_final_probs=use_final_probs)]


def _same(G, got, want, what):
    for c, (y, x) in enumerate(zip(got, want)):
        assert bool(y.ok) == bool(x.ok), what
        G.assert_same_path(y, x.words, x.tids, x.path_ilabel, x.path_olabel, x.path_graph, x.path_ac, [x.tot_score, x.lm_score], "%s channel %d" % (what, c))


def _want(env, dt, ci):
    """Item 3's results: `advance` on the host-transformed matrices (computed once per dtype and config)."""
    key = (dt, ci)
    if key not in env["cache"]:
        _, host = _raw_and_scores(env, dt)
        env["cache"][key] = env["G"].decode_batch(env["graph"], dict(env["g"].meta["cfgs"][ci]), host)
    return env["cache"][key]


def _golden_check(env, dec, ci=0):
    """Item 2 for one configuration on `dec` (3 channels): float32 chunks, scale 1, no priors, against the reference-made golden."""
    g, torch = env["g"], env["torch"]
    cd = dict(g.meta["cfgs"][ci])
    raw = [torch.from_numpy(x).to("cuda:0") for x in g.utts]
    n = 0
    for mi, md in enumerate(g.meta["modes"]):
        md = dict(md)
        md.pop("trace", None)
        md.pop("chunk", None)
        res = _chunk_decode(env, dec, raw, **md)
        for k, c in enumerate(g.meta["cases"]):
            if c["cfg"] == ci and c["mode"] == mi:
                check_result(res[c["utt"]], g.expected(k), "case %d" % k, check_counts=False)
                n += 1
    assert n > 0


# ---- 1. every bit pattern ------------------------------------------------------------------------------------------------------
def _np_expect(x32, prior, scale):
    with np.errstate(all="ignore"):
        y = x32 if prior is None else x32 - prior[None, :]
        return (y if scale == 1.0 else y * np.float32(scale)).astype(np.float32)


def _assert_bits(got, want, what):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what + ": NaN positions"
    assert np.array_equal(bits(got)[~nan], bits(want)[~nan]), what + ": %d elements differ" % int((bits(got)[~nan] != bits(want)[~nan]).sum())


@pytest.mark.parametrize("case", ["plain", "scaled", "scaled_priors"])
@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
def test_every_bit_pattern(env, dt, case):
    torch, W = env["torch"], env["W"]
    scale = 1.0 if case == "plain" else SCALE
    prior = np.random.RandomState(5).normal(-4.0, 2.0, 1024).astype(np.float32) if case == "scaled_priors" else None
    if dt == "f32":
        rs = np.random.RandomState(11)
        x32 = (rs.standard_normal((64, 1024)) * 10.0 ** rs.uniform(-44, 38, (64, 1024))).astype(np.float32)
        x32[0, :8] = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1.1754942e-38, -5e-42], np.float32)   # +-0, +-inf, denormals
        x32[1] = rs.randint(0, 1 << 23, 1024).astype(np.uint32).view(np.float32)   # a row of denormals
        t = torch.from_numpy(x32).to("cuda:0")
    else:
        u16 = np.arange(65536, dtype=np.uint16).reshape(64, 1024)
        x32 = u16.view(np.float16).astype(np.float32) if dt == "f16" else (u16.astype(np.uint32) << 16).view(np.float32)
        t = torch.from_numpy(u16.view(np.int16)).to("cuda:0").view(_torch_dtype(torch, dt))
    dec = W.BatchDecoder(env["graph"], env["G"].gpu_config(dict(beam=13.0)), 1, **LIM)
    try:
        dec.set_score_transform(scale, prior)
        dec.init()
        dec.advance_chunk([t], max_num_frames=0)
        got = dec.scores(0, 0, 64)
        assert got.shape == (64, 1024) and dec.num_frames_decoded(0) == 0
        want = _np_expect(x32, prior, scale)
        if dt == "f32" and case == "plain":
            assert np.array_equal(bits(got), bits(x32)), "float32, scale 1, no priors is a bit copy"
        _assert_bits(got, want, "%s %s" % (dt, case))
    finally:
        dec.free()


# ---- 2. the reference goldens through the chunk path ---------------------------------------------------------------------------
def test_goldens_through_ragged_f32_chunks(env):
    g = env["g"]
    n = 0
    for ci, cd in enumerate(g.meta["cfgs"]):
        if not _beam_only(cd):
            continue
        dec = env["W"].BatchDecoder(env["graph"], env["G"].gpu_config(dict(cd)), 3, **LIM)
        try:
            _golden_check(env, dec, ci)
            n += 1
        finally:
            dec.free()
    assert n >= 2


# ---- 3. transform + dtype against the oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_transform_and_dtype_against_the_oracle(env, oracle, dt):
    G, g = env["G"], env["g"]
    raw, host = _raw_and_scores(env, dt)
    n_path = 0
    for ci, cd in enumerate(g.meta["cfgs"]):
        dec = env["W"].BatchDecoder(env["graph"], G.gpu_config(dict(cd)), 3, **LIM)
        try:
            dec.set_score_transform(SCALE, env["prior"])
            got = _chunk_decode(env, dec, raw)
            for c in range(3):
                assert np.array_equal(bits(dec.scores(c, 0, 40)), bits(host[c])), "ingested scores of channel %d" % c
        finally:
            dec.free()
        _same(G, got, _want(env, dt, ci), "%s cfg %d against advance" % (dt, ci))
        try:
            oracle.set_order_free(not _beam_only(cd))
            for c in range(3):
                o = oracle.decode(env["h"], pyoracle.Config(**cd), host[c], g.tid2pdf)
                assert o.ok, "%s cfg %d utt %d: the oracle keeps no path" % (dt, ci, c)
                if o.extra.get("ties", 0) == 0:
                    G.assert_same_as_oracle(got[c], o, "%s cfg %d utt %d" % (dt, ci, c))
                n_path += int(got[c].ok)
        finally:
            oracle.set_order_free(False)
    assert n_path == 15


def _as_raw(d):
    return pyoracle.RawLattice(True, d["n_states"], 0, d["st_final"], d["a_src"], d["a_dst"], d["a_ilabel"], d["a_olabel"],
                               d["a_graph"], d["a_acoustic"], d["st_frame"], d["st_state"], d["st_cost"])


def _nodes(L):
    k = np.stack([L.st_frame, L.st_gstate, L.st_final, bits(L.st_cost)], axis=1)
    return k[np.lexsort(k.T[::-1])]


# ---- 4. all decoder kinds ------------------------------------------------------------------------------------------------------
def test_biglm_decoder_fed_by_f16_chunks(env, tmp_path):
    G, W = env["G"], env["W"]
    z = np.load(os.path.join(GOLDEN_DIR, "biglm_hclg600.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    with open(tmp_path / "g.bin", "wb") as f:
        f.write(bytes(z["graph"]))
    graph = W.Graph.load(str(tmp_path / "g.bin"))
    graph.set_tid2pdf(z["tid2pdf"])
    lms = []
    for tag, sc in (("old", -1.0), ("new", 1.0)):
        p = str(tmp_path / ("lm_%s.bin" % tag))
        with open(p, "wb") as f:
            f.write(bytes(z["lm_ngram_%s" % tag]))
        lms.append(W.Lm.load(p, sc))
    utts = [z["ll_%d" % i] for i in range(int(z["n_utt"]))]
    raw, host = _raw_and_scores(env, "f16", utts)
    cd = dict(meta["cfgs"][0])
    lim = dict(max_frames=512, max_tokens_per_frame=32768, arena_tokens=1 << 21)
    try:
        a = W.BatchDecoder(graph, G.gpu_config(cd), len(utts), old_lm=lms[0], new_lm=lms[1], **lim)
        a.set_score_transform(SCALE, env["prior"])
        got = _chunk_decode(env, a, raw)
        a.free()
        b = W.BatchDecoder(graph, G.gpu_config(cd), len(utts), old_lm=lms[0], new_lm=lms[1], **lim)
        want = G.decode_batch(graph, cd, host, dec=b)
        b.free()
        assert any(r.ok for r in want)
        _same(G, got, want, "biglm")
    finally:
        for lm in lms:
            lm.free()
        graph.free()


def test_lattice_decoder_fed_by_f16_chunks(env, tmp_path):
    G, W = env["G"], env["W"]
    g = Golden("lattice_hclg600")
    graph = W.Graph.load(g.write_graph(str(tmp_path / "g.bin")))
    graph.set_tid2pdf(g.tid2pdf)
    raw, host = _raw_and_scores(env, "f16", g.utts)
    lim = dict(max_frames=512, max_tokens_per_frame=32768, arena_tokens=1 << 21, lattice_links=1 << 22)
    try:
        for cd in (dict(g.meta["cfgs"][0]), dict(g.meta["cfgs"][1])):
            a = W.BatchDecoder(graph, G.gpu_config(cd), 3, **lim)
            a.set_score_transform(SCALE, env["prior"])
            got = _chunk_decode(env, a, raw)
            la = [a.raw_lattice(c) for c in range(3)]
            a.free()
            b = W.BatchDecoder(graph, G.gpu_config(cd), 3, **lim)
            want = G.decode_batch(graph, cd, host, dec=b)
            lb = [b.raw_lattice(c) for c in range(3)]
            b.free()
            _same(G, got, want, "lattice")
            for c in range(3):   # identical up to the numbering of the states inside a frame, which the header leaves open
                assert la[c] is not None and lb[c] is not None
                x, y = _as_raw(la[c]), _as_raw(lb[c])
                assert x.n_states == y.n_states and np.array_equal(x.labelled_arcs(), y.labelled_arcs()), "raw lattice %d arcs" % c
                assert np.array_equal(_nodes(x), _nodes(y)), "raw lattice %d states" % c
    finally:
        graph.free()


# ---- 5. layout edges -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["pitch2x", "offset1", "cols301"])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_layout_edges(env, dt, layout):
    G, torch = env["G"], env["torch"]
    raw, host = _raw_and_scores(env, dt)
    prior, cols = env["prior"], 300
    if layout == "pitch2x":
        wide = [torch.full((40, 600), 3.0, dtype=t.dtype, device="cuda:0") for t in raw]
        for w, t in zip(wide, raw):
            w[:, :300] = t
        raw = [w[:, :300] for w in wide]
        assert raw[0].stride() == (600, 1)
    elif layout == "offset1":
        flat = [torch.zeros(40 * 300 + 1, dtype=t.dtype, device="cuda:0") for t in raw]
        for f, t in zip(flat, raw):
            f[1:] = t.reshape(-1)
        raw = [f[1:].view(40, 300) for f in flat]
        assert raw[0].data_ptr() % 4 == 2
    else:
        cols = 301
        raw = [torch.cat([t, torch.full((40, 1), 2.0, dtype=t.dtype, device="cuda:0")], dim=1).contiguous() for t in raw]
        prior = np.concatenate([prior, np.float32([0.5])])
    cd = dict(env["g"].meta["cfgs"][0])
    dec = env["W"].BatchDecoder(env["graph"], G.gpu_config(cd), 3, **LIM)
    try:
        dec.set_score_transform(SCALE, prior)
        got = _chunk_decode(env, dec, raw)
        s = dec.scores(1, 0, 40)
        assert s.shape == (40, cols) and np.array_equal(bits(s[:, :300]), bits(host[1]))
        if layout == "cols301":
            assert np.array_equal(bits(s[:, 300]), bits(np.full(40, (np.float32(2.0) - np.float32(0.5)) * np.float32(SCALE), np.float32)))
            assert dec.path_flags()["ll_row"] == 1   # the stride is 304: the staged row path stays
    finally:
        dec.free()
    _same(G, got, _want(env, dt, 0), "%s %s" % (dt, layout))


# ---- 6. ordering ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["side_stream", "no_stream"])
def test_ordering_with_the_producer(env, mode):
    G, torch = env["G"], env["torch"]
    raw, _ = _raw_and_scores(env, "f16")
    cd = dict(env["g"].meta["cfgs"][0])
    dec = env["W"].BatchDecoder(env["graph"], G.gpu_config(cd), 3, **LIM)
    try:
        dec.set_score_transform(SCALE, env["prior"])
        if mode == "side_stream":
            side = torch.cuda.Stream()
            bufs = [torch.zeros((16, 300), dtype=torch.float16, device="cuda:0") for _ in raw]
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                def make(c, rows):   # produced on the side stream by an op enqueued just before the call ...
                    bufs[c][: rows.shape[0]].copy_(rows)
                    return bufs[c][: rows.shape[0]]

                def after(chunks):   # ... and overwritten on it right after
                    for b in bufs:
                        b.fill_(123.0)

                got = _chunk_decode(env, dec, raw, make=make, after=after)
        else:
            kept = []

            def make(c, rows):
                kept.append(rows.clone())
                torch.cuda.synchronize()
                return kept[-1]

            got = _chunk_decode(env, dec, raw, make=make, stream=None)
    finally:
        dec.free()
    _same(G, got, _want(env, "f16", 0), mode)


# ---- 7. restart and mixing -----------------------------------------------------------------------------------------------------
def test_restart_and_mixing_with_advance_host(env):
    G, W, g, torch = env["G"], env["W"], env["g"], env["torch"]
    raw, _ = _raw_and_scores(env, "bf16")
    cd = dict(g.meta["cfgs"][0])
    dec = W.BatchDecoder(env["graph"], G.gpu_config(cd), 3, **LIM)
    try:
        dec.set_score_transform(SCALE, env["prior"])
        for rep in range(2):   # init, then a second utterance on the same channels
            _same(G, _chunk_decode(env, dec, raw[::-1] if rep else raw), _want(env, "bf16", 0)[::-1] if rep else _want(env, "bf16", 0), "utterance %d" % rep)
        dec.set_score_transform(1.0, None)   # (every utterance is finished)
        dec.init()
        dec.advance_host(g.utts, [14] * 3)
        dev = [torch.from_numpy(x).to("cuda:0") for x in g.utts]
        with pytest.raises(W.WfstError) as ei:   # a stride of 304 behind rows of 300
            dec.advance_chunk([torch.zeros((2, 301), device="cuda:0")] * 3)
        assert ei.value.code == -1 and "stride changed" in str(ei.value)
        dec.advance_chunk([t[14:30] for t in dev])
        dec.advance_chunk([t[30:] for t in dev])
        dec.finalize()
        res = [G.GpuResult(d) for d in dec.best_paths()]
        for k, c in enumerate(g.meta["cases"]):
            if c["cfg"] == 0 and c["mode"] == 1:
                check_result(res[c["utt"]], g.expected(k), "mixed, case %d" % k, check_counts=False)
    finally:
        dec.free()


# ---- 8. errors -----------------------------------------------------------------------------------------------------------------
def _raw_call(W, dec, channels, ptrs, nf, pitch, dtype, cols, stream=None, maxf=-1):
    n = len(ptrs)
    ch = None if channels is None else np.ascontiguousarray(channels, np.int32)
    p = (C.c_void_p * n)(*[int(x) if x else None for x in ptrs])
    f = np.ascontiguousarray(nf, np.int32)
    pt = None if pitch is None else np.ascontiguousarray(pitch, np.int64)
    return W.lib().wfst_decoder_advance_chunk(dec.h, None if ch is None else ch.ctypes.data_as(C.POINTER(C.c_int32)), 0 if ch is None else len(ch), p,
                                              f.ctypes.data_as(C.POINTER(C.c_int32)), None if pt is None else pt.ctypes.data_as(C.POINTER(C.c_int64)),
                                              int(dtype), int(cols), C.c_void_p(W.WFST_STREAM_NONE if stream is None else stream), int(maxf))


def test_errors_leave_the_decoder_usable(env):
    G, W, torch = env["G"], env["W"], env["torch"]
    cd = dict(env["g"].meta["cfgs"][0])
    dec = W.BatchDecoder(env["graph"], G.gpu_config(cd), 3, max_frames=64, max_tokens_per_frame=32768, arena_tokens=1 << 22)
    t = torch.zeros((8, 300), dtype=torch.float32, device="cuda:0")
    P = t.data_ptr()
    msg = lambda: W.lib().wfst_last_error().decode()
    try:
        # a channel that was never initialised
        assert _raw_call(W, dec, None, [P] * 3, [8] * 3, None, 0, 300) == -5 and "before InitDecoding" in msg()
        _golden_check(env, dec)
        arg_cases = [
            ("unknown dtype", dict(dtype=3)),
            ("n_cols <= 0", dict(cols=0)),
            ("n_cols too small", dict(cols=8)),
            ("row pitch below n_cols", dict(pitch=[300, 299, 300])),
            ("negative n_new_frames", dict(nf=[8, -1, 8])),
            ("not aligned to its element size", dict(ptrs=[P, P + 2, P])),
            ("channel index out of range", dict(channels=[0, 1, 3])),
            ("duplicate channel", dict(channels=[0, 1, 1])),
            ("bad channel count", dict(channels=[0, 1, 2, 0], ptrs=[P] * 4, nf=[8] * 4)),
            ("NULL row pointer with frames to append", dict(ptrs=[P, 0, P])),
        ]
        for want, kw in arg_cases:
            dec.init()
            a = dict(channels=None, ptrs=[P] * 3, nf=[8] * 3, pitch=None, dtype=0, cols=300)
            a.update(kw)
            assert _raw_call(W, dec, **a) == -1, want
            assert want in msg(), (want, msg())
            assert all(dec.num_frames_decoded(c) == 0 for c in range(3))
            _golden_check(env, dec)
        # priors of another width
        dec.finalize()   # (the last golden mode leaves its utterance open, and a transform does not change mid-utterance)
        dec.set_score_transform(SCALE, np.zeros(301, np.float32))
        dec.init()
        assert _raw_call(W, dec, None, [P] * 3, [8] * 3, None, 0, 300) == -1 and "log priors" in msg()
        dec.set_score_transform(1.0, None)
        _golden_check(env, dec)
        # capacity: 40 + 40 frames into max_frames = 64, refused before anything is enqueued
        dec.init()
        big = torch.zeros((40, 300), dtype=torch.float32, device="cuda:0")
        dec.advance_chunk([big] * 3)
        assert _raw_call(W, dec, None, [big.data_ptr()] * 3, [40] * 3, None, 0, 300) == -4 and "max_frames" in msg()
        assert all(dec.num_frames_decoded(c) == 40 for c in range(3))
        # a transform does not change mid-utterance
        with pytest.raises(W.WfstError) as ei:
            dec.set_score_transform(0.5, None)
        assert ei.value.code == -5 and "mid-utterance" in str(ei.value)
        # scores: a range outside the frames held
        with pytest.raises(W.WfstError) as ei:
            dec.scores(0, 30, 11)
        assert ei.value.code == -1 and "frame range" in str(ei.value)
        # a finalized channel
        dec.finalize()
        assert _raw_call(W, dec, None, [P] * 3, [8] * 3, None, 0, 300) == -5 and "after FinalizeDecoding" in msg()
        _golden_check(env, dec)
        # scores of a channel that reads the caller's own matrix
        dec.init()
        dev = G.upload(env["g"].utts)
        dec.advance([x.data_ptr() for x in dev], [40] * 3, 300)
        with pytest.raises(W.WfstError) as ei:
            dec.scores(0, 0, 1)
        assert ei.value.code == -5 and "own matrix" in str(ei.value)
        assert _raw_call(W, dec, None, [P] * 3, [8] * 3, None, 0, 300) == -5 and "wfst_decoder_advance" in msg()
        dec.sync()
        _golden_check(env, dec)
    finally:
        dec.free()


# ---- 9. the CLI ----------------------------------------------------------------------------------------------------------------
def test_cli_device_chunks(env, tmp_path):
    import struct

    pkg_dir = os.path.dirname(os.path.abspath(env["W"].__file__))
    exe = os.path.join(pkg_dir, "host", "wfst-decode")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(pkg_dir, "host")], stdout=subprocess.DEVNULL)
    g = env["g"]
    raw, _ = _raw_and_scores(env, "bf16")
    with open(tmp_path / "ll.bin", "wb") as f:   # the model's raw output, float32 on disk (bfloat16 values: the CLI's conversion is exact)
        for i, t in enumerate(raw):
            m = t.float().cpu().numpy()
            key = ("utt%d" % i).encode()
            f.write(struct.pack("<i", len(key)) + key + struct.pack("<ii", m.shape[0], m.shape[1]) + m.tobytes())
    env["prior"].tofile(str(tmp_path / "priors.bin"))
    g.tid2pdf.astype(np.int32).tofile(str(tmp_path / "tid2pdf.bin"))
    cd = dict(g.meta["cfgs"][0])
    with open(tmp_path / "conf", "w") as f:
        f.write("".join("--%s=%s\n" % (k.replace("_", "-"), v) for k, v in cd.items()))
    out = subprocess.run([exe, "--tid2pdf=" + str(tmp_path / "tid2pdf.bin"), "--batch=3", "--device-chunks", "--chunk=7", "--acoustic-scale=0.1",
                          "--log-priors=" + str(tmp_path / "priors.bin"), "--score-dtype=bf16", str(tmp_path / "conf"), env["path"], str(tmp_path / "ll.bin")],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = dict(l.split(" ", 1) if " " in l else (l, "") for l in out.stdout.strip().splitlines())
    for i, x in enumerate(_want(env, "bf16", 0)):
        assert [int(w) for w in lines["utt%d" % i].split()] == [int(w) for w in x.words], "utt%d" % i
