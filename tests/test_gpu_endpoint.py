"""-m gpu: endpoint detection on the device (wfst_decoder_endpoint_detected, Kaldi's online2/online-endpoint.cc semantics).
TrailingSilenceLength walks the best path GetBestPath(use_final_probs = false) reports; FinalRelativeCost is ComputeFinalCosts'
best_cost_with_final - best_cost over the frontier.  Against the oracle's prefix decodes (its best path's ilabels, its frontier
dump) and against the decoder's own get_best_path / get_frontier, for best-path and lattice decoders, in batches streamed in
chunks; then the CLI's segmentation against a Python replay of the service loop (v1-asr/asr-source.h:280-287).
tid2phone is the identity: the silence phones are a set of transition-ids."""
import os
import struct
import subprocess

import numpy as np
import pytest

import pyoracle
from golden_util import bits
from test_endpoint_rules import rule_py

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "asr-decoder_amd", "host", "wfst-decode")
N_TID = 600
CD = dict(beam=12.0, max_active=1000000, min_active=0, lattice_beam=6.0, prune_interval=10)
INF = float("inf")


def trailing_of(ilabels, sil):
    """TrailingSilenceLength over a hop list in start->final order."""
    n = 0
    for il in ilabels[::-1]:
        if il == 0:
            continue
        if int(il) in sil:
            n += 1
        else:
            break
    return n


@pytest.fixture(scope="module")
def S(synth, oracle, tmp_path_factory):
    import gpu_util as G

    d = tmp_path_factory.mktemp("ep")
    g = synth.make_hclg_like(3000, seed=21, n_tid=N_TID, n_words=500)
    m = synth.default_tid2pdf(N_TID)
    path = str(d / "g.bin")
    g.write(path)
    graph = G.wfstdec.Graph.load(path)
    graph.set_tid2pdf(m)
    graph.set_tid2phone(np.arange(N_TID + 1, dtype=np.int32))
    h = oracle.load_graph(path)
    yield dict(G=G, g=g, m=m, path=path, graph=graph, h=h, dir=d)
    oracle.free_graph(h)
    graph.free()


def mats_for(S, synth, lengths, seed0):
    return [synth.make_loglikes(S["g"], T, N_TID // 2, S["m"], seed=seed0 + i, mu=-2.2)[0] for i, T in enumerate(lengths)]


def oracle_inputs(S, oracle, x, t):
    """(best-path ilabels, f32 relative cost, ties) of the oracle decoding x[:t] without FinalizeDecoding."""
    cfg = pyoracle.Config(**{k: v for k, v in CD.items()})
    o = oracle.decode(S["h"], cfg, x[:t], S["m"], finalize=False, use_final_probs=False)
    dmp = oracle.decode(S["h"], cfg, x[:t], S["m"], finalize=False, use_final_probs=False, trace=True, dump_frame=t, dump_cap=1 << 18)
    st, co, n = dmp.dump
    assert n == len(st)
    fin = co[st == S["g"].final_state]
    rel = np.float32(INF) if len(fin) == 0 else np.float32(np.float32(fin.min()) - np.float32(dmp.frame_best[t]))
    return o.path_ilabel, rel, o.extra.get("ties", 0)


def make_decoder(S, n, lattice):
    lim = dict(max_frames=256, max_tokens_per_frame=32768, arena_tokens=1 << 21)
    if lattice:
        lim["lattice_links"] = 1 << 21
    return S["G"].wfstdec.BatchDecoder(S["graph"], S["G"].wfstdec.Config(**CD), n, **lim)


def ep_cfg(wd, sil, fs=0.1, rules=None):
    return wd.EndpointConfig(silence_phones=sorted(sil), frame_shift=fs, rules=rules)


def test_vs_oracle_every_rule(S, synth, oracle):
    """Probe frames of a few utterances; silence sets taken from the oracle's own path (its last k transition-ids, with and
    without the one that breaks the run); per case, configs that make each rule fire exactly at its threshold and not one
    frame of silence (or of length) below it."""
    wd = S["G"].wfstdec
    lengths = [150, 120, 97]
    mats = mats_for(S, synth, lengths, 700)
    dev = S["G"].upload(mats)
    dec = make_decoder(S, len(mats), False)
    dec.init()
    fired, n_cases, n_finite = set(), 0, 0
    for t in (13, 40, 75, 97):
        dec.advance([x.data_ptr() for x in dev], [min(t, T) for T in lengths], mats[0].shape[1])
        for c, x in enumerate(mats):
            tc = min(t, lengths[c])
            il, rel, ties = oracle_inputs(S, oracle, x, tc)
            tids = [int(v) for v in il[::-1] if v != 0]
            sets = []
            for k in (1, 2, 3, 6):
                s = set(tids[:k])
                sets.append(s)
                rest = [v for v in tids[k:] if v not in s]
                if rest:
                    sets.append(s | {rest[0]})   # the breaking transition-id too: the run goes on
            absent = [v for v in range(1, N_TID + 1) if v not in set(tids)]
            sets.append({absent[0]})             # nothing on the path: no trailing silence
            for sil in sets:
                want_tr = trailing_of(il, sil)
                dec.set_endpoint_config(ep_cfg(wd, sil))
                det, rule, tr, rl = dec.endpoint([c])
                assert bits([rl[0]]) == bits([rel]), "utt %d frame %d relative cost" % (c, tc)
                if ties:
                    continue
                assert tr[0] == want_tr, "utt %d frame %d trailing silence (%s)" % (c, tc, sorted(sil))
                n_finite += rel != np.float32(INF)
                base = ep_cfg(wd, sil)
                assert rule[0] == rule_py(base, tc, want_tr, rel) and det[0] == (rule[0] != 0)
                # rule j alone, at its threshold and just short of it
                off_rules = {k: dict(min_trailing_silence=INF) for k in range(5)}
                for j in range(5):
                    for short in (False, True):
                        r = {k: dict(v) for k, v in off_rules.items()}
                        if j == 4:
                            r[j] = dict(must_contain_nonsilence=False, min_trailing_silence=0.0, max_relative_cost=INF,
                                        min_utterance_length=float(np.float32(tc + (1 if short else 0)) * np.float32(1.0)))
                        else:
                            r[j] = dict(must_contain_nonsilence=False, min_trailing_silence=float(want_tr + (1 if short else 0)),
                                        max_relative_cost=INF if j in (0, 3) else (float(rel) if rel != np.float32(INF) else INF),
                                        min_utterance_length=0.0)
                        cfg = ep_cfg(wd, sil, fs=1.0, rules=r)
                        dec.set_endpoint_config(cfg)
                        det, rule, tr, rl = dec.endpoint([c])
                        want = rule_py(cfg, tc, want_tr, rel)
                        assert rule[0] == want, (c, tc, sorted(sil), j, short)
                        assert want == (0 if short else j + 1)
                        fired.add(int(rule[0]))
                n_cases += 1
    assert fired == {0, 1, 2, 3, 4, 5} and n_cases >= 60
    dec.free()


@pytest.mark.parametrize("lattice", [False, True])
def test_streaming_batch(lattice, S, synth, oracle):
    """16 ragged channels advanced in 25-frame chunks, polled after every chunk (one call for the list): trailing silence, relative
    cost and rule equal the oracle's prefix decode, the decoder's own get_best_path(use_final_probs = false) hops and its
    frontier.  Lattice decoders: prune_interval 10, so the walk crosses the running prune's compactions."""
    wd = S["G"].wfstdec
    rng = np.random.default_rng(5)
    lengths = [int(v) for v in rng.integers(40, 190, 16)]
    mats = mats_for(S, synth, lengths, 900 + (50 if lattice else 0))
    dev = S["G"].upload(mats)
    dec = make_decoder(S, len(mats), lattice)
    sil = set(int(v) for v in rng.choice(np.arange(1, N_TID + 1), N_TID // 2, replace=False))
    cfg = ep_cfg(wd, sil, fs=0.1, rules={1: dict(max_relative_cost=INF)})
    dec.set_endpoint_config(cfg)
    dec.init()
    final = S["g"].final_state
    seen_tr = set()
    for r in range(25, max(lengths) + 25, 25):
        ready = [min(r, T) for T in lengths]
        dec.advance([x.data_ptr() for x in dev], ready, mats[0].shape[1])
        ch = np.arange(len(mats), dtype=np.int32)[::-1].copy()   # (a list in another order than the channels)
        det, rule, tr, rl = dec.endpoint(ch)
        bp = dec.best_paths(channels=ch, use_final_probs=False)
        for i, c in enumerate(ch):
            nd = ready[c]
            il, rel, ties = oracle_inputs(S, oracle, mats[c], nd)
            assert bits([rl[i]]) == bits([rel]), "channel %d frame %d relative cost vs oracle" % (c, nd)
            st, co = dec.frontier(int(c))
            fin = co[st == final]
            own = np.float32(INF) if len(fin) == 0 else np.float32(np.float32(fin.min()) - np.float32(co.min()))
            assert bits([rl[i]]) == bits([own]), "channel %d frame %d relative cost vs frontier" % (c, nd)
            assert tr[i] == trailing_of(bp[i]["ilabel"], sil), "channel %d frame %d trailing vs get_best_path" % (c, nd)
            assert rule[i] == rule_py(cfg, nd, tr[i], rl[i]) and det[i] == (rule[i] != 0)
            if not ties:
                assert tr[i] == trailing_of(il, sil), "channel %d frame %d trailing vs oracle" % (c, nd)
            seen_tr.add(int(tr[i]))
    assert len(seen_tr) >= 3
    dec.finalize()
    dec.free()


@pytest.mark.parametrize("lattice", [False, True])
def test_walk_across_chunks(lattice, S, synth, oracle):
    """Trailing runs that span one to nine of endpoint_kernel's 64-hop chunks, against the oracle: the silence set = every
    transition-id on the oracle's path (the walk goes to the root: trailing == frames), and sets whose breaking hop lies just
    before, on or just after the 64th, 128th, ... 448th hop from the end.  Kaldi's own rules at the default 0.01 s frame
    shift decide these runs (rule1: 500 frames of silence, rule3: 100, rule4: 200).  Epsilon hops at chunk edges are among the walked hops."""
    wd = S["G"].wfstdec
    lengths = [520, 300, 230, 180, 150, 97]
    mats = mats_for(S, synth, lengths, 1700 + (30 if lattice else 0))
    dev = S["G"].upload(mats)
    lim = dict(max_frames=600, max_tokens_per_frame=32768, arena_tokens=1 << 22)
    if lattice:
        lim["lattice_links"] = 1 << 22
    dec = wd.BatchDecoder(S["graph"], wd.Config(**CD), len(mats), **lim)
    dec.init()
    dec.advance([x.data_ptr() for x in dev], lengths, mats[0].shape[1])
    base_rules, n_checked, longest, eps_at_edge = set(), 0, 0, 0
    for c, x in enumerate(mats):
        T = lengths[c]
        il, rel, ties = oracle_inputs(S, oracle, x, T)
        rev = [int(v) for v in il[::-1]]   # hop q from the end: q = 0..63 the walk's first chunk, 64..127 its second, ...
        sets = [set(v for v in rev if v != 0)]
        for edge in (64, 128, 192, 256, 320, 384, 448):
            for q in range(edge - 2, edge + 3):
                if q < len(rev) and rev[q] != 0 and rev[q] not in set(rev[:q]):
                    sets.append(set(v for v in rev[:q] if v != 0))   # the run breaks at hop q
        eps_at_edge += sum(1 for e in (64, 128, 192, 256, 320, 384, 448, 512) for q in (e - 1, e) if q < len(rev) and rev[q] == 0)
        for sil in sets:
            cfg = wd.EndpointConfig(silence_phones=sorted(sil))   # Kaldi's defaults, frame shift 0.01 s
            dec.set_endpoint_config(cfg)
            det, rule, tr, rl = dec.endpoint([c])
            assert bits([rl[0]]) == bits([rel]), "utt %d relative cost" % c
            if ties:
                continue
            want = trailing_of(il, sil)
            assert tr[0] == want, "utt %d (%d frames): trailing silence of a %d-hop run" % (c, T, want)
            assert rule[0] == rule_py(cfg, T, want, rel) and det[0] == (rule[0] != 0)
            if len(sil) == len(sets[0]) and sil == sets[0]:
                assert want == T   # every emitting hop is silence
            base_rules.add(int(rule[0]))
            longest = max(longest, want)
            n_checked += 1
    assert n_checked >= 20 and longest >= 500
    assert 1 in base_rules and base_rules & {3, 4}, base_rules   # (rule3 comes first where the relative cost is <= 8)
    assert eps_at_edge >= 1
    dec.free()


def test_errors_are_loud(S, synth, tmp_path):
    wd = S["G"].wfstdec
    mats = mats_for(S, synth, [30, 30], 1300)
    dev = S["G"].upload(mats)
    dec = make_decoder(S, 2, False)
    with pytest.raises(wd.WfstError) as ei:   # no config
        dec.endpoint([0])
    assert ei.value.code == -5
    with pytest.raises(wd.WfstError) as ei:   # a bad config
        dec.set_endpoint_config(ep_cfg(wd, [3, 3]))
    assert ei.value.code == -1
    dec.set_endpoint_config(ep_cfg(wd, [3]))
    with pytest.raises(wd.WfstError) as ei:   # before InitDecoding
        dec.endpoint([0])
    assert ei.value.code == -5
    dec.init([0])
    with pytest.raises(wd.WfstError) as ei:   # channel 1 never initialised
        dec.endpoint([0, 1])
    assert ei.value.code == -5
    dec.advance([dev[0].data_ptr()], [30], mats[0].shape[1], channels=[0])
    assert dec.endpoint([0])[2][0] >= 0
    dec.finalize([0])
    with pytest.raises(wd.WfstError) as ei:   # after FinalizeDecoding
        dec.endpoint([0])
    assert ei.value.code == -5
    dec.free()
    # a graph without tid2phone
    g2 = wd.Graph.load(S["path"])
    d2 = wd.BatchDecoder(g2, wd.Config(**CD), 1, max_frames=64, max_tokens_per_frame=8192, arena_tokens=1 << 18)
    with pytest.raises(wd.WfstError) as ei:
        d2.set_endpoint_config(ep_cfg(wd, [3]))
    assert ei.value.code == -5
    d2.free()
    with pytest.raises(wd.WfstError) as ei:   # an ilabel beyond the table
        g2.set_tid2phone(np.arange(10, dtype=np.int32))
    assert ei.value.code == -1
    g2.free()
    # biglm: refused with a message
    lmsynth = __import__("importlib").import_module("asr-decoder_amd.lmsynth")
    lm = lmsynth.make_lm(500, 2, 400, 5, 0, 0, seed=3)
    p = str(tmp_path / "lm.bin")
    lm.to_fsa().write(p)
    L1, L2 = wd.Lm.load(p, -1.0), wd.Lm.load(p, 1.0)
    db = wd.BatchDecoder(S["graph"], wd.Config(**CD), 1, max_frames=64, max_tokens_per_frame=8192, arena_tokens=1 << 18,
                         old_lm=L1, new_lm=L2, lm_pairs=1 << 14)
    with pytest.raises(wd.WfstError) as ei:
        db.set_endpoint_config(ep_cfg(wd, [3]))
    assert ei.value.code == -1 and "biglm" in str(ei.value)
    db.init()
    with pytest.raises(wd.WfstError) as ei:
        db.endpoint([0])
    assert ei.value.code == -1 and "biglm" in str(ei.value)
    db.free()
    L1.free()
    L2.free()


def replay(S, oracle, x, chunk, sil, cfg):
    """The service loop in Python: oracle prefix decodes at each chunk boundary decide the endpoint; each segment finalized on
    its own frames.  Returns [(t_beg, t_end, words, rule)]."""
    out, begin, T = [], 0, x.shape[0]
    c = pyoracle.Config(**CD)
    while begin < T:
        end, rule = T, 0
        ready = (begin // chunk + 1) * chunk
        while ready < T:
            il, rel, _ = oracle_inputs(S, oracle, x[begin:], ready - begin)
            rule = rule_py(cfg, ready - begin, trailing_of(il, sil), rel)
            if rule:
                end = ready
                break
            ready += chunk
        o = oracle.decode(S["h"], c, x[begin:end], S["m"])
        out.append((begin, end, o.words.tolist(), rule))
        begin = end
    return out


@pytest.mark.parametrize("mode", ["single", "pool"])
def test_cli_segments(mode, S, synth, oracle):
    wd = S["G"].wfstdec
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(CLI)])
    d = S["dir"]
    S["m"].astype("<i4").tofile(str(d / "tid2pdf.bin"))
    np.arange(N_TID + 1, dtype="<i4").tofile(str(d / "tid2phone.bin"))
    (d / "decoder.conf").write_text("--beam=12\n--max-active=1000000\n--min-active=0\n--lattice-beam=6\n--prune-interval=10\n")
    lengths = [160, 75, 200, 120, 51, 180, 99, 140]
    mats = mats_for(S, synth, lengths, 1500)
    with open(d / "ll.bin", "wb") as f:
        for i, x in enumerate(mats):
            key = ("utt%03d" % i).encode()
            f.write(struct.pack("<i", len(key)) + key + struct.pack("<ii", x.shape[0], x.shape[1]) + x.tobytes())
    sil = set(range(1, N_TID + 1, 2))
    opts = ["--endpoint.silence-phones=" + ":".join(str(v) for v in sorted(sil)), "--endpoint.frame-shift=0.1",
            "--endpoint.rule2.max-relative-cost=inf", "--endpoint.rule2.min-trailing-silence=0.2"]
    cfg = ep_cfg(wd, sil, fs=0.1, rules={1: dict(max_relative_cost=INF, min_trailing_silence=0.2)})
    args = [CLI, "--tid2pdf=" + str(d / "tid2pdf.bin"), "--tid2phone=" + str(d / "tid2phone.bin"), "--chunk=25", "--print-endpoints"] + opts
    args += ["--single-stream"] if mode == "single" else ["--threads=8", "--pool=8"]
    p = subprocess.run(args + [str(d / "decoder.conf"), S["path"], str(d / "ll.bin")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    want = []
    n_seg = 0
    for i, x in enumerate(mats):
        for b, e, words, rule in replay(S, oracle, x, 25, sil, cfg):
            if rule:
                want.append("utt%03d@%d endpoint rule%d" % (i, e, rule))
            want.append(" ".join(["utt%03d[%d,%d]" % (i, b, e)] + [str(w) for w in words]))
            n_seg += 1
    assert p.stdout.strip().splitlines() == want
    assert n_seg >= len(mats) + 4   # endpoints did split streams
