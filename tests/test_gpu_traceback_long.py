"""-m gpu: one best path beyond both LDS tables of the traceback kernels (wfst_kernels.hip): more frames than kBpFrames = 3072,
so the frame bounds are searched in HBM, and more hops than kBpChainLds = 4096, so the hop list of best_path_kernel goes on in
HBM.  One channel, a small graph and a narrow beam (the oracle's decode stays well under a second); against the oracle bit for
bit: after FinalizeDecoding; mid-utterance above 4096 frames with use_final_probs = False; and there endpoint_kernel's trailing
silence over more than one 64-hop chunk, and over the whole path down to the root."""
import numpy as np
import pytest

import pyoracle
from golden_util import bits
from test_gpu_endpoint import trailing_of
from test_gpu_token_gc import _same

pytestmark = pytest.mark.gpu

N_TID = 600
T, T_MID = 4200, 4150   # > kBpFrames; T_MID > kBpChainLds too
CD = dict(beam=6.0, max_active=1000000, min_active=0, lattice_beam=4.0)
INF = float("inf")


@pytest.fixture(scope="module")
def S(synth, oracle, tmp_path_factory):
    g = synth.make_hclg_like(300, seed=31, n_tid=N_TID, n_words=500)
    m = synth.default_tid2pdf(N_TID)
    path = str(tmp_path_factory.mktemp("tb") / "g.bin")
    g.write(path)
    x = synth.make_loglikes(g, T, N_TID // 2, m, seed=90, mu=-2.2)[0]   # (the seed: chosen so that the oracle meets no ties)
    h = oracle.load_graph(path)
    cfg = pyoracle.Config(**CD)
    fin = oracle.decode(h, cfg, x, m)
    mid = oracle.decode(h, cfg, x[:T_MID], m, finalize=False, use_final_probs=False)
    dmp = oracle.decode(h, cfg, x[:T_MID], m, finalize=False, use_final_probs=False, trace=True, dump_frame=T_MID, dump_cap=1 << 18)
    oracle.free_graph(h)
    st, co, n = dmp.dump
    assert n == len(st)
    f = co[st == g.final_state]
    rel = np.float32(INF) if len(f) == 0 else np.float32(np.float32(f.min()) - np.float32(dmp.frame_best[T_MID]))
    assert fin.ok and mid.ok and fin.extra["ties"] == 0 and mid.extra["ties"] == 0
    return dict(g=g, m=m, path=path, x=x, fin=fin, mid=mid, rel=rel)


@pytest.mark.parametrize("lattice", [False, True])
def test_path_beyond_both_lds_tables(S, lattice):
    import gpu_util as G

    wd = G.wfstdec
    graph = wd.Graph.load(S["path"])
    graph.set_tid2pdf(S["m"])
    graph.set_tid2phone(np.arange(N_TID + 1, dtype=np.int32))   # (the identity: silence phones are transition-ids)
    lim = dict(max_frames=T + 56, max_tokens_per_frame=8192, arena_tokens=1 << 20)
    if lattice:
        lim["lattice_links"] = 1 << 21
    dec = wd.BatchDecoder(graph, G.gpu_config(CD), 1, **lim)
    try:
        dev = G.upload([S["x"]])
        dec.init()
        dec.advance([dev[0].data_ptr()], [T_MID], S["x"].shape[1])
        # mid-utterance: the best path, then the endpoint inputs over it
        mid, part = S["mid"], dec.best_paths(use_final_probs=False, cap=8192)[0]
        assert len(part["ilabel"]) > 4096
        _same(part, mid, "mid-utterance @%d" % T_MID)
        rev = [int(v) for v in mid.path_ilabel[::-1]]
        q = next(q for q in range(100, len(rev)) if rev[q] != 0 and rev[q] not in set(rev[:q]))   # the run breaks at hop q
        for sil, lo in ((set(v for v in rev[:q] if v != 0), 65), (set(v for v in rev if v != 0), T_MID)):
            want = trailing_of(mid.path_ilabel, sil)
            assert want >= lo
            dec.set_endpoint_config(wd.EndpointConfig(silence_phones=sorted(sil)))
            _, _, tr, rl = dec.endpoint([0])
            assert tr[0] == want, "trailing silence of a %d-hop run" % want
            assert bits([rl[0]]) == bits([S["rel"]]), "relative cost"
        dec.advance([dev[0].data_ptr()], [T], S["x"].shape[1])
        dec.finalize()
        best = dec.best_paths(cap=8192)[0]
        assert len(best["ilabel"]) > 4096
        _same(best, S["fin"], "after FinalizeDecoding")
    finally:
        dec.free()
        graph.free()
