"""Device time of one endpoint query against one best-path query over the same channel list, mid-utterance, on bench.py's
headline workload (configs[1]: the 2.85 M-state / 10.1 M-arc hclg-like graph, 128 channels, beam 13, the multi-hypothesis
log-likelihoods).  Meant to run under a kernel trace, which then shows endpoint_kernel beside best_path_kernel:

    timeout -k 10 900 rocprofv3 --kernel-trace --stats -d OUT -- python tools/endpoint_probe.py [--frame 150] [--repeat 5]

The script itself prints host wall times of the two calls (the trace's kernel times are the numbers to quote)."""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", type=int, default=2850000)
    ap.add_argument("--pdfs", type=int, default=3000)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--frame", type=int, default=150)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--graph-cache", default="/tmp/wfst_bench_graph_%d.bin")
    a = ap.parse_args()
    import torch

    pkg = importlib.import_module("asr-decoder_amd")
    synth, wd = pkg.synth, pkg.wfstdec
    P, B, T = a.pdfs, a.batch, a.frame
    n_tid = 2 * P
    m = synth.default_tid2pdf(n_tid)
    gpath = a.graph_cache % a.states
    g = synth.Graph.read(gpath) if os.path.exists(gpath) else None
    if g is None:
        g = synth.make_hclg_like(a.states, seed=7, n_tid=n_tid)
        g.write(gpath)
    mats = np.empty((B, T, P), np.float32)
    for i in range(B):   # (bench.py's make_utts for the multi workload, cut at the probe frame)
        mats[i] = synth.make_loglikes_multi(g, T, P, m, seed=i, n_paths=272, mu=-4.0, sigma=1.0, jitter=0.5, ac_lo=0.5)[0]
    ll = torch.from_numpy(mats).to("cuda:0")
    graph = wd.Graph.from_arrays(g.start, g.final_state, g.state_info, g.arcs)
    graph.set_tid2pdf(m)
    t2p = np.zeros(n_tid + 1, np.int32)
    t2p[1:] = (np.arange(1, n_tid + 1) - 1) // 20 + 1   # 300 "phones" of 20 transition-ids each; phones 1-5 are silence
    graph.set_tid2phone(t2p)
    dec = wd.BatchDecoder(graph, wd.Config(beam=13.0, max_active=1000000, min_active=0, lattice_beam=8.0), B,
                          max_frames=T + 8, max_tokens_per_frame=65536)
    dec.set_endpoint_config(wd.EndpointConfig(silence_phones=[1, 2, 3, 4, 5], frame_shift=0.03))
    dec.init()
    stride = P
    dec.advance([ll[i].data_ptr() for i in range(B)], [T] * B, stride)
    dec.sync()
    ch = np.arange(B, dtype=np.int32)
    cap = 4 * T + 64
    for k in range(a.repeat):
        t0 = time.perf_counter()
        det, rule, tr, rel = dec.endpoint(ch)
        t1 = time.perf_counter()
        bp = dec.best_paths(channels=ch, use_final_probs=False, cap=cap)
        t2 = time.perf_counter()
        print("pass %d: endpoint %.3f ms (host wall), best path %.3f ms (host wall); trailing frames mean %.1f, finite relative costs %d, "
              "detected %d, mean hops %.0f" % (k, (t1 - t0) * 1e3, (t2 - t1) * 1e3, float(np.mean(tr)), int(np.isfinite(rel).sum()),
                                                int(det.sum()), float(np.mean([len(bp[i]["ilabel"]) for i in range(B)]))))
    dec.free()
    graph.free()


if __name__ == "__main__":
    main()
