"""What word times for n-best paths cost (wfst_decoder_align_words), on the set-up of profiles/nbest_words_probe.json and
profiles/live_prune_probe.json: 64 live channels at frame 150 of bench.py's headline lattice configuration (the 2.85 M-state
hclg-like graph, beam 13, lattice beam 7, prune_interval 25, the multi-hypothesis log-likelihoods), live-prune mode 1, the 5 paths of
nbest_words aligned on every channel that answers.

    python tools/align_probe.py --out profiles/align_probe.json [--frame 150] [--channels 64]

Recorded: the wall time of align_words and of nbest_words on the same list in the same run (median of three after one warm-up call
each), the sequences asked and found, the workspace bytes (from the lattices' sizes and the sequences, as the header documents them),
and -- from a second run of the same program under `rocprofv3 --kernel-trace` (the program after `--`) -- the time of
align_index_kernel and align_kernel per call.  Each run is a child under a time limit of its own; one that ends badly ends the probe."""
import argparse
import csv
import glob
import importlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N_CALLS = 4   # one warm-up + three timed


def child(a):
    import torch

    pkg = importlib.import_module("asr-decoder_amd")
    synth, wd = pkg.synth, pkg.wfstdec
    P, B, T = a.pdfs, a.channels, a.frame
    m = synth.default_tid2pdf(2 * P)
    gpath = a.graph_cache % a.states
    g = synth.Graph.read(gpath) if os.path.exists(gpath) else None
    if g is None:
        g = synth.make_hclg_like(a.states, seed=7, n_tid=2 * P)
        g.write(gpath)
    mats = [synth.make_loglikes_multi(g, T, P, m, seed=i, n_paths=272, mu=-4.0, sigma=1.0, jitter=0.5, ac_lo=0.5)[0] for i in range(B)]
    dev = [torch.from_numpy(x).to("cuda:0") for x in mats]
    graph = wd.Graph.from_arrays(g.start, g.final_state, g.state_info, g.arcs)
    graph.set_tid2pdf(m)
    cfg = dict(beam=13.0, max_active=1000000, min_active=0, lattice_beam=7.0, prune_interval=25)
    dec = wd.BatchDecoder(graph, wd.Config(**cfg), B, max_frames=T + 8, max_tokens_per_frame=65536, lattice_links=a.lattice_links)
    dec.init()
    for r in list(range(25, T, 25)) + [T]:
        dec.advance([t.data_ptr() for t in dev], [r] * B, P)
    dec.sync()
    dec.set_live_lattice_prune(True)

    def timed(f):
        ms, res = [], None
        for _ in range(N_CALLS):
            t0 = time.perf_counter()
            res = f()
            ms.append((time.perf_counter() - t0) * 1e3)
        return ms[1:], res

    nb_ms, nb = timed(lambda: dec.nbest_words(5, use_final_probs=True))
    seqs = [[p["words"] for p in paths] if st == 0 else [] for st, paths in nb]
    al_ms, al = timed(lambda: dec.align_words(seqs, use_final_probs=True))
    states, arcs = [], []
    for c in range(B):
        L = dec.raw_lattice(c, True)
        states.append(0 if L is None else int(L["n_states"]))
        arcs.append(0 if L is None else len(L["a_src"]))
    cells = sum(states[c] * (len(w) + 1) for c in range(B) for w in seqs[c])
    out = dict(channels=B, frame=T, n_paths=5, live_prune_mode=1, config=cfg,
               nbest_words=dict(wall_ms=nb_ms, wall_ms_median=float(np.median(nb_ms)), answered=int(sum(1 for s, _ in nb if s == 0))),
               align_words=dict(wall_ms=al_ms, wall_ms_median=float(np.median(al_ms)), sequences=int(sum(len(s) for s in seqs)),
                                found=int(sum(r["found"] for a_ in al for r in a_)), channel_failures=int(sum(1 for a_ in al if a_ and a_[0]["status"] != 0)),
                                words_mean=float(np.mean([len(w) for s in seqs for w in s] or [0]))),
               raw_states=dict(min=int(min(states)), median=float(np.median(states)), max=int(max(states))),
               workspace_bytes=dict(tables=4 * cells, path_scratch=4 * max(states) * sum(len(s) for s in seqs),
                                    index=B * (32 * max(arcs) + 8 * max(states))))
    dec.free()
    graph.free()
    json.dump(out, open(a.child, "w"))


def kernel_ms(trace_dir):
    """{kernel: [milliseconds of each launch, in launch order]} of the two alignment kernels"""
    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            for r in csv.DictReader(f):
                for key in ("align_index_kernel", "align_kernel"):
                    if key in r.get("Kernel_Name", ""):
                        rows.append((int(r["Start_Timestamp"]), key, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6))
                        break
    out = {"align_index_kernel": [], "align_kernel": []}
    for _, key, ms in sorted(rows):
        out[key].append(ms)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", type=int, default=2850000)
    ap.add_argument("--pdfs", type=int, default=3000)
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--frame", type=int, default=150)
    ap.add_argument("--lattice-links", type=int, default=25165824)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--graph-cache", default="/tmp/wfst_bench_graph_%d.bin")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_probe.json"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        return child(a)
    tmp = tempfile.mkdtemp(prefix="align_probe_")
    args = ["--states", str(a.states), "--pdfs", str(a.pdfs), "--channels", str(a.channels), "--frame", str(a.frame),
            "--lattice-links", str(a.lattice_links), "--graph-cache", a.graph_cache]
    plain = os.path.join(tmp, "plain.json")
    rc = subprocess.call(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", plain] + args)
    if rc != 0:
        sys.exit("the plain run ended with status %d: nothing more is started" % rc)
    d = json.load(open(plain))
    json.dump(d, open(a.out, "w"), indent=1)   # (kept even if the traced run does not finish)
    if not a.no_trace:
        rc = subprocess.call(["timeout", "-k", "10", str(a.timeout), "rocprofv3", "--kernel-trace", "-d", tmp, "--output-format", "csv", "--",
                              sys.executable, os.path.abspath(__file__), "--child", os.path.join(tmp, "traced.json")] + args)
        if rc != 0:
            sys.exit("the traced run ended with status %d: nothing more is started" % rc)
        k = kernel_ms(tmp)
        # a call is one launch of each kernel per round; the first call of the run is the warm-up
        per_call = lambda v: float(np.sum(v[len(v) // N_CALLS:]) / (N_CALLS - 1)) if len(v) >= N_CALLS and len(v) % N_CALLS == 0 else None
        d["align_words"]["kernel_ms_per_call"] = {name: per_call(v) for name, v in k.items()}
        d["align_words"]["launches_per_call"] = {name: len(v) // N_CALLS for name, v in k.items()}
        json.dump(d, open(a.out, "w"), indent=1)
    print(json.dumps(d))


if __name__ == "__main__":
    main()
