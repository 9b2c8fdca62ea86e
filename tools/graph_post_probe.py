"""What graph posteriors cost (wfst_decoder_graph_posteriors), in tools/force_align_probe.py's setting: bench.py's headline workload,
128 channels x 300 frames of the 2.85 M-state hclg-like graph's multi-hypothesis log-likelihoods, per channel a transcript graph
built from that channel's own best path (that probe's transcript_of).

    python tools/graph_post_probe.py --out profiles/graph_post_probe.json [--channels 128] [--frames 300]

Recorded, all in the same run and on the same list:
 - the wall time of one graph_posteriors call for pdf classes with lists, and with the dense output only (median of five calls after
   a warm-up call), and the workspace bytes;
 - the same of force_align, beside it;
 - the numpy restatement (tests/graph_post_util.py) over a few channels, scaled to all, and whether the device's answers lie within
   its tolerance on those channels;
 - from a run of the same program under `rocprofv3 --kernel-trace` (the program after `--`): graphpost_kernel, graphpost_pack_kernel,
   graphpost_dense_kernel and forced_align_kernel per call, and the multiple graphpost_kernel is of forced_align_kernel.
The setting of every figure is "behind a decode": the calls follow the decode of the utterances in the same process.
Each run is a child under a time limit of its own; one that ends badly ends the probe."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

N_CALLS = 6
KERNELS = ("graphpost_kernel", "graphpost_pack_kernel", "graphpost_dense_kernel", "forced_align_kernel")


def med(v):
    return float(np.median(v))


def timed(f):
    ms, res = [], None
    for _ in range(N_CALLS):
        t0 = time.perf_counter()
        res = f()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms[1:], res


def child(a):
    import torch

    import graph_post_util as U
    from force_align_probe import transcript_of

    pkg = importlib.import_module("asr-decoder_amd")
    synth, wd = pkg.synth, pkg.wfstdec
    P, B, T = a.pdfs, a.channels, a.frames
    m = synth.default_tid2pdf(2 * P)
    gpath = a.graph_cache % a.states
    g = synth.Graph.read(gpath) if os.path.exists(gpath) else None
    if g is None:
        g = synth.make_hclg_like(a.states, seed=7, n_tid=2 * P)
        g.write(gpath)
    print("graph_post_probe: graph ready", file=sys.stderr, flush=True)
    cache = os.path.join(a.work, "mats.npy")   # (the traced run reads what the plain run made)
    if os.path.exists(cache):
        mats = list(np.load(cache))
    else:
        mats = [synth.make_loglikes_multi(g, T, P, m, seed=i, n_paths=272, mu=-4.0, sigma=1.0, jitter=0.5, ac_lo=0.5)[0] for i in range(B)]
        np.save(cache, np.stack(mats))
    dev = [torch.from_numpy(x).to("cuda:0") for x in mats]
    graph = wd.Graph.from_arrays(g.start, g.final_state, g.state_info, g.arcs)
    graph.set_tid2pdf(m)
    cfg = dict(beam=13.0, max_active=1000000, min_active=0, lattice_beam=7.0, prune_interval=25)
    dec = wd.BatchDecoder(graph, wd.Config(**cfg), B, max_frames=T + 8, max_tokens_per_frame=65536)
    dec.init()
    dec.advance([t.data_ptr() for t in dev], [T] * B, P)
    dec.finalize()
    graphs = [transcript_of(bp, U) for bp in dec.best_paths()]
    ag = wd.AlignGraphs.from_arrays([U.as_tuple(x) for x in graphs])
    info = ag.info()
    print("graph_post_probe: %d channels, %d frames decoded" % (B, T), file=sys.stderr, flush=True)
    grad = [torch.zeros((T, P), device="cuda:0") for _ in range(B)]
    fa_ms, fa = timed(lambda: dec.force_align(ag))
    # (one call outside the timing tells the room the lists take, so that no timed call is made twice)
    cape = max(r.n_entries for r in dec.graph_posteriors(ag, label_map=m))
    li_ms, res = timed(lambda: dec.graph_posteriors(ag, label_map=m, cap_frames=T, cap_entries=cape))
    de_ms, den = timed(lambda: dec.graph_posteriors(ag, label_map=m, grad=grad, lists=False, consumer_stream=wd.WFST_STREAM_NONE))
    stat = lambda v: dict(min=int(np.min(v)), median=med(v), max=int(np.max(v)))
    out = dict(channels=B, frames=T, config=cfg, setting="behind a decode, median of five calls after a warm-up call",
               graph_posteriors_lists=dict(wall_ms=li_ms, wall_ms_median=med(li_ms), found=int(sum(r.found for r in res)),
                                           channel_failures=int(sum(r.status != 0 for r in res)), entries_per_frame=med([r.n_entries / max(r.n_frames, 1) for r in res])),
               graph_posteriors_dense_only=dict(wall_ms=de_ms, wall_ms_median=med(de_ms), found=int(sum(r.found for r in den))),
               workspace_bytes=dec.graph_posteriors_workspace(),
               force_align=dict(wall_ms=fa_ms, wall_ms_median=med(fa_ms), found=int(sum(r.found for r in fa)), workspace_bytes=dec.force_align_workspace()),
               graphs=dict(states=stat(info["n_states"]), arcs=stat(info["n_arcs"]), distinct_ilabels=stat(info["n_labels"]),
                           eps_depth=stat(info["eps_depth"]), device_bytes=int(info["device_bytes"])))
    few = list(range(0, B, max(B // a.host_channels, 1)))[:a.host_channels]
    t0 = time.perf_counter()
    want = [U.graph_posteriors(graphs[c], mats[c], T, m, m) for c in few]
    np_ms = (time.perf_counter() - t0) * 1e3
    worst, within = 0.0, True
    for c, w in zip(few, want):
        try:
            worst = max(worst, U.compare(res[c], w, "channel %d" % c))
        except AssertionError as e:
            within = False
            print("graph_post_probe: %s" % (e,), file=sys.stderr, flush=True)
    out["numpy_restatement"] = dict(channels=len(few), ms=np_ms, ms_scaled_to_all_channels=np_ms * B / len(few),
                                    over_device_call=np_ms * B / len(few) / max(med(li_ms), 1e-9), device_within_tolerance=bool(within),
                                    largest_difference_over_tolerance=worst)
    ag.free()
    dec.free()
    graph.free()
    json.dump(out, open(a.child, "w"))


def kernel_ms(trace_dir):
    """{kernel: [milliseconds of each launch, in launch order]}"""
    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            for r in csv.DictReader(f):
                for key in KERNELS:
                    if key in r.get("Kernel_Name", ""):   # (no kernel's name contains another's)
                        rows.append((int(r["Start_Timestamp"]), key, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6))
                        break
    out = {k: [] for k in KERNELS}
    for _, key, ms in sorted(rows):
        out[key].append(ms)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", type=int, default=2850000)
    ap.add_argument("--pdfs", type=int, default=3000)
    ap.add_argument("--channels", type=int, default=128)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--host-channels", type=int, default=4)
    ap.add_argument("--timeout", type=int, default=420)
    ap.add_argument("--graph-cache", default="/tmp/wfst_bench_graph_%d.bin")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_post_probe.json"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", default="")
    ap.add_argument("--work", default="")
    a = ap.parse_args()
    if a.child:
        return child(a)
    tmp = tempfile.mkdtemp(prefix="graph_post_probe_")
    args = ["--states", str(a.states), "--pdfs", str(a.pdfs), "--channels", str(a.channels), "--frames", str(a.frames),
            "--host-channels", str(a.host_channels), "--graph-cache", a.graph_cache, "--work", tmp]
    me = [sys.executable, os.path.abspath(__file__)]

    def run(name, traced):
        res, tdir = os.path.join(tmp, name + ".json"), os.path.join(tmp, name)
        head = ["timeout", "-k", "10", str(a.timeout)] + (["rocprofv3", "--kernel-trace", "-d", tdir, "--output-format", "csv", "--"] if traced else [])
        rc = subprocess.call(head + me + ["--child", res] + args)
        if rc != 0:
            sys.exit("the %s run ended with status %d: nothing more is started" % (name, rc))
        return json.load(open(res)), (kernel_ms(tdir) if traced else None)

    d, _ = run("plain", False)
    json.dump(d, open(a.out, "w"), indent=1)   # (kept even if the traced run does not finish)
    if a.no_trace:
        d["kernel_ms_per_call"] = "not measured: --no-trace"
    else:
        _, k = run("traced", True)
        # behind the launches of the sizing call(s): graphpost_kernel and the pack kernel run in 2 x N_CALLS calls (lists, dense
        # only), the dense kernel and forced_align_kernel in N_CALLS; the first call of each N_CALLS is the warm-up
        def per_call(v, groups):
            if not len(v) or len(v) % (groups * N_CALLS):
                return None
            per = len(v) // (groups * N_CALLS)
            return [float(np.sum(v[(q * N_CALLS + 1) * per:(q + 1) * N_CALLS * per]) / (N_CALLS - 1)) for q in range(groups)]
        gk, pk, dk, fk = (k[x] for x in KERNELS)
        gk, pk = gk[len(gk) % (2 * N_CALLS):], pk[len(pk) % (2 * N_CALLS):]   # (the sizing call's launches come first)
        g2, p2, d1, f1 = per_call(gk, 2), per_call(pk, 2), per_call(dk, 1), per_call(fk, 1)
        d["kernel_ms_per_call"] = dict(graphpost_kernel_lists=g2 and g2[0], graphpost_kernel_dense_only=g2 and g2[1],
                                       graphpost_pack_kernel_lists=p2 and p2[0], graphpost_pack_kernel_dense_only=p2 and p2[1],
                                       graphpost_dense_kernel=d1 and d1[0], forced_align_kernel=f1 and f1[0])
        if g2 and f1 and f1[0]:
            d["graphpost_kernel_over_forced_align_kernel"] = g2[0] / f1[0]
    json.dump(d, open(a.out, "w"), indent=1)
    print(json.dumps(d))


if __name__ == "__main__":
    main()
