"""What batched forced alignment costs (wfst_decoder_force_align), on bench.py's headline workload: 128 channels x 300 frames of the
2.85 M-state hclg-like graph's multi-hypothesis log-likelihoods.  Per channel the alignment graph is a transcript graph built from
that channel's own best path: runs of equal transition-ids collapsed into self-loop states, an optional silence (a self-loop state
and an epsilon skip) in front of every word.

    python tools/force_align_probe.py --out profiles/force_align_probe.json [--channels 128] [--frames 300]

Recorded:
 - the wall time of one force_align call over all channels (median of the calls after a warm-up call), the workspace bytes, and
   states, arcs, distinct ilabels and epsilon depth per graph;
 - beside it, on the same inputs: best_paths of the same channel list, the oracle at a beam under which nothing is pruned on one
   host core and the numpy restatement (tests/force_align_util.py), both over a few channels and scaled to all, and whether the
   device's answers equal the restatement's bit for bit on those channels;
 - from runs of the same program under `rocprofv3 --kernel-trace` (the program after `--`): forced_align_kernel and
   best_path_kernel per call, and forced_align_kernel of two variant builds of the library where they lie beside it
   (`build.py --variant fa_nostage -DWFST_FALIGN_NO_STAGING`: every score gathered from its row, no one-frame-ahead staging;
   `--variant fa_notrace -DWFST_FALIGN_NO_TRACEBACK`: the table only), from which the staging's gain and the traceback's share follow.
Each run is a child under a time limit of its own; one that ends badly ends the probe."""
import argparse
import csv
import glob
import importlib
import json
import os
import pickle
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

N_CALLS = 6
KERNELS = ("forced_align_kernel", "best_path_kernel")
SIL_TID = 1


def transcript_of(bp, U):
    """the graph of a best path: a run of equal transition-ids is one state with a self-loop, every word gets an optional silence in
    front (a self-loop state on SIL_TID and an epsilon skip), epsilon hops stay epsilon arcs"""
    B = U.Builder()
    s = B.state()
    last = None   # the transition-id of the state's self-loop
    for il, ol, w in zip(bp["ilabel"], bp["olabel"], bp["graph"]):
        il, ol, w = int(il), int(ol), float(w)
        if ol != 0:
            sil, after = B.state(), B.state()
            B.arc(s, SIL_TID, 0, 1.0, sil)
            B.arc(sil, SIL_TID, 0, 0.25, sil)
            B.arc(sil, 0, 0, 0.0, after)
            B.arc(s, 0, 0, 0.0, after)
            s, last = after, None
        if il != 0 and ol == 0 and il == last:
            continue   # the run goes on: the self-loop takes the frame
        t = B.state()
        B.arc(s, il, ol, w, t)
        if il != 0:
            B.arc(t, il, 0, w, t)
        s, last = t, (il if il != 0 else None)
    return B.build(0, s)


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
    import force_align_util as U

    pkg = importlib.import_module("asr-decoder_amd")
    synth, wd = pkg.synth, pkg.wfstdec
    P, B, T = a.pdfs, a.channels, a.frames
    m = synth.default_tid2pdf(2 * P)
    cache = os.path.join(a.work, "inputs.pkl")
    out = dict(channels=B, frames=T, library_variant=os.environ.get("WFST_LIB_VARIANT", ""))
    if a.mode == "kernel":
        # the alignment alone: the saved scores and graphs, a decoder over a toy graph with the same tid2pdf, nothing decoded
        mats, graphs = pickle.load(open(cache, "rb"))
        toy = synth.make_hclg_like(50, seed=1, n_tid=2 * P, n_words=5)
        graph = wd.Graph.from_arrays(toy.start, toy.final_state, toy.state_info, toy.arcs)
        graph.set_tid2pdf(m)
        dec = wd.BatchDecoder(graph, wd.Config(beam=13.0, max_active=1000000, min_active=0, lattice_beam=7.0, prune_interval=25), B, max_frames=T + 8,
                              max_tokens_per_frame=4096)
        dec.init()
        dec.advance_host(mats, [T] * B, max_num_frames=0)
        ag = wd.AlignGraphs.from_arrays([U.as_tuple(g) for g in graphs])
        ms, res = timed(lambda: dec.force_align(ag))
        out["force_align"] = dict(wall_ms=ms, wall_ms_median=med(ms), found=int(sum(r.found for r in res)))
        json.dump(out, open(a.child, "w"))
        return
    import torch

    gpath = a.graph_cache % a.states
    g = synth.Graph.read(gpath) if os.path.exists(gpath) else None
    if g is None:
        g = synth.make_hclg_like(a.states, seed=7, n_tid=2 * P)
        g.write(gpath)
    print("force_align_probe: graph ready", file=sys.stderr, flush=True)
    if os.path.exists(cache):
        mats, _ = pickle.load(open(cache, "rb"))
    else:
        mats = [synth.make_loglikes_multi(g, T, P, m, seed=i, n_paths=272, mu=-4.0, sigma=1.0, jitter=0.5, ac_lo=0.5)[0] for i in range(B)]
    dev = [torch.from_numpy(x).to("cuda:0") for x in mats]
    graph = wd.Graph.from_arrays(g.start, g.final_state, g.state_info, g.arcs)
    graph.set_tid2pdf(m)
    cfg = dict(beam=13.0, max_active=1000000, min_active=0, lattice_beam=7.0, prune_interval=25)
    dec = wd.BatchDecoder(graph, wd.Config(**cfg), B, max_frames=T + 8, max_tokens_per_frame=65536)
    dec.init()
    dec.advance([t.data_ptr() for t in dev], [T] * B, P)
    dec.finalize()
    bp_ms, bps = timed(lambda: dec.best_paths())
    graphs = [transcript_of(bp, U) for bp in bps]
    if not os.path.exists(cache):
        pickle.dump((mats, graphs), open(cache, "wb"), protocol=4)
    ag = wd.AlignGraphs.from_arrays([U.as_tuple(x) for x in graphs])
    info = ag.info()
    print("force_align_probe: %d channels, %d frames decoded" % (B, T), file=sys.stderr, flush=True)
    ms, res = timed(lambda: dec.force_align(ag))
    stat = lambda v: dict(min=int(np.min(v)), median=med(v), max=int(np.max(v)))
    out.update(config=cfg,
               force_align=dict(wall_ms=ms, wall_ms_median=med(ms), found=int(sum(r.found for r in res)),
                                channel_failures=int(sum(r.status != 0 for r in res)), workspace_bytes=dec.force_align_workspace(),
                                hops_per_path=stat([r.n_hops for r in res]), words_per_path=stat([r.n_words for r in res])),
               graphs=dict(states=stat(info["n_states"]), arcs=stat(info["n_arcs"]), distinct_ilabels=stat(info["n_labels"]),
                           eps_depth=stat(info["eps_depth"]), device_bytes=int(info["device_bytes"])),
               best_paths=dict(wall_ms=bp_ms, wall_ms_median=med(bp_ms)))
    # the host's ways to the same answers, over a few channels
    import pyoracle

    few = list(range(0, B, max(B // a.host_channels, 1)))[:a.host_channels]
    t0 = time.perf_counter()
    want = [U.force_align(graphs[c], mats[c], T, m) for c in few]
    np_ms = (time.perf_counter() - t0) * 1e3
    same = True
    for c, w in zip(few, want):
        try:
            U.compare(res[c], w, "channel %d" % c)
        except AssertionError as e:
            same = False
            print("force_align_probe: %s" % (e,), file=sys.stderr, flush=True)
    out["numpy_restatement"] = dict(channels=len(few), ms=np_ms, ms_scaled_to_all_channels=np_ms * B / len(few),
                                    over_device_call=np_ms * B / len(few) / max(med(ms), 1e-9), device_equals_it_bit_for_bit=bool(same))
    pyoracle.build_oracle()
    orc = pyoracle.OracleDecoder()
    orc.set_tie_rule(1)
    ocfg = pyoracle.Config(beam=1.0e30, max_active=2147483647, min_active=0, lattice_beam=1.0e30)
    o_ms, agree = 0.0, 0
    for c in few:
        path = os.path.join(a.work, "g%d.flat" % c)
        graphs[c].write(path)
        h = orc.load_graph(path)
        t0 = time.perf_counter()
        o = orc.decode(h, ocfg, mats[c], tid2pdf=m)
        o_ms += (time.perf_counter() - t0) * 1e3
        orc.free_graph(h)
        cost = np.float32(0)
        for il, gc, ac in zip(o.path_ilabel, o.path_graph, o.path_ac):
            cost = np.float32(np.float32(cost + ac) + gc) if il != 0 else np.float32(cost + gc)
        agree += int(o.ok and U.bits(cost) == U.bits(res[c].path_cost))
    out["oracle_one_core"] = dict(channels=len(few), ms=o_ms, ms_scaled_to_all_channels=o_ms * B / len(few),
                                  over_device_call=o_ms * B / len(few) / max(med(ms), 1e-9), cost_bits_equal=agree)
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
                    if key in r.get("Kernel_Name", ""):
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "force_align_probe.json"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", default="")
    ap.add_argument("--mode", default="plain")
    ap.add_argument("--work", default="")
    a = ap.parse_args()
    if a.child:
        return child(a)
    tmp = tempfile.mkdtemp(prefix="force_align_probe_")
    args = ["--states", str(a.states), "--pdfs", str(a.pdfs), "--channels", str(a.channels), "--frames", str(a.frames),
            "--host-channels", str(a.host_channels), "--graph-cache", a.graph_cache, "--work", tmp]
    me = [sys.executable, os.path.abspath(__file__)]

    def run(name, mode, traced, variant=""):
        env = dict(os.environ, WFST_LIB_VARIANT=variant)
        res, tdir = os.path.join(tmp, name + ".json"), os.path.join(tmp, name)
        head = ["timeout", "-k", "10", str(a.timeout)] + (["rocprofv3", "--kernel-trace", "-d", tdir, "--output-format", "csv", "--"] if traced else [])
        rc = subprocess.call(head + me + ["--child", res, "--mode", mode] + args, env=env)
        if rc != 0:
            sys.exit("the %s run ended with status %d: nothing more is started" % (name, rc))
        return json.load(open(res)), (kernel_ms(tdir) if traced else None)

    d, _ = run("plain", "plain", False)
    json.dump(d, open(a.out, "w"), indent=1)   # (kept even if a later run does not finish)
    if not a.no_trace:
        # per call: the launches of the timed calls (the first of N_CALLS is the warm-up)
        per_call = lambda v: float(np.sum(v[len(v) // N_CALLS:]) / (N_CALLS - 1)) if len(v) and len(v) % N_CALLS == 0 else None
        _, k = run("traced", "plain", True)
        d["force_align"]["kernel_ms_per_call"] = per_call(k["forced_align_kernel"])
        d["force_align"]["launches_per_call"] = len(k["forced_align_kernel"]) // N_CALLS
        d["best_paths"]["kernel_ms_per_call"] = per_call(k["best_path_kernel"])
        _, k = run("alone", "kernel", True)
        d["force_align"]["kernel_ms_per_call_alone"] = per_call(k["forced_align_kernel"])
        lib = importlib.import_module("asr-decoder_amd").wfstdec.LIB_PATH
        for variant, key in (("fa_nostage", "without_score_staging"), ("fa_notrace", "without_traceback")):
            if not os.path.exists(lib.replace("libwfstdec", "libwfstdec_" + variant)):
                d["force_align"][key] = "not measured: lib/libwfstdec_%s.so is not built" % variant
                continue
            r, k = run(variant, "kernel", True, variant)
            d["force_align"][key] = dict(kernel_ms_per_call=per_call(k["forced_align_kernel"]), wall_ms_median=r["force_align"]["wall_ms_median"],
                                        found=r["force_align"]["found"])
        base = d["force_align"]["kernel_ms_per_call_alone"]
        nt = d["force_align"]["without_traceback"]
        if base and isinstance(nt, dict) and nt["kernel_ms_per_call"]:
            d["force_align"]["traceback_share_of_kernel"] = 1.0 - nt["kernel_ms_per_call"] / base
        json.dump(d, open(a.out, "w"), indent=1)
    print(json.dumps(d))


if __name__ == "__main__":
    main()
