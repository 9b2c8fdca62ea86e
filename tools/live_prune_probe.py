"""What pruned live lattices (wfst_decoder_set_live_lattice_prune) buy the per-chunk n-best text, on the set-up of
profiles/nbest_words_probe.json: 64 live channels of bench.py's headline lattice configuration (the 2.85 M-state hclg-like graph,
beam 13, lattice beam 7, prune_interval 25, the multi-hypothesis log-likelihoods, default determinizer bounds), n_paths = 5, no
LMs, asked at frame 150 and again at the longest utterance the probe runs (--frames).

    python tools/live_prune_probe.py --out profiles/live_prune_probe.json [--frames 150,300] [--channels 64]

For mode 0 and mode 1 at every probed frame: channels answered / refused, the wall time of get_nbest_words (median of three after
one warm-up call), the time of lattice_snapshot_kernel and of the emit launches per call, raw-lattice states per channel
(min / median / max) and scratch_bytes.  THE CONDITION (checked, not measured): in mode 1 every channel whose finalized twin's
lattice fits the determinizer's bounds answers, with the twin's answer -- the probe decodes the twins (a second decoder, the same
frames, FinalizeDecoding) and compares.

The probe runs ITSELF twice as a child, each under a time limit of its own: once plain (the wall times, the condition), once under
`rocprofv3 --kernel-trace` (the kernel times; the program after `--`).  A child that ends badly ends the probe: nothing more is
started."""
import argparse
import csv
import ctypes as C
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
    frames = sorted(int(x) for x in a.frames.split(","))
    P, B, T = a.pdfs, a.channels, frames[-1]
    n_tid = 2 * P
    m = synth.default_tid2pdf(n_tid)
    gpath = a.graph_cache % a.states
    g = synth.Graph.read(gpath) if os.path.exists(gpath) else None
    if g is None:
        g = synth.make_hclg_like(a.states, seed=7, n_tid=n_tid)
        g.write(gpath)
    mats = [synth.make_loglikes_multi(g, T, P, m, seed=i, n_paths=272, mu=-4.0, sigma=1.0, jitter=0.5, ac_lo=0.5)[0] for i in range(B)]
    dev = [torch.from_numpy(x).to("cuda:0") for x in mats]
    ptrs = [t.data_ptr() for t in dev]
    graph = wd.Graph.from_arrays(g.start, g.final_state, g.state_info, g.arcs)
    graph.set_tid2pdf(m)
    cfg = dict(beam=13.0, max_active=1000000, min_active=0, lattice_beam=7.0, prune_interval=25)
    mk = lambda: wd.BatchDecoder(graph, wd.Config(**cfg), B, max_frames=T + 8, max_tokens_per_frame=65536, lattice_links=a.lattice_links)
    A = mk()
    A.init()

    def sizes(dec):
        out = []
        ns, na = C.c_int32(0), C.c_int32(0)
        for c in range(B):
            wd.lib().wfst_decoder_get_raw_lattice(dec.h, c, 1, 0, 0, C.byref(ns), C.byref(na), *([None] * 10))   # (the sizes; WFST_E_CAPACITY with them is the answer)
            out.append((int(ns.value), int(na.value)))
        return out

    def ask(dec):
        ms, res = [], None
        for _ in range(N_CALLS):
            t0 = time.perf_counter()
            res = dec.nbest_words(5, use_final_probs=True)
            ms.append((time.perf_counter() - t0) * 1e3)
        st = [s for s, _ in res]
        return dict(wall_ms=ms[1:], wall_ms_median=float(np.median(ms[1:])), answered=int(sum(1 for s in st if s == 0)),
                    refused=int(sum(1 for s in st if s == -4)), other=int(sum(1 for s in st if s not in (0, -4))),
                    words_mean=float(np.mean([len(p["words"]) for s, ps in res for p in ps] or [0]))), res

    def stats3(v):
        return dict(min=int(np.min(v)), median=float(np.median(v)), max=int(np.max(v)))

    out = dict(channels=B, n_paths=5, frames=frames, config=cfg, at={})
    done = 0
    for f in frames:
        for r in list(range(done + 25, f, 25)) + [f]:
            A.advance(ptrs, [r] * B, P)
        done = f
        A.sync()
        here = {}
        for mode in (0, 1):
            A.set_live_lattice_prune(bool(mode))
            here["mode%d" % mode], res = ask(A)
            if mode == 1:
                res1 = res
        # (behind the timed calls: these launch emits of their own)
        for mode in (1, 0):
            A.set_live_lattice_prune(bool(mode))
            sz = sizes(A)
            here["mode%d" % mode]["raw_states"] = stats3([s for s, _ in sz])
            here["mode%d" % mode]["raw_arcs"] = stats3([x for _, x in sz])
            here["mode%d" % mode]["scratch_bytes"] = int(A.live_lattice_prune()[1])
        if not a.no_twins:   # the condition: the finalized twins, fed the same frames
            Bd = mk()
            Bd.init()
            for r in list(range(25, f, 25)) + [f]:
                Bd.advance(ptrs, [r] * B, P)
            Bd.finalize()
            twin = Bd.nbest_words(5, use_final_probs=True)
            fits = [c for c in range(B) if twin[c][0] == 0]
            same = all(res1[c][0] == 0 and len(res1[c][1]) == len(twin[c][1]) and
                       all(np.array_equal(p["words"], q["words"]) and np.float32(p["path_tot"]).tobytes() == np.float32(q["path_tot"]).tobytes()
                           for p, q in zip(res1[c][1], twin[c][1])) for c in fits)
            here["condition"] = dict(twins_within_bounds=len(fits), of_them_answered_in_mode_1=int(sum(1 for c in fits if res1[c][0] == 0)),
                                     answers_equal_the_twins=bool(same), holds=bool(same))
            Bd.free()
        out["at"][str(f)] = here
    A.free()
    graph.free()
    json.dump(out, open(a.child, "w"))


def kernel_times(trace_dir, n_frames):
    """per probed frame and mode: microseconds per timed call of lattice_snapshot_kernel and of the emit launches (reset + emit + tokens) --
    the launches of the N_CALLS get_nbest_words calls of a mode are the first of that mode at that frame (the size queries and the twins
    come behind them); a mode-1 emit launch is one that follows a snapshot launch"""
    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            for r in csv.DictReader(f):
                name = r.get("Kernel_Name", "")
                for key in ("lattice_snapshot_kernel", "lattice_emit_reset_kernel", "lattice_emit_kernel", "lattice_emit_tokens_kernel", "determinize"):
                    if key in name:
                        rows.append((int(r["Start_Timestamp"]), key, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
                        break
    rows.sort()
    # a "round" = [snapshot] reset emit tokens [determinize ...]; group the launches into rounds at every reset kernel
    rounds, cur = [], None
    pending_snap = None
    for _, key, us in rows:
        if key == "lattice_snapshot_kernel":
            pending_snap = us
        elif key == "lattice_emit_reset_kernel":
            cur = dict(snapshot=pending_snap, emit=us, det=0.0)
            pending_snap = None
            rounds.append(cur)
        elif cur is not None and key in ("lattice_emit_kernel", "lattice_emit_tokens_kernel"):
            cur["emit"] += us
        elif cur is not None:
            cur["det"] += us
    return rounds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", type=int, default=2850000)
    ap.add_argument("--pdfs", type=int, default=3000)
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--frames", default="150,300")
    ap.add_argument("--lattice-links", type=int, default=25165824)
    ap.add_argument("--timeout", type=int, default=420)
    ap.add_argument("--graph-cache", default="/tmp/wfst_bench_graph_%d.bin")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "live_prune_probe.json"))
    ap.add_argument("--no-twins", action="store_true")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        return child(a)
    tmp = tempfile.mkdtemp(prefix="live_prune_probe_")
    args = ["--states", str(a.states), "--pdfs", str(a.pdfs), "--channels", str(a.channels), "--frames", a.frames,
            "--lattice-links", str(a.lattice_links), "--graph-cache", a.graph_cache]
    plain = os.path.join(tmp, "plain.json")
    rc = subprocess.call(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", plain] + args +
                         (["--no-twins"] if a.no_twins else []))
    if rc != 0:
        sys.exit("the plain run ended with status %d: nothing more is started" % rc)
    d = json.load(open(plain))
    json.dump(d, open(a.out, "w"), indent=1)   # (kept even if the traced run does not finish)
    if not a.no_trace:
        traced = os.path.join(tmp, "traced.json")
        rc = subprocess.call(["timeout", "-k", "10", str(a.timeout), "rocprofv3", "--kernel-trace", "-d", tmp, "--output-format", "csv", "--",
                              sys.executable, os.path.abspath(__file__), "--child", traced, "--no-twins"] + args)
        if rc != 0:
            sys.exit("the traced run ended with status %d: nothing more is started" % rc)
        rounds = kernel_times(tmp, len(d["frames"]))
        # the traced child's launches in order: per frame, mode 0's N_CALLS calls, mode 1's N_CALLS calls, then the size queries
        # (mode 1: 64 rounds of one channel with a snapshot; mode 0: 64 without).  A call is one or more rounds (the determinizer's slots).
        pos = 0
        for f in d["frames"]:
            for mode in (0, 1):
                want_snap = mode == 1
                n = 0
                while pos + n < len(rounds) and (rounds[pos + n]["snapshot"] is not None) == want_snap:
                    n += 1
                if mode == 0:
                    take = n                      # every round up to the first snapshot launch
                else:
                    take = n - a.channels         # ... up to the size queries of mode 1 (one round per channel)
                per_call = take // N_CALLS if take > 0 and take % N_CALLS == 0 else 0
                k = d["at"][str(f)]["mode%d" % mode]
                if per_call:
                    calls = [rounds[pos + i * per_call: pos + (i + 1) * per_call] for i in range(1, N_CALLS)]
                    k["rounds_per_call"] = per_call
                    k["emit_us_per_call"] = float(np.median([sum(r["emit"] for r in c) for c in calls]))
                    k["determinize_us_per_call"] = float(np.median([sum(r["det"] for r in c) for c in calls]))
                    if mode == 1:
                        k["snapshot_kernel_us_per_call"] = float(np.median([sum(r["snapshot"] for r in c) for c in calls]))
                else:
                    k["kernel_times"] = "the trace did not line up with the calls (%d rounds)" % take
                pos += n
            pos += a.channels   # mode 0's size queries
        json.dump(d, open(a.out, "w"), indent=1)
    print(json.dumps(d["at"]))


if __name__ == "__main__":
    main()
