"""What the sequence-training statistics cost (wfst_decoder_sequence_stats), on the set-up of profiles/framepost_probe.json: 64 live
channels at frame 150 of bench.py's headline lattice configuration (the 2.85 M-state hclg-like graph, beam 13, lattice beam 7,
prune_interval 25, the multi-hypothesis log-likelihoods), live-prune mode 1, pdf classes; ref = each channel's 1-best alignment.

    python tools/seqstat_probe.py --out profiles/seqstat_probe.json [--frame 150] [--channels 64]

Recorded:
 - the wall time of one sequence_stats call for sMBR lists, for MMI lists and for sMBR with the dense output only (no lists fetched)
   and, in the same run, of frame_posteriors on the same channels with the same classes (median of three calls after one warm-up
   call each); recorded, not gated;
 - tot_acc over the frames, entries per lattice, the most emitting arcs of a frame and how many frames left LDS;
 - for orientation, the numpy restatement's (tests/seqstat_util.py) time for ONE fetched lattice, posteriors included, scaled to the
   channels;
 - from a second run of the same program under `rocprofv3 --kernel-trace` (the program after `--`) the time of acc_kernel,
   seqstat_frame_kernel, seqstat_pack_kernel and seqstat_dense_kernel per call, beside align_index_kernel and posterior_kernel in the
   same calls, and beside frame_post_kernel and frame_pack_kernel of the sibling call in the same run.
Each run is a child under a time limit of its own; one that ends badly ends the probe."""
import argparse
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import posterior_probe as PP  # noqa: E402  (kernel_ms: the trace reader)

N_CALLS = PP.N_CALLS
LDS_RECS = 1024   # WFST_SEQSTAT_LDS_RECS
PP.KERNELS = ("acc_kernel", "seqstat_frame_kernel", "seqstat_pack_kernel", "seqstat_dense_kernel", "frame_post_kernel", "frame_pack_kernel",
              "posterior_kernel", "align_index_kernel")
PHASES = ("smbr_lists", "mmi_lists", "smbr_dense_only", "frame_posteriors")   # in the order the child makes its calls
# which kernels a phase launches, once per call and round
LAUNCHED = dict(smbr_lists=("align_index_kernel", "posterior_kernel", "acc_kernel", "seqstat_frame_kernel", "seqstat_pack_kernel"),
                mmi_lists=("align_index_kernel", "posterior_kernel", "seqstat_frame_kernel", "seqstat_pack_kernel"),
                smbr_dense_only=("align_index_kernel", "posterior_kernel", "acc_kernel", "seqstat_frame_kernel", "seqstat_pack_kernel", "seqstat_dense_kernel"),
                frame_posteriors=("align_index_kernel", "posterior_kernel", "frame_post_kernel", "frame_pack_kernel"))


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
    ptrs = [t.data_ptr() for t in dev]
    graph = wd.Graph.from_arrays(g.start, g.final_state, g.state_info, g.arcs)
    graph.set_tid2pdf(m)
    cfg = dict(beam=13.0, max_active=1000000, min_active=0, lattice_beam=7.0, prune_interval=25)
    dec = wd.BatchDecoder(graph, wd.Config(**cfg), B, max_frames=T + 8, max_tokens_per_frame=65536, lattice_links=a.lattice_links)
    dec.init()
    for r in list(range(25, T, 25)) + [T]:
        dec.advance(ptrs, [r] * B, P)
    dec.sync()
    dec.set_live_lattice_prune(True)
    pdf = np.asarray(m, np.int32)
    refs = [pdf[np.asarray(b["tids"], np.int64)] for b in dec.best_paths(use_final_probs=True)]
    grads = [torch.zeros((T, P), dtype=torch.float32, device="cuda:0") for _ in range(B)]

    def timed(f):
        ms, res = [], None
        for _ in range(N_CALLS):
            t0 = time.perf_counter()
            res = f()
            ms.append((time.perf_counter() - t0) * 1e3)
        return ms[1:], res

    med = lambda v: float(np.median(v))
    out = dict(channels=B, frame=T, live_prune_mode=1, classes="pdf", config=cfg, lds_recs=LDS_RECS, calls={})
    # (the traced run reads the kernels' times in this order: N_CALLS calls per phase)
    calls = dict(smbr_lists=lambda: dec.sequence_stats(refs, criterion="smbr", label_map=pdf),
                 mmi_lists=lambda: dec.sequence_stats(refs, criterion="mmi", label_map=pdf),
                 smbr_dense_only=lambda: dec.sequence_stats(refs, criterion="smbr", label_map=pdf, grad=grads, stream=None, lists=False),
                 frame_posteriors=lambda: dec.frame_posteriors(use_final_probs=True, label_map=pdf))
    for name in PHASES:
        ms, res = timed(calls[name])
        entries = [int(r["n_entries"]) for r in res]
        d = dict(wall_ms=ms, wall_ms_median=med(ms), channel_failures=int(sum(r["status"] != 0 for r in res)),
                 entries_per_lattice=dict(min=int(min(entries)), median=med(entries), max=int(max(entries))))
        if name.startswith("smbr"):
            d["tot_acc"] = dict(min=float(min(r["tot_acc"] for r in res)), median=med([r["tot_acc"] for r in res]), max=float(max(r["tot_acc"] for r in res)))
        if name == "mmi_lists":
            d["ref_entries_outside_the_lattice"] = int(sum(int((r["posts"] == 0.0).sum()) for r in res))
        out["calls"][name] = d
    fp = out["calls"]["frame_posteriors"]["wall_ms_median"]
    for name in PHASES[:3]:
        out["calls"][name]["over_frame_posteriors_wall"] = out["calls"][name]["wall_ms_median"] / max(fp, 1e-9)
    states, arcs, recs, left = [], [], [], 0
    for c in range(B):
        L = dec.raw_lattice(c, True)
        if L is None:
            continue
        states.append(int(L["n_states"]))
        arcs.append(len(L["a_src"]))
        il = np.asarray(L["a_ilabel"])
        per_frame = np.bincount(np.asarray(L["st_frame"])[np.asarray(L["a_src"])][il > 0])   # the emitting arcs of each frame
        recs.append(int(per_frame.max()))
        left += int((per_frame > LDS_RECS).sum())
    out.update(raw_states=dict(min=int(min(states)), median=med(states), max=int(max(states))),
               raw_arcs=dict(min=int(min(arcs)), median=med(arcs), max=int(max(arcs))),
               emitting_arcs_per_frame_max=int(max(recs)), frames_that_left_lds=left)
    # the numpy restatement on one fetched lattice (the tests' reference), for orientation
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from align_util import from_gpu
    from posterior_util import posteriors
    from seqstat_util import sequence_stats
    L0 = from_gpu(dec.raw_lattice(0, True))
    t0 = time.perf_counter()
    P0 = posteriors(L0)
    t1 = time.perf_counter()
    w = sequence_stats(L0, refs[0], "smbr", label_map=pdf, post=P0)
    t2 = time.perf_counter()
    out["numpy_restatement"] = dict(lattice_states=int(L0.n_states), posteriors_ms=(t1 - t0) * 1e3, sequence_stats_ms=(t2 - t1) * 1e3,
                                    scaled_to_the_channels_ms=(t2 - t0) * 1e3 * B, tot_acc=float(w["tot_acc"]))
    dec.free()
    graph.free()
    json.dump(out, open(a.child, "w"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", type=int, default=2850000)
    ap.add_argument("--pdfs", type=int, default=3000)
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--frame", type=int, default=150)
    ap.add_argument("--lattice-links", type=int, default=25165824)
    ap.add_argument("--timeout", type=int, default=420)
    ap.add_argument("--graph-cache", default="/tmp/wfst_bench_graph_%d.bin")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seqstat_probe.json"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        return child(a)
    tmp = tempfile.mkdtemp(prefix="seqstat_probe_")
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
        k = PP.kernel_ms(tmp)
        # The traced child makes N_CALLS calls per phase, the first of each the warm-up; a call launches each of its kernels once per
        # round.  The rounds per call follow from a kernel only one phase launches.
        rounds, ok = len(k["frame_post_kernel"]) // N_CALLS, True
        at = {key: 0 for key in PP.KERNELS}
        for name in PHASES:
            per = rounds * N_CALLS
            row = {}
            for key in LAUNCHED[name]:
                v = k[key][at[key]:at[key] + per]
                at[key] += per
                ok = ok and len(v) == per and per > 0
                row[key] = float(np.sum(v[rounds:]) / (N_CALLS - 1)) if len(v) == per and per > 0 else None
            d["calls"][name]["kernel_ms_per_call"] = row
            d["calls"][name]["launches_per_call"] = rounds
        d["trace_complete"] = bool(ok and all(at[key] == len(k[key]) for key in PP.KERNELS))
        json.dump(d, open(a.out, "w"), indent=1)
    print(json.dumps(d))


if __name__ == "__main__":
    main()
