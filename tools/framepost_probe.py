"""What frame posteriors cost (wfst_decoder_frame_posteriors), on the set-up of profiles/posterior_probe.json: 64 live channels at
frame 150 of bench.py's headline lattice configuration (the 2.85 M-state hclg-like graph, beam 13, lattice beam 7, prune_interval 25,
the multi-hypothesis log-likelihoods), live-prune mode 1.

    python tools/framepost_probe.py --out profiles/framepost_probe.json [--frame 150] [--channels 64]

Recorded:
 - the wall time of one frame_posteriors call for transition-id, pdf and phone classes and, in the same run, of word_confidences on
   the same channels with their best words (median of three calls after one warm-up call each); recorded, not gated;
 - entries per lattice, the most distinct classes and the most emitting arcs of a frame, how many frames left LDS (more emitting arcs
   than WFST_FRAMEPOST_LDS_RECS), and the bytes of the staged lists and the sort's workspace beyond word_confidences' workspace;
 - from a second run of the same program under `rocprofv3 --kernel-trace` (the program after `--`) the time of frame_post_kernel and
   frame_pack_kernel per call, beside align_index_kernel and posterior_kernel in the same calls.
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
LDS_RECS = 1024   # WFST_FRAMEPOST_LDS_RECS
PP.KERNELS = ("frame_post_kernel", "frame_pack_kernel", "posterior_kernel", "confidence_kernel", "align_index_kernel", "align_kernel")
CLASSES = ("tid", "pdf", "phone")


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
    phone = (np.arange(2 * P + 1, dtype=np.int32) - 1) // 40 + 1    # 40 transition-ids a phone: 150 phones
    phone[0] = 0
    maps = dict(tid=None, pdf=np.asarray(m, np.int32), phone=phone)

    def timed(f):
        ms, res = [], None
        for _ in range(N_CALLS):
            t0 = time.perf_counter()
            res = f()
            ms.append((time.perf_counter() - t0) * 1e3)
        return ms[1:], res

    med = lambda v: float(np.median(v))
    out = dict(channels=B, frame=T, live_prune_mode=1, config=cfg, lds_recs=LDS_RECS, frame_posteriors={})
    # (the traced run reads the kernels' times in this order: N_CALLS calls per class, then word_confidences)
    for name in CLASSES:
        ms, res = timed(lambda: dec.frame_posteriors(use_final_probs=True, label_map=maps[name]))
        entries = [int(r["n_entries"]) for r in res]
        out["frame_posteriors"][name] = dict(wall_ms=ms, wall_ms_median=med(ms), channel_failures=int(sum(r["status"] != 0 for r in res)),
                                             entries_per_lattice=dict(min=int(min(entries)), median=med(entries), max=int(max(entries))),
                                             distinct_per_frame_max=int(max(int(r["n_distinct"].max()) for r in res if len(r["n_distinct"]))),
                                             frame_mass_min=float(min(float(r["frame_mass"].min()) for r in res if len(r["frame_mass"]))))
    seqs = [[[int(x) for x in w[0]]] for w in dec.words(use_final_probs=True)]
    wc_ms, _ = timed(lambda: dec.word_confidences(seqs, use_final_probs=True))
    out["word_confidences"] = dict(wall_ms=wc_ms, wall_ms_median=med(wc_ms))
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
               emitting_arcs_per_frame_max=int(max(recs)), frames_that_left_lds=left,
               # 24 bytes per arc and 16 per frame of the round's largest lattice, per channel (include/wfst_decoder.h)
               workspace_bytes_beyond_word_confidences=B * (24 * max(arcs) + 16 * (T + 2)))
    for name in CLASSES:
        out["frame_posteriors"][name]["over_word_confidences_wall"] = out["frame_posteriors"][name]["wall_ms_median"] / max(med(wc_ms), 1e-9)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "framepost_probe.json"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        return child(a)
    tmp = tempfile.mkdtemp(prefix="framepost_probe_")
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
        # The traced child makes N_CALLS calls of frame_posteriors per class (one launch of each of the four kernels per call and round),
        # the first of each the warm-up; word_confidences' launches of align_index_kernel and posterior_kernel come behind them.
        n = len(k["frame_post_kernel"])
        per = n // len(CLASSES) if n % (len(CLASSES) * N_CALLS) == 0 else 0
        for i, name in enumerate(CLASSES):
            if not per:
                break
            cut = lambda v: v[i * per:(i + 1) * per]
            per_call = lambda v: float(np.sum(cut(v)[per // N_CALLS:]) / (N_CALLS - 1))
            d["frame_posteriors"][name]["kernel_ms_per_call"] = {key: per_call(k[key]) for key in
                                                                 ("align_index_kernel", "posterior_kernel", "frame_post_kernel", "frame_pack_kernel")}
            d["frame_posteriors"][name]["launches_per_call"] = per // N_CALLS
        json.dump(d, open(a.out, "w"), indent=1)
    print(json.dumps(d))


if __name__ == "__main__":
    main()
