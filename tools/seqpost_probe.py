"""What sentence and phrase posteriors cost (wfst_decoder_sequence_posterior), on the set-up of profiles/align_probe.json and
profiles/posterior_probe.json: 64 live channels at frame 150 of bench.py's headline lattice configuration (the 2.85 M-state hclg-like
graph, beam 13, lattice beam 7, prune_interval 25, the multi-hypothesis log-likelihoods), live-prune mode 1, per channel the 5 paths
of nbest_words.

    python tools/seqpost_probe.py --out profiles/seqpost_probe.json [--frame 150] [--channels 64]

Recorded:
 - the wall time of one sentence_posteriors call over the 5 paths per channel, of one phrase_posteriors call over every 2-word run of
   each channel's 1-best with hit_mass on, and, in the same run on the sentences' list, of word_confidences and align_words (median of
   three calls after one warm-up call each); the ratios are recorded, not gated;
 - the workspace bytes (from the lattices' sizes and the sequences, as the header documents them);
 - how many channels' five posteriors sum above 0.5, and the share of phrases with count > 1;
 - from a second run of the same program under `rocprofv3 --kernel-trace` (the program after `--`) the kernels' times per call.  A
   call emits the live channels' lattices once, whatever its rounds: the launches of lattice_emit_kernel cut the trace into calls, and
   a call is told by the kernels it holds.
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
N_CALLS = 4   # one warm-up + three timed
EMIT = "lattice_emit_kernel"
KERNELS = ("seqpost_kernel", "posterior_kernel", "confidence_kernel", "align_index_kernel", "align_kernel", EMIT)


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

    nb = dec.nbest_words(5, use_final_probs=True)
    seqs = [[[int(x) for x in p["words"]] for p in paths] if st == 0 else [] for st, paths in nb]
    phrases = [[s[0][j:j + 2] for j in range(len(s[0]) - 1)][:64] if s else [] for s in seqs]
    states, arcs = [], []
    for c in range(B):
        L = dec.raw_lattice(c, True)
        states.append(0 if L is None else int(L["n_states"]))
        arcs.append(0 if L is None else len(L["a_src"]))

    def timed(f):
        ms, res = [], None
        for _ in range(N_CALLS):
            t0 = time.perf_counter()
            res = f()
            ms.append((time.perf_counter() - t0) * 1e3)
        return ms[1:], res

    # (the timed calls come last and in this order: main() reads the trace's last 4 * N_CALLS calls by it)
    sp_ms, sp = timed(lambda: dec.sentence_posteriors(seqs, use_final_probs=True))
    ph_ms, ph = timed(lambda: dec.phrase_posteriors(phrases, use_final_probs=True, hit_mass=True))
    wc_ms, wc = timed(lambda: dec.word_confidences(seqs, use_final_probs=True))
    al_ms, al = timed(lambda: dec.align_words(seqs, use_final_probs=True))
    med = lambda v: float(np.median(v))
    n_seqs, n_phr = int(sum(len(s) for s in seqs)), int(sum(len(s) for s in phrases))
    mass = [float(sum(np.exp(x["logpost"]) for x in a_ if x["found"])) for a_ in sp if a_]
    counts = np.array([x["count"] for a_ in ph for x in a_ if x["found"]] or [0.0])
    cells_s = sum(states[c] * (len(w) + 1) for c in range(B) for w in seqs[c])
    cells_p = sum(states[c] * (len(w) + 1) for c in range(B) for w in phrases[c])
    post = B * (24 * max(states) + 16 * max(arcs))
    out = dict(channels=B, frame=T, n_paths=5, live_prune_mode=1, config=cfg,
               sentence_posteriors=dict(wall_ms=sp_ms, wall_ms_median=med(sp_ms), sequences=n_seqs,
                                        found=int(sum(x["found"] for a_ in sp for x in a_)), us_per_sequence=1e3 * med(sp_ms) / max(n_seqs, 1),
                                        channel_failures=int(sum(1 for a_ in sp if a_ and a_[0]["status"] != 0)),
                                        five_best_mass=dict(channels=len(mass), above_half=int(sum(x > 0.5 for x in mass)),
                                                            median=med(mass) if mass else None, max=max(mass) if mass else None)),
               phrase_posteriors=dict(wall_ms=ph_ms, wall_ms_median=med(ph_ms), phrases=n_phr, hit_mass=True,
                                      found=int(sum(x["found"] for a_ in ph for x in a_)), us_per_phrase=1e3 * med(ph_ms) / max(n_phr, 1),
                                      channel_failures=int(sum(1 for a_ in ph if a_ and a_[0]["status"] != 0)),
                                      count_above_1_share=float((counts > 1.0).mean()), count_max=float(counts.max())),
               word_confidence=dict(wall_ms=wc_ms, wall_ms_median=med(wc_ms), sequences=n_seqs, found=int(sum(x["found"] for a_ in wc for x in a_))),
               align_words=dict(wall_ms=al_ms, wall_ms_median=med(al_ms), sequences=n_seqs, found=int(sum(x["found"] for a_ in al for x in a_))),
               raw_states=dict(min=int(min(states)), median=med(states), max=int(max(states))),
               workspace_bytes=dict(sentence_tables=8 * cells_s, phrase_tables=8 * cells_p, level_flags=4 * max(states) * max(n_seqs, n_phr),
                                    index=B * (32 * max(arcs) + 8 * max(states)), posteriors=post,
                                    hit_mass_rows=8 * n_phr * (T + 1)))
    out["sentence_over_confidence_wall"] = out["sentence_posteriors"]["wall_ms_median"] / max(out["word_confidence"]["wall_ms_median"], 1e-9)
    out["sentence_over_align_wall"] = out["sentence_posteriors"]["wall_ms_median"] / max(out["align_words"]["wall_ms_median"], 1e-9)
    dec.free()
    graph.free()
    json.dump(out, open(a.child, "w"))


def calls_of(trace_dir):
    """the trace cut at the launches of lattice_emit_kernel: [{kernel: milliseconds summed, "launches": {kernel: n}}], in order"""
    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            for r in csv.DictReader(f):
                for key in KERNELS:
                    if key in r.get("Kernel_Name", ""):
                        rows.append((int(r["Start_Timestamp"]), key, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6))
                        break
    calls = []
    for _, key, ms in sorted(rows):
        if key == EMIT:
            calls.append(dict(launches={}))
        if not calls:
            continue
        calls[-1][key] = calls[-1].get(key, 0.0) + ms
        calls[-1]["launches"][key] = calls[-1]["launches"].get(key, 0) + 1
    return calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", type=int, default=2850000)
    ap.add_argument("--pdfs", type=int, default=3000)
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--frame", type=int, default=150)
    ap.add_argument("--lattice-links", type=int, default=25165824)
    ap.add_argument("--timeout", type=int, default=420)
    ap.add_argument("--graph-cache", default="/tmp/wfst_bench_graph_%d.bin")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seqpost_probe.json"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        return child(a)
    tmp = tempfile.mkdtemp(prefix="seqpost_probe_")
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
        calls = calls_of(tmp)[-4 * N_CALLS:]
        kinds = ("sentence_posteriors", "phrase_posteriors", "word_confidence", "align_words")
        marks = ("seqpost_kernel", "seqpost_kernel", "confidence_kernel", "align_kernel")
        ok = len(calls) == 4 * N_CALLS and all(mark in c for k, mark in enumerate(marks) for c in calls[k * N_CALLS:(k + 1) * N_CALLS])
        d["kernel_trace_calls_recognised"] = bool(ok)
        for k, kind in enumerate(kinds if ok else ()):
            mine = calls[k * N_CALLS + 1:(k + 1) * N_CALLS]   # (without the warm-up call)
            d[kind]["kernel_ms_per_call"] = {key: float(np.mean([c.get(key, 0.0) for c in mine])) for key in KERNELS if any(key in c for c in mine)}
            d[kind]["launches_per_call"] = {key: n for key, n in mine[-1]["launches"].items()}
        json.dump(d, open(a.out, "w"), indent=1)
    print(json.dumps(d))


if __name__ == "__main__":
    main()
