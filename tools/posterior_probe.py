"""What word confidences cost (wfst_decoder_word_confidence) and what they are for, on the set-up of profiles/align_probe.json: 64 live
channels at frame 150 of bench.py's headline lattice configuration (the 2.85 M-state hclg-like graph, beam 13, lattice beam 7,
prune_interval 25, the multi-hypothesis log-likelihoods), live-prune mode 1, per channel the 5 paths of nbest_words.

    python tools/posterior_probe.py --out profiles/posterior_probe.json [--frame 150] [--channels 64]

Recorded:
 - the wall time of one word_confidences call and, in the same run, of align_words on the same list (median of three calls after one
   warm-up call each); the ratio is recorded, not gated;
 - the workspace bytes (from the lattices' sizes and the sequences, as the header documents them);
 - from a second run of the same program under `rocprofv3 --kernel-trace` (the program after `--`) the time of posterior_kernel and
   confidence_kernel per call;
 - what the feature is for: the 64 utterances finalized at beam 13, their 1-best words labelled correct or wrong against a SYNTHETIC
   transcript (the words of a beam-16 best-path decode of the same log-likelihoods; a least-edit alignment on the host labels them), and
   the mean confidence of either group and the share of wrong words below 0.5, at acoustic_scale 1 and 0.1.  There is no human
   transcript of synthetic scores: the figures show whether the number separates the two groups, not an accuracy.
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
KERNELS = ("posterior_kernel", "confidence_kernel", "align_index_kernel", "align_kernel")


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

    def decoder(c, links):
        return wd.BatchDecoder(graph, wd.Config(**c), B, max_frames=T + 8, max_tokens_per_frame=65536, lattice_links=links)

    def advance(dec):
        dec.init()
        for r in list(range(25, T, 25)) + [T]:
            dec.advance(ptrs, [r] * B, P)
        dec.sync()

    # ---- the cost: live channels at frame T ------------------------------------------------------------------------------------
    dec = decoder(cfg, a.lattice_links)
    advance(dec)
    dec.set_live_lattice_prune(True)

    def timed(f):
        ms, res = [], None
        for _ in range(N_CALLS):
            t0 = time.perf_counter()
            res = f()
            ms.append((time.perf_counter() - t0) * 1e3)
        return ms[1:], res

    nb = dec.nbest_words(5, use_final_probs=True)
    seqs = [[[int(x) for x in p["words"]] for p in paths] if st == 0 else [] for st, paths in nb]
    wc_ms, wc = timed(lambda: dec.word_confidences(seqs, use_final_probs=True))
    al_ms, al = timed(lambda: dec.align_words(seqs, use_final_probs=True))
    states, arcs = [], []
    for c in range(B):
        L = dec.raw_lattice(c, True)
        states.append(0 if L is None else int(L["n_states"]))
        arcs.append(0 if L is None else len(L["a_src"]))
    cells = sum(states[c] * (len(w) + 1) for c in range(B) for w in seqs[c])
    n_seqs = int(sum(len(s) for s in seqs))
    answers = [x for a_ in wc for x in a_]
    conf = np.concatenate([x["conf"] for x in answers if x["found"]] or [np.zeros(0)])
    out = dict(channels=B, frame=T, n_paths=5, live_prune_mode=1, config=cfg,
               word_confidence=dict(wall_ms=wc_ms, wall_ms_median=float(np.median(wc_ms)), sequences=n_seqs,
                                    found=int(sum(x["found"] for x in answers)), words=int(len(conf)),
                                    conf_mean=float(conf.mean()) if len(conf) else None,
                                    word_post_above_1=int(sum((x["word_post"] > 1.0).sum() for x in answers if x["found"])),
                                    channel_failures=int(sum(1 for a_ in wc if a_ and a_[0]["status"] != 0))),
               align_words=dict(wall_ms=al_ms, wall_ms_median=float(np.median(al_ms)), sequences=n_seqs,
                                found=int(sum(r["found"] for a_ in al for r in a_))),
               raw_states=dict(min=int(min(states)), median=float(np.median(states)), max=int(max(states))),
               workspace_bytes=dict(tables=4 * cells, path_scratch=4 * max(states) * B * 5, index=B * (32 * max(arcs) + 8 * max(states)),
                                    posteriors=B * (24 * max(states) + 16 * max(arcs))))
    out["confidence_over_align_wall"] = out["word_confidence"]["wall_ms_median"] / max(out["align_words"]["wall_ms_median"], 1e-9)
    dec.free()

    # ---- what it is for: does the confidence separate the 1-best's correct words from its wrong ones? ---------------------------
    if not a.no_groups:
        wide = decoder(dict(cfg, beam=16.0), 0)
        advance(wide)
        wide.finalize()
        transcripts = [[int(x) for x in w[0]] for w in wide.words()]
        wide.free()
        dec = decoder(cfg, a.lattice_links)
        advance(dec)
        dec.finalize()
        best = [[int(x) for x in w[0]] for w in dec.words()]
        # label the 1-best's words by a least-edit alignment with the transcript, on the host: nearest_words' ref_hyp maps a
        # transcript to the LATTICE path nearest it, which need not be the 1-best
        labels = [edit_labels(best[i], transcripts[i]) for i in range(B)]
        rows = []
        for sc in (1.0, 0.1):
            res = dec.word_confidences([[w] for w in best], use_final_probs=True, graph_scale=1.0, acoustic_scale=sc, max_cells=64 << 20)
            good, bad = [], []
            for i in range(B):
                r = res[i][0]
                if r["status"] != 0 or not r["found"]:
                    continue
                for c, ok in zip(r["conf"], labels[i]):
                    (good if ok else bad).append(float(c))
            rows.append(dict(graph_scale=1.0, acoustic_scale=sc, correct_words=len(good), wrong_words=len(bad),
                             conf_mean_correct=float(np.mean(good)) if good else None, conf_mean_wrong=float(np.mean(bad)) if bad else None,
                             wrong_below_half=float(np.mean(np.array(bad) < 0.5)) if bad else None,
                             correct_below_half=float(np.mean(np.array(good) < 0.5)) if good else None))
        dec.free()
        out["groups"] = dict(transcript="SYNTHETIC: the words of a beam-16 best-path decode of the same log-likelihoods", beam=13.0, lattice_beam=7.0, rows=rows)
    graph.free()
    json.dump(out, open(a.child, "w"))


def edit_labels(hyp, ref):
    """per hypothesis word: True where a least-edit alignment with `ref` matches it (substituted and inserted words: False)"""
    n, m = len(hyp), len(ref)
    d = np.zeros((n + 1, m + 1), np.int64)
    d[:, 0] = np.arange(n + 1)
    d[0, :] = np.arange(m + 1)
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            d[i, j] = min(d[i - 1, j] + 1, d[i, j - 1] + 1, d[i - 1, j - 1] + (hyp[i - 1] != ref[j - 1]))
    ok, i, j = [False] * n, n, m
    while i > 0 and j > 0:
        if d[i, j] == d[i - 1, j - 1] + (hyp[i - 1] != ref[j - 1]):
            ok[i - 1] = hyp[i - 1] == ref[j - 1]
            i, j = i - 1, j - 1
        elif d[i, j] == d[i - 1, j] + 1:
            i -= 1
        else:
            j -= 1
    return ok


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
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--frame", type=int, default=150)
    ap.add_argument("--lattice-links", type=int, default=25165824)
    ap.add_argument("--timeout", type=int, default=420)
    ap.add_argument("--graph-cache", default="/tmp/wfst_bench_graph_%d.bin")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posterior_probe.json"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--no-groups", action="store_true")
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        return child(a)
    tmp = tempfile.mkdtemp(prefix="posterior_probe_")
    args = ["--states", str(a.states), "--pdfs", str(a.pdfs), "--channels", str(a.channels), "--frame", str(a.frame),
            "--lattice-links", str(a.lattice_links), "--graph-cache", a.graph_cache]
    plain = os.path.join(tmp, "plain.json")
    rc = subprocess.call(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", plain] + args +
                         (["--no-groups"] if a.no_groups else []))
    if rc != 0:
        sys.exit("the plain run ended with status %d: nothing more is started" % rc)
    d = json.load(open(plain))
    json.dump(d, open(a.out, "w"), indent=1)   # (kept even if the traced run does not finish)
    if not a.no_trace:
        rc = subprocess.call(["timeout", "-k", "10", str(a.timeout), "rocprofv3", "--kernel-trace", "-d", tmp, "--output-format", "csv", "--",
                              sys.executable, os.path.abspath(__file__), "--child", os.path.join(tmp, "traced.json"), "--no-groups"] + args)
        if rc != 0:
            sys.exit("the traced run ended with status %d: nothing more is started" % rc)
        k = kernel_ms(tmp)
        # The traced child makes N_CALLS calls of word_confidences (one launch of each of the four kernels per round), then N_CALLS
        # of align_words (align_index_kernel + align_kernel per round); the first call of each is the warm-up.
        def per_call(v):
            return float(np.sum(v[len(v) // N_CALLS:]) / (N_CALLS - 1)) if len(v) >= N_CALLS and len(v) % N_CALLS == 0 else None
        n_post = len(k["posterior_kernel"])
        d["word_confidence"]["kernel_ms_per_call"] = dict(align_index_kernel=per_call(k["align_index_kernel"][:n_post]),
                                                          align_kernel=per_call(k["align_kernel"][:n_post]),
                                                          posterior_kernel=per_call(k["posterior_kernel"]),
                                                          confidence_kernel=per_call(k["confidence_kernel"]))
        d["word_confidence"]["launches_per_call"] = n_post // N_CALLS
        d["align_words"]["kernel_ms_per_call"] = dict(align_index_kernel=per_call(k["align_index_kernel"][n_post:]),
                                                      align_kernel=per_call(k["align_kernel"][n_post:]))
        json.dump(d, open(a.out, "w"), indent=1)
    print(json.dumps(d))


if __name__ == "__main__":
    main()
