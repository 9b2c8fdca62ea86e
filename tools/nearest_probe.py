"""What the lattice edit distance costs (wfst_decoder_nearest_words) and what it is for, on the set-up of profiles/align_probe.json:
64 live channels at frame 150 of bench.py's headline lattice configuration (the 2.85 M-state hclg-like graph, beam 13, lattice beam 7,
prune_interval 25, the multi-hypothesis log-likelihoods), live-prune mode 1.

    python tools/nearest_probe.py --out profiles/nearest_probe.json [--frame 150] [--channels 64]

Recorded:
 - the wall time of nearest_words for, per channel, the 5 paths of nbest_words, each also with one word replaced (by a word the graph
   lacks) and with one word dropped -- 15 references a channel -- and, in the same run, of align_words on the 5 unperturbed sequences
   as the yardstick (median of three calls after one warm-up call each); the ratio is recorded, not gated;
 - the references asked, the errors found, the workspace bytes (from the lattices' sizes and the references, as the header
   documents them);
 - from a second run of the same program under `rocprofv3 --kernel-trace` (the program after `--`) the time of align_index_kernel,
   nearest_kernel and align_kernel per call;
 - what the feature is for: the lattices' oracle word errors beside the 1-best's at lattice_beam 4 / 7 / 10 (the finalized utterances,
   beam 13).  THE TRANSCRIPTS ARE SYNTHETIC: the words of a beam-16 best-path decode of the same log-likelihoods -- there is no
   human transcript of synthetic scores -- so the figures show how the two errors move with lattice_beam, not a recogniser's accuracy.
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
KERNELS = ("align_index_kernel", "nearest_kernel", "align_kernel")


def levenshtein(a, b):
    row = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        new = [i]
        for j, y in enumerate(b, 1):
            new.append(min(row[j] + 1, new[j - 1] + 1, row[j - 1] + (x != y)))
        row = new
    return row[-1]


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
    no_word = int(g.arcs["olabel"].max()) + 1   # a word id the graph lacks
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
    refs = []
    for s in seqs:
        r = []
        for w in s:
            swapped, dropped = list(w), list(w)
            if w:
                swapped[len(w) // 2] = no_word
                del dropped[len(w) // 2]
            r += [w, swapped, dropped]
        refs.append(r)
    nr_ms, nr = timed(lambda: dec.nearest_words(refs, use_final_probs=True))
    al_ms, al = timed(lambda: dec.align_words(seqs, use_final_probs=True))
    states, arcs = [], []
    for c in range(B):
        L = dec.raw_lattice(c, True)
        states.append(0 if L is None else int(L["n_states"]))
        arcs.append(0 if L is None else len(L["a_src"]))
    cells = sum(states[c] * (len(w) + 1) for c in range(B) for w in refs[c])
    n_refs = int(sum(len(r) for r in refs))
    cap = max([len(w) for r in refs for w in r] + [1])
    answers = [x for a_ in nr for x in a_]
    out = dict(channels=B, frame=T, n_paths=5, live_prune_mode=1, config=cfg,
               nearest_words=dict(wall_ms=nr_ms, wall_ms_median=float(np.median(nr_ms)), references=n_refs,
                                  found=int(sum(x["found"] for x in answers)), without_error=int(sum(x["found"] and x["n_err"] == 0 for x in answers)),
                                  errors_by_kind=dict(sub=int(sum(x["n_sub"] for x in answers)), ins=int(sum(x["n_ins"] for x in answers)),
                                                      dele=int(sum(x["n_del"] for x in answers))),
                                  channel_failures=int(sum(1 for a_ in nr if a_ and a_[0]["status"] != 0)),
                                  words_mean=float(np.mean([len(w) for r in refs for w in r] or [0]))),
               align_words=dict(wall_ms=al_ms, wall_ms_median=float(np.median(al_ms)), sequences=int(sum(len(s) for s in seqs)),
                                found=int(sum(r["found"] for a_ in al for r in a_))),
               raw_states=dict(min=int(min(states)), median=float(np.median(states)), max=int(max(states))),
               workspace_bytes=dict(tables=8 * cells, path_scratch=4 * (max(states) + cap) * n_refs, index=B * (32 * max(arcs) + 8 * max(states))))
    out["nearest_over_align_wall"] = out["nearest_words"]["wall_ms_median"] / max(out["align_words"]["wall_ms_median"], 1e-9)
    dec.free()

    # ---- what it is for: oracle word errors beside the 1-best's, against a synthetic transcript --------------------------------
    if not a.no_oracle:
        wide = decoder(dict(cfg, beam=16.0), 0)
        advance(wide)
        wide.finalize()
        transcripts = [[int(x) for x in w[0]] for w in wide.words()]
        wide.free()
        rows = []
        for lb in (4.0, 7.0, 10.0):
            dec = decoder(dict(cfg, lattice_beam=lb), a.lattice_links)
            advance(dec)
            dec.finalize()
            best = [[int(x) for x in w[0]] for w in dec.words()]
            res = dec.nearest_words([[t] for t in transcripts], use_final_probs=True, max_cells=64 << 20)   # (finalized lattices: beyond the default bound)
            ok = [i for i in range(B) if res[i][0]["status"] == 0 and res[i][0]["found"]]
            words = sum(len(transcripts[i]) for i in ok)
            rows.append(dict(lattice_beam=lb, utterances=len(ok), reference_words=int(words),
                             one_best_errors=int(sum(levenshtein(best[i], transcripts[i]) for i in ok)),
                             oracle_errors=int(sum(res[i][0]["n_err"] for i in ok)),
                             oracle_ins_del_sub=[int(sum(res[i][0][k] for i in ok)) for k in ("n_ins", "n_del", "n_sub")],
                             raw_states_median=float(np.median([dec.raw_lattice(i, True)["n_states"] for i in ok[:8]] or [0]))))
            dec.free()
        out["oracle_error"] = dict(transcript="SYNTHETIC: the words of a beam-16 best-path decode of the same log-likelihoods", beam=13.0, rows=rows)
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
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--frame", type=int, default=150)
    ap.add_argument("--lattice-links", type=int, default=25165824)
    ap.add_argument("--timeout", type=int, default=420)
    ap.add_argument("--graph-cache", default="/tmp/wfst_bench_graph_%d.bin")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nearest_probe.json"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        return child(a)
    tmp = tempfile.mkdtemp(prefix="nearest_probe_")
    args = ["--states", str(a.states), "--pdfs", str(a.pdfs), "--channels", str(a.channels), "--frame", str(a.frame),
            "--lattice-links", str(a.lattice_links), "--graph-cache", a.graph_cache]
    plain = os.path.join(tmp, "plain.json")
    rc = subprocess.call(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", plain] + args +
                         (["--no-oracle"] if a.no_oracle else []))
    if rc != 0:
        sys.exit("the plain run ended with status %d: nothing more is started" % rc)
    d = json.load(open(plain))
    json.dump(d, open(a.out, "w"), indent=1)   # (kept even if the traced run does not finish)
    if not a.no_trace:
        rc = subprocess.call(["timeout", "-k", "10", str(a.timeout), "rocprofv3", "--kernel-trace", "-d", tmp, "--output-format", "csv", "--",
                              sys.executable, os.path.abspath(__file__), "--child", os.path.join(tmp, "traced.json"), "--no-oracle"] + args)
        if rc != 0:
            sys.exit("the traced run ended with status %d: nothing more is started" % rc)
        k = kernel_ms(tmp)
        # The traced child makes N_CALLS calls of nearest_words (align_index_kernel + nearest_kernel per round), then N_CALLS of
        # align_words (align_index_kernel + align_kernel per round); the first call of each is the warm-up.
        def per_call(v):
            return float(np.sum(v[len(v) // N_CALLS:]) / (N_CALLS - 1)) if len(v) >= N_CALLS and len(v) % N_CALLS == 0 else None
        # (one index launch and one nearest_kernel / align_kernel launch per round: the first len(nearest) index launches are nearest_words')
        idx, n_near = k["align_index_kernel"], len(k["nearest_kernel"])
        d["nearest_words"]["kernel_ms_per_call"] = dict(align_index_kernel=per_call(idx[:n_near]), nearest_kernel=per_call(k["nearest_kernel"]))
        d["nearest_words"]["launches_per_call"] = dict(align_index_kernel=n_near // N_CALLS, nearest_kernel=n_near // N_CALLS)
        d["align_words"]["kernel_ms_per_call"] = dict(align_index_kernel=per_call(idx[n_near:]), align_kernel=per_call(k["align_kernel"]))
        json.dump(d, open(a.out, "w"), indent=1)
    print(json.dumps(d))


if __name__ == "__main__":
    main()
