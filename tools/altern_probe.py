"""What word alternatives cost (wfst_decoder_word_alternatives) and what they are for, on the set-up of profiles/posterior_probe.json:
64 live channels at frame 150 of bench.py's headline lattice configuration (the 2.85 M-state hclg-like graph, beam 13, lattice beam
7, prune_interval 25, the multi-hypothesis log-likelihoods), live-prune mode 1, per channel the 5 paths of nbest_words.

    python tools/altern_probe.py --out profiles/altern_probe.json [--frame 150] [--channels 64]

Recorded:
 - the wall time of one word_alternatives call and, in the same run, of word_confidences and align_words on the same list (median of
   three calls after one warm-up call each); recorded, not gated;
 - the workspace bytes beyond word_confidences' (from the lattices' sizes and the sequences, as the header documents them), the most
   distinct (cell, word) pairs of a sequence and of a cell, and how many sequences left the LDS table (more pairs than
   WFST_ALTERN_LDS_KEYS);
 - from a second run of the same program under `rocprofv3 --kernel-trace` (the program after `--`) the time of slot_mass_kernel and
   slot_none_kernel per call;
 - what the feature is for, on the 64 utterances finalized at beam 13, their 1-best words labelled against a SYNTHETIC transcript (the
   words of a beam-16 best-path decode of the same log-likelihoods) by a least-edit alignment on the host: how often the transcript's
   word is among the slot's first five alternatives where the 1-best's word is a substitution, and the mean none_post of the 1-best's
   inserted words against its correct ones, at acoustic_scale 1 and 0.1.  There is no human transcript of synthetic scores: the
   figures show whether the slots carry the information, not an accuracy.
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
LDS_KEYS = 1024   # WFST_ALTERN_LDS_KEYS
PP.KERNELS = ("slot_mass_kernel", "slot_none_kernel", "posterior_kernel", "confidence_kernel", "align_index_kernel", "align_kernel")


def edit_ops(hyp, ref):
    """per hypothesis word of a least-edit alignment with `ref`: ("cor", word), ("sub", the reference's word) or ("ins", None)"""
    n, m = len(hyp), len(ref)
    d = np.zeros((n + 1, m + 1), np.int64)
    d[:, 0] = np.arange(n + 1)
    d[0, :] = np.arange(m + 1)
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            d[i, j] = min(d[i - 1, j] + 1, d[i, j - 1] + 1, d[i - 1, j - 1] + (hyp[i - 1] != ref[j - 1]))
    ops, i, j = [("ins", None)] * n, n, m
    while i > 0 and j > 0:
        if d[i, j] == d[i - 1, j - 1] + (hyp[i - 1] != ref[j - 1]):
            ops[i - 1] = ("cor", ref[j - 1]) if hyp[i - 1] == ref[j - 1] else ("sub", ref[j - 1])
            i, j = i - 1, j - 1
        elif d[i, j] == d[i - 1, j] + 1:
            i -= 1
        else:
            j -= 1
    return ops


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
    wa_ms, wa = timed(lambda: dec.word_alternatives(seqs, use_final_probs=True, n_alts=5))
    wc_ms, _ = timed(lambda: dec.word_confidences(seqs, use_final_probs=True))
    al_ms, _ = timed(lambda: dec.align_words(seqs, use_final_probs=True))
    states, arcs = [], []
    for c in range(B):
        L = dec.raw_lattice(c, True)
        states.append(0 if L is None else int(L["n_states"]))
        arcs.append(0 if L is None else len(L["a_src"]))
    n_seqs = int(sum(len(s) for s in seqs))
    answers = [x for a_ in wa for x in a_]
    found = [x for x in answers if x["found"]]
    keys = [int(x["n_distinct"].sum()) for x in found]
    none = np.concatenate([x["none_post"] for x in found] or [np.zeros(0)])
    slots = 2
    while slots <= max(arcs):
        slots <<= 1
    cap = max([len(w) for s in seqs for w in s] + [1])
    med = lambda v: float(np.median(v))
    out = dict(channels=B, frame=T, n_paths=5, n_alts=5, live_prune_mode=1, config=cfg,
               word_alternatives=dict(wall_ms=wa_ms, wall_ms_median=med(wa_ms), sequences=n_seqs, found=len(found), slots=int(len(none)),
                                      none_post_mean=float(none.mean()) if len(none) else None,
                                      keys_per_sequence=dict(median=med(keys) if keys else None, max=max(keys) if keys else None),
                                      words_per_cell_max=int(max([int(x["n_distinct"].max()) for x in found if len(x["n_distinct"])] + [0])),
                                      lds_keys=LDS_KEYS, sequences_that_left_lds=int(sum(k > LDS_KEYS for k in keys)),
                                      channel_failures=int(sum(1 for a_ in wa if a_ and a_[0]["status"] != 0))),
               word_confidences=dict(wall_ms=wc_ms, wall_ms_median=med(wc_ms)),
               align_words=dict(wall_ms=al_ms, wall_ms_median=med(al_ms)),
               raw_states=dict(min=int(min(states)), median=med(states), max=int(max(states))),
               raw_arcs=dict(min=int(min(arcs)), median=med(arcs), max=int(max(arcs))),
               workspace_bytes_beyond_word_confidences=dict(a_per_state=8 * max(states) * B * 5, early_per_word=8 * cap * B * 5,
                                                            table_slots=slots, tables=16 * slots * B * 5,
                                                            results=B * 5 * cap * (8 + 4 + 12 * 5)))
    out["alternatives_over_confidences_wall"] = out["word_alternatives"]["wall_ms_median"] / max(out["word_confidences"]["wall_ms_median"], 1e-9)
    dec.free()

    # ---- what it is for -------------------------------------------------------------------------------------------------------------
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
        ops = [edit_ops(best[i], transcripts[i]) for i in range(B)]
        rows = []
        for sc in (1.0, 0.1):
            res = dec.word_alternatives([[w] for w in best], use_final_probs=True, graph_scale=1.0, acoustic_scale=sc, n_alts=5, max_cells=64 << 20)
            hit = sub = 0
            none_of = dict(cor=[], sub=[], ins=[])
            for i in range(B):
                r = res[i][0]
                if r["status"] != 0 or not r["found"]:
                    continue
                for k, (kind, ref) in enumerate(ops[i]):
                    none_of[kind].append(float(r["none_post"][k]))
                    if kind == "sub":
                        sub += 1
                        hit += ref in [w for w, _ in r["alts"][k]]
            mean = lambda v: float(np.mean(v)) if v else None
            rows.append(dict(graph_scale=1.0, acoustic_scale=sc, correct_words=len(none_of["cor"]), substituted_words=sub,
                             inserted_words=len(none_of["ins"]), transcript_word_among_first_5=hit,
                             transcript_word_among_first_5_share=hit / sub if sub else None,
                             none_post_mean_correct=mean(none_of["cor"]), none_post_mean_substituted=mean(none_of["sub"]),
                             none_post_mean_inserted=mean(none_of["ins"])))
        dec.free()
        out["groups"] = dict(transcript="SYNTHETIC: the words of a beam-16 best-path decode of the same log-likelihoods", beam=13.0, lattice_beam=7.0, rows=rows)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "altern_probe.json"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--no-groups", action="store_true")
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        return child(a)
    tmp = tempfile.mkdtemp(prefix="altern_probe_")
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
        k = PP.kernel_ms(tmp)
        # The traced child makes N_CALLS calls of word_alternatives first (one launch of each of the six kernels per round); the first
        # call is the warm-up.
        def per_call(v):
            return float(np.sum(v[len(v) // N_CALLS:]) / (N_CALLS - 1)) if len(v) >= N_CALLS and len(v) % N_CALLS == 0 else None
        n_alt = len(k["slot_mass_kernel"])
        d["word_alternatives"]["kernel_ms_per_call"] = dict(align_index_kernel=per_call(k["align_index_kernel"][:n_alt]),
                                                            align_kernel=per_call(k["align_kernel"][:n_alt]),
                                                            posterior_kernel=per_call(k["posterior_kernel"][:n_alt]),
                                                            confidence_kernel=per_call(k["confidence_kernel"][:n_alt]),
                                                            slot_mass_kernel=per_call(k["slot_mass_kernel"]),
                                                            slot_none_kernel=per_call(k["slot_none_kernel"]))
        d["word_alternatives"]["launches_per_call"] = n_alt // N_CALLS
        json.dump(d, open(a.out, "w"), indent=1)
    print(json.dumps(d))


if __name__ == "__main__":
    main()
