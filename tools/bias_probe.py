"""What phrase boosting costs (wfst_decoder_biased_words), on the set-up of profiles/rescale_probe.json: 64 live channels at frame 150
of bench.py's headline lattice configuration (the 2.85 M-state hclg-like graph, beam 13, lattice beam 7, prune_interval 25, the
multi-hypothesis log-likelihoods), live-prune mode 1.

    python tools/bias_probe.py --out profiles/bias_probe.json [--frame 150] [--channels 64]

Per channel a list is built from word runs (1..3 words, a bonus of 1.0 per word) of the 2nd..5th paths of its nbest_words that its
1-best does not say, so that the phrases are in the lattice; the lists are sized to about 2 / 16 / 64 / 256 nodes (filled up with
words no lattice holds where the paths give too few runs).  Recorded, per size:
 - the wall time of one biased_words call over all channels with four settings (1, 1, 0, bs), bs = 0.5 / 1 / 2 / 4 (median of three
   calls after one warm-up call); recorded, not gated;
 - the cells' bytes (8 per lattice state, node and setting) and the rounds they take;
 - the share of channels whose words differ from their unbiased 1-best at each bs, and the hits per answer;
 - in the same run rescaled_words at (1, 1, 0) four times over, whose kernel does the work of one node;
 - from a second run of the same program under `rocprofv3 --kernel-trace` (the program after `--`) the time of bias_kernel,
   rescale_kernel and align_index_kernel per call.
Not measured: an idle card (the machines are shared) and a service end to end.
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
PP.KERNELS = ("bias_kernel", "rescale_kernel", "align_index_kernel")
SIZES = (2, 16, 64, 256)
BOOSTS = (0.5, 1.0, 2.0, 4.0)
ABSENT = 1 << 24   # word ids no lattice holds


def make_list(best, others, nodes):
    """phrases out of the runs of `others` that `best` does not say, up to `nodes` trie nodes (the root included)"""
    best = [int(w) for w in best]
    said = {tuple(best[i:i + k]) for k in (1, 2, 3) for i in range(len(best) - k + 1)}
    prefixes, phrases = {()}, []
    for k in (2, 3, 1):
        for path in others:
            path = [int(w) for w in path]
            for i in range(len(path) - k + 1):
                run = tuple(path[i:i + k])
                new = [run[:j] for j in range(1, k + 1) if run[:j] not in prefixes]
                if run in said or not new or run in [p[0] for p in phrases] or len(prefixes) + len(new) > nodes:
                    continue
                prefixes.update(new)
                phrases.append((run, float(k)))
    in_lattice = len(phrases)
    for k in range(nodes - len(prefixes)):
        phrases.append(((ABSENT + k,), 1.0))
    return phrases, in_lattice


def rounds_of(need, budget=32 << 20):
    """the rounds the driver cuts: the next channels whose tables fit the budget together, at least one"""
    n, cells = 0, None
    for x in need:
        if cells is None or cells + x > budget:
            n, cells = n + 1, 0
        cells += x
    return n


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
    print("bias_probe: graph ready", file=sys.stderr, flush=True)
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
    print("bias_probe: %d channels at frame %d" % (B, T), file=sys.stderr, flush=True)

    def timed(f):
        ms, res = [], None
        for _ in range(N_CALLS):
            t0 = time.perf_counter()
            res = f()
            ms.append((time.perf_counter() - t0) * 1e3)
        return ms[1:], res

    med = lambda v: float(np.median(v))
    out = dict(channels=B, frame=T, live_prune_mode=1, config=cfg, boosts=list(BOOSTS), sizes=list(SIZES),
               not_measured=["an idle card: the machine is shared", "a service end to end"])
    # (the traced run reads the kernels' times in this order: N_CALLS calls of rescaled_words, then N_CALLS of biased_words per size)
    ms, plain = timed(lambda: dec.rescaled_words([(1.0, 1.0, 0.0)] * len(BOOSTS), use_final_probs=True))
    out["rescaled_words"] = dict(settings=len(BOOSTS), wall_ms=ms, wall_ms_median=med(ms))
    states = [int(dec.raw_lattice(c, True)["n_states"]) for c in range(B)]
    out["raw_states"] = dict(min=int(min(states)), median=med(states), max=int(max(states)), total=int(sum(states)))
    nb = dec.nbest_words(5)
    out["by_size"] = {}
    for nodes in SIZES:
        made = [make_list(plain[c][0]["hyp_words"], [p["words"] for p in nb[c][1][1:]], nodes) for c in range(B)]
        lists = wd.BiasLists.from_phrases([x[0] for x in made])
        info = lists.info()
        settings = [(1.0, 1.0, 0.0, bs) for bs in BOOSTS]
        ms, res = timed(lambda: dec.biased_words(lists, None, settings, use_final_probs=True))
        lists.free()
        need = [s * int(j) * len(BOOSTS) for s, j in zip(states, info["n_nodes"])]
        cells = int(sum(need))
        changed = [float(np.mean([not np.array_equal(res[c][q]["hyp_words"], plain[c][0]["hyp_words"]) for c in range(B)])) for q in range(len(BOOSTS))]
        out["by_size"][str(nodes)] = dict(
            nodes=dict(min=int(info["n_nodes"].min()), max=int(info["n_nodes"].max())), phrases_from_the_lattice_median=med([x[1] for x in made]),
            wall_ms=ms, wall_ms_median=med(ms), over_rescaled_words_wall=med(ms) / max(out["rescaled_words"]["wall_ms_median"], 1e-9),
            cell_bytes=8 * cells, rounds=rounds_of(need), channel_failures=int(sum(row[0]["status"] != 0 for row in res)),
            share_of_channels_whose_words_changed=dict(zip(["bs=%g" % b for b in BOOSTS], changed)),
            hits_per_answer_mean=[float(np.mean([res[c][q]["n_hits"] for c in range(B)])) for q in range(len(BOOSTS))])
        print("bias_probe: %d nodes done" % nodes, file=sys.stderr, flush=True)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bias_probe.json"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        return child(a)
    tmp = tempfile.mkdtemp(prefix="bias_probe_")
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
        # The traced child makes N_CALLS calls of rescaled_words (one launch of rescale_kernel each), then per size N_CALLS calls of
        # biased_words, the first of each the warm-up; a call of biased_words launches bias_kernel once per round, and the rounds of a
        # size are the same in all its calls.  The launches are told apart by their order.
        v = k["rescale_kernel"]
        if len(v) == N_CALLS:
            d["rescaled_words"]["kernel_ms_per_call"] = float(np.sum(v[1:]) / (N_CALLS - 1))
        v, at = k["bias_kernel"], 0
        rounds = [d["by_size"][str(n)]["rounds"] for n in SIZES]
        d["bias_kernel_launches"] = len(v)
        if len(v) == N_CALLS * sum(rounds):
            for n, r in zip(SIZES, rounds):
                part = v[at:at + N_CALLS * r]
                at += N_CALLS * r
                d["by_size"][str(n)]["bias_kernel_ms_per_call"] = float(np.sum(part[r:]) / (N_CALLS - 1))
                if "kernel_ms_per_call" in d["rescaled_words"]:
                    d["by_size"][str(n)]["bias_kernel_over_rescale_kernel"] = d["by_size"][str(n)]["bias_kernel_ms_per_call"] / max(
                        d["rescaled_words"]["kernel_ms_per_call"], 1e-9)
        else:   # (the launches do not come in the expected count: the raw times are kept instead)
            d["bias_kernel_ms_all_launches"] = [float(x) for x in v]
        json.dump(d, open(a.out, "w"), indent=1)
    print(json.dumps(d))


if __name__ == "__main__":
    main()
