"""What a sweep of best paths under new scales costs (wfst_decoder_rescaled_words), on the set-up of profiles/posterior_probe.json: 64
live channels at frame 150 of bench.py's headline lattice configuration (the 2.85 M-state hclg-like graph, beam 13, lattice beam 7,
prune_interval 25, the multi-hypothesis log-likelihoods), live-prune mode 1, with a sweep of 33 settings (LMWT 7..17 as acoustic
scale 1 / LMWT, word penalties 0, 0.5 and 1).

    python tools/rescale_probe.py --out profiles/rescale_probe.json [--frame 150] [--channels 64]

Recorded:
 - the wall time of one rescaled_words call over all channels and settings, with and without the alignment (median of three calls
   after one warm-up call each), and in the same run of align_words on the same channels with their 1-best words; recorded, not gated;
 - the numpy restatement (tests/rescale_util.py) of the same sweep over ONE channel's fetched lattice, and that time scaled up to all
   channels -- what the host loop over fetched lattices would cost, the fetch itself not counted;
 - how many distinct word sequences the sweep finds per channel, and whether the device's answers equal the restatement's bit for bit
   on that channel;
 - from a second run of the same program under `rocprofv3 --kernel-trace` (the program after `--`) the time of rescale_kernel and
   align_index_kernel per call.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import posterior_probe as PP  # noqa: E402  (kernel_ms: the trace reader)

N_CALLS = PP.N_CALLS
PP.KERNELS = ("rescale_kernel", "align_index_kernel", "align_kernel")
SWEEP = [(1.0, 1.0 / lmwt, wip) for lmwt in range(7, 18) for wip in (0.0, 0.5, 1.0)]


def child(a):
    import torch

    from align_util import from_gpu
    from rescale_util import bits64, rescale_many

    pkg = importlib.import_module("asr-decoder_amd")
    synth, wd = pkg.synth, pkg.wfstdec
    P, B, T = a.pdfs, a.channels, a.frame
    m = synth.default_tid2pdf(2 * P)
    gpath = a.graph_cache % a.states
    g = synth.Graph.read(gpath) if os.path.exists(gpath) else None
    if g is None:
        g = synth.make_hclg_like(a.states, seed=7, n_tid=2 * P)
        g.write(gpath)
    print("rescale_probe: graph ready", file=sys.stderr, flush=True)
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
    print("rescale_probe: %d channels at frame %d" % (B, T), file=sys.stderr, flush=True)

    def timed(f):
        ms, res = [], None
        for _ in range(N_CALLS):
            t0 = time.perf_counter()
            res = f()
            ms.append((time.perf_counter() - t0) * 1e3)
        return ms[1:], res

    med = lambda v: float(np.median(v))
    out = dict(channels=B, frame=T, live_prune_mode=1, config=cfg, settings=len(SWEEP), sweep=SWEEP)
    # (the traced run reads the kernels' times in this order: N_CALLS calls without the alignment, N_CALLS with it, then align_words)
    ms, res = timed(lambda: dec.rescaled_words(SWEEP, use_final_probs=True))
    ms_t, res_t = timed(lambda: dec.rescaled_words(SWEEP, use_final_probs=True, cap_tids=T + 8))
    distinct = [len({tuple(r["hyp_words"].tolist()) for r in row}) for row in res]
    out["rescaled_words"] = dict(wall_ms=ms, wall_ms_median=med(ms), with_alignment_wall_ms=ms_t, with_alignment_wall_ms_median=med(ms_t),
                                 channel_failures=int(sum(row[0]["status"] != 0 for row in res)),
                                 not_found=int(sum(not r["found"] for row in res for r in row)),
                                 distinct_word_sequences_per_channel=dict(min=int(min(distinct)), median=med(distinct), max=int(max(distinct))),
                                 words_per_path=dict(min=int(min(r["n_hyp"] for row in res for r in row)), max=int(max(r["n_hyp"] for row in res for r in row))))
    seqs = [[[int(x) for x in w[0]]] for w in dec.words(use_final_probs=True)]
    al_ms, _ = timed(lambda: dec.align_words(seqs, use_final_probs=True))
    out["align_words"] = dict(wall_ms=al_ms, wall_ms_median=med(al_ms), sequences=B)
    states, arcs = [], []
    for c in range(B):
        L = dec.raw_lattice(c, True)
        if L is None:
            continue
        states.append(int(L["n_states"]))
        arcs.append(len(L["a_src"]))
    out.update(raw_states=dict(min=int(min(states)), median=med(states), max=int(max(states))),
               raw_arcs=dict(min=int(min(arcs)), median=med(arcs), max=int(max(arcs))),
               # 8 bytes per state and setting for the cells and 4 for the traced path (include/wfst_decoder.h)
               cells_and_path_bytes=12 * int(sum(states)) * len(SWEEP))
    # the host loop's cost: the restatement over one channel's fetched lattice (the channel with the median number of states)
    c = int(np.argsort(states)[len(states) // 2])
    L = from_gpu(dec.raw_lattice(c, True))
    t0 = time.perf_counter()
    want = rescale_many(L, SWEEP)
    one = (time.perf_counter() - t0) * 1e3
    same = all(bool(r["found"]) == bool(w["found"]) and (not w["found"] or (bits64(r["scaled_cost"]) == bits64(w["scaled_cost"]) and
                                                                               np.array_equal(r["hyp_words"], w["words"]) and np.array_equal(r["tids"], w["tids"])))
               for r, w in zip(res_t[c], want))
    out["numpy_restatement"] = dict(channel=c, states=int(L.n_states), ms_one_channel=one, ms_scaled_to_all_channels=one * B,
                                    over_device_call=one * B / max(med(ms), 1e-9), device_equals_it_bit_for_bit=bool(same))
    out["rescaled_words"]["over_align_words_wall"] = med(ms) / max(med(al_ms), 1e-9)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rescale_probe.json"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        return child(a)
    tmp = tempfile.mkdtemp(prefix="rescale_probe_")
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
        # The traced child makes N_CALLS calls of rescaled_words without the alignment and N_CALLS with it (one launch of
        # rescale_kernel and of align_index_kernel per call and round), the first of each the warm-up; align_words' launches of
        # align_index_kernel come behind them.
        n = len(k["rescale_kernel"])
        if n and n % (2 * N_CALLS) == 0:
            per = n // 2
            for i, name in enumerate(("kernel_ms_per_call", "with_alignment_kernel_ms_per_call")):
                cut = lambda v: v[i * per:(i + 1) * per]
                per_call = lambda v: float(np.sum(cut(v)[per // N_CALLS:]) / (N_CALLS - 1))
                d["rescaled_words"][name] = {key: per_call(k[key]) for key in ("align_index_kernel", "rescale_kernel")}
            d["rescaled_words"]["launches_per_call"] = per // N_CALLS
            d["align_words"]["kernel_ms_per_call"] = {"align_kernel": float(np.sum(k["align_kernel"][len(k["align_kernel"]) // N_CALLS:]) / (N_CALLS - 1))}
        json.dump(d, open(a.out, "w"), indent=1)
    print(json.dumps(d))


if __name__ == "__main__":
    main()
