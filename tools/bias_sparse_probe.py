"""What phrase boosting over reachable cells costs (wfst_decoder_biased_words_sparse) beside the dense call
(wfst_decoder_biased_words), on the set-up of profiles/bias_probe.json: 64 live channels at frame 150 of bench.py's headline lattice
configuration, live-prune mode 1, four settings (1, 1, 0, bs) with bs = 0.5 / 1 / 2 / 4, tools/bias_probe.py's lists.

    python tools/bias_sparse_probe.py --out profiles/bias_sparse_probe.json [--frame 150] [--channels 64]

Recorded:
 - at 2, 16, 64 and 256 nodes the wall time of one call of each kind over all channels (median of three calls after one warm-up
   call), in the same run; at 1 024, 4 096, 16 384 and 65 536 nodes (the lists padded with words no lattice holds) the sparse call's;
 - per size n_cells / states at the median and the maximum over the channels (the device's n_cells), and from the restatement
   (tests/bias_sparse_util.py) on the fetched lattices the largest |R(t)|, the edges, and the reach regions' bytes by the driver's
   rule of first sizes and growth;
 - the device's answers on channel 0 against the restatement, bit for bit (a mismatch ends the probe);
 - from a second run under `rocprofv3 --kernel-trace` (the program after `--`) the time of bias_kernel, bias_reach_kernel,
   bias_sparse_kernel and align_index_kernel per call.  The calls are told apart by their align_index_kernel launches: the dense
   call launches it once per round, the sparse call once.
Not measured: an idle card (the machines are shared) and a service end to end.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bias_probe as BP  # noqa: E402  (make_list, rounds_of)

N_CALLS = 4
SMALL = (2, 16, 64, 256)
LARGE = (1024, 4096, 16384, 65536)
BOOSTS = BP.BOOSTS
KERNELS = ("align_index_kernel", "rescale_kernel", "bias_kernel", "bias_reach_kernel", "bias_sparse_kernel")


def region_ints(states, arcs, cells, edges, ns_cap, na_cap, limit=4 << 20):
    """the ints of a channel's reach region once it holds `cells` and `edges`: the driver's first sizes, grown fourfold"""
    ccap, ecap = min(limit, max(1024, 4 * states)), min(16 * limit, max(4096, 8 * arcs))
    launches = 1
    while ccap < cells:
        ccap, launches = min(limit, 4 * ccap), launches + 1
    while ecap < edges:
        ecap, launches = min(16 * limit, 4 * ecap), launches + 1
    return (ns_cap + 1) + ns_cap + (na_cap + 1) + 2 * ccap + 2 * ecap + ns_cap, launches


def child(a):
    import torch

    import bias_sparse_util as S
    import bias_util as B
    from align_util import from_gpu

    pkg = importlib.import_module("asr-decoder_amd")
    synth, wd = pkg.synth, pkg.wfstdec
    P, nB, T = a.pdfs, a.channels, a.frame
    m = synth.default_tid2pdf(2 * P)
    gpath = a.graph_cache % a.states
    g = synth.Graph.read(gpath) if os.path.exists(gpath) else None
    if g is None:
        g = synth.make_hclg_like(a.states, seed=7, n_tid=2 * P)
        g.write(gpath)
    print("bias_sparse_probe: graph ready", file=sys.stderr, flush=True)
    mats = [synth.make_loglikes_multi(g, T, P, m, seed=i, n_paths=272, mu=-4.0, sigma=1.0, jitter=0.5, ac_lo=0.5)[0] for i in range(nB)]
    dev = [torch.from_numpy(x).to("cuda:0") for x in mats]
    ptrs = [t.data_ptr() for t in dev]
    graph = wd.Graph.from_arrays(g.start, g.final_state, g.state_info, g.arcs)
    graph.set_tid2pdf(m)
    cfg = dict(beam=13.0, max_active=1000000, min_active=0, lattice_beam=7.0, prune_interval=25)
    dec = wd.BatchDecoder(graph, wd.Config(**cfg), nB, max_frames=T + 8, max_tokens_per_frame=65536, lattice_links=a.lattice_links)
    dec.init()
    for r in list(range(25, T, 25)) + [T]:
        dec.advance(ptrs, [r] * nB, P)
    dec.sync()
    dec.set_live_lattice_prune(True)
    print("bias_sparse_probe: %d channels at frame %d" % (nB, T), file=sys.stderr, flush=True)

    def timed(f):
        ms, res = [], None
        for _ in range(N_CALLS):
            t0 = time.perf_counter()
            res = f()
            ms.append((time.perf_counter() - t0) * 1e3)
        return ms[1:], res

    med = lambda v: float(np.median(v))
    settings = [(1.0, 1.0, 0.0, bs) for bs in BOOSTS]
    out = dict(channels=nB, frame=T, live_prune_mode=1, config=cfg, boosts=list(BOOSTS), small=list(SMALL), large=list(LARGE), calls=N_CALLS,
               not_measured=["an idle card: the machine is shared", "a service end to end"])
    ms, plain = timed(lambda: dec.rescaled_words([(1.0, 1.0, 0.0)] * len(BOOSTS), use_final_probs=True))
    out["rescaled_words"] = dict(settings=len(BOOSTS), wall_ms=ms, wall_ms_median=med(ms))
    lat = [from_gpu(dec.raw_lattice(c, True)) for c in range(nB)]
    states, arcs = [L.n_states for L in lat], [len(L.a_src) for L in lat]
    out["raw_states"] = dict(min=int(min(states)), median=med(states), max=int(max(states)), total=int(sum(states)))
    out["raw_arcs"] = dict(min=int(min(arcs)), median=med(arcs), max=int(max(arcs)), total=int(sum(arcs)))
    nb = dec.nbest_words(5)
    out["by_size"] = {}
    for nodes in SMALL + LARGE:
        made = [BP.make_list(plain[c][0]["hyp_words"], [p["words"] for p in nb[c][1][1:]], nodes) for c in range(nB)]
        phrases = [x[0] for x in made]
        row = dict(phrases_from_the_lattice_median=med([x[1] for x in made]))
        if nodes in SMALL:   # the dense call first, on the same lists in the same run
            lists = wd.BiasLists.from_phrases(phrases)
            need = [s * int(j) * len(BOOSTS) for s, j in zip(states, lists.info()["n_nodes"])]
            dms, dres = timed(lambda: dec.biased_words(lists, None, settings, use_final_probs=True))
            lists.free()
            row.update(dense_wall_ms=dms, dense_wall_ms_median=med(dms), dense_cell_bytes=8 * int(sum(need)), dense_rounds=BP.rounds_of(need))
        books = wd.BiasBooks.from_phrases(phrases)
        info = books.info()
        sms, res = timed(lambda: dec.biased_words_sparse(books, None, settings, use_final_probs=True))
        books.free()
        cells = [row_[0]["n_cells"] for row_ in res]
        need = [c * len(BOOSTS) for c in cells]
        row.update(nodes=dict(min=int(info["n_nodes"].min()), max=int(info["n_nodes"].max())), book_device_bytes=int(info["device_bytes"]),
                   sparse_wall_ms=sms, sparse_wall_ms_median=med(sms), channel_failures=int(sum(r[0]["status"] != 0 for r in res)),
                   n_cells=dict(total=int(sum(cells)), max=int(max(cells))),
                   n_cells_per_state=dict(median=med([c / float(s) for c, s in zip(cells, states)]), max=float(max(c / float(s) for c, s in zip(cells, states)))),
                   sparse_cell_bytes=8 * int(sum(need)), sparse_rounds=BP.rounds_of(need),
                   hits_per_answer_mean=[float(np.mean([res[c][q]["n_hits"] for c in range(nB)])) for q in range(len(BOOSTS))])
        if nodes in SMALL:
            same = all(np.asarray(res[c][q][k]).tobytes() == np.asarray(dres[c][q][k]).tobytes() for c in range(nB) for q in range(len(BOOSTS))
                       for k in ("found", "n_arcs", "n_hyp", "hyp_words", "begin", "end", "biased_cost", "bonus", "tot", "lm", "n_hits", "hit_phrase", "hit_word", "status"))
            row["equals_the_dense_call_in_every_byte"] = bool(same)
            if not same:
                sys.exit("%d nodes: the sparse call's answers differ from the dense call's" % nodes)
        if not a.no_restatement:
            # channel 0 against the restatement, bit for bit; the sets' sizes of every channel from the restatement
            A0 = S.compile_book(phrases[0])
            want = S.bias_many_sparse(lat[0], A0, settings)
            for q in range(len(BOOSTS)):
                B.same_answer(res[0][q], want[q], "%d nodes, channel 0, setting %d" % (nodes, q))
                assert res[0][q]["n_cells"] == want[q]["n_cells"]
            row["channel_0_equals_the_restatement"] = True
            biggest, edges, ints, launches = 0, [], 0, 1
            ns_cap, na_cap = max(states), max(arcs)
            for c in range(nB):
                # (the padding is one-word phrases of words no lattice holds: their nodes are never reached, the sets' sizes are those
                # under the phrases from the lattice alone)
                Ac = A0 if c == 0 else S.compile_book(phrases[c][:made[c][1]])
                R = S.reach(lat[c], Ac)
                assert sum(len(r) for r in R) == cells[c], "the device's n_cells is the restatement's"
                biggest = max(biggest, max(len(r) for r in R))
                g32 = lat[c].a_graph.astype(np.float32) + lat[c].a_ac.astype(np.float32)
                e = int(sum(len(R[int(s)]) for s, ok in zip(lat[c].a_src, np.isfinite(g32)) if ok))
                edges.append(e)
                n, k = region_ints(states[c], arcs[c], cells[c], e, ns_cap, na_cap)
                ints, launches = ints + n, max(launches, k)
            row.update(largest_set=int(biggest), edges=dict(total=int(sum(edges)), max=int(max(edges))), reach_region_bytes=4 * int(ints),
                       reach_launches_by_the_growth_rule=int(launches), n_cells_equal_the_restatement_on_every_channel=True)
        out["by_size"][str(nodes)] = row
        print("bias_sparse_probe: %d nodes done" % nodes, file=sys.stderr, flush=True)
    dec.free()
    graph.free()
    json.dump(out, open(a.child, "w"))


def trace_rows(trace_dir):
    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            for r in csv.DictReader(f):
                for key in KERNELS:
                    if key in r.get("Kernel_Name", ""):
                        rows.append((int(r["Start_Timestamp"]), key, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6))
                        break
    return sorted(rows)


def split_calls(rows, d):
    """per call the kernels' summed times, the calls cut at their align_index_kernel launches; None where the launches do not come in
    the expected count"""
    plan = [("rescaled_words", None, 1)] * N_CALLS   # (what, size, align_index launches of one call)
    for n in SMALL + LARGE:
        if n in SMALL:
            plan += [("dense", n, d["by_size"][str(n)]["dense_rounds"])] * N_CALLS
        plan += [("sparse", n, 1)] * N_CALLS
    starts = [i for i, r in enumerate(rows) if r[1] == "align_index_kernel"]
    if len(starts) != sum(p[2] for p in plan):
        return None
    calls, at = [], 0
    for what, n, k in plan:
        lo = starts[at]
        hi = starts[at + k] if at + k < len(starts) else len(rows)
        at += k
        ms = {key: 0.0 for key in KERNELS}
        count = {key: 0 for key in KERNELS}
        for _, key, t in rows[lo:hi]:
            ms[key] += t
            count[key] += 1
        calls.append((what, n, ms, count))
    return calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", type=int, default=2850000)
    ap.add_argument("--pdfs", type=int, default=3000)
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--frame", type=int, default=150)
    ap.add_argument("--lattice-links", type=int, default=25165824)
    ap.add_argument("--timeout", type=int, default=540)
    ap.add_argument("--graph-cache", default="/tmp/wfst_bench_graph_%d.bin")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bias_sparse_probe.json"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--no-restatement", action="store_true")
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        return child(a)
    tmp = tempfile.mkdtemp(prefix="bias_sparse_probe_")
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
                              sys.executable, os.path.abspath(__file__), "--child", os.path.join(tmp, "traced.json"), "--no-restatement"] + args)
        if rc != 0:
            sys.exit("the traced run ended with status %d: nothing more is started" % rc)
        rows = trace_rows(tmp)
        calls = split_calls(rows, d)
        if calls is None:   # (the launches do not come in the expected count: the totals are kept instead)
            d["kernel_ms_totals_of_the_traced_run"] = {k: float(sum(t for _, key, t in rows if key == k)) for k in KERNELS}
            d["kernel_launches_of_the_traced_run"] = {k: int(sum(1 for _, key, _t in rows if key == k)) for k in KERNELS}
        else:
            for i in range(0, len(calls), N_CALLS):
                what, n, _, _ = calls[i]
                part = calls[i + 1:i + N_CALLS]   # (the first call of each kind and size is the warm-up)
                mean = {k: float(np.mean([c[2][k] for c in part])) for k in KERNELS}
                launches = {k: int(part[-1][3][k]) for k in KERNELS}
                if what == "rescaled_words":
                    d["rescaled_words"]["kernel_ms_per_call"] = mean["rescale_kernel"]
                elif what == "dense":
                    d["by_size"][str(n)].update(bias_kernel_ms_per_call=mean["bias_kernel"], dense_align_index_ms_per_call=mean["align_index_kernel"])
                else:
                    d["by_size"][str(n)].update(bias_reach_kernel_ms_per_call=mean["bias_reach_kernel"], bias_sparse_kernel_ms_per_call=mean["bias_sparse_kernel"],
                                                sparse_align_index_ms_per_call=mean["align_index_kernel"], bias_reach_kernel_launches_per_call=launches["bias_reach_kernel"],
                                                bias_sparse_kernel_launches_per_call=launches["bias_sparse_kernel"])
        json.dump(d, open(a.out, "w"), indent=1)
    print(json.dumps(d))


if __name__ == "__main__":
    main()
