"""Graphs whose lattices stand at the constants the two n-best kernels (asr-decoder_amd/csrc/wfst_nbest.hip) are cut along (plain
numpy, no GPU).  nbest_kernel: K = 16 entries per state, 64 - K = 48 candidates per selection pass, 16 waves per workgroup, the
final merge.  nbest_paths_kernel: the sort buffer's size S2 (doubled from 64 up to 8192 slots), its chunks, the one-wave variant.

Every graph is a layered DAG on synth.graph_from_arc_lists: emitting arcs go from a layer to the next, epsilon arcs stay inside a
layer, and an utterance has one frame per layer step; decoded at CFG (beam 200, lattice_beam 100: nothing is pruned) the raw lattice
IS the graph, a lattice state per graph state.  Parallel arcs carry distinct transition-ids (each its own log-likelihood column)
and, unless a case wants otherwise, distinct words.  Two families of costs: QUANTISED (every graph weight and log-likelihood a
multiple of 1/8 in [-1, 1]: sums are exact, exact ties dense) and CONTINUOUS (normal draws of both signs).

A graph without final weights has no reachable final state: every state of the last frame is then final (base-inl.h:936-940).

facts() recomputes, from a raw lattice, what a case is named for; tests/test_nbest_geometry.py holds the oracle's lattice of every
case to the case's check, tests/test_gpu_nbest_exact.py the device's."""
import numpy as np

from nbest_util import F32, f2o, kbest_distinct, kbest_paths_dp

CFG = dict(beam=200.0, max_active=1000000, min_active=0, lattice_beam=100.0, prune_interval=10)
LIM = dict(max_frames=32, max_tokens_per_frame=4096, arena_tokens=1 << 14, lattice_links=1 << 15)
NS = (1, 2, 15, 16)                       # nbest_kernel's n
NS_PATHS = (1, 2, 63, 64, 65, 4096)       # nbest_paths_kernel's n: 64 | 65 the one-wave variant's limit, 4096 half the sort buffer


class Net:
    def __init__(self, seed, quantised):
        self.rng, self.quantised = np.random.default_rng(seed), quantised
        self.arcs, self.layer, self.finals, self.fixed = [], [], {}, {}
        self.next_word = 0

    def cost(self):
        return float(self.rng.integers(-8, 9) / 8.0) if self.quantised else float(F32(self.rng.normal(0.0, 1.0)))

    def state(self, layer):
        self.arcs.append([])
        self.layer.append(layer)
        return len(self.arcs) - 1

    def word(self):
        self.next_word += 1
        return self.next_word

    def emit(self, s, t, word=0, w=None, ll=None):
        """an emitting arc with a transition-id of its own among s's arcs; ll: its log-likelihood in its frame, fixed"""
        assert self.layer[t] == self.layer[s] + 1
        lab = 1 + sum(1 for a in self.arcs[s] if a[0])
        self.arcs[s].append((lab, int(word), self.cost() if w is None else float(w), t))
        if ll is not None:
            self.fixed[(self.layer[s], lab)] = float(ll)

    def eps(self, s, t, word=0, w=None):
        assert self.layer[t] == self.layer[s] and t > s
        self.arcs[s].append((0, int(word), self.cost() if w is None else float(w), t))

    def fan(self, s, t, k, words=True):
        for _ in range(k):
            self.emit(s, t, self.word() if words else 0)

    def finish(self, synth, n_utts=1):
        g = synth.graph_from_arc_lists(len(self.arcs), 0, dict(enumerate(self.arcs)), self.finals)
        T = max(self.layer)
        n_cols = 1 + max([a[0] for row in self.arcs for a in row] + [1])
        mats = []
        for _ in range(n_utts):
            x = (self.rng.integers(-8, 9, (T, n_cols)) / 8.0 if self.quantised else self.rng.normal(0.0, 1.0, (T, n_cols))).astype(np.float32)
            for (f, lab), v in self.fixed.items():
                x[f, lab] = v
            mats.append(x)
        return g, mats


# ---- nbest_kernel ----------------------------------------------------------------------------------------------------------------
def fan(synth, quantised):
    """layer 1: nine states of 10 entries, four of 6, 7, 8 and 9, and 130 of one; layer 2: states of 47, 48, 49, 96 and 97
    candidates (4 or 9 sources of ten and one more: every pass boundary cuts a source's list) and of 65 and 130 single-entry
    sources; layer 3: one final state that merges them all (7 x 16 candidates)"""
    N = Net(11, quantised)
    root = N.state(0)
    tens = [N.state(1) for _ in range(9)]
    odd = {k: N.state(1) for k in (6, 7, 8, 9)}
    ones = [N.state(1) for _ in range(130)]
    for s in tens:
        N.fan(root, s, 10)
    for k, s in odd.items():
        N.fan(root, s, k)
    for s in ones:
        N.fan(root, s, 1)
    mids = []
    for srcs in (tens[:4] + [odd[7]], tens[:4] + [odd[8]], tens[:4] + [odd[9]], tens + [odd[6]], tens + [odd[7]], ones[:65], ones):
        x = N.state(2)
        for i, s in enumerate(srcs):
            N.emit(s, x, N.word() if i % 2 else 0)
        mids.append(x)
    end = N.state(3)
    for i, x in enumerate(mids):
        N.emit(x, end, N.word() if i % 3 else 0)
    N.finals[end] = N.cost()
    return N.finish(synth, n_utts=3)


def check_fan(f, quantised):
    assert {47, 48, 49, 96, 97} <= set(f["cands"].tolist()), sorted(set(f["cands"].tolist()))
    single = f["cands"] == f["indeg"]
    assert {65, 130} <= set(f["indeg"][single].tolist())
    assert (f["distinct"] > 16).sum() >= 7 and f["final_cands"] == 16       # (the super-final state: one source of 16)
    assert 112 in f["cands"].tolist()
    if quantised:
        assert f["tie_at_K"].any(), "no bit-equal totals across a 16th place"
        assert f["final_ties"], "no bit-equal totals across the n-th place of the answer for any n of %s" % (NS,)
    else:
        assert not f["tie_at_K"].any() and not f["final_ties"]


def widths(synth, quantised):
    """frames of 15, 16, 17 and 33 lattice states: the workgroup's batches of 16 waves and their tails"""
    N = Net(12, quantised)
    prev = [N.state(0)]
    for layer, wd in enumerate((15, 16, 17, 33, 1), 1):
        cur = [N.state(layer) for _ in range(wd)]
        for i, t in enumerate(cur):      # (every state of a layer is a source: none is pruned for leading nowhere)
            for s in sorted({prev[i % len(prev)], int(N.rng.choice(prev))} if wd > 1 else prev):
                N.emit(s, t, N.word() if N.rng.random() < 0.5 else 0)
        prev = cur
    N.finals[prev[0]] = N.cost()
    return N.finish(synth)


def check_widths(f, quantised):
    assert f["widths"][:6] == [1, 15, 16, 17, 33, 2], f["widths"]


def finals(synth, quantised, m):
    """no final weight anywhere: the m states of the last frame are all final, each with 16 entries (m = 4: 64 candidates, two
    passes of the final merge)"""
    N = Net(13 + m, quantised)
    root, hub = N.state(0), N.state(1)
    N.fan(root, hub, 20)
    for _ in range(m):
        N.emit(hub, N.state(2), N.word())
    return N.finish(synth)


def check_finals(m):
    def check(f, quantised):
        assert f["final_states"] == m and f["final_cands"] == 16 * m and f["final_distinct"] == 16 * m, (f["final_states"], f["final_cands"])
    return check


def merge(synth, quantised):
    """word 5 into a and into b at a bit-equal tot (1.5) and lm 0.5 | 0.25; c takes both without a word at equal cost: the same
    history twice, bit-equal tot, the lower lm must stay.  d takes both with word 7 at different costs: the same history twice,
    different totals.  The same once more with word 6 and the two lm the other way round, so that the lower lm arrives over the
    later arc in one of the two whatever order the device lists them in.  (Quantised costs only: the ties are the case.)"""
    N = Net(14, True)
    root, end = N.state(0), None
    mids = []
    for word, (wa, wb) in ((5, (0.5, 0.25)), (6, (0.25, 0.5))):
        a, b = N.state(1), N.state(1)
        N.emit(root, a, word, w=wa, ll=wa - 1.5)        # tot 1.5 over either arc
        N.emit(root, b, word, w=wb, ll=wb - 1.5)
        mids.append((a, b))
    for a, b in mids:
        c, d = N.state(2), N.state(2)
        N.emit(a, c, 0, w=0.5, ll=-0.5)
        N.emit(b, c, 0, w=0.5, ll=-0.5)
        N.emit(a, d, 7, w=0.125, ll=-0.5)
        N.emit(b, d, 7, w=0.75, ll=-0.5)
        end = N.state(3) if end is None else end
        N.emit(c, end, 0, w=0.25, ll=0.25)
        N.emit(d, end, 0, w=0.25, ll=0.25)
    N.finals[end] = 0.5
    return N.finish(synth)


def check_merge(f, quantised):
    two = (f["cands"] == 2) & (f["distinct"] == 1)
    assert (two & f["merged_lm"]).sum() == 2 and (two & ~f["merged_lm"]).sum() == 2
    assert f["final_distinct"] == 4


def eps_chains(synth, quantised):
    """epsilon chains of depth 1, 2 and 5 inside frame 1, every other arc with a word, each chain's states entered from the root as
    well; and a triangle p -> s -> d, p -> d inside frame 2 in which d receives p's histories twice (directly, cheaper, and over
    s): when the device computes s before p, a later round inserts p's histories into s's list, which moves s's own entries to
    other ranks -- d's backpointers into s change while none of d's costs does (a kernel that compares costs and hashes
    only, not the backpointers, keeps stale ones and fails this case and the epsilon-chains golden: tried)"""
    N = Net(15, quantised)
    root = N.state(0)
    heads = []
    for depth in (1, 2, 5):
        chain = [N.state(1) for _ in range(depth + 1)]
        for i, s in enumerate(chain):
            N.fan(root, s, 2)
            if i:
                N.eps(chain[i - 1], s, N.word() if i % 2 else 0)
        heads.append(chain[-1])
    s, p, d = N.state(2), N.state(2), N.state(2)      # (s before p in the graph; the lattice numbers p first)
    for h in heads:
        N.emit(h, s, N.word())
        N.emit(h, p, N.word())
    N.arcs[p].append((0, 0, 0.125, s))                # p -> s: an epsilon arc to a lower graph state id
    N.eps(p, d, 0, w=-1.0)
    N.eps(s, d, 0, w=0.125)
    end = N.state(3)
    N.emit(d, end, N.word())
    N.emit(s, end, 0)
    N.finals[end] = N.cost()
    return N.finish(synth)


def check_eps_chains(f, quantised):
    assert f["eps_depths"][1] == 5 and f["eps_depths"][2] == 2 and f["n_eps_words"] >= 3, (f["eps_depths"], f["n_eps_words"])


def few(synth, quantised, k):
    """k distinct word sequences only (k = 1: a line of 3 words; k = 3: four parallel arcs, two without a word and one each with
    word 1 and word 2, then a line without words: the path without any word is among the answers, over two paths)"""
    N = Net(16 + k, quantised)
    s0, s1, s2 = N.state(0), N.state(1), N.state(2)
    if k == 1:
        N.emit(s0, s1, N.word())
        N.emit(s1, s2, N.word())
    else:
        for w in (0, 0, 1, 2):
            N.emit(s0, s1, w)
        N.emit(s1, s2, 0)
    end = N.state(3)
    N.emit(s2, end, N.word() if k == 1 else 0)
    N.finals[end] = N.cost()
    return N.finish(synth)


def check_few(k):
    def check(f, quantised):
        assert f["final_distinct"] == k, f["final_distinct"]
        assert k == 1 or f["wordless_answer"]
    return check


def line20(synth, quantised):
    """tests/test_gpu_nearest.py's line of 20 words, the last step doubled: two paths of 20 words each"""
    N = Net(19, quantised)
    prev = N.state(0)
    for k in range(1, 21):
        s = N.state(k)
        N.emit(prev, s, k)
        if k == 20:
            N.emit(prev, s, 21)
        prev = s
    N.finals[prev] = 0.0
    return N.finish(synth)


def check_line20(f, quantised):
    assert f["final_distinct"] == 2 and f["widths"][:20] == [1] * 20


NBEST_CASES = {
    "fan": (fan, check_fan, (False, True)),
    "widths": (widths, check_widths, (False, True)),
    "finals1": (lambda s, q: finals(s, q, 1), check_finals(1), (False,)),
    "finals4": (lambda s, q: finals(s, q, 4), check_finals(4), (False, True)),
    "finals7": (lambda s, q: finals(s, q, 7), check_finals(7), (False,)),
    "merge": (merge, check_merge, (True,)),
    "eps_chains": (eps_chains, check_eps_chains, (False, True)),
    "few1": (lambda s, q: few(s, q, 1), check_few(1), (False,)),
    "few3": (lambda s, q: few(s, q, 3), check_few(3), (False, True)),
    "line20": (line20, check_line20, (False,)),
}


def nbest_case_ids():
    return [(name, q) for name, (_, _, fam) in NBEST_CASES.items() for q in fam]


def facts(L):
    """what the cases are named for, from a raw lattice (pyoracle.RawLattice / align_util.from_gpu)"""
    st = {}
    best = kbest_distinct(L, 16, stats=st)
    frame = np.asarray(L.st_frame)
    st["widths"] = np.bincount(frame).tolist()
    o = f2o(st["final_tots"])
    st["final_ties"] = [n for n in NS if n < len(o) and o[n - 1] == o[n]]
    depth = np.zeros(L.n_states, np.int64)     # along the arcs inside a frame
    eps = np.nonzero(np.asarray(L.a_il) == 0)[0]
    for a in eps[np.argsort(np.asarray(L.a_src)[eps], kind="stable")]:
        depth[L.a_dst[a]] = max(depth[L.a_dst[a]], depth[L.a_src[a]] + 1)
    st["eps_depths"] = [int(depth[frame == f].max()) for f in range(int(frame.max()) + 1)]
    st["n_eps_words"] = int((np.asarray(L.a_ol)[eps] != 0).sum())
    st["wordless_answer"] = any(b["n_words"] == 0 for b in best)
    return st


# ---- nbest_paths_kernel ----------------------------------------------------------------------------------------------------------
def chain(synth, quantised, steps, ways_after=()):
    """`steps` two-way word choices in a row (2^steps paths at their end), then one step of each of ways_after's widths; a final
    weight shared by all paths.  Words stay below 150 (the LM pair of tests/test_compose_lattice.py)."""
    N = Net(20 + steps, quantised)
    prev = N.state(0)
    for k, ways in enumerate([2] * steps + list(ways_after), 1):
        s = N.state(k)
        N.fan(prev, s, ways)
        prev = s
    N.finals[prev] = N.cost()
    return N.finish(synth)


def sortbuf(synth, quantised):
    """layer 1: states of 31, 32, 33 and 64 paths; layer 2: states whose candidates are 63 = 31 + 32, 64 = 32 + 32 (parallel arcs),
    65 = 32 + 33, 127 = 64 + 32 + 31, 128 = 64 + 32 + 32 and 129 = 64 + 32 + 33; one final state"""
    N = Net(40, quantised)
    root = N.state(0)
    a, b, c, d = (N.state(1) for _ in range(4))
    for s, k in ((a, 31), (b, 32), (c, 33), (d, 64)):
        N.fan(root, s, k)
    end_srcs = []
    for srcs in ((a, b), (b, b), (b, c), (d, b, a), (d, b, b), (d, b, c)):
        x = N.state(2)
        for s in srcs:
            N.emit(s, x, N.word())
        end_srcs.append(x)
    end = N.state(3)
    for x in end_srcs:
        N.emit(x, end, N.word())
    N.finals[end] = N.cost()
    return N.finish(synth)


def check_chain14(f, quantised):
    c = f["cands"].tolist()
    assert 8192 in c and 12288 in c and max(c) == 12288 and f["n_paths"] == 4096
    o = f2o(f["widest_costs"])
    order = np.argsort(o, kind="stable")
    assert o[order[4095]] == o[order[4096]], "no tie across the 4096th place"
    kept = order[:4096]
    # the kept entries of the first chunk (q < 8192) and of the second share totals: the order inside such a tie is the candidate number's
    assert len(np.intersect1d(o[kept[kept < 8192]], o[kept[kept >= 8192]])) > 0, "no tie across the chunk boundary among the kept"


PATHS_CASES = {
    "small": (lambda s, q: chain(s, q, 7), lambda f, q: f["cands"].max() == 128 and f["final_cands"] == 128, (False, True)),
    "sortbuf": (sortbuf, lambda f, q: {63, 64, 65, 127, 128, 129} <= set(f["cands"].tolist()), (False, True)),
    "chain14": (lambda s, q: chain(s, q, 12, (2, 3)), check_chain14, (True,)),
}


def paths_case_ids():
    return [(name, q) for name, (_, _, fam) in PATHS_CASES.items() for q in fam]


def paths_facts(D):
    st = {}
    st["n_paths"] = len(kbest_paths_dp(D, 4096, stats=st))
    return st
