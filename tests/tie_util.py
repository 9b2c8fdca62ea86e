"""Tie-dense workloads (tests/test_oracle_ties.py on the CPU, tests/test_gpu_ties.py on the device).

Graph weights and log-likelihoods are quantised to a quantum q (a power of two): every path cost is then a small multiple of q,
exact in float32 whatever the order of addition, so equal sums are BIT-equal and exact cost ties abound -- what quantised
production weights and f16 / bf16 scores do.  The rest of the suite picks its data so that ties do not occur.

The rule on a tie (deviation 3; oracle/wfst_oracle.c g_tie_rule): of the arrivals that equal a token's final
cost, the emitting arc before the epsilon arc, then the lowest arc index; the path ends in the cheapest token, then the lowest
graph state.  The oracle's tie mode states it; its default is the reference's first arrival."""
import numpy as np

import pyoracle
import signed_util as S

Q = 0.5
UTT_SEEDS = [7, 12, 24, 31]   # four utterances of 40 frames over the 3000-state graph
FRAMES = 40


def quantise(x, q=Q):
    """round to multiples of q in float32; + 0.0 turns a -0.0 into +0.0"""
    q = np.float32(q)
    return (np.round(np.asarray(x, np.float32) / q) * q + np.float32(0.0)).astype(np.float32)


def quantised_graph(synth, g, q=Q):
    arcs = g.arcs.copy()
    arcs["w"] = quantise(arcs["w"], q)
    return synth.Graph(g.start, g.final_state, g.state_info, arcs)


def big_workload(synth):
    """(a): the 3000-state graph of the signed-cost workloads, quantised: (graph, tid2pdf, [loglikes])"""
    g = synth.make_hclg_like(S.GRAPH["n_states"], seed=S.GRAPH["seed"], n_tid=S.GRAPH["n_tid"], n_words=S.GRAPH["n_words"])
    m = synth.default_tid2pdf(S.GRAPH["n_tid"])
    mats = [quantise(synth.make_loglikes(g, FRAMES, S.N_PDF, m, seed=s)[0]) for s in UTT_SEEDS]
    return quantised_graph(synth, g), m, mats


# (b): small random graphs (test_gpu_fuzz.random_graph: no planted path, parallel arcs, dense forward epsilon arcs), quantised.
# (seed, states, labels, negative epsilon weights: such a graph cannot take fused closures, signed_util.signed_graph)
SMALL = [(101, 12, 4, False), (102, 25, 5, False), (103, 40, 6, True), (104, 60, 7, False), (105, 33, 3, False), (106, 48, 5, True)]
SMALL_CFGS = [dict(beam=8.0, max_active=1000000, min_active=0, lattice_beam=6.0, prune_interval=10),
              dict(beam=10.0, max_active=20, min_active=5, lattice_beam=6.0, prune_interval=10)]
SMALL_LENS = [9, 23, 40]


def small_workloads(synth):
    """[(name, graph, [loglikes])]"""
    out = []
    for seed, n_states, n_labels, neg in SMALL:
        rng = np.random.default_rng(seed)
        g = S.signed_graph(synth, rng, n_states, n_labels, True)[0] if neg else S.signed_graph(synth, rng, n_states, n_labels, False)[1]
        mats = [quantise(rng.normal(-1.5, 1.0, size=(T, n_labels + 1))) for T in SMALL_LENS]
        out.append(("small%d" % seed, quantised_graph(synth, g), mats))
    return out


HALF_GRAPHS = [1, 4]   # of SMALL: the graphs on which raw half-precision scores tie (tests/test_gpu_ties.py)


def half_workload(synth, wi):
    """(name, graph, raw float32 scores): rng.normal scores, NOT quantised, over the quantised small graph wi"""
    seed, _, n_labels, _ = SMALL[wi]
    name, g, _ = small_workloads(synth)[wi]
    rng = np.random.default_rng(seed + 1000)
    return name, g, [rng.normal(-1.5, 1.0, size=(T, n_labels + 1)).astype(np.float32) for T in SMALL_LENS]


def has_parallel_arcs(g):
    a = g.arcs
    off = 0
    for s in range(len(g.state_info)):
        n = int(g.state_info[s][0])
        row = a[off: off + n]
        em = row[row["ilabel"] != 0]["to"]
        if len(set(em.tolist())) < len(em):
            return True
        off += n
    return False


# (c): three graphs of a few states on which the tie is certain.  Arc lists are (ilabel, olabel, weight, to); every log-likelihood
# is 0, so a path costs the sum of its weights.
HAND_CFG = dict(beam=20.0, max_active=1000000, min_active=0, lattice_beam=10.0, prune_interval=25)


def hand_graphs(synth):
    """[(name, graph, loglikes, use_final_probs, the word of the tie rule's path, the word of the first-arrival path)]"""
    ll = lambda T, n: np.zeros((T, n + 1), np.float32)
    out = []
    # an emitting arrival against an epsilon arrival: in frame 2 state 3 is reached at cost 2 over the emitting arc 2 -> 3 (word 7) and
    # over 1 -> 3, an epsilon arc (word 8), from state 1, which an emitting arc reached at cost 1 in the same frame.  The epsilon arc
    # belongs to the LOWER state, so it has the lower arc index: only the class decides, and without it the word is 8.  (The
    # reference agrees with the rule here whatever the graph: ProcessEmitting runs before the closure, so the emitting arrival
    # is always the first.)
    out.append(("emit_vs_eps", synth.graph_from_arc_lists(5, 0, {
        0: [(1, 0, 0.0, 2)],
        1: [(0, 8, 1.0, 3), (2, 0, 3.0, 1)],
        2: [(2, 0, 1.0, 1), (2, 7, 2.0, 3)],
        3: [(3, 0, 0.0, 4)],
        4: []}, {4: 0.0}), ll(3, 3), True, 7, 7))
    # two epsilon paths of one closure at equal cost: 1 -> 2 -> 4 and 1 -> 3 -> 4, words 5 and 6.  The rule takes the lower arc
    # (2 -> 4, word 5); the reference's closure pops state 3 first (its queue is a stack), so its first arrival says word 6.
    out.append(("two_eps_paths", synth.graph_from_arc_lists(6, 0, {
        0: [(1, 0, 0.0, 1)],
        1: [(0, 0, 1.0, 2), (0, 0, 1.0, 3)],
        2: [(0, 5, 1.0, 4)],
        3: [(0, 6, 1.0, 4)],
        4: [(2, 0, 0.0, 5)],
        5: []}, {5: 0.0}), ll(2, 2), True, 5, 6))
    # two frontier tokens on different states at the best cost in the last frame, no final state reached: words 4 (state 2) and 3
    # (state 1).  The rule ends in state 1 (word 3); the reference's token list holds the last token created first: word 4.
    out.append(("two_ends", synth.graph_from_arc_lists(4, 0, {
        0: [(1, 3, 1.0, 1), (1, 4, 1.0, 2)],
        1: [(1, 0, 0.0, 1)],
        2: [(1, 0, 0.0, 2)],
        3: []}, {3: 0.0}), ll(3, 1), False, 3, 4))
    return out


# (d): biglm.  Two hand-made LM pairs and graphs on which two LM histories of equal cost sit on ONE graph state.
def flat_lm(lmsynth, lp, bo):
    """words 1..4, every unigram log10 prob `lp` and back-off weight `bo`, one bigram (3 4) so that the back-off weights count:
    every history has a state of its own, and histories that differ in their last word cost the same"""
    V = 4
    uni = [((w,), np.float32(-99.0 if w == V + 1 else lp), np.float32(0.0 if w == V + 2 else bo)) for w in range(1, V + 3)]
    return lmsynth.NgramLm(V, [uni, [((3, 4), np.float32(lp), np.float32(0.0))]])


def biglm_hand_graphs(synth):
    """[(name, graph, loglikes, words under the rule, words under rule 2 (highest source pair key))]"""
    ll = lambda T, n: np.zeros((T, n + 1), np.float32)
    out = []
    # words 1 and 2 lead into state 1 at the same cost, in two LM pairs; word 3 then takes both over ONE arc into ONE pair (neither
    # history has a bigram with 3: back-off merges them) at the same cost: equal (cost, arc) from two source tokens
    out.append(("merge", synth.graph_from_arc_lists(4, 0, {
        0: [(1, 2, 0.0, 1), (1, 1, 0.0, 1)],
        1: [(2, 3, 0.0, 2)],
        2: [(3, 0, 0.0, 3)],
        3: []}, {3: 0.0}), ll(3, 3), [1, 3], [2, 3]))
    # the same two histories END on the final state at the same cost: the end token goes to the lower pair key (fin and wf of bp_frontier)
    out.append(("two_final_pairs", synth.graph_from_arc_lists(3, 0, {
        0: [(1, 2, 0.0, 1), (1, 1, 0.0, 1)],
        1: [(2, 0, 0.0, 2)],
        2: []}, {2: 0.0}), ll(2, 2), [1], [1]))
    return out


BIGLM_CFG = dict(beam=12.0, max_active=1000000, min_active=0, lattice_beam=20.0, prune_interval=10)


def quantised_lm(lm, q=Q):
    f = lm.to_fsa()
    f.arcs["weight"] = quantise(f.arcs["weight"], q)
    f.states["backoff_prob"] = quantise(f.states["backoff_prob"], q)
    return f


def biglm_random(lmsynth):
    """(old, new) automata with quantised weights over the words 1..29 of the small random graphs"""
    return (quantised_lm(lmsynth.make_lm(30, 2, 12, 3, 0, 0, seed=11)), quantised_lm(lmsynth.make_lm(30, 3, 15, 3, 12, 2, seed=12)))


class TieOracle:
    """The C oracle in the mode the device is held to here: order-free (deviations 1, 2) AND tie mode."""

    def __init__(self, oracle):
        self.o = oracle

    def decode(self, h, cd, x, m=None, tie=True, **kw):
        try:
            self.o.set_order_free(True)
            self.o.set_tie_rule(tie)
            return self.o.decode(h, pyoracle.Config(**cd), x, m, **kw)
        finally:
            self.o.set_order_free(False)
            self.o.set_tie_rule(False)

    def biglm_decode(self, h, cd, o1, o2, x, m=None, tie=1, **kw):
        try:
            self.o.set_order_free(True)
            self.o.set_tie_rule(tie)
            return pyoracle.biglm_decode(self.o, h, pyoracle.Config(**cd), o1, o2, x, m, fixed=True, **kw)
        finally:
            self.o.set_order_free(False)
            self.o.set_tie_rule(False)

    def prefixes(self, h, cd, x, m=None, tie=True):
        """the best path without final costs after every frame 1..T, decoded frame by frame"""
        return [self.decode(h, cd, x[:k], m, tie, chunk=1, finalize=False, use_final_probs=False) for k in range(1, len(x) + 1)]


def labels(r):
    return (tuple(r.path_ilabel.tolist()), tuple(r.path_olabel.tolist()))
