"""Workloads whose path costs are negative or change sign (tests/test_gpu_signed_costs.py and its CPU companion in
tests/test_oracle_vs_reference.py).  Every other workload of the suite keeps path costs positive: log-likelihoods around -2 over
graphs with weights >= 0.  Here the same recipe is shifted upwards, as pseudo-log-likelihoods after prior division are:

  zero      no shift: the positive control (a failure there is not about the sign)
  crossing  + 2.0, about the mean cost of a frame: the best cost of a frame changes sign several times per utterance, and a
            frame's costs lie on both sides of zero (the orderable keys of such a frame share no leading bit)
  negative  + 4.0: every path cost is negative from frame 1 on and falls throughout the utterance

The utterances (frames, seed) were picked on the CPU oracle: with both configurations each of them changes the sign of its
per-frame best cost 5 or 6 times under `crossing`, holds 9 to 19 frames with more than max_active tokens whose costs straddle zero
under the binding configuration, ends below -100 under `negative`, and has no exact cost tie on its best path."""
import numpy as np

GRAPH = dict(n_states=3000, seed=17, n_tid=600, n_words=500)
N_PDF = 300
UTTS = [(55, 7), (60, 12), (60, 24)]   # (frames, make_loglikes seed)
SHIFTS = dict(zero=0.0, crossing=2.0, negative=4.0)
BEAM_ONLY = dict(beam=11.0, max_active=1000000, min_active=0, lattice_beam=6.0)
BINDING = dict(beam=13.0, max_active=300, min_active=50, lattice_beam=6.0)
CFGS = [BEAM_ONLY, BINDING]


def shifted(x, shift):
    return (x + np.float32(shift)).astype(np.float32)


def workloads(synth, utts=UTTS):
    """(graph, tid2pdf, {shift name: [float32 [frames][N_PDF] per utterance]})"""
    g = synth.make_hclg_like(GRAPH["n_states"], seed=GRAPH["seed"], n_tid=GRAPH["n_tid"], n_words=GRAPH["n_words"])
    m = synth.default_tid2pdf(GRAPH["n_tid"])
    base = [synth.make_loglikes(g, T, N_PDF, m, seed=s)[0] for T, s in utts]
    return g, m, {name: [shifted(x, sh) for x in base] for name, sh in SHIFTS.items()}


def sign_changes(frame_best):
    """how often the per-frame best cost (frames 1..T of a trace) changes sign; exact zeros do not count"""
    s = np.sign(np.asarray(frame_best, np.float32)[1:])
    s = s[s != 0]
    return int((s[1:] != s[:-1]).sum())


def straddling_frames(frame_ntoks, frame_best, cd):
    """frames with more tokens than max_active whose beam reaches across zero: GetCutoff's k-th smallest runs over costs of both signs"""
    fb = np.asarray(frame_best, np.float32)
    return int(((np.asarray(frame_ntoks) > cd["max_active"]) & (fb < 0) & (fb + np.float32(cd["beam"]) > 0)).sum())


def signed_graph(synth, rng, n_states, n_labels, negative_eps):
    """tests/test_gpu_fuzz.py's random_graph with weights of both signs: 1.0 off every emitting arc (uniform 0..3 before).
    negative_eps: also 1.0 off the final costs and 0.5 off the forward epsilon arcs (uniform 0.01..2.5 before; they go forward only,
    so there is still no cycle, let alone a negative one).  In the flat format a final cost IS an epsilon arc (into the super-final
    state), so a negative one is a negative epsilon weight like any other: such a graph cannot take fused closures.
    Returns (the signed graph, random_graph's own)."""
    from test_gpu_fuzz import random_graph

    g = random_graph(synth, rng, n_states, n_labels)
    arcs = g.arcs.copy()
    emit = arcs["ilabel"] != 0
    arcs["w"][emit] -= np.float32(1.0)
    if negative_eps:
        final = ~emit & (arcs["to"] == g.final_state)
        arcs["w"][final] -= np.float32(1.0)
        arcs["w"][~emit & ~final] -= np.float32(0.5)
    return synth.Graph(g.start, g.final_state, g.state_info, arcs), g
