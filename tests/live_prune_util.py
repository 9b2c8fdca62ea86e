"""Shared by the pruned-live-lattice tests (wfst_decoder_set_live_lattice_prune): the numpy restatement of the snapshot lattice, and
what the GPU tests need to set a case up.

restate(L, lattice_beam, all_final): FinalizeDecoding's pruning (PruneForwardLinksFinal + PruneForwardLinks + PruneTokensForFrame,
my-decoder/online-decoder-base-inl.h:725-847) in float32 over a LIVE raw lattice L -- the history as the last PruneActiveTokens pass
left it plus the raw frames since, as GetRawLattice lists it mid-utterance (states with frame, graph state and forward cost, arcs
with graph and acoustic cost):
  newest frame: extra = cost + final_cost - final_best over the final tokens (final_cost 0: the project's graphs have one final state
    of weight one; L.st_final, taken with use_final_probs, marks them -- every token of the frame if none is final in the graph);
    all_final: every token of the frame final at cost 0.  extra > lattice_beam: +inf.
  a link s -> d: link_extra = extra[d] + ((cost[s] + ac + graph) - cost[d]), alive iff <= lattice_beam; extra[s] = the
    least of its living links' link_extras, none below 0.
  frames newest to oldest; the epsilon links inside a frame to their fixpoint (min is order-free) before the emitting links into it
    are priced.  A token is alive iff its extra is finite.
tests/test_live_prune_restatement.py proves it against the order-free oracle's finalized lattices; the GPU tests then use it as the
yardstick where no twin exists (use_final_probs = 0)."""
import numpy as np

import pyoracle
from golden_util import bits

F32 = np.float32
INF = F32(np.inf)


def as_raw(d):
    return pyoracle.RawLattice(True, d["n_states"], 0, d["st_final"], d["a_src"], d["a_dst"], d["a_ilabel"], d["a_olabel"],
                               d["a_graph"], d["a_acoustic"], d["st_frame"], d["st_state"], d["st_cost"])


def nodes(L):
    k = np.stack([L.st_frame, L.st_gstate, L.st_final, bits(L.st_cost)], axis=1)
    return k[np.lexsort(k.T[::-1])]


def same_lattice(L, O, what):
    assert np.array_equal(nodes(L), nodes(O)), what + " states"
    assert np.array_equal(L.labelled_arcs(), O.labelled_arcs()), what + " arcs"


def frame_counts(L):
    """states per frame of a raw lattice"""
    return np.bincount(L.st_frame, minlength=int(L.st_frame.max()) + 1)


def restate(L, lattice_beam, all_final=False):
    lb = F32(lattice_beam)
    cost = L.st_cost.astype(F32)
    frame = L.st_frame
    nd = int(frame.max())
    src, dst = L.a_src, L.a_dst
    # link cost - cost of the destination, in the decoder's order: ((cost_src + ac) + graph) - cost_dst
    with np.errstate(invalid="ignore", over="ignore"):
        rel = ((cost[src] + L.a_ac.astype(F32)) + L.a_graph.astype(F32)) - cost[dst]
    newest = frame == nd
    fin = newest if all_final else (newest & (L.st_final != 0))
    assert fin.any()
    extra = np.full(L.n_states, INF, F32)
    final_best = cost[fin].min()
    extra[fin] = (cost[fin] + F32(0.0)) - final_best
    extra[extra > lb] = INF
    alive_arc = np.zeros(len(src), bool)
    is_eps = frame[src] == frame[dst]
    a_frame = frame[dst]

    def price(idx):
        with np.errstate(invalid="ignore"):
            le = extra[dst[idx]] + rel[idx]
        le[~np.isfinite(extra[dst[idx]])] = INF
        return le

    for k in range(nd, -1, -1):
        if k < nd:   # the emitting links frame k -> k + 1, priced from frame k + 1's final extras
            idx = np.nonzero(~is_eps & (a_frame == k + 1))[0]
            le = price(idx)
            ok = le <= lb
            alive_arc[idx] = ok
            np.minimum.at(extra, src[idx[ok]], np.maximum(le[ok], F32(0.0)))
        idx = np.nonzero(is_eps & (a_frame == k))[0]
        if len(idx):
            for _ in range(4096):
                le = price(idx)
                ok = le <= lb
                before = extra.copy()
                np.minimum.at(extra, src[idx[ok]], np.maximum(le[ok], F32(0.0)))
                if np.array_equal(bits(before), bits(extra)):
                    break
            else:
                raise AssertionError("the epsilon links of frame %d do not settle" % k)
            alive_arc[idx] = price(idx) <= lb
    alive = np.isfinite(extra)
    assert np.all(alive[src[alive_arc]]) and np.all(alive[dst[alive_arc]])
    new_id = np.cumsum(alive) - 1
    st_final = np.where(newest, 1, 0).astype(np.int32) if all_final else L.st_final.astype(np.int32)
    return pyoracle.RawLattice(True, int(alive.sum()), 0, st_final[alive], new_id[src[alive_arc]].astype(np.int32),
                               new_id[dst[alive_arc]].astype(np.int32), L.a_il[alive_arc], L.a_ol[alive_arc], L.a_graph[alive_arc],
                               L.a_ac[alive_arc], frame[alive], L.st_gstate[alive], L.st_cost[alive])


# ---- set-up of the GPU cases ---------------------------------------------------------------------------------------------------
PREFIXES = (1, 24, 25, 26, 53)
LENGTHS = (60, 53, 41, 26)
LIM = dict(max_frames=128, max_tokens_per_frame=32768, arena_tokens=1 << 20, lattice_links=1 << 21)


def config(lattice_beam, beam=11.0, prune_interval=25):
    return dict(beam=beam, max_active=1000000, min_active=0, lattice_beam=lattice_beam, prune_interval=prune_interval)


def small_graph(synth, tmp_path, n_states=2000, seed=13, name="g.bin"):
    """the 2000-state graph of the twin cases: (synthetic graph, tid2pdf, its file)"""
    g = synth.make_hclg_like(n_states, seed=seed, n_tid=2000, n_words=3000)
    m = synth.default_tid2pdf(2000)
    path = str(tmp_path / name)
    g.write(path)
    return g, m, path


def utterances(synth, g, m, lengths=LENGTHS, seed=40):
    return [synth.make_loglikes(g, t, 1000, m, seed=seed + i, mu=-2.3)[0] for i, t in enumerate(lengths)]


def advance_to(dec, dev, lengths, r):
    dec.advance([t.data_ptr() for t in dev], [min(r, t) for t in lengths], 1000)


def advance_in_two_chunks(dec, dev, lengths, frm, to):
    """from `frm` to `to` frames in two advance calls"""
    mid = frm + (to - frm) // 2
    if mid > frm:
        advance_to(dec, dev, lengths, mid)
    advance_to(dec, dev, lengths, to)
