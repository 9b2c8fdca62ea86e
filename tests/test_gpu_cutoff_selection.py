"""-m gpu: GetCutoff's radix selection (wfst_kernels.hip kth_smallest_t) at its register, cache, batch, rank and pass-count edges, on
the cases of tests/selection_util.py (tests/test_selection_cases.py proves that each does what it claims and that moving its limit by
one changes the frame that follows).  The selection is driven through the decoders; every case names the kernel path it is about
and asserts dec.path_flags() before and after, and everything is held bit for bit to the ORDER-FREE oracle:

* the frontier after every frame: distinct states, the oracle's count, every state at a bit-equal cost, the same best cost (biglm:
  a token is a (state, LM state) pair -- the oracle's count, and the same multiset of (graph state, cost bits));
* the best path after finalize(), hop for hop (the ladder's rungs, whose coarse costs tie: against the oracle under the decoders' tie
  rule, which holds the total cost's bits and the choice among equally cheap arcs too);
* in lattice legs the raw lattice, state by state and arc by arc;
* degraded_frames: 0, or in the soft-limit case the oracle's count of frames over the limit; a decoder error raises.

Each case is fed three ways.  Which kernel selects depends on the feed: a multi-frame advance call of a two-launch decoder closes its
inner frames in the insert launch (frame_boundary_fused -> kth_smallest_cold), the first frame of every call is prepared by the
closure launch (prep_frame).  "one call" selects on frames 1 and 2 inside the call; "two and one" stops behind frame 2, whose
frontier then shows what the selection at n = N admitted; "frame by frame" shows every frontier and selects in prep_frame."""
import numpy as np
import pytest

import geometry_util as U
import selection_util as S
from golden_util import bits

pytestmark = pytest.mark.gpu

CASES = S.cases()
FEEDS = (("one call", (S.T_FRAMES,)), ("two and one", (2, S.T_FRAMES)), ("frame by frame", tuple(range(1, S.T_FRAMES + 1))))


@pytest.fixture(scope="module")
def gpu(synth, oracle, tmp_path_factory):
    g = U.Gpu(S.World(synth, oracle, str(tmp_path_factory.mktemp("selection"))))
    yield g
    g.free()


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_selection(gpu, case):
    G, W, world = gpu.G, gpu.W, gpu.world
    leg = S.LEGS[case.leg]
    biglm, lattice = bool(leg.get("biglm")), bool(leg.get("lattice"))
    flags = dict(leg["flags"], soft_limit=1) if case.max_tok else dict(leg["flags"])
    key = world.key(S.oracle_cfg(case))
    graph = gpu.graph(case.graph, leg.get("gopt"))
    utts = world.mats(case.graph)
    dev = G.upload(utts)
    stride = int(utts[0].shape[1])
    kw = S.limits(case)
    if leg.get("opt"):
        kw["options"] = W.Options(**leg["opt"])
    if biglm:
        kw["old_lm"], kw["new_lm"] = gpu.lm_pair()
    B = len(utts)
    dec = W.BatchDecoder(graph, G.gpu_config(case.cfg), B, **kw)

    def check_flags(when):
        pf = dec.path_flags()
        assert {k: pf[k] for k in flags} == flags, "%s, %s: path flags %s" % (case.id, when, pf)

    def check_frontier(utt, r, when):
        for c, u in enumerate(utt):
            what = "%s, %s: channel %d utt %d frame %d" % (case.id, when, c, u, r)
            st, co = dec.frontier(c)
            if biglm:
                # a biglm token is a (graph state, LM state) pair, several per state: the oracle's pairs and the device's, as multisets
                # of (graph state, cost bits)
                ost, oco, on = world.oracle_biglm_dump(case.graph, key, u, r)
                assert on == len(ost) and len(st) == on, what + ": %d tokens, the oracle %d" % (len(st), on)
                assert S.pair_multiset(st, co) == S.pair_multiset(ost, oco), what + ": (state, cost) pairs"
                assert bits([co.min()]) == bits([oco.min()]), what + " best cost"
                continue
            ost, oco, on = world.oracle_dump(case.graph, key, u, r)
            assert on == len(ost) and len(set(st.tolist())) == len(st), what + ": states repeat"
            assert len(st) == on, what + ": %d tokens, the oracle %d" % (len(st), on)
            ref = dict(zip(ost.tolist(), bits(oco).tolist()))
            bad = [a for a, b in zip(st.tolist(), bits(co).tolist()) if ref.get(a) != b]
            assert not bad, what + ": %d states off, the first %d" % (len(bad), bad[0])
            assert bits([co.min()]) == bits([oco.min()]), what + " best cost"

    def check_end(utt, when):
        for c, (u, d) in enumerate(zip(utt, dec.best_paths())):
            what = "%s, %s: channel %d utt %d" % (case.id, when, c, u)
            if case.kind == "ladder":
                # a rung's coarse costs tie (two arcs into one state at the same rounded cost): which of the equally cheap paths is
                # reported is the decoders' tie rule's, so the reference is the order-free oracle under that rule -- hop for hop
                want = world.tie_rule_decode(case.graph, S.oracle_cfg(case), u)
            else:
                want = (world.oracle_biglm if biglm else world.oracle_decode)(case.graph, key, u)
                assert want.extra["ties"] == 0, what
            assert want.ok, what
            G.assert_same_as_oracle(G.GpuResult(d), want, what)
            if lattice:
                U.same_lattice(dec.raw_lattice(c), world.oracle_lattice(case.graph, key, u), what)
            over = 0
            if case.max_tok:
                tr = world.oracle_trace(case.graph, key, u)
                over = sum(int(tr.frame_ntoks[f] > case.max_tok) for f in range(S.T_FRAMES))
                assert over >= 1
            assert dec.degraded_frames(c) == over, what + ": %d degraded frames, the oracle counts %d over the limit" % (dec.degraded_frames(c), over)

    def decode(utt, steps, when):
        ptrs = [dev[u].data_ptr() for u in utt]
        dec.init()
        check_flags(when + ", before")
        if len(steps) == S.T_FRAMES:
            check_frontier(utt, 0, when)
        for r in steps:
            dec.advance(ptrs, [r] * B, stride)
            check_frontier(utt, r, when)
        dec.finalize()
        check_flags(when + ", after")
        check_end(utt, when)

    try:
        for when, steps in FEEDS:
            decode(list(range(B)), steps, when)
        if case.kind == "frame0":
            # the same channels, initialised again, on each other's utterances
            for when, steps in FEEDS[:1] + FEEDS[2:]:
                decode(list(range(B))[::-1], steps, when + ", channels swapped")
    finally:
        dec.free()
