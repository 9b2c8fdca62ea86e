"""The cases of tests/selection_util.py do what they claim, under the order-free oracle (no GPU): the constants they are sized by are
the ones in the sources; the frontier of frame 1 holds exactly the count a case names; the limit binds where it is meant to; moving
the limit by one changes the frame that follows (so a selection that is one rank off, or miscounts one token, cannot pass
tests/test_gpu_cutoff_selection.py unseen); the pass-count ladder covers one to four passes with a narrow last pass in each class; and
outside the ladder every case is `ok` and free of exact ties on the best path.  A condition of the GPU comparison, not a measurement:
a case that misses one gets another seed in selection_util.SEEDS; nothing is skipped or capped."""
import numpy as np
import pytest

import selection_util as S
from golden_util import bits

CASES = S.cases()
IDS = [c.id for c in CASES]


@pytest.fixture(scope="module")
def world(synth, oracle, tmp_path_factory):
    return S.World(synth, oracle, str(tmp_path_factory.mktemp("selection")))


def test_restated_constants_are_the_sources():
    """512 x 4, 1024 x 8, batches of 4 and 8, 3 * lds_slots, 2^12 slots: retune one and this fails before a case loses its aim"""
    assert S.source_constants() == S.RESTATED
    assert (S.COLD_REGS, S.WARM_REGS, S.cold_cache(8), S.cold_cache()) == (2048, 8192, 768, 12288)
    sizes = dict(S.SIZE_EDGES)
    assert sizes["cold"] == (2047, 2048, 2049, 14335, 14336, 14337)
    assert sizes["cold_lds8"] == (2815, 2816, 2817, 2048 + 768 + 4 * 512 + 1)
    assert sizes["three_launch"] == sizes["lattice"] == (8191, 8192, 8193, 16385)
    assert sizes["plain"] == sizes["biglm"] == (8191, 8193)
    assert S.RANK_N == 2049


def test_case_ids_are_unique_and_every_size_meets_three_limits():
    assert len(set(IDS)) == len(IDS)
    for leg, sizes in S.SIZE_EDGES:
        for n in sizes:
            got = sorted(c.cfg["max_active"] for c in CASES if c.kind == "size" and c.leg == leg and c.n == n)
            assert got == [S.MIN_MAX_ACTIVE, n // 2, n - 1], (leg, n, got)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_decoder_limits_name_the_launch_path(case):
    """(restated sizing, wfst_capi.cc) a cold case closes frames 1 and 2 of a three-frame call in the insert launch: a collection
    stride of 3 at least; a three-launch case leaves room for none; every arena holds the utterance"""
    leg, lim = S.LEGS[case.leg], S.limits(case)
    stride = S.gc_stride(lim["max_tokens_per_frame"], lim["arena_tokens"])
    if leg["flags"].get("two_launch") == 1:
        assert stride >= S.T_FRAMES, (case.id, stride)
    if leg.get("three"):
        assert stride < 1, (case.id, stride)
    if not leg.get("biglm"):
        assert 1 + S.T_FRAMES * S.frame_cap(case) <= lim["arena_tokens"]
    assert (lim["max_tokens_per_frame"] < case.n) == bool(case.max_tok)


def _frontier(world, case, cd, ui, frame):
    """What identifies a frame's frontier, and what tests/test_gpu_cutoff_selection.py compares: its states and cost bits (biglm:
    the multiset of (graph state, cost bits) over its (state, LM state) pairs)"""
    dump = world.oracle_biglm_dump if S.LEGS[case.leg].get("biglm") else world.oracle_dump
    st, co, n = dump(case.graph, world.key(cd), ui, frame)
    assert n == len(st)
    return S.pair_multiset(st, co)


def _run_ends(sorted_costs, k):
    """The first and the last rank of the run of bit-equal costs that rank k lies in"""
    b = bits(sorted_costs)
    lo = hi = k
    while lo > 0 and b[lo - 1] == b[k]:
        lo -= 1
    while hi + 1 < len(b) and b[hi + 1] == b[k]:
        hi += 1
    return lo, hi


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_does_what_it_claims(world, case):
    biglm = bool(S.LEGS[case.leg].get("biglm"))
    cd = S.oracle_cfg(case)
    key = world.key(cd)
    f_sel = 0 if case.kind == "frame0" else 1    # the frame whose frontier the case is about
    _, facts = world.graph(case.graph)
    if case.kind == "frame0":
        assert facts["root_paths"] == S.CLOSURE[0] > S.FRAME0_MAX_ACTIVE and facts["fusable"]
    for ui in range(len(world.mats(case.graph))):
        what = "%s utt %d" % (case.id, ui)
        t = (world.oracle_biglm_trace if biglm else world.oracle_trace)(case.graph, key, ui)
        o = (world.oracle_biglm if biglm else world.oracle_decode)(case.graph, key, ui)
        assert t.ok and o.ok, what
        if case.kind != "ladder":
            assert o.extra["ties"] == 0, what + ": an exact tie on the best path -- change the seed"
        else:
            # (coarse costs tie; the GPU test's reference there is the oracle under the decoders' tie rule: the same cost, to the bit)
            tied = world.tie_rule_decode(case.graph, cd, ui)
            assert tied.ok and bits(np.cumsum(tied.path_graph + tied.path_ac, dtype=np.float32)[-1:]) == bits(np.cumsum(o.path_graph + o.path_ac, dtype=np.float32)[-1:]), what
        if biglm:
            assert o.extra["lm_oob"] == 0 and t.frame_ntoks.max() < S.BIGLM_MAX_TOK, what
        # the count the case names
        assert t.frame_ntoks[f_sel] == case.n, (what, t.frame_ntoks)
        # the limit binds on that frame
        beam_cutoff = np.float32(t.frame_best[f_sel]) + np.float32(cd["beam"])
        if case.limit == "max_active":
            assert t.frame_cutoff[f_sel] < beam_cutoff, what
            assert bits([t.frame_adaptive_beam[f_sel]]) == bits([np.float32(t.frame_cutoff[f_sel]) - np.float32(t.frame_best[f_sel]) + np.float32(0.5)])
        else:
            assert t.frame_cutoff[f_sel] > beam_cutoff, what
            assert np.isinf(t.frame_cutoff[f_sel]) == (cd["min_active"] >= case.n), what
        if case.kind == "rank_min":
            assert np.isinf(t.frame_adaptive_beam[0])   # (not the plain beam: the boundary that closes frame 1 takes the need_min path)
        if case.kind == "soft":
            assert sum(int(t.frame_ntoks[f] > case.max_tok) for f in range(S.T_FRAMES)) >= 1
    # sensitivity: the limit moved by one, either way, gives another frontier behind the frame, in one of the case's channels at
    # least (the plateau's ranks are utterance 0's; inside the plateau a move changes nothing, in any channel of it).  A ladder rung's
    # coarse costs come in runs of bit-equal ones, each a plateau: there the limit is moved off the ends of the run its rank lies in
    # (one below the run's first rank, one above its last), per channel.
    utts = [0] if case.kind in ("rank_max", "rank_min") else list(range(len(world.mats(case.graph))))
    k = cd[case.limit]
    for by in (-1, 1):
        changed = []
        for ui in utts:
            move = by
            if case.kind == "ladder":
                lo, hi = _run_ends(np.sort(world.oracle_dump(case.graph, key, ui, f_sel)[1]), k)
                move = (lo - 1 if by < 0 else hi + 1) - k
                assert S.MIN_MAX_ACTIVE <= k + move < case.n, (case.id, ui, lo, hi)
            changed.append(_frontier(world, case, S.oracle_cfg(case, **{case.limit: move}), ui, f_sel + 1) != _frontier(world, case, cd, ui, f_sel + 1))
        assert any(changed) == (by in case.moves), "%s: limit %+d, the frame behind %s -- change the seed" % (case.id, by, "is the same" if by in case.moves else "changes")


def test_plateau_ranks(world):
    """frontier_of(2049, plateau=600): in frame 1 of utterance 0 the plateau's 600 bit-equal costs hold ranks PLATEAU_RANK0 .. + 599"""
    name = "p%d" % S.RANK_N
    _, f = world.graph(name)
    assert len(f["plateau"]) == S.PLATEAU
    st, co, n = world.oracle_dump(name, world.key(S._cfg("cold")), 0, 1)
    assert n == S.RANK_N == len(st)
    cost = dict(zip(st.tolist(), bits(co).tolist()))
    pc = {cost[int(s)] for s in f["plateau"]}
    assert len(pc) == 1
    flat = np.sort(co)[S.PLATEAU_RANK0:S.PLATEAU_RANK0 + S.PLATEAU]
    assert set(bits(flat).tolist()) == pc
    assert int((bits(co) == pc.pop()).sum()) == S.PLATEAU                      # nothing else costs the same
    assert S.PLATEAU_RANK0 > 0 and S.PLATEAU_RANK0 + S.PLATEAU < S.RANK_N - 1   # distinct costs on both sides of it


def test_ladder_covers_every_pass_count(world):
    """Over the ladder's rungs, on the frames a bounded decoder selects on (more tokens than max_active), R = the bits in which the
    frame's best cost and the next_cutoff it was built under differ: one to four passes of 8 bits, and in each of the one-, two-
    and three-pass classes a last pass narrower than 8 bits."""
    seen = {}
    for case in CASES:
        if case.kind != "ladder" or case.leg != S.LADDER_LEGS[0]:
            continue
        for ui in range(len(world.mats(case.graph))):
            t = world.oracle_trace(case.graph, world.key(case.cfg), ui)
            for f, r in S.frame_ranges(t, case.cfg).items():
                seen.setdefault((r + 7) // 8, set()).add(r)
    assert set(seen) == {1, 2, 3, 4}, seen
    for passes in (1, 2, 3):
        assert any(r % 8 for r in seen[passes]), (passes, seen)
    assert {c.leg for c in CASES if c.kind == "ladder"} == {leg for leg in S.LADDER_LEGS if S.LEGS[leg]["bounded"]}
