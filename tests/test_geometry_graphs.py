"""The graphs of tests/geometry_util.py do what they claim (shape facts recomputed from the arrays), and every (graph,
configuration, utterance) triple that tests/test_gpu_tile_geometry.py decodes is `ok` and free of exact ties on the best path
under the order-free oracle: a condition of that comparison, not a measurement (a draw with a tie gets another seed HERE; the GPU
test skips nothing).  Where the reference is built, its own decode of the beam-only triples equals the order-free oracle's."""
import numpy as np
import pytest

import geometry_util as U
import pyoracle


@pytest.fixture(scope="module")
def world(synth, oracle, tmp_path_factory):
    return U.World(synth, oracle, str(tmp_path_factory.mktemp("geometry")))


# ---- shape facts ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,P", [(16, 4), (257, 8), (1400, 70), (1401, 70), (3000, 40)])
def test_hub_is_a_one_token_tile_of_the_size_asked_for(synth, E, P):
    g, f = U.hub(synth, E, P, paths=2, depth=2)
    assert g.start == 0 and f["E"] == E and f["hub_eps"] == 0 and f["hub_targets_distinct"]
    assert f["hub_pseudo"] == 2 * P and f["hub_slots"] == E + 4 * P
    assert f["fusable"]
    # every leaf has a self-loop and arcs back into the graph; some state is final
    assert (f["n_emit"][1:-1] >= 3).all() and g.state_info["num_arcs"][g.final_state] == 0
    assert int((g.arcs["to"] == g.final_state).sum()) == 3
    if E == 3000:
        assert f["n_states"] <= 3500 and f["row_slots"] <= 20000


def test_cut_pair_slot_arithmetic(synth):
    _, odd = U.GRAPHS["cut1401"](synth)
    _, even = U.GRAPHS["cut1400"](synth)
    assert odd["E"] == 1401 and odd["hub_pseudo"] == 140 and even["E"] == 1400 and even["hub_pseudo"] == 140
    # pair i occupies slots E + 2 i and E + 2 i + 1 of the one-token tile; a pass ends behind slot S - 1
    i, j = odd["cut_row"], odd["cut_gather"]
    assert (i, j) == (3, 67)
    assert odd["E"] + 2 * i == U.SLOTS_ROW - 1 and odd["E"] + 2 * j == U.SLOTS_GATHER - 1
    assert 0 <= i < odd["hub_pseudo"] and 0 <= j < odd["hub_pseudo"]
    assert odd["hub_slots"] > U.SLOTS_GATHER   # both forms run a second pass
    assert even["cut_row"] is None and even["cut_gather"] is None
    for S in (U.SLOTS_ROW, U.SLOTS_GATHER):
        assert (S - 1 - even["E"]) % 2 == 1 and S - even["E"] >= 0   # the even twin: the pass ends between two pairs


def test_code_edges_stand_on_both_sides_of_every_field(synth):
    g, f = U.code_edges(synth)
    sp = f["special"]
    shape = lambda name: (int(f["n_eps"][sp[name]]), int(f["n_emit"][sp[name]]), int(f["n_pseudo"][sp[name]]))
    assert shape("eps3") == (3, 4, 0) and shape("eps4") == (4, 4, 0)
    assert shape("emit15") == (0, 15, 0) and shape("emit16") == (0, 16, 0)
    assert shape("pseudo31") == (0, 3, 31) and shape("pseudo32") == (0, 3, 32)
    assert shape("all_max") == (3, 15, 31) and shape("below_max") == (3, 15, 30)
    assert shape("eps7") == (7, 2, 0) and shape("emit40") == (0, 40, 0) and shape("pseudo41") == (0, 2, 41)
    assert shape("no_arcs") == (0, 0, 0) and shape("eps_only") == (2, 0, 0)
    known = {k: U.code_known(f, s) for k, s in sp.items()}
    assert known == dict(eps3=True, eps4=False, emit15=True, emit16=False, pseudo31=True, pseudo32=False, all_max=False, below_max=True,
                         eps7=False, emit40=False, pseudo41=False, no_arcs=True, eps_only=True)
    # all of them one emitting arc away from the fan state: one frame, one tile
    off = g.row_offsets()
    assert set(sp.values()) <= set(g.arcs["to"][off[0]:off[1]].tolist()) and f["E"] < 256
    assert f["fusable"]


@pytest.mark.parametrize("paths,depth,fusable", [(48, 8, True), (49, 8, False), (20, 9, False), (2, 2, True)])
def test_closure_limits(synth, paths, depth, fusable):
    g, f = U.closure_limits(synth, paths, depth)
    assert f["root_paths"] == paths and f["root_depth"] == depth
    assert f["fusable"] == fusable
    if fusable:
        assert f["paths"].max() == paths and f["depth"].max() == depth   # nothing else in the graph is nearer the caps
    else:
        # the root alone crosses the line, and one cap alone
        others = np.arange(f["n_states"]) != f["root"]
        assert f["paths"][others].max() <= U.PATH_CAP and f["depth"][others].max() <= U.DEPTH_CAP
        assert (paths > U.PATH_CAP) != (depth > U.DEPTH_CAP)
    if depth >= 8:
        assert {1, 2, 3, 8} <= set(f["root_hops"])
    # the hub's arc into the root carries one pseudo arc per path
    assert f["hub_pseudo"] == paths


@pytest.mark.parametrize("n_cols", [4, 3072, 3076])
def test_wide_columns_read_the_lowest_and_the_highest_column(synth, n_cols):
    g, f = U.wide_columns(synth, n_cols)
    assert f["min_label"] == 1 and f["max_label"] == n_cols - 1 and f["fusable"]
    off = g.row_offsets()
    hub_labels = g.arcs["ilabel"][off[0]:off[1]]
    assert hub_labels.min() == 1 and hub_labels.max() == n_cols - 1
    assert f["hub_pseudo"] == 12


@pytest.mark.parametrize("N", [127, 128, 129, 255, 256, 257, 1024, 1025, 1280, 1281])
def test_frontier_of_holds_exactly_n_tokens(world, N):
    name = "frontier%d" % N
    g, f = world.graph(name)
    assert f["E"] == N - 1 and f["hub_targets_distinct"] and f["fusable"]
    for ui, x in enumerate(world.mats(name)):
        t = world.oracle_trace(name, "wide", ui)
        assert t.ok and t.frame_ntoks[0] == 1 and (t.frame_ntoks[1:] == N).all(), (name, ui, t.frame_ntoks)


def test_plateau_holds_more_live_tokens_than_max_active(world):
    """frontier_of(1025, plateau=860) under max_active 600: the 600-th cheapest token of every frame >= 1 lies on the plateau, so all
    of its 860 tokens (and whatever is cheaper) stay live: at least 860 / 1025 = 84 % of the tokens of tiles cut for 600 live ones
    in 1025 (320 tokens: 268 live expected, more than a round's 256)."""
    g, f = world.graph("plateau1025")
    flat = np.asarray(f["plateau"])
    assert len(flat) == 860 and f["E"] == 1024
    cfg = pyoracle.Config(**U.MAX600)
    held = 0   # frontiers that are expanded (another frame follows) with the max_active-th cheapest token on the plateau
    for ui, x in enumerate(world.mats("plateau1025")):
        for fr in range(1, x.shape[0]):
            st, co, n = world.oracle_dump("plateau1025", "max600", ui, fr)
            assert n == len(st)
            cost = dict(zip(st.tolist(), co.view(np.int32).tolist()))
            pc = {cost.get(int(s)) for s in flat}
            if n <= cfg.max_active or None in pc:
                continue    # (the adaptive beam has dropped the plateau: it lasts a frame or two)
            assert len(pc) == 1, "utterance %d frame %d: the plateau is not flat" % (ui, fr)
            kth = np.sort(co)[cfg.max_active - 1]
            if int(kth.view(np.int32)) == pc.pop():
                assert int((co <= kth).sum()) >= 860
                held += 1
    assert held >= 3, held


# ---- every triple of the GPU test ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cfg", U.all_triples(), ids=lambda v: str(v))
def test_every_gpu_case_is_ok_and_tie_free(world, name, cfg):
    _, f = world.graph(name)
    assert f["max_label"] < U.n_cols_of(name)
    for ui, x in enumerate(world.mats(name)):
        o = world.oracle_decode(name, cfg, ui)
        assert o.ok, (name, cfg, ui)
        assert o.extra["ties"] == 0, "%s %s utt %d: an exact tie on the best path -- change the seed" % (name, cfg, ui)
        # the partial results the GPU test compares after frames 1 and 2
        for k in (1, 2):
            if k <= x.shape[0]:
                p = world.oracle_decode(name, cfg, ui, frames=k, partial=True)
                assert p.ok and p.extra["ties"] == 0, (name, cfg, ui, k)
    if (name, cfg) in U.leg_cases()["compacting"] and cfg not in ("min_active", "min_binds"):   # the limit binds on some frame
        t = world.oracle_trace(name, cfg, 0)
        assert t.frame_ntoks.max() > U.CFGS[cfg]["max_active"], (name, cfg, t.frame_ntoks)
    if cfg == "min_binds":
        # min_active binds: on some frame more than 600 tokens, fewer than 600 of them within the beam of the best one
        cd = U.CFGS[cfg]
        binds = []
        for fr in range(1, world.mats(name)[0].shape[0]):
            st, co, n = world.oracle_dump(name, cfg, 0, fr)
            binds.append(n > cd["min_active"] and int((co <= co.min() + np.float32(cd["beam"])).sum()) < cd["min_active"])
        assert sum(binds) >= 2, (name, cfg, binds)


def test_biglm_cases_are_ok_and_tie_free(world):
    for name, cfg in U.leg_cases()["biglm"]:
        for ui in range(len(world.mats(name))):
            o = world.oracle_biglm(name, cfg, ui)
            assert o.ok and o.extra["ties"] == 0 and o.extra["lm_oob"] == 0, (name, cfg, ui)


def test_reference_agrees_on_the_beam_only_cases(world, refdec):
    """The reference's own (visiting-order dependent) decode equals the order-free oracle's words and transition-ids; it may differ
    only on a hop with parallel arcs, where GetBestPath reports the first surviving forward link (either side then reports quirk_hops)."""
    n = n_same = 0
    for name, cfg in U.all_triples():
        cd = U.CFGS[cfg]
        if cd["max_active"] < 1000000 or cd["min_active"] > 0:
            continue
        path = world.path(name)
        h = refdec.load_graph(path)
        try:
            for ui, x in enumerate(world.mats(name)):
                o = world.oracle_decode(name, cfg, ui)
                r = refdec.decode(h, pyoracle.Config(**cd), x, None)
                ref_mode = world.oracle_decode(name, cfg, ui, order_free=False)
                what = "%s %s utt %d" % (name, cfg, ui)
                assert bool(r.ok) == bool(o.ok), what
                assert np.array_equal(r.tids, ref_mode.tids) and np.array_equal(r.words, ref_mode.words), what + ": oracle (reference mode) vs reference"
                same_as_ref = np.array_equal(o.tids, r.tids) and np.array_equal(o.words, r.words)
                n += 1
                n_same += int(same_as_ref)
                if not same_as_ref:  # only where parallel arcs are in play, and never in length
                    assert ref_mode.extra["quirk_hops"] + o.extra["quirk_hops"] > 0 and len(o.tids) == len(r.tids), what
        finally:
            refdec.free_graph(h)
    assert n >= 30 and n_same >= n - 2, (n, n_same)
