"""CPU: the numpy restatement of the snapshot lattice (tests/live_prune_util.py restate: FinalizeDecoding's pruning in float32 over a
live, unpruned raw lattice) proved with the oracle alone.  For prefixes of an utterance, in the oracle's order-free mode:
restate(raw lattice of the prefix WITHOUT FinalizeDecoding, use_final_probs) == raw lattice of the prefix after FinalizeDecoding,
states (frame, graph state, final flag, forward cost bits) and labelled arcs (labels, both costs bit for bit).  That makes the
restatement the yardstick of tests/test_gpu_live_prune.py where no finalized twin exists (use_final_probs = 0: every token of the
newest frame final at cost 0).  It needs nothing of the feature and passes without it: that is its purpose."""
import numpy as np
import pytest

import pyoracle
from live_prune_util import PREFIXES, config, frame_counts, restate, same_lattice, small_graph, utterances


@pytest.fixture(scope="module")
def case(synth, oracle, tmp_path_factory):
    g, m, path = small_graph(synth, tmp_path_factory.mktemp("lpr"))
    (ll,) = utterances(synth, g, m, lengths=(60,))
    h = oracle.load_graph(path)
    yield m, ll, h
    oracle.free_graph(h)


@pytest.mark.parametrize("lattice_beam", [0.5, 7.0])
@pytest.mark.parametrize("prefix", PREFIXES)
def test_restatement_of_the_live_lattice_is_the_finalized_lattice(prefix, lattice_beam, case, oracle):
    m, ll, h = case
    cfg = pyoracle.Config(**config(lattice_beam))
    try:
        oracle.set_order_free(True)
        live = pyoracle.oracle_raw_lattice(oracle, h, cfg, ll[:prefix], m, finalize=False, use_final_probs=True)
        want = pyoracle.oracle_raw_lattice(oracle, h, cfg, ll[:prefix], m, finalize=True)
    finally:
        oracle.set_order_free(False)
    assert live.ok and want.ok
    got = restate(live, lattice_beam)
    what = "prefix %d lattice_beam %g" % (prefix, lattice_beam)
    same_lattice(got, want, what)
    assert np.all(got.a_dst > got.a_src), what
    # the case is not empty: the live lattice holds raw frames the pruning thins out (except where a pass has just run)
    print(what, "live", live.n_states, len(live.a_src), "finalized", want.n_states, len(want.a_src))
    if prefix % 25 and prefix > 1:
        assert live.n_states > want.n_states, (what, live.n_states, want.n_states)
    assert frame_counts(got)[0] >= 1 and int(got.st_frame.max()) == prefix


def test_all_final_seed_equals_the_final_probs_seed_where_no_token_is_final(case, oracle):
    """ComputeFinalCosts with no final token on the frontier: every token is final at cost 0 -- the restatement's two seeds agree there"""
    m, ll, h = case
    cfg = pyoracle.Config(**config(7.0))
    n = 0
    try:
        oracle.set_order_free(True)
        for prefix in PREFIXES:
            live = pyoracle.oracle_raw_lattice(oracle, h, cfg, ll[:prefix], m, finalize=False, use_final_probs=True)
            newest = live.st_frame == prefix
            if not np.all(live.st_final[newest] != 0):
                continue   # some token of the frontier is final in the graph
            same_lattice(restate(live, 7.0, all_final=True), restate(live, 7.0), "prefix %d" % prefix)
            n += 1
    finally:
        oracle.set_order_free(False)
    assert n >= 1
