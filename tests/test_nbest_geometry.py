"""The graphs of tests/nbest_geometry_util.py do what they are named for: the order-free oracle's raw lattice of every case (and, for
the n-best-paths cases, the host build of the determinizer on it) has the candidate counts, in-degrees, frame widths, final states and
exact ties the case claims -- recomputed from the lattice, so that a case cannot silently lose its aim.  No GPU."""
import numpy as np
import pytest

import nbest_geometry_util as U
import pyoracle


def oracle_lattices(synth, oracle, tmp_path, build, quantised):
    g, mats = build(synth, quantised)
    path = str(tmp_path / "g.bin")
    g.write(path)
    h = oracle.load_graph(path)
    try:
        oracle.set_order_free(True)
        out = [pyoracle.oracle_raw_lattice(oracle, h, pyoracle.Config(**U.CFG), x, None) for x in mats]
    finally:
        oracle.set_order_free(False)
        oracle.free_graph(h)
    return g, mats, out


@pytest.mark.parametrize("name,quantised", U.nbest_case_ids(), ids=lambda v: str(v))
def test_nbest_case_has_its_shape(name, quantised, synth, oracle, tmp_path):
    build, check, _ = U.NBEST_CASES[name]
    g, mats, lats = oracle_lattices(synth, oracle, tmp_path, build, quantised)
    for x, L in zip(mats, lats):
        assert L.ok and np.all(L.a_dst > L.a_src)
        # the lattice is the graph unrolled: a state per graph state (and the super-final state where one is reachable), every arc once
        n_final_arcs = int((g.arcs["to"] == g.final_state).sum())
        assert L.n_states == g.n_states - (0 if n_final_arcs else 1) and len(L.a_src) == g.n_arcs, (L.n_states, g.n_states, len(L.a_src), g.n_arcs)
        assert int(L.st_frame.max()) == x.shape[0]
        check(U.facts(L), quantised)


@pytest.mark.parametrize("name,quantised", U.paths_case_ids(), ids=lambda v: str(v))
def test_paths_case_has_its_shape(name, quantised, synth, oracle, tmp_path):
    build, check, _ = U.PATHS_CASES[name]
    g, mats, lats = oracle_lattices(synth, oracle, tmp_path, build, quantised)
    lib = pyoracle.build_det_host()
    rc, D = pyoracle.det_host_run(lib, lats[0], cap_scale=32)
    assert rc == 0
    f = U.paths_facts(D)
    r = check(f, quantised)
    assert r is None or r, (name, sorted(set(f["cands"].tolist())))
    # a final weight shared by all paths: one arc into the one final state
    assert int(D.st_final.sum()) == 1 and int(D.st_final[D.a_dst].sum()) == 1
