"""CPU: the constructed lattices of tests/det_edge_util.py (one per branch of asr-decoder_amd/csrc/wfst_determinize_wave.h) are what
they claim to be -- closure sizes by breadth-first search, arc counts per state, the searched collisions against the restated hashes
-- the restated constants are the sources', and on every one of them the host build of the shared algorithm (wfst_determinize.h
through tests/det_host.cc, with the closure's fast buffers absent, at the device's size and at 5 elements) gives the lattice of the
reference's own DeterminizeLatticeWrapper (oracle/_ref): same counts, same arc multiset bit for bit.  That makes the host build a
legitimate reference for tests/test_gpu_detwave_edges.py on these shapes, not on random lattices alone."""
import importlib
import os
import re

import numpy as np
import pytest

import det_edge_util as E
import pyoracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "asr-decoder_amd", "csrc")
NAMES = [c.name for c in E.cases()]
BY_NAME = {c.name: c for c in E.cases()}


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_restated_constants_are_the_sources():
    w, d, k = _src("wfst_determinize_wave.h"), _src("wfst_determinize.h"), _src("wfst_determinize.hip")
    num = lambda pat, text: int(re.search(pat, text).group(1))
    assert num(r"#define DETW_CUR (\d+)", w) == E.K_CUR and re.search(r"kDwCur = DETW_CUR;", w) and re.search(r"kDwQueue = DETW_CUR;", w)
    assert E.K_QUEUE == E.K_CUR
    assert num(r"#define DETW_ARCS (\d+)", w) == E.K_ARCS and re.search(r"kDwArcs = DETW_ARCS;", w)
    assert num(r"#define DETW_LABS (\d+)", w) == E.K_LABS and re.search(r"kDwLabs = DETW_LABS;", w)
    assert num(r"kDwMap = (\d+);", w) == E.K_MAP == 1 << E.MAP_SHIFT
    assert re.search(r"kDwWin = 64 / kDwArcs;", w) and E.K_WIN == 64 // E.K_ARCS
    # the state index's word and the sort key, every place they are made or taken apart
    assert len(re.findall(r"state << 11\) \| \(uint32_t\)\(\w+ \+ 1\)", w)) == 3 and "(v >> 11) == state" in w and "(v & 2047u) - 1" in w
    assert "state << 10) | (uint32_t)i" in w and "S.sortk[i] & 1023u" in w
    assert E.K_CUR <= 1 << E.SORT_SHIFT and E.K_CUR + 1 <= (1 << E.MAP_SHIFT)
    assert "W.n_states >= (1 << 21)" in w and E.MAX_STATES == 1 << 21
    assert "* 2654435761u) >> (32 - 11)" in w
    assert "claim[s & 255u]" in w and "uint16_t claim[256]" in w and E.CLAIM == 256
    # the first table of the trie: the harness's copy and the product's
    assert "h = 4096; while (h < 16 * n_states && h < hcap_full) h <<= 1;" in w
    assert re.search(r"h = 4096;\s+while \(h < 16 \* nt && h < hcap_full\) h <<= 1;", k)
    assert (E.TRIE_FIRST, E.TRIE_PER_STATE) == (4096, 16)
    for text in ("uint32_t h = (uint32_t)a * 2654435761u;", "h ^= ((uint32_t)b + 0x9E3779B9u) * 0x85EBCA6Bu;", "h ^= h >> 15;", "return h * 0x2C1B3C6Du;",
                 "return (uint64_t)(uint32_t)parent | ((uint64_t)(uint32_t)label << 32);"):
        assert text in d, text
    assert "W.delta = 1.0f / 1024" in w and E.DELTA == 1.0 / 1024
    # the restated hashes on a few values worked out by hand from the C expressions
    assert E.mapslot(1) == 2654435761 >> 21 and E.mapslot(0) == 0
    assert E.hash2(0, 0) == ((((0x9E3779B9 * 0x85EBCA6B) & 0xFFFFFFFF) ^ (((0x9E3779B9 * 0x85EBCA6B) & 0xFFFFFFFF) >> 15)) * 0x2C1B3C6D) & 0xFFFFFFFF
    assert E.first_table(256) == 4096 and E.first_table(257) == 8192 and E.first_table(1 << 21) == 1 << 20


def test_every_branch_of_the_issue_has_a_case():
    assert len(NAMES) == len(set(NAMES)) == 53
    counters = set(re.search(r"#define DETW_COUNTERS\(X\) \\\n((?:.*\\\n)*.*)\n", _src("wfst_determinize_wave.h")).group(1).replace("\\", " ").replace("X(", " ").replace(")", " ").split())
    moved = set()
    for c in E.cases():
        assert c.refuse is not None or any(op == ">=" or v > 0 for op, v in c.want.values()), c.name + ": no counter it must move"
        assert set(c.want) <= counters, (c.name, set(c.want) - counters)
        moved |= {k for k, (op, v) in c.want.items() if op == ">=" or v > 0}
    # counters no case is built for: totals (closure, window), fb_inorder (the in-order commit outgrowing LDS: it needs a window of
    # the kind "two_new_states_after_one_slot" at 1024 elements), init_found / init_new / pairs_wave / run_sub / norm_wave (the rule)
    assert counters - moved <= {"closure", "window", "fb_inorder", "init_found", "init_new", "run_sub", "norm_wave"}, counters - moved


@pytest.mark.parametrize("name", NAMES)
def test_the_construction_is_what_it_claims(name):
    c = BY_NAME[name]
    L = c.lat
    assert E.well_formed(L), "a state without arcs that is not final, or a final state with arcs"
    assert L.st_final[0] == 0 and L.a_src.min() >= 0 and L.a_dst.min() >= 0
    fin = np.isfinite(L.a_graph)
    assert np.all(L.a_graph[fin] * 2048 == np.round(L.a_graph[fin] * 2048)) and np.all(L.a_graph[fin] >= 0) and np.all(L.a_graph[fin] < 4)
    if "apart" not in name:
        assert np.all(L.a_graph[fin] * 16 == np.round(L.a_graph[fin] * 16))
    for what, got, claimed in c.facts:
        assert got == claimed, (what, got, claimed)


@pytest.fixture(scope="module")
def det_host():
    return pyoracle.build_det_host()


@pytest.mark.parametrize("name", NAMES)
def test_host_build_equals_the_reference(name, refdec, det_host, tmp_path):
    c = BY_NAME[name]
    shard = importlib.import_module("asr-decoder_amd.shard")
    p = str(tmp_path / "case.lat")
    with open(p, "wb") as f:
        f.write(shard.lattice_to_bytes(E.as_dict(c.lat)))
    big = c.lat.n_states > 1 << 20
    cap = dict(max_states=max(1 << 12, c.lat.n_states + 8) if big else 1 << 20, max_arcs=1 << 14 if big else 1 << 21)
    R = pyoracle.ref_determinize_lattice_file(refdec, p, 0, **cap)
    assert R is not None, "the reference refuses the lattice"
    want = [R.n_states, int(R.st_final.sum()), len(R.a_src)]
    for low in (0, 1024, 5):   # (the closure's fast buffers: none / the device's size / so small that closures outgrow them)
        rc, D = pyoracle.det_host_run(det_host, c.lat, cap_scale=0 if big else 32, low_tmp=low, max_states=1 << 14, max_arcs=1 << 16)
        assert rc == 0, (name, low)
        assert [D.n_states, int(D.st_final.sum()), len(D.a_src)] == want, (name, low, "counts")
        assert np.array_equal(D.arc_multiset(), R.arc_multiset()), (name, low, "arcs")
        assert np.all(D.a_il == 0) and not np.isin(D.a_src, np.nonzero(D.st_final)[0]).any()


@pytest.mark.parametrize("shape", E.DECODER_SHAPES)
def test_decoder_graphs_give_lattices_of_the_intended_shape(shape, synth, oracle, det_host, tmp_path):
    """the three graphs tests/test_gpu_detwave_edges.py decodes for the product kernel's own CSR build and retry loop: from the
    oracle's raw lattice (order-free mode: what the device's decoder leaves) the lattice has the shape the case is about, the host
    build determinizes it, and the chain's trie outgrows half of the first table"""
    g, ll, facts = E.decoder_shape(synth, shape)
    gp = str(tmp_path / "g.bin")
    g.write(gp)
    oracle.set_order_free(True)
    try:
        h = oracle.load_graph(gp)
        O = pyoracle.oracle_raw_lattice(oracle, h, pyoracle.Config(**E.DECODER_CFG), ll, None)
        oracle.free_graph(h)
    finally:
        oracle.set_order_free(False)
    assert O is not None and O.ok
    for what, got, claimed in facts(O):
        assert got == claimed, (what, got, claimed)
    rc, D = pyoracle.det_host_run(det_host, O, cap_scale=32)
    assert rc == 0 and D.n_states > 0
    if shape == "chain_of_parallel_arcs":
        assert det_host.det_host_last_trie() > E.TRIE_FIRST // 2
