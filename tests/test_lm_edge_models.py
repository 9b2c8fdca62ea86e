"""CPU: the edge LMs of tests/lm_edge_util.py are what they claim to be, and the checkers agree on them.

1. lmsynth.NgramLm.to_fsa() == the reference converter's file, byte for byte, for every edge LM: orders 4 and 5, the "no A B, but have
   A B C" line the converter drops, the <unk> line it refuses, the on-demand start arc of a word without a unigram.
2. The oracle's LM walk == the compiled reference's ComposeArpaLm, bit for bit on next state and cost, at scale -1 and 1: on every
   (state, word) the scripts ask for, on the full grid state x word id below the empty history's arc count, Start and every Final --
   and the plain restatement that counts probes (lm_edge_util.get_arc) == both on the scripts' look-ups.
3. Conditions on the INPUTS of tests/test_gpu_lm_edges.py: the mirror table of each cluster LM holds the runs and displacements it
   was built for, and the scripts' look-ups cover the probe rounds {1, 2, 3, >= 4} at depth 0, back-off depths 1 .. 4, misses that
   cross a run of 8 slots or more, and every case the deep LM was built for."""
import numpy as np
import pytest

import lm_edge_util as U
import pyoracle
from golden_util import bits

NAMES = ["clusterA", "clusterB", "deep", "unigram"]


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    m = U.write_models(tmp_path_factory.mktemp("lm_edges"))
    m["tab"] = {k: U.MirrorTable(m["fsa"][k]) for k in NAMES}
    m["rec"] = {k: U.walk_records(m["fsa"][k], m["scripts"], m["tab"][k]) for k in NAMES}
    return m


@pytest.mark.parametrize("name", NAMES)
def test_edge_lm_fsa_is_byte_identical_to_the_reference_converter(name, models, refdec, tmp_path):
    lm = models["lms"][name]
    (tmp_path / "a.arpa").write_text(lm.arpa_text())
    (tmp_path / "w.txt").write_text(lm.wordlist_text())
    pyoracle.ref_arpa2fsa(refdec, str(tmp_path / "a.arpa"), str(tmp_path / "w.txt"), str(tmp_path / "ref.bin"))
    f = models["fsa"][name]
    assert f.to_bytes() == (tmp_path / "ref.bin").read_bytes()
    lines = sum(len(g) for g in lm.grams[1:])
    if name == "deep":
        assert len(lm.grams) == 5 and min(len(g) for g in lm.grams[1:]) >= 24
        assert f.states["arc_num"][0] == U.EOS + 1                       # the <unk> line gave the empty history no arc
        assert f.n_states == 1 + (U.EOS + 1) + lines - 1                 # ... and the trigram without its bigram no state
        a = f.arcs[U.NO_UNIGRAM]
        assert (a["wordid"], a["weight"], a["tostateid"]) == (U.NO_UNIGRAM, 0.0, U.NO_UNIGRAM + 1)   # the on-demand start arc
        assert f.states["backoff_prob"][U.NO_UNIGRAM + 1] == 0 and f.states["arc_num"][U.NO_UNIGRAM + 1] == 0
    else:
        assert f.n_states == 1 + (U.EOS + 1) + lines
    # no two weights equal: an arc or a back-off weight taken from the wrong place changes bits
    w = np.concatenate([f.arcs["weight"][f.arcs["weight"] != 0], f.states["backoff_prob"][f.states["backoff_prob"] != 0]])
    assert len(np.unique(bits(w))) == len(w)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_lm_walk_equals_the_compiled_reference(name, models, oracle, refdec):
    f, path = models["fsa"][name], models["paths"][name]
    n_words = int(f.states["arc_num"][0])
    asked = sorted({(r["state"], r["word"]) for r in models["rec"][name]})
    gs, gw = np.meshgrid(np.arange(f.n_states), np.arange(n_words), indexing="ij")
    for scale in (-1.0, 1.0):
        o, r = pyoracle.Lm(oracle, path, scale), pyoracle.Lm(refdec, path, scale)
        try:
            assert o.start() == r.start() == int(f.arcs["tostateid"][f.bos])
            for st, wd, what in ((np.array([a for a, _ in asked]), np.array([b for _, b in asked]), "scripts"), (gs.ravel(), gw.ravel(), "grid")):
                n1, c1 = o.getarc_many(st, wd)
                n2, c2 = r.getarc_many(st, wd)
                assert np.array_equal(n1, n2) and np.array_equal(bits(c1), bits(c2)), (name, scale, what)
            fo = np.array([o.final(s) for s in range(f.n_states)], np.float32)
            fr = np.array([r.final(s) for s in range(f.n_states)], np.float32)
            assert np.array_equal(bits(fo), bits(fr)), (name, scale, "final")
            # the counting restatement walks the same arcs to the same bits (so its probe lengths and depths are those of this walk)
            fs = f.rescaled(scale)
            nx, co = o.getarc_many([a for a, _ in asked], [b for _, b in asked])
            for k, (s, w) in enumerate(asked):
                to, cost, _, _ = U.get_arc(fs, models["tab"][name], s, w)
                assert to == nx[k] and np.float32(cost).tobytes() == np.float32(co[k]).tobytes(), (name, scale, s, w)
        finally:
            o.free()
            r.free()


@pytest.mark.parametrize("name", ["clusterA", "clusterB"])
def test_cluster_lm_tables_hold_the_runs_they_were_built_for(name, models):
    lm, tab, rec = models["lms"][name], models["tab"][name], models["rec"][name]
    assert len(lm.grams) == 2 and len(lm.grams[1]) <= 256 and tab.size == 1024
    runs = dict(tab.runs())
    for r in lm.edge["runs"]:
        first, L = r["first"], r["length"]
        assert runs.get(first) == L, (first, L)                                   # exactly L slots, an empty one before and behind
        slots = [(first + k) & tab.mask for k in range(L)]
        assert sorted((int(tab.state[s]) - 1, int(tab.word[s])) for s in slots) == r["keys"]
        assert sorted(tab.disp[(a + 1, b)] for a, b in r["keys"]) == list(range(L))
        a, b = r["absent"]
        assert (a + 1, b) not in tab.disp and int(U.lm_hash(a + 1, b)) & tab.mask == first
    assert sorted(r["length"] for r in lm.edge["runs"]) == sorted(U.RUN_LENGTHS + (U.WRAP_LENGTH,))
    wrap = lm.edge["runs"][-1]
    assert wrap["length"] >= 12 and wrap["first"] + wrap["length"] > 1024 and tab.stats()["wraps"]   # covers slot 1023 and slot 0
    required = {s for r in lm.edge["runs"] for s in range(r["first"] - 1, r["first"] + r["length"] + 1)}
    for first, L in runs.items():                                                 # the filler touches none of them
        assert first in [r["first"] for r in lm.edge["runs"]] or (L == 1 and first not in {s & tab.mask for s in required})
    d = set(tab.disp.values())
    assert {0, 3, 4, 7, 8} <= d and max(d) >= 9
    assert tab.stats() == dict(table_size=1024, used=len(lm.grams[1]), longest_run=U.WRAP_LENGTH, max_displacement=U.WRAP_LENGTH - 1, wraps=True)
    # every key of a required run is asked for -- from its own state, found without a back-off, after disp + 1 slots --
    hits = {(x["state"], x["word"]): x for x in rec if x["depth"] == 0 and x["state"] != 0}
    for r in lm.edge["runs"]:
        for a, b in r["keys"]:
            x = hits.get((a + 1, b))
            assert x is not None and x["probes"] == [(a + 1, tab.disp[(a + 1, b)] + 1, True)], (a, b)
        # ... and the absent bigram too: its look-up crosses the whole run, meets the empty slot behind it and backs off
        a, b = r["absent"]
        miss = [x for x in rec if x["state"] == a + 1 and x["word"] == b]
        assert miss and miss[0]["probes"][0] == (a + 1, r["length"] + 1, False) and miss[0]["depth"] == 1, (a, b)
    # a miss in a third round or later, then a back-off to a state whose key sits in ITS home slot: the probe offset starts over
    for r in lm.edge["resets"]:
        x, y, w = r["words"]
        hit = [z for z in rec if z["state"] == r["leaf"] and z["word"] == w]
        assert r["crossed"] >= 8 and hit and hit[0]["probes"] == [(r["leaf"], r["crossed"] + 1, False), (y + 1, 1, True)], r
    prof = U.walk_profile(models["fsa"][name], models["scripts"])
    assert {(1, 0), (2, 0), (3, 0)} <= prof and any(k >= 4 and dp == 0 for k, dp in prof)
    assert max(n - 1 for x in rec for _, n, found in x["probes"] if not found) >= 8   # a miss across a run of >= 8 slots
    # a wrapped probe sequence: a key at home near the end of the table, found in a slot near its start
    assert any(x["depth"] == 0 and x["state"] and (int(U.lm_hash(x["state"], x["word"])) & tab.mask) + x["probes"][0][1] > tab.size for x in rec)


def _script_with(models, words, at):
    for i, sc in enumerate(models["scripts"]):
        if list(sc["words"][at:at + len(words)]) == list(words):
            return i
    raise AssertionError("no script holds %s at %d" % (words, at))


def test_deep_lm_scripts_meet_every_case_it_was_built_for(models):
    f, rec = models["fsa"]["deep"], models["rec"]["deep"]
    at = {(x["script"], x["pos"]): x for x in rec}
    bo = lambda x: [float(f.states["backoff_prob"][s]) for s, _, _ in x["probes"][:-1]]   # the weights a look-up's chain adds
    for fam in U.DEEP_FAMILIES:
        # the word case: from the state of (a b c d), x is found after word_depth back-offs, through every suffix state in turn
        i = _script_with(models, list(fam["ctx"]) + [fam["x"]], 0)
        x = at[(i, 4)]
        assert x["depth"] == fam["word_depth"] and [at[(i, k)]["depth"] for k in (1, 2, 3)] == [0, 0, 0], fam
        assert all(w != 0 for w in bo(x)) and len(set(bo(x))) == len(bo(x))
        if fam["word_depth"] == 4:
            assert x["probes"][-1][0] == 0 and x["probes"][3][0] == fam["ctx"][3] + 1   # ... (d)'s unigram state, then the empty history
        # the </s> case: a script that ENDS in the state of (a b c d); its final cost finds </s> after eos_depth back-offs
        i = _script_with(models, list(fam["ctx"]), 2)
        x = at[(i, U.N_WORDS)]
        assert x["word"] == f.eos and x["depth"] == fam["eos_depth"] and at[(i, 5)]["depth"] == 0, fam
        assert all(w != 0 for w in bo(x)) and len(set(bo(x))) == len(bo(x))
    assert {x["depth"] for x in rec if x["pos"] == U.N_WORDS} == {0, 1, 2, 3, 4}
    assert {dp for _, dp in U.walk_profile(f, models["scripts"])} >= {0, 1, 2, 3, 4}
    # the 5-gram whose context chain exists at every order: four arcs found in a row, the fifth too
    i = _script_with(models, list(U.DEEP_FAMILIES[0]["ctx"]) + [U.DEEP_FAMILIES[0]["x"]], 0)
    assert [at[(i, k)]["depth"] for k in (1, 2, 3, 4)] == [0, 0, 0, 0] and f.states["arc_num"][at[(i, 4)]["next"]] == 0   # ... into a leaf
    # a back-off that skips a level: the trigram state's suffix bigram is absent, so it backs off to the unigram state
    for word, depth in ((U.SKIP["bigram_word"], 1), (U.SKIP["unigram_word"], 2)):
        i = _script_with(models, list(U.SKIP["ctx"]) + [word], 0)
        x = at[(i, 3)]
        assert at[(i, 2)]["depth"] == 0 and x["depth"] == depth and x["probes"][1][0] == U.SKIP["ctx"][2] + 1
    # the dropped trigram: its words walk on as if the line were not there
    i = _script_with(models, list(U.DROPPED), 0)
    assert at[(i, 1)]["depth"] == 1 and at[(i, 2)]["depth"] >= 1
    # the word without a unigram: asked for, priced by the on-demand arc, and looked up FROM (its state has neither arcs nor weight)
    x = [y for y in rec if y["word"] == U.NO_UNIGRAM]
    assert x and all(y["next"] == U.NO_UNIGRAM + 1 and y["probes"][-1][0] == 0 for y in x)
    assert any(y["state"] == U.NO_UNIGRAM + 1 for y in rec)
    # leaf states are looked up from (the table is probed for a state that has no entry at all)
    assert sum(1 for y in rec if y["state"] and f.states["arc_num"][y["state"]] == 0) >= 10


def test_script_graph_shape(models):
    g, sc = models["graph"], models["scripts"]
    assert 48 <= len(sc) <= 72 and g.n_arcs < 400
    assert sum(s["tail"] for s in sc) * 2 >= len(sc) - 8                      # about half join the shared tail
    assert sum(s["eps"] is not None for s in sc) == (len(sc) + 3) // 4        # a quarter hold a word on an input-epsilon arc
    assert {e[1] for e in (s["eps"] for s in sc) if e} == {"before", "after"}
    il = g.arcs["ilabel"]
    assert len(set(il[il > 0].tolist())) == int((il > 0).sum()) == models["n_tid"]   # a transition id (and a pdf) of its own per emitting arc
    ol = g.arcs["olabel"]
    assert ol.max() <= U.V and (ol[il == 0] > 0).sum() == sum(s["eps"] is not None for s in sc)
    # the tail states are reached with several LM histories: the tail scripts differ in the LM state they bring along
    for name in ("clusterA", "clusterB", "deep"):
        pre = {x["state"] for x in models["rec"][name] if x["pos"] == 4 and sc[x["script"]]["tail"]}
        assert len(pre) >= 8, name
