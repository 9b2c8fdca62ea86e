"""The oracle's tie mode (oracle/wfst_oracle.c g_tie_rule; DESIGN.md section 4, deviation 3) and the tie-dense workloads of
tests/tie_util.py, on the CPU.

 - Where no exact cost tie occurs the tie mode IS the default mode: every golden and every signed-cost workload, bit for bit.
 - The hand-written graphs: the tie is there, the tie mode gives the path the rule names, the default mode the other one.
 - test_the_data_does_what_it_claims: the quantised workloads are tie-dense and tell the two rules apart (tests/test_gpu_ties.py
   runs it too: its comparisons would prove nothing on data without ties)."""
import numpy as np
import pytest

import pyoracle
import signed_util as S
import tie_util as TU
from golden_util import GOLDEN_NAMES, Golden, bits


def _same(a, b, what):
    assert a.ok == b.ok, what
    assert TU.labels(a) == TU.labels(b), what + " labels"
    assert np.array_equal(bits(a.path_graph), bits(b.path_graph)) and np.array_equal(bits(a.path_ac), bits(b.path_ac)), what + " costs"
    assert np.array_equal(bits([a.tot_score, a.lm_score]), bits([b.tot_score, b.lm_score])), what + " scores"
    assert (a.num_toks_end, a.num_links_end) == (b.num_toks_end, b.num_links_end), what + " token / link counts"
    assert a.extra == b.extra, what + " counters"


def _both(oracle, h, cd, x, m, order_free=False, **kw):
    try:
        oracle.set_order_free(order_free)
        a = oracle.decode(h, pyoracle.Config(**cd), x, m, **kw)
        oracle.set_tie_rule(True)
        b = oracle.decode(h, pyoracle.Config(**cd), x, m, **kw)
    finally:
        oracle.set_tie_rule(False)
        oracle.set_order_free(False)
    return a, b


@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_tie_mode_is_the_default_mode_where_nothing_ties_goldens(name, oracle, tmp_path):
    g = Golden(name)
    h = oracle.load_graph(g.write_graph(str(tmp_path / "g.bin")))
    n = tied = 0
    try:
        for k, cd, md, ui in g.cases():
            kw = dict(chunk=md.get("chunk", 0), finalize=md.get("finalize", True), use_final_probs=md.get("use_final_probs", True))
            for of in (False, True):
                a, b = _both(oracle, h, cd, g.utts[ui], g.tid2pdf, of, **kw)
                if a.extra["ties"] == 0:
                    _same(a, b, "%s case %d order-free %d" % (name, k, of))
                    n += 1
                else:
                    tied += 1
    finally:
        oracle.free_graph(h)
    assert n > 0 or name == "quirk_parallel_arcs", (n, tied)   # (that golden's parallel arcs tie in every case)


def test_tie_mode_is_the_default_mode_where_nothing_ties_signed_costs(synth, oracle, tmp_path):
    g, m, mats = S.workloads(synth)
    p = str(tmp_path / "g.bin")
    g.write(p)
    h = oracle.load_graph(p)
    n = 0
    try:
        for name in mats:
            for cd in S.CFGS:
                for ui, x in enumerate(mats[name]):
                    a, b = _both(oracle, h, cd, x, m, True)
                    if a.extra["ties"] == 0:
                        _same(a, b, "%s utt %d" % (name, ui))
                        n += 1
    finally:
        oracle.free_graph(h)
    assert n >= 16


def test_hand_written_ties(synth, oracle, tmp_path):
    to = TU.TieOracle(oracle)
    for name, g, x, uf, w_rule, w_first in TU.hand_graphs(synth):
        p = str(tmp_path / (name + ".bin"))
        g.write(p)
        h = oracle.load_graph(p)
        a = to.decode(h, TU.HAND_CFG, x, None, True, finalize=uf, use_final_probs=uf)
        b = to.decode(h, TU.HAND_CFG, x, None, False, finalize=uf, use_final_probs=uf)
        oracle.free_graph(h)
        assert a.ok and b.ok and bits([a.tot_score]) == bits([b.tot_score]), name
        assert a.words.tolist() == [w_rule] and b.words.tolist() == [w_first], (name, a.words, b.words)
        if name != "two_ends":   # (a tie between END tokens is no tied hop: extra["ties"] counts hops)
            assert a.extra["ties"] > 0 and b.extra["ties"] > 0, name


def test_hand_written_biglm_ties(synth, oracle, tmp_path):
    """(d): each biglm case ties, and the rule's path differs from the first-arrival path at an equal total"""
    import importlib

    lmsynth = importlib.import_module("asr-decoder_amd.lmsynth")
    to = TU.TieOracle(oracle)
    p1, p2 = str(tmp_path / "old.bin"), str(tmp_path / "new.bin")
    TU.flat_lm(lmsynth, -1.0, -0.5).to_fsa().write(p1)
    TU.flat_lm(lmsynth, -2.0, -0.25).to_fsa().write(p2)
    o1, o2 = pyoracle.Lm(oracle, p1, -1.0), pyoracle.Lm(oracle, p2, 1.0)
    try:
        for name, g, x, w_rule, w_rule2 in TU.biglm_hand_graphs(synth):
            p = str(tmp_path / (name + ".bin"))
            g.write(p)
            h = oracle.load_graph(p)
            first, rule, rule2 = (to.biglm_decode(h, TU.BIGLM_CFG, o1, o2, x, None, t) for t in (0, 1, 2))
            oracle.free_graph(h)
            assert first.ok and rule.ok and rule2.ok and rule.extra["lm_oob"] == 0, name
            assert rule.words.tolist() == w_rule and rule2.words.tolist() == w_rule2, name
            assert first.words.tolist() != rule.words.tolist(), name + ": first arrival gives the rule's path"
            assert bits([first.tot_score]) == bits([rule.tot_score]) == bits([rule2.tot_score]), name
            if name == "merge":   # (two_final_pairs ties between END tokens: no tied hop)
                assert rule.extra["ties"] > 0
    finally:
        o1.free()
        o2.free()


def tie_figures(synth, oracle, d):
    """(pairs, tied pairs, pairs whose final or some prefix path differs in labels between the two rules, differing paths) over
    the (utterance, configuration) pairs of workloads (a) and (b)"""
    to = TU.TieOracle(oracle)
    pairs = tied = discr = paths = 0
    work = []
    g, m, mats = TU.big_workload(synth)
    work.append(("big", g, m, mats, S.CFGS))
    work += [(n, g, None, mats, TU.SMALL_CFGS) for n, g, mats in TU.small_workloads(synth)]
    for name, g, m, mats, cfgs in work:
        p = str(d / (name + ".bin"))
        g.write(p)
        h = oracle.load_graph(p)
        for cd in cfgs:
            for x in mats:
                a = [to.decode(h, cd, x, m, True)] + to.prefixes(h, cd, x, m, True)
                b = [to.decode(h, cd, x, m, False)] + to.prefixes(h, cd, x, m, False)
                assert all(r.ok for r in a + b), name
                nd = sum(TU.labels(u) != TU.labels(v) for u, v in zip(a, b))
                pairs += 1
                tied += int(any(r.extra["ties"] > 0 for r in a))
                discr += int(nd > 0)
                paths += nd
        oracle.free_graph(h)
    return pairs, tied, discr, paths


def test_the_data_does_what_it_claims(synth, oracle, tmp_path):
    pairs, tied, discr, paths = tie_figures(synth, oracle, tmp_path)
    print("figures: %d of %d (utterance, configuration) pairs with an exact cost tie on a final or per-frame-prefix best path; "
          "the two rules differ in labels on %d of the %d, on %d paths" % (tied, pairs, discr, pairs, paths))
    assert 2 * tied >= pairs, (tied, pairs)
    assert discr >= 5, discr
    small = TU.small_workloads(synth)
    assert any(TU.has_parallel_arcs(g) for _, g, _ in small)
    assert any((g.arcs["w"][g.arcs["ilabel"] == 0] < 0).any() for _, g, _ in small), "no graph that cannot take fused closures"


# ---- the rule stated independently (tests/tie_reference.py) -----------------------------------------------------------------------
REF_CFG = dict(beam=8.0, max_active=2147483647, min_active=0, lattice_beam=1.0e6, prune_interval=10)


def _equals_rule(r, want, what):
    assert bool(r.ok) == (want is not None), what
    if want is None:
        return
    hops, tot, lm = want
    assert r.path_ilabel.tolist() == [h[0] for h in hops] and r.path_olabel.tolist() == [h[1] for h in hops], what + " labels"
    assert np.array_equal(bits(r.path_graph), bits([h[2] for h in hops])) and np.array_equal(bits(r.path_ac), bits([h[3] for h in hops])), what + " costs"
    assert np.array_equal(bits([r.tot_score, r.lm_score]), bits([tot, lm])), what + " scores"


@pytest.mark.parametrize("biglm", [False, True])
def test_tie_mode_equals_the_rule_stated_in_numpy(biglm, synth, oracle, tmp_path):
    """the best path and the best path of every prefix, labels and float bits, on the small quantised graphs (and the hand-written
    ones): the C oracle's tie mode (order-free) against tests/tie_reference.py"""
    import importlib

    import tie_reference as TR

    to = TU.TieOracle(oracle)
    lms = []
    if biglm:
        lmsynth = importlib.import_module("asr-decoder_amd.lmsynth")
        p1, p2 = str(tmp_path / "old.bin"), str(tmp_path / "new.bin")
        f1, f2 = TU.biglm_random(lmsynth)
        f1.write(p1)
        f2.write(p2)
        lms = [pyoracle.Lm(oracle, p1, -1.0), pyoracle.Lm(oracle, p2, 1.0)]
    work = [(n, g, mats[:2]) for n, g, mats in TU.small_workloads(synth)]
    if not biglm:
        work += [(n, g, [x]) for n, g, x, _, _, _ in TU.hand_graphs(synth)]
    else:
        work = work[:4] + [(n, g, [x]) for n, g, x, _, _ in TU.biglm_hand_graphs(synth)]
    n_paths = n_tied = 0
    try:
        for name, g, mats in work:
            p = str(tmp_path / (name + ".bin"))
            g.write(p)
            h = oracle.load_graph(p)
            rule = TR.Rule(g, REF_CFG["beam"], *lms)
            dec = (lambda x, **kw: to.biglm_decode(h, REF_CFG, lms[0], lms[1], x, None, 1, **kw)) if biglm else \
                  (lambda x, **kw: to.decode(h, REF_CFG, x, None, True, **kw))
            for ui, x in enumerate(mats):
                r = dec(x)
                _equals_rule(r, rule.decode(x, None, True), "%s utt %d" % (name, ui))
                n_paths += 1
                n_tied += int(r.extra["ties"] > 0)
                for k in range(1, len(x) + 1):
                    r = dec(x[:k], chunk=1, finalize=False, use_final_probs=False)
                    _equals_rule(r, rule.decode(x[:k], None, False), "%s utt %d prefix %d" % (name, ui, k))
                    n_paths += 1
                    n_tied += int(r.extra["ties"] > 0)
            oracle.free_graph(h)
    finally:
        for l in lms:
            l.free()
    print("figures: %d paths equal to the numpy statement of the rule, %d of them through a tied hop (biglm %d)" % (n_paths, n_tied, biglm))
    assert n_tied > 0, "no tie on any path: the comparison would not reach the ordering key"
