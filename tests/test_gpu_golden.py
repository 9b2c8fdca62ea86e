"""-m gpu: the HIP path, called through the C ABI, against the reference-generated golden vectors
(tests/golden/*.npz).  Bit-exact: words, transition-ids, per-hop labels and float costs, tot/lm
score.  Per-frame best cost must match bit for bit; the per-frame token count may only be
SMALLER than the reference's (the reference keeps order-dependent 'extras' that lost against the
final next_cutoff and are never expanded, base-inl.h:330-333; DESIGN.md 'Deviations').
Where max_active / min_active bind, the reference's own result depends on those extras; there the
GPU is held, bit for bit, to the oracle's order-free mode on the golden's inputs."""
import numpy as np
import pytest

from golden_util import GOLDEN_NAMES, Golden, bits

pytestmark = pytest.mark.gpu


def _beam_only(cd, g):
    """max_active / min_active never bind for this golden group?"""
    return cd["max_active"] >= 100000 and cd["min_active"] == 0


@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_gpu_reproduces_golden(name, oracle, tmp_path):
    import gpu_util as G
    import pyoracle

    g = Golden(name)
    graph = G.wfstdec.Graph.load(g.write_graph(str(tmp_path / "g.bin")))
    if g.tid2pdf is not None:
        graph.set_tid2pdf(g.tid2pdf)
    # group cases by (cfg, mode): all utterances of a group decode as one batch
    groups = {}
    for k, cd, md, ui in g.cases():
        groups.setdefault((g.meta["cases"][k]["cfg"], g.meta["cases"][k]["mode"]), []).append((k, ui))
    n_checked = 0
    for (ci, mi), items in groups.items():
        cd = dict(g.meta["cfgs"][ci])
        md = dict(g.meta["modes"][mi])
        trace = md.pop("trace", False)
        mats = [g.utts[ui] for _, ui in items]
        # the eps_chains group holds matrices of different widths only across groups, not within
        res = G.decode_batch(graph, cd, mats, trace=trace, **md)
        for (k, ui), r in zip(items, res):
            e = g.expected(k)
            what = "%s case %d (cfg %d mode %d utt %d)" % (name, k, ci, mi, ui)
            assert bool(r.ok) == bool(int(e["ok"])), what
            exact = _beam_only(cd, g) or name not in ("hclg600", "neg_hclg600")
            if exact:
                G.assert_same_path(r, e["words"], e["tids"], e["path_ilabel"], e["path_olabel"],
                                   e["path_graph"], e["path_ac"], e["scores"], what)
                if trace:
                    assert np.array_equal(bits(r.frame_best), bits(e["frame_best"])), what + " best cost per frame"
                    assert np.all(r.frame_ntoks <= e["frame_ntoks"]), what + " token counts exceed the reference's"
                n_checked += 1
            else:
                ho = oracle.load_graph(str(tmp_path / "g.bin"))
                try:
                    oracle.set_order_free(True)
                    o = oracle.decode(ho, pyoracle.Config(**cd), g.utts[ui], g.tid2pdf, **md)
                finally:
                    oracle.set_order_free(False)
                    oracle.free_graph(ho)
                assert o.extra["ties"] == 0, what + ": exact cost tie on the best path of a golden case"
                G.assert_same_as_oracle(r, o, what + " (order-free)")
                n_checked += 1
    graph.free()
    assert n_checked > 0
