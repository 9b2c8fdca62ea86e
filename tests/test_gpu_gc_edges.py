"""-m gpu: the token collection of best-path decoders (gc_pass in wfst_kernels.hip, the reserve and stride of wfst_capi.cc) at its
table, sweep, chunk and mark edges, on the cases of tests/gc_util.py (each aimed at one of the constants the code is cut along;
tests/test_gc_graphs.py proves on the CPU the frame sizes, that every decode compared here is `ok` and tie-free under the oracle,
and how many of the host's checks find the arena beyond its mark).  Every case asserts dec.path_flags() -- two_launch, gc_stride,
degcode, staged --, so none can silently run another path, and stats(c)["collections"] against the CPU file's count.  Bit for bit:

* after finalize: words, transition-ids, per-hop labels, graph and acoustic cost bits and tot_score against the order-free oracle;
* after every advance behind which stats(c)["collections"] has moved: best_paths(use_final_probs=False) against the oracle's
  decode of the same prefix, and dec.frontier(c), sorted by state, equal in states and cost bits to the oracle's tokens of that
  frame below its final cutoff -- a collection must not lose, duplicate or reprice a frontier token (biglm, whose tokens are
  (state, LM state) pairs: the multiset of (graph state, cost bits));
* at the end: dec.words() -- word times go through the rewritten frame_off[] -- equal to those of a twin decoder on the same input
  whose arena is roomy enough for collections == 0.

The channels of a decoder are ragged: one has 3 frames and never collects, one stops on the frame at which the others collect
(a channel at its target is not collected)."""
import time

import numpy as np
import pytest

import gc_util as GC
import geometry_util as U
from golden_util import bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(synth, oracle, tmp_path_factory):
    g = U.Gpu(GC.World(synth, oracle, str(tmp_path_factory.mktemp("gc"))))
    yield g
    g.free()


def _same_words(a, b, what):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), what + " words and times"
    assert np.array_equal(bits([a[3], a[4]]), bits([b[3], b[4]])) and a[5] == b[5], what + " scores, hops"


@pytest.mark.parametrize("case", GC.CASES, ids=[c.id for c in GC.CASES])
def test_leg(gpu, case):
    G, W, world = gpu.G, gpu.W, gpu.world
    t0 = time.time()
    name, B, T = case.graph, len(case.T), case.T
    graph = gpu.graph(name, case.gopt)
    _, facts = world.graph(name)
    assert facts["fusable"] == case.fusable
    dev = G.upload(world.mats(name))
    ptrs = [dev[u].data_ptr() for u in case.utt]
    kw = {}
    if case.biglm:
        kw["old_lm"], kw["new_lm"] = gpu.lm_pair()
    if case.options:
        kw["options"] = W.Options(**case.options)
    decode = world.oracle_biglm if case.biglm else world.oracle_decode
    cfg = G.gpu_config(GC.CFGS[case.cfg])
    expected = [world.expected(case, c) for c in range(B)]
    dec = W.BatchDecoder(graph, cfg, B, **dict(case.limits(), **kw))
    # (the mark lies at half the arena or above: twice the utterance's tokens and four frames at the limit are never beyond it)
    created = max(int(world.counts(case, u)[:max(T) + 1].sum()) for u in set(case.utt))
    roomy = dict(case.limits(), arena_tokens=2 * created + 4 * case.max_tok + 4096)
    twin = W.BatchDecoder(graph, cfg, B, **dict(roomy, **kw))

    def check_flags(when):
        pf = dec.path_flags()
        assert {k: pf[k] for k in case.flags} == case.flags, "%s, %s: path flags %s" % (case.id, when, pf)

    try:
        twin.init()
        twin.advance(ptrs, T, GC.N_COLS)
        twin.finalize()
        twin_words = twin.words()
        assert all(twin.stats(c)["collections"] == 0 for c in range(B)), "the twin's arena is not roomy"
        for si, sched in enumerate(case.schedules):
            dec.init()
            seen = [0] * B
            for r in sched:
                dec.advance(ptrs, [min(r, t) for t in T], GC.N_COLS)
                for c in range(B):
                    n = int(dec.stats(c)["collections"])
                    if n == seen[c]:
                        continue
                    seen[c] = n
                    k = min(r, T[c])
                    what = "%s schedule %d channel %d, %d frames, %d collections" % (case.id, si, c, k, n)
                    po = decode(name, case.ocfg, case.utt[c], frames=k, partial=True)
                    assert po.ok and po.extra["ties"] == 0, what
                    G.assert_same_as_oracle(G.GpuResult(dec.best_paths(channels=[c], use_final_probs=False)[0]), po, what + ", partial")
                    st, co = dec.frontier(c, cap=1 << 16)
                    st, co = GC.by_state_and_cost(st, co)
                    ost, oco = world.frontier(case, case.utt[c], k)
                    assert np.array_equal(st, ost), what + ": frontier states (%d, the oracle %d)" % (len(st), len(ost))
                    assert np.array_equal(bits(co), bits(oco)), what + ": frontier costs"
            dec.finalize()
            check_flags("schedule %d" % si)
            got, words = dec.best_paths(), dec.words()
            for c in range(B):
                what = "%s schedule %d channel %d" % (case.id, si, c)
                want = decode(name, case.ocfg, case.utt[c], frames=T[c])
                assert want.ok and want.extra["ties"] == 0, what
                G.assert_same_as_oracle(G.GpuResult(got[c]), want, what)
                _same_words(words[c], twin_words[c], what)
                lo, hi, fits = expected[c][si]
                n = int(dec.stats(c)["collections"])
                assert fits and n >= len(lo), what + ": %d collections, the CPU file's count %d" % (n, len(lo))
                if lo == hi:
                    assert n == len(lo), what + ": %d collections, the CPU file's count %d" % (n, len(lo))
                if T[c] == max(T):
                    assert n >= case.min_collections, what
                if T[c] == 3 and case.arena >= 6 * case.n_tok:
                    assert n == 0, what
                if case.leg != "soft_limit":
                    assert dec.degraded_frames(c) == 0, what + " degraded frames"
                elif T[c] > 3:
                    assert dec.degraded_frames(c) > 0, what + ": the limit never bound"
            if case.stopper and si == 0:
                c, k = case.stopper
                assert int(dec.stats(c)["collections"]) == k - 1, "%s: the channel that stops on a collecting frame" % case.id
        if case.error_T:
            # the same decoder, the utterances (not finalized this time) continued: a collection frees nothing, the arena fills -- a
            # loud capacity error that stays the channel's; channel 4, initialised again, decodes 10 frames in the arena right
            # behind a failing channel's
            dec.init()
            for r in case.schedules[0]:
                dec.advance(ptrs, [min(r, t) for t in T], GC.N_COLS)
            dec.sync()
            assert int(dec.stats(0)["collections"]) >= case.min_collections
            dec.init(channels=[4])
            target = [case.error_T if t == max(T) else t for t in T]
            target[4] = 10
            codes = []
            with pytest.raises(W.WfstError) as e:
                dec.advance(ptrs, target, GC.N_COLS)
                dec.sync()
            codes.append(e.value.code)
            assert "arena" in str(e.value)
            with pytest.raises(W.WfstError) as e:
                dec.sync()
            codes.append(e.value.code)
            assert codes == [-4, -4]
            dec.finalize(channels=[4])
            r = G.GpuResult(dec.best_paths(channels=[4])[0])
            want = decode(name, case.ocfg, case.utt[4], frames=10)
            assert want.ok and want.extra["ties"] == 0
            G.assert_same_as_oracle(r, want, "%s: the channel behind the failing one" % case.id)
    finally:
        dec.free()
        twin.free()
    print("%s: %.1f s" % (case.id, time.time() - t0))
