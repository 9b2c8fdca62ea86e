"""The cases of tests/gc_util.py do what they claim, on the CPU: the shape facts of every graph recomputed from its arrays (the
epsilon-won states W, the distinct states they want, the chain depth, whether the loader fuses it); every (graph, configuration,
utterance, prefix) that tests/test_gpu_gc_edges.py decodes is `ok` and free of exact ties under the order-free oracle (a draw
with a tie gets another seed HERE; the GPU file skips nothing); the oracle's per-frame token counts are exactly what each leg aims
at; and from those counts and the restated reserve and stride rule (gc_util.reserve_and_stride, gc_util.simulate) at least the
intended number of the host's checks find the arena beyond its mark -- with the fewest survivors a collection can leave (one
token per old frame for fan, everything but the super-final state's for comb) for the count, with the most (the hub's
predecessor chain for fan, everything for comb) for "it fits the arena".  Where both give the same frames the count is exact.

The constants the legs stand on are restated in gc_util (NEED_SLOTS, NEED_STOP, MOVER_CHUNK, reserve_and_stride) and held to
the sources below: when one moves, this file fails; the GPU legs do not lose their aim silently."""
import os
import re

import numpy as np
import pytest

import gc_util as GC

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "asr-decoder_amd", "csrc")
BY_LEG = {}
for _c in GC.CASES:
    BY_LEG.setdefault(_c.leg, []).append(_c)


@pytest.fixture(scope="module")
def world(synth, oracle, tmp_path_factory):
    return GC.World(synth, oracle, str(tmp_path_factory.mktemp("gc")))


# ---- the constants ---------------------------------------------------------------------------------------------------------------
def test_the_constants_the_legs_stand_on():
    k = open(os.path.join(CSRC, "wfst_kernels.hip")).read()
    assert int(re.search(r"constexpr int kGcNeedSlots = (\d+);", k).group(1)) == GC.NEED_SLOTS
    assert "atomicAdd(&gs.n_need, 0) < (kGcNeedSlots * 3) / 4" in k and GC.NEED_STOP == 1536
    assert int(re.search(r"constexpr int kBT = (\d+);", k).group(1)) == 1024
    gc = k[k.index("__device__ __forceinline__ void gc_pass("):k.index("__global__ __launch_bounds__(kBT) void closure_kernel(")]
    assert int(re.search(r"constexpr int kCU = (\d+);", gc).group(1)) * 1024 == GC.MOVER_CHUNK
    assert "i0 += kBT * kCU" in gc
    # the error word is zeroed once, at entry: phase 1's diagnostic (no token on a wanted state) reaches kErrInternal
    assert gc.count("ps.err = 0") == 1 and gc.index("ps.err = 0") < gc.index("(1) mark") and "if (ps.err) ctl->error |= kErrInternal" in gc
    assert "new_end + (int)((D.arena_cap - new_end) / 2)" in gc and "(int64_t)(D.gc_stride + 1) * D.max_tok" in gc
    h = open(os.path.join(CSRC, "wfst_capi.cc")).read()
    for line in ("int64_t reserve = std::max<int64_t>(2 * M, A / 8);", "std::min<int64_t>(17 * M, A / 4)", "if (reserve >= A / 2) reserve = A / 2;",
                 "const int64_t stride = reserve / M - 1;", "std::min<int64_t>(stride, 16)", "(s % d->D.gc_stride) == d->D.gc_stride - 1"):
        assert line in h, line
    assert "const int64_t bucket_cap = std::max<int64_t>(2048, 8 * M / n_part);" in h and "(int64_t)lds_slots << (log2part - 1) >= 4 * M" in h
    assert "o->log2_lds_slots = 12;" in h and "(L.lattice_links > 0 && !big) ? 6 : 5" in h and GC.bucket_cap(16384) == 8192 == GC.bucket_cap(32768)
    assert int(re.search(r"constexpr int kHeadSteps = (\d+);", h).group(1)) * 4 <= 130   # stride_s: one call is split in head and rest


def test_reserve_and_stride():
    r = GC.reserve_and_stride
    # stride_s: three launches, then strides 1, 2, 7 and 16
    assert [r(1024, a) for a in (3072, 4096, 12288, 32768, 1 << 17)] == [(1536, 0, 0), (2048, 1, 1), (3072, 1, 2), (8192, 1, 7), (17408, 1, 16)]
    assert [c.flags["gc_stride"] for c in BY_LEG["stride_s"]] == [1, 1, 2, 7, 16] and [c.flags["two_launch"] for c in BY_LEG["stride_s"]] == [0, 1, 1, 1, 1]
    assert r(4096, 1 << 17) == (32768, 1, 7) and r(16384, 1 << 19) == (131072, 1, 7) and r(32768, (1 << 22) + 4096) == (557056, 1, 16)
    assert r(16384, 18520) == (9260, 0, 0) and r(2048, 24080) == (6020, 1, 1)
    # decoders that keep no best row (plain closure, biglm) never run two launches: an eighth, two frames at least, half at most
    assert r(1024, 1 << 17, best_row=False) == (16384, 0, 0) and r(1024, 3072, best_row=False) == (1536, 0, 0)
    # the schedules of stride_s: one call, frame by frame, 7, and stride - 1, stride, stride + 1
    for c in BY_LEG["stride_s"]:
        s = c.flags["gc_stride"]
        chunks = [sc[0] for sc in c.schedules]
        assert chunks[:3] == [130, 1, 7] and set(chunks[3:]) == {k for k in (s - 1, s, s + 1) if k > 1 and k != 7}, (c.id, chunks)


def test_simulate_on_a_hand_made_case():
    # 10 tokens a frame (frame 0: 1), arena 100, limit 10: reserve 25 (a quarter), stride 1 (two launches, every step classic), base mark 75
    keep1 = lambda f, n: 1
    assert GC.reserve_and_stride(10, 100) == (25, 1, 1)
    ran, peak, fits = GC.simulate([1] + [10] * 30, 30, [30], [30], 10, 100, keep1)
    # 1 + 10 k > 75 first at k = 8: 8 old frames of 1 + the frontier's 10 = 18 left; mark max(75, min(59, 100 - 20)) = 75; then every 6 frames,
    # and every 5 once 25 old frames have left a token each (25 + 10 + 50 = 85 at the end, the peak)
    assert ran == [8, 14, 20, 25] and peak == 85 and fits
    # frame by frame: the check is the call's first launch -- the same frames
    assert GC.simulate([1] + [10] * 30, 30, list(range(1, 31)), [30], 10, 100, keep1)[0] == ran
    # a channel at its target is not collected; one that stops earlier than a check never sees it
    assert GC.simulate([1] + [10] * 30, 8, [30], [30, 8], 10, 100, keep1)[0] == []
    # nothing freed: the arena fills
    assert not GC.simulate([1] + [10] * 30, 30, [30], [30], 10, 100, lambda f, n: n)[2]


# ---- shape facts ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GC.GRAPHS))
def test_shape_facts(world, name):
    g, f = world.graph(name)
    m = re.match(r"fan(\d+)x(\d+)(?:p(\d+))?(?:w\d+)?$", name)
    assert f["max_label"] < GC.N_COLS and f["single_eps_in"]
    if m:
        E, depth, pend = int(m.group(1)), int(m.group(2)), int(m.group(3) or 0)
        # the v states and the super-final state: no emitting arc enters them; each wants a state of its own (the hub among them)
        assert f["W"] == E * depth + 1 and f["sources"] == E * depth + 1 and f["chain_depth"] == depth
        assert f["n_states"] == 1 + E * (1 + depth) + pend + 1 == GC.fan_tokens(E, depth, pend)
        assert f["fusable"] == (depth <= 8)
        assert int(f["n_emit"][0]) == 1 + E + pend and int(f["n_eps"][0]) == 1
    else:
        N = int(name[4:])
        # the a states (the b states are entered by emitting arcs) and the super-final state, which all N * R a states enter
        assert f["W"] == 3 * N + 1 and f["sources"] == 6 * N and f["chain_depth"] == 2 and f["fusable"]
        assert (np.bincount(g.arcs["to"], minlength=g.n_states)[1:-1] <= 2).all()   # nothing merges (ring entry: the start's arc and the ring's)


def test_the_need_table_edges():
    """W + 1 distinct wanted states in the frontier's frame (fan) or N in every old frame (comb) on both sides of the claim stop,
    of the full table, and beyond what 1024 threads can overshoot the stop by."""
    need = sorted({int(c.graph[3:].split("x")[0]) + 1 for c in BY_LEG["need_W"]})
    assert need == [1401, 1536, 1537, 1538, 2048, 2049, 2050, 2601, 5001]
    assert GC.NEED_STOP - 1 in need or GC.NEED_STOP in need
    assert {GC.NEED_STOP, GC.NEED_STOP + 1, GC.NEED_SLOTS, GC.NEED_SLOTS + 1} <= set(need)
    assert max(n for n in need if n < GC.NEED_OVERSHOOT) > GC.NEED_SLOTS and need[-2] > GC.NEED_OVERSHOOT
    assert need[-1] > 2 * GC.NEED_OVERSHOOT - GC.NEED_STOP   # three sweeps at least, however the race goes: 5001 > 2 * 2559
    for leg in ("need_plain", "need_biglm"):
        assert all(int(c.graph[3:].split("x")[0]) + 1 > GC.NEED_STOP for c in BY_LEG[leg])
    assert [(c.graph, c.fusable) for c in BY_LEG["chain"]] == [("fan400x8", True), ("fan250x12", False)]
    assert 1600 > GC.NEED_STOP and 4097 > GC.NEED_SLOTS   # comb: every old frame


def test_the_mover_chunk_edges():
    sizes = [c.n_tok for c in BY_LEG["chunk_edge"]]
    assert sizes == [GC.MOVER_CHUNK - 1, GC.MOVER_CHUNK, GC.MOVER_CHUNK + 1, 2 * GC.MOVER_CHUNK + 1, 8195]
    assert 2 * 4097 > GC.MOVER_CHUNK   # comb(4097): 8194 survivors of 8195 in every old frame, across a round's edge


def eps_runs(ilabels):
    """(frame, hops) of every run of epsilon hops on a best path (frame: the emitting hops before it)"""
    runs, frame, n = [], 0, 0
    for il in list(ilabels) + [1]:
        if il == 0:
            n += 1
            continue
        if n:
            runs.append((frame, n))
        frame, n = frame + 1, 0
    return runs


# ---- every case of the GPU test --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GC.CASES, ids=[c.id for c in GC.CASES])
def test_case(world, case):
    name, T, B = case.graph, case.T, len(case.T)
    _, f = world.graph(name)
    assert f["fusable"] == case.fusable and (3 <= B <= 8 or case.leg == "big_arena")
    assert case.flags["staged"] == int(case.fusable and case.gopt is None and not case.biglm)
    decode = world.oracle_biglm if case.biglm else world.oracle_decode
    Tl = max(T)
    for c in range(B):
        ui = case.utt[c]
        what = "%s channel %d" % (case.id, c)
        o = decode(name, case.ocfg, ui, frames=T[c])
        assert o.ok and o.extra["ties"] == 0, what + ": an exact tie on the best path -- change the seed"
        counts = world.counts(case, ui)
        if not case.biglm and case.leg != "soft_limit":
            # the exact tokens per frame the leg aims at (frame 0: the start state and its closure)
            assert counts[0] == (2 if case.kind == "fan" else 1) and (counts[1:] == case.n_tok).all(), (what, counts)
        elif case.biglm:
            # (state, LM state) pairs: the frame size the arena is cut for, from frame 3 on; every v state and the super-final
            # state occupied in the frames at which a collection runs -- W distinct wanted states, beyond the claim stop
            assert (counts[3:Tl + 1] == case.n_tok).all() and (counts[:3] <= case.n_tok).all(), (what, counts)
            if T[c] == Tl:
                for nd in world.expected(case, c)[0][1][:3]:
                    st, _, n = world.biglm_dump(case, ui, nd)
                    assert n == len(st) == counts[nd]
                    assert len(set(st[f["eps_won"][st]].tolist())) == f["W"] > GC.NEED_STOP, (what, nd)
        for si, (lo, hi, fits) in enumerate(world.expected(case, c)):
            assert fits, what + ": the live tokens do not fit the arena"
            assert len(lo) <= len(hi)   # (more survivors: less room behind a collection, the next one no later)
            if T[c] == Tl:
                assert len(lo) >= case.min_collections, (what, si, lo)
            if T[c] == 3 and case.arena >= 6 * case.n_tok:   # (stride_s: the arena of 3072 tokens is three frames)
                assert hi == []
            if case.kind == "fan" and case.leg not in ("soft_limit", "need_biglm", "stride_s"):
                assert lo == hi, (what, si, lo, hi)   # the count is exact (stride_s: 130 frames leave up to 3 tokens each in arenas of 3 to 130 frames)
            # the prefixes the GPU file compares after an advance behind which a collection ran (where the count is not exact:
            # every prefix of the schedule, whichever of them the device collects behind)
            sched, seen = case.schedules[si], 0
            for r in sched:
                k = min(r, T[c])
                n = sum(1 for x in lo if x < k)
                if n == seen and lo == hi:
                    continue
                seen = n
                p = decode(name, case.ocfg, ui, frames=k, partial=True)
                assert p.ok and p.extra["ties"] == 0, (what, si, k)
        if case.leg == "chain" and T[c] == Tl:
            # an old frame is re-swept once per epsilon hop of the chain that survives in it: the best path runs through a WHOLE
            # chain (depth hops) in a frame that a later collection finds old
            last = world.expected(case, c)[0][0][-1]
            runs = eps_runs(o.path_ilabel)
            assert max(n for fr, n in runs if fr < last) == case.depth, (what, runs)
    if case.stopper:
        c, k = case.stopper
        counts = world.counts(case, case.utt[c])
        going_on = GC.simulate(counts, Tl, case.schedules[0], T[:c] + [Tl] + T[c + 1:], case.max_tok, case.arena, case.survivors(False), case.best_row)[0]
        assert T[c] == going_on[k - 1], (case.id, T[c], going_on)
        assert len(world.expected(case, c)[0][1]) == k - 1
    if case.kind == "fan":
        # the hub's hash partition takes a candidate from every token of the frame and the hub's own to its neighbours
        cap = GC.bucket_cap(case.max_tok, **(case.options or {}))
        assert 2 * max(world.counts(case, case.utt[0])[:Tl + 1]) <= cap, (case.id, cap)
    if case.leg == "soft_limit":
        assert max(world.counts(case, case.utt[0])[1:Tl + 1]) > case.max_tok   # the limit binds
    if case.error_T:
        # continued to error_T frames nothing is freed: the arena fills, and the 10-frame neighbour's own tokens fit
        counts = world.counts(case, case.utt[0])
        assert not GC.simulate(counts, case.error_T, case.schedules[0] + [case.error_T], [case.error_T], case.max_tok, case.arena, case.survivors(False))[2]
        o = decode(name, case.ocfg, case.utt[4], frames=10)
        assert o.ok and o.extra["ties"] == 0 and world.counts(case, case.utt[4])[:11].sum() < case.arena
    if case.leg == "big_arena":
        assert case.arena > 1 << 22 and case.flags["degcode"] == 0
    elif case.fusable and case.gopt is None and not case.biglm:
        assert case.arena <= 1 << 22 and case.flags["degcode"] == 1
