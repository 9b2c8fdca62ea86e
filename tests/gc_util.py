"""Graphs and cases aimed at the constants the token collection of best-path decoders is cut along (plain numpy, no GPU):
gc_pass in wfst_kernels.hip -- the need table of kGcNeedSlots = 2048 wanted states whose claims stop at 3/4 (1536; the check is
racy, so 1024 threads can overshoot it and fill the table), the re-sweeps of a frame over epsilon chains, the mover's rounds of
kBT * kCU = 8192 tokens, the next mark ("halfway", clamped for two-launch decoders) -- and the host's reserve and stride rule in
wfst_capi.cc, restated here (reserve_and_stride) from the rule in its comments.

Two graph families on synth.graph_from_arc_lists, deterministic from their seed:

* fan(E, depth, pend): a hub (state 0, final, an emitting self-loop) with one emitting arc to each of E states u_i; behind every
  u_i an epsilon chain of `depth` states v_i1 .. v_i,depth; every u and v has one emitting arc back to the hub (chains of two hops
  and more: a cheap one from the chain's end, dear ones before it and a dear self-loop, so that best paths run through whole chains); `pend` pendant
  states (hub -> p -> hub, emitting) set an exact frame size.  With a beam that prunes nothing every frame >= 1 holds
  E * (1 + depth) + pend + 2 tokens (the hub and the super-final state are the two).  The v states have no emitting in-arc:
  every token on one is won by an epsilon arc and wants a source state of its own (so does the super-final state's: the hub).
  Old frames keep the chain of the hub's token only: a collection frees nearly everything.
* comb(N, R): the start state enters N rings by emitting arcs; ring k alternates a_j --emit, label 1 + k % 40--> b_j+1 --eps-->
  a_j+1 over R pairs; every a is final.  Nothing merges: every frame >= 1 holds 2 N + 1 tokens, all of every old frame but the
  super-final state's stay reachable (a collection frees next to nothing), and every old frame holds N epsilon-won tokens with
  N distinct wanted states.

simulate() restates WHEN the host looks at the mark (the closure launch at the start of every advance call and behind every
gc_stride-th step of a call) and what gc_pass makes of the mark afterwards: tests/test_gc_graphs.py proves from the oracle's
per-frame token counts how many of those checks find the arena beyond its mark, tests/test_gpu_gc_edges.py asserts it on the
device."""
import zlib

import numpy as np

import geometry_util as U

NEED_SLOTS = 2048                     # wfst_kernels.hip kGcNeedSlots
NEED_STOP = (NEED_SLOTS * 3) // 4     # claims stop at n_need >= 1536 ...
NEED_OVERSHOOT = NEED_STOP - 1 + 1024  # ... but 1024 threads can pass that check together: up to 1535 + 1024 claims
MOVER_CHUNK = 1024 * 8                # kBT * kCU: tokens the mover renumbers and moves per round
N_COLS = 41                           # labels 1 .. 40, column = label (no tid2pdf)
STRIDE_MAX = 16


# ---- the host's reserve and stride (wfst_capi.cc, "the token collection's reserve") -------------------------------------------------
def reserve_and_stride(max_tok, arena, best_row=True):
    """(reserve, two_launch, stride): the arena is collected when less than `reserve` of it is left -- an eighth of the arena, two
    frames at the per-frame limit at least; a decoder that may run two launches per frame (best_row: fused, best-path, no biglm)
    takes up to a quarter where that buys a longer stride (17 frames at the limit cover the longest stride, 16); never more than
    half.  stride = reserve / max_tok - 1 frames between two looks at the mark: below 1 the decoder keeps three launches per frame
    (path_flags: two_launch 0, gc_stride 1), above 16 it is 16."""
    M, A = max(1, int(max_tok)), int(arena)
    reserve = max(2 * M, A // 8)
    if best_row:
        reserve = max(reserve, min(17 * M, A // 4))
    if reserve >= A // 2:
        reserve = A // 2
    stride = reserve // M - 1 if best_row else 0
    two = int(stride >= 1)
    return reserve, two, (min(stride, STRIDE_MAX) if two else 0)


def bucket_cap(max_tok, log2_partitions=5, log2_lds_slots=12):
    """Candidates one hash partition of a frame's insert takes (wfst_capi.cc: `bucket_cap`, with the library's default launch
    shape of a best-path decoder).  Every token of a fan frame sends a candidate to the hub, and the hub sends one to every other
    state: the hub's partition takes up to 2 * n_tok of them.  Where that is beyond the default shape's bucket, the case's decoders
    run with two partitions (Case.options): a launch-shape knob of the insert, which the collection never sees."""
    lp, M = int(log2_partitions), int(max_tok)
    while lp > 0 and (1 << log2_lds_slots) << (lp - 1) >= 4 * M:
        lp -= 1
    return max(2048, 8 * M // (1 << lp))


def flags_of(max_tok, arena, best_row=True):
    _, two, stride = reserve_and_stride(max_tok, arena, best_row)
    return dict(two_launch=two, gc_stride=max(1, stride))


def simulate(counts, T, schedule, all_T, max_tok, arena, survivors, best_row=True):
    """The collections of one channel that decodes frames 1 .. T of an utterance whose frame f holds counts[f] tokens, in a decoder
    whose channels (lengths all_T) are advanced together to min(r, T_c) frames for r in `schedule`.
    survivors(f, n): what a collection keeps of an OLD frame f of n tokens (the frontier's frame stays whole).
    Returns (frames at which a collection ran, the arena's peak fill, whether every frame fitted the arena)."""
    reserve, two, stride = reserve_and_stride(max_tok, arena, best_row)
    gs = max(1, stride)
    base = arena - reserve
    sz = [int(counts[0])]
    mark, ran, peak, fits = base, [], int(counts[0]), True
    prev = 0

    def check(nd):
        nonlocal mark
        if sum(sz) <= mark:
            return
        for f in range(nd):
            sz[f] = int(survivors(f, sz[f]))
        new_end = sum(sz)
        m = max(base, new_end + (arena - new_end) // 2)
        if two:
            m = max(base, min(m, arena - (gs + 1) * max_tok))
        mark = m
        ran.append(nd)

    for r in schedule:
        gsteps = max(min(r, t) - min(prev, t) for t in all_T)
        a, b = min(prev, T), min(r, T)
        prev = r
        if gsteps <= 0:
            continue
        if 0 < a < b:
            check(a)              # the closure launch at the start of the call
        for s in range(gsteps):
            if a + s >= b:
                break
            sz.append(int(counts[a + s + 1]))
            peak = max(peak, sum(sz))
            fits = fits and sum(sz) <= arena
            classic = (not two) or s % gs == gs - 1
            if classic and s + 1 < gsteps and a + s + 1 < b:
                check(a + s + 1)
    return ran, peak, fits


# ---- the graphs ------------------------------------------------------------------------------------------------------------------
def _word(k):
    return 1 + k % (U.N_WORDS - 1)


def fan(synth, E, depth, pend=0, n_words=0, seed=11):
    """n_words: so many distinct words on the hub's arcs (biglm: a token is a (state, LM state) pair, and few words keep the LM states few)"""
    rng = np.random.default_rng(seed + 1000 * depth + E)
    lab = lambda: int(rng.integers(1, N_COLS))
    deep = depth > 1   # chains of two hops and more: staying on the hub and leaving a chain early cost 3 to 4 more, the way back from a
    # chain's end a tenth -- the best path runs through whole chains (all within the beam: the frame sizes do not move)
    arcs = {0: [(lab(), 0, float(rng.uniform(0.05, 0.8)) + (4.0 if deep else 0.0), 0)]}
    n = 1
    for i in range(E):
        u = n
        arcs[0].append((lab(), (1 + i % n_words if n_words else _word(i)) if i % 3 == 0 else 0, float(rng.uniform(0.0, 3.0)), u))
        for j in range(depth + 1):
            s = u + j
            w = float(rng.uniform(0.0, 3.0))
            arcs[s] = [(lab(), 0, (0.1 * w if j == depth else 3.0 + w) if deep else w, 0)]
            if j < depth:
                arcs[s].append((0, 0, float(rng.uniform(0.01, 0.3)), s + 1))
        n += depth + 1
    for _ in range(pend):
        arcs[0].append((lab(), 0, float(rng.uniform(0.0, 3.0)), n))
        arcs[n] = [(lab(), 0, float(rng.uniform(0.0, 3.0)), 0)]
        n += 1
    g = synth.graph_from_arc_lists(n, 0, arcs, {0: float(rng.uniform(0.0, 2.0))})
    return g, gc_facts(g)


def comb(synth, N, R=3, seed=12):
    rng = np.random.default_rng(seed + N)
    arcs, finals = {0: []}, {}
    for k in range(N):
        a0 = 1 + 2 * R * k           # a_j = a0 + 2 j, b_j = a_j + 1
        lab = 1 + k % 40
        arcs[0].append((lab, 0, float(rng.uniform(0.0, 0.3)), a0 + 1))
        for j in range(R):
            a, b = a0 + 2 * j, a0 + 2 * j + 1
            arcs[b] = [(0, 0, float(rng.uniform(0.01, 0.3)), a)]
            arcs[a] = [(lab, _word(k + j) if j == 0 else 0, float(rng.uniform(0.0, 0.3)), a0 + 2 * ((j + 1) % R) + 1)]
            finals[a] = float(rng.uniform(0.0, 2.0))
    g = synth.graph_from_arc_lists(1 + 2 * R * N, 0, arcs, finals)
    return g, gc_facts(g)


def gc_facts(g):
    """U.shape_facts plus, from the arrays: eps_won -- states no emitting arc enters (a token on one is always won by an epsilon
    arc) --, their number W, and the number of DISTINCT source states of the epsilon arcs into them (what one sweep's need table
    is asked to hold when all of them are marked); single_eps_in: but for the super-final state each is entered by ONE epsilon arc."""
    f = U.shape_facts(g)
    off = g.row_offsets()
    src = np.repeat(np.arange(g.n_states), np.diff(off))
    to, il = g.arcs["to"], g.arcs["ilabel"]
    emit_in = np.zeros(g.n_states, bool)
    emit_in[to[il != 0]] = True
    eps_in = np.zeros(g.n_states, bool)
    eps_in[to[il == 0]] = True
    won = eps_in & ~emit_in
    won[g.start] = False
    into = (il == 0) & won[to]
    f.update(eps_won=won, W=int(won.sum()), sources=int(len(set(src[into].tolist()))), chain_depth=int(f["depth"].max()),
             single_eps_in=bool((np.delete(np.bincount(to[il == 0], minlength=g.n_states) * won, g.final_state) <= 1).all()))
    return f


def fan_tokens(E, depth, pend=0):
    return E * (1 + depth) + pend + 2


def comb_tokens(N):
    return 2 * N + 1


GRAPHS = {}


def _fan_name(E, depth, pend=0, n_words=0):
    name = "fan%dx%d" % (E, depth) + ("p%d" % pend if pend else "") + ("w%d" % n_words if n_words else "")
    GRAPHS[name] = lambda sy: fan(sy, E, depth, pend, n_words)
    return name


def _comb_name(N):
    name = "comb%d" % N
    GRAPHS[name] = lambda sy: comb(sy, N)
    return name


# ---- configurations --------------------------------------------------------------------------------------------------------------
CFGS = dict(beam30=dict(beam=30.0, max_active=1000000, min_active=0, lattice_beam=8.0),
            beam60=dict(beam=60.0, max_active=1000000, min_active=0, lattice_beam=8.0),
            # (biglm: the reference's final pruning ranges over non-final tokens too -- geometry_util.BIGLM)
            biglm30=dict(beam=30.0, max_active=1000000, min_active=0, lattice_beam=40.0),
            # the soft_limit leg's ORACLE: the per-frame limit of 2048 as a max_active
            soft2048=dict(beam=30.0, max_active=2048, min_active=0, lattice_beam=8.0))


# ---- the cases -------------------------------------------------------------------------------------------------------------------
class Case:
    """One decoder of a leg: graph, limits, channels (utterance index and length each), the advance schedule(s)."""

    def __init__(self, leg, graph, kind, n_tok, T, max_tok, arena, schedules, cfg="beam30", gopt=None, biglm=False, best_row=True,
                 flags=None, utt=None, ocfg=None, min_collections=1, aim="", error_T=None, lm_pairs=0, depth=1, stopper=None, fusable=True):
        self.leg, self.graph, self.kind, self.n_tok, self.T = leg, graph, kind, n_tok, list(T)
        self.max_tok, self.arena, self.schedules = max_tok, arena, schedules
        self.cfg, self.ocfg, self.gopt, self.biglm, self.best_row = cfg, ocfg or cfg, gopt, biglm, best_row
        self.utt = list(utt) if utt is not None else [c % 2 for c in range(len(T))]
        self.flags = dict(flags_of(max_tok, arena, best_row), **(flags or {}))
        self.min_collections, self.aim, self.error_T, self.lm_pairs, self.depth = min_collections, aim, error_T, lm_pairs, depth
        self.id = "%s-%s-a%d" % (leg, graph, arena)
        self.options = dict(log2_partitions=1) if kind == "fan" and 2 * n_tok > bucket_cap(max_tok) else None
        self.fusable = fusable   # what the loader must find (shape facts); gopt fuse_closures=0 leaves a fusable graph unfused
        self.stopper = stopper
        if stopper and self.T[stopper[0]] is None:
            self._place_stopper()

    def _place_stopper(self):
        """stopper = (channel, k): that channel stops on the frame at which a channel that goes on runs its k-th collection -- its
        last, if it runs fewer -- (a channel at its target is not collected: it reports k - 1).  Its length, where the table gives
        None, from the nominal frame size and the first schedule; tests/test_gc_graphs.py proves it again from the oracle's counts."""
        c, k = self.stopper
        lengths = [t for t in self.T if t is not None]
        Tl = max(lengths)
        ran = simulate([2 if self.kind == "fan" else 1] + [self.n_tok] * Tl, Tl, self.schedules[0], lengths, self.max_tok, self.arena,
                       self.survivors(False), self.best_row)[0]
        k = min(k, len(ran))
        self.stopper, self.T[c] = (c, k), ran[k - 1]

    def limits(self):
        d = dict(max_frames=max(self.T + [self.error_T or 0]) + 4, max_tokens_per_frame=self.max_tok, arena_tokens=self.arena)
        if self.lm_pairs:
            d["lm_pairs"] = self.lm_pairs
        return d

    def survivors(self, upper):
        """(f, n) -> what a collection keeps of an old frame: fan -- the chain of the hub's token, one token at least, the hub's, its
        predecessor u and that one's chain at most; comb -- everything but the super-final state's token (frame 0: the start token)."""
        if self.kind == "fan":
            k = 8 if self.biglm else 1   # (biglm: every token on a wanted state is kept, one per LM state -- four at most here -- and each has a chain)
            return (lambda f, n: min(n, k * (self.depth + 2))) if upper else (lambda f, n: min(n, 1))
        return (lambda f, n: n) if upper else (lambda f, n: n if f == 0 else min(n, self.n_tok - 1))


def _sched(T, chunk):
    return list(range(chunk, T, chunk)) + [T] if chunk else [T]


def _fan_case(leg, E, depth, T=40, frames=6, chunk=8, pend=0, max_tok=16384, stop_at=2, stop_T=None, n_words=0, n_tok=None, **kw):
    """A fan decoder of four channels: two of T frames (different matrices), one of 3 frames (never collects), and one that stops
    on the frame at which the long ones run their `stop_at`-th collection (a channel at its target is not collected)."""
    n = n_tok or fan_tokens(E, depth, pend)
    arena = kw.pop("arena", None) or frames * n + 64
    return Case(leg, _fan_name(E, depth, pend, n_words), "fan", n, [T, T, 3, stop_T], max_tok, arena, [_sched(T, chunk)], depth=depth, stopper=(3, stop_at), **kw)


def cases():
    out = []
    # need_W: the frontier's frame asks the need table for W + 1 distinct states (the v states' sources and the hub)
    for E in (1400, 1535, 1536, 1537, 2047, 2048, 2049, 2600, 5000):
        out.append(_fan_case("need_W", E, 1, flags=dict(staged=1, degcode=1),
                             aim="claims stop at 3/4 of the table; a full table; W beyond the overshoot; three or more sweeps"))
    for E in (1537, 5000):
        out.append(_fan_case("need_plain", E, 1, gopt=dict(fuse_closures=0), best_row=False, flags=dict(staged=0, degcode=0),
                             aim="the plain closure pass: best_row 0, best_next remapped, no degree codes"))
    # (two words on the hub's arcs: from frame 3 on every frame holds 7176 / 12138 (state, LM state) pairs on its 3078 / 5204 states)
    for E, n in ((1537, 7176), (2600, 12138)):
        out.append(_fan_case("need_biglm", E, 1, n_words=2, n_tok=n, stop_T=8, biglm=True, best_row=False, cfg="biglm30", flags=dict(staged=0, degcode=0), lm_pairs=1 << 18,
                             aim="gc_pass<true>: every token on a wanted state kept, nothing written back"))
    out.append(_fan_case("chain", 400, 8, flags=dict(staged=1, degcode=1), aim="an old frame re-swept once per hop of a surviving chain of 8 epsilon hops; the frontier's frame overflows the table (W 3200)"))
    out.append(_fan_case("chain", 250, 12, best_row=False, fusable=False, flags=dict(staged=0, degcode=0), aim="the same over 12 hops on a graph the loader leaves unfused (W 3000)"))
    # comb_keep / comb_full: one decoder; six channels with different matrices and a 10-frame neighbour
    N = 1600
    out.append(Case("comb_keep", _comb_name(N), "comb", comb_tokens(N), [38, 38, 38, 38, 3, None], 4096, 1 << 17, [_sched(38, 4)], cfg="beam60",
                    utt=[0, 1, 2, 3, 4, 5], stopper=(5, 2), flags=dict(staged=1, degcode=1), min_collections=2, error_T=60,
                    aim="every old frame overflows the table; written-back same-frame backpointers with degree codes; the halfway mark and its clamp"))
    # chunk_edge: frames of exactly one mover round, one less, one more, two rounds and one more; three rounds all alive
    for n in (8191, 8192, 8193):
        out.append(_fan_case("chunk_edge", 4000, 1, pend=n - fan_tokens(4000, 1), flags=dict(staged=1, degcode=1), aim="a frame of %d tokens" % n))
    out.append(_fan_case("chunk_edge", 8000, 1, pend=16385 - fan_tokens(8000, 1), max_tok=32768, flags=dict(staged=1, degcode=1), aim="a frame of 16385 tokens"))
    N = 4097
    out.append(Case("chunk_edge", _comb_name(N), "comb", comb_tokens(N), [60, 60, 3, None], 16384, 1 << 19, [_sched(60, 10)], cfg="beam60",
                    utt=[0, 1, 2, 3], stopper=(3, 2), flags=dict(staged=1, degcode=1), min_collections=2, aim="frames of 8195 tokens all alive: survivors across a round's edge"))
    # stride_s: three launches, then strides 1, 2, 7 and 16; one call (head and rest graphs) and chunks of 1, 7, stride - 1, stride, stride + 1
    for arena in (3072, 4096, 12288, 32768, 1 << 17):
        s = max(1, reserve_and_stride(1024, arena)[2])
        chunks = [0, 1, 7] + [k for k in (s - 1, s, s + 1) if k > 1 and k != 7]
        T = 130   # (a call of 128 frames and more is split in head and rest graphs; one long channel: the oracle is asked behind every collection)
        out.append(Case("stride_s", _fan_name(500, 1), "fan", fan_tokens(500, 1), [T, 3, None], 1024, arena, [_sched(T, k) for k in chunks], utt=[0, 1, 1], stopper=(2, 2),
                        flags=dict(staged=1, degcode=1), aim="the check at call start and on every stride-th step; no arena error under the limit"))
    # soft_limit: frames of 3002 tokens under a limit of 2048 (the oracle: max_active 2048)
    out.append(_fan_case("soft_limit", 1500, 1, frames=8, max_tok=2048, stop_T=14, ocfg="soft2048", flags=dict(staged=1, degcode=1, soft_limit=1),
                         aim="collections while the limit degrades frames"))
    # big_arena: more than 2^22 tokens leave no room for degree codes
    n = fan_tokens(15000, 1)
    out.append(Case("big_arena", _fan_name(15000, 1), "fan", n, [160, 3], 32768, (1 << 22) + 4096, [[144, 160]], utt=[0, 1],
                    flags=dict(staged=1, degcode=0), aim="no degree-code bits in fused tokens; index mask 0x7FFFFFFF"))
    return out


CASES = cases()
T_OF = {}
N_UTT = {}
for _c in CASES:
    T_OF[_c.graph] = max(T_OF.get(_c.graph, 0), max(_c.T), _c.error_T or 0)
    N_UTT[_c.graph] = max(N_UTT.get(_c.graph, 0), max(_c.utt) + 1)


def utterances(name):
    """N(-1.5, 0.3) log-likelihoods over 41 columns, as long as the longest leg on graph `name` needs; legs decode prefixes."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    return [rng.normal(-1.5, 0.3, size=(T_OF[name], N_COLS)).astype(np.float32) for _ in range(N_UTT[name])]


def by_state_and_cost(st, co):
    """A frame's tokens sorted by (graph state, cost bits): one token per state, or (biglm) one per (state, LM state) pair -- the multiset"""
    st, co = np.asarray(st), np.asarray(co, np.float32)
    o = np.lexsort((co.view(np.int32), st))
    return st[o], co[o]


class World(U.World):
    """geometry_util.World over this module's graphs, utterances and configurations."""

    def graph(self, name):
        if name not in self._g:
            g, f = GRAPHS[name](self.synth)
            p = "%s/%s.bin" % (self.dir, name)
            g.write(p)
            self._g[name] = (g, f, p)
        return self._g[name][:2]

    def mats(self, name):
        if name not in self._mats:
            self._mats[name] = utterances(name)
        return self._mats[name]

    def _cfg(self, cfg):
        import pyoracle

        return pyoracle.Config(**CFGS[cfg])

    def counts(self, case, ui):
        """tokens per frame of utterance ui under the case's oracle configuration"""
        t = self.oracle_biglm_trace(case.graph, case.ocfg, ui) if case.biglm else self.oracle_trace(case.graph, case.ocfg, ui)
        assert t.ok
        return t.frame_ntoks

    def frontier(self, case, ui, frame):
        """The oracle's tokens of `frame`, sorted by (state, cost bits), those at or above the frame's final cutoff dropped (the relation of
        tests/test_gpu_parity.py::test_per_frame_best_cost_and_token_subset: the device never keeps them)."""
        st, co, n = self.biglm_dump(case, ui, frame) if case.biglm else self.oracle_dump(case.graph, case.ocfg, ui, frame)
        assert n == len(st)
        if frame >= 1:
            tr = self.oracle_biglm_trace(case.graph, case.ocfg, ui) if case.biglm else self.oracle_trace(case.graph, case.ocfg, ui)
            keep = co < tr.frame_next_cutoff[frame - 1]
            st, co = st[keep], co[keep]
        return by_state_and_cost(st, co)

    def biglm_dump(self, case, ui, frame):
        """(graph states, costs, count) of the tokens of `frame` of the biglm decode of that prefix: one entry per (state, LM state) pair"""
        import pyoracle

        self.oracle_biglm(case.graph, case.ocfg, ui)   # (loads the LM pair)
        o1, o2 = self._res["olm"]
        x = self.mats(case.graph)[ui][:max(frame, 1)]
        return self._cached(("biglm_dump", case.graph, case.ocfg, ui, frame),
                            lambda: pyoracle.biglm_decode(self.oracle, self.handle(case.graph), self._cfg(case.ocfg), o1, o2, x, None, fixed=True,
                                                          dump_frame=frame, dump_cap=1 << 16).dump)

    def expected(self, case, c):
        """What the device must report for channel c: the collections a simulation on the oracle's frame counts gives per schedule,
        with the fewest and the most survivors a collection can leave: (lower, upper, fits with the most)."""
        counts = self.counts(case, case.utt[c])
        out = []
        for sched in case.schedules:
            lo = simulate(counts, case.T[c], sched, case.T, case.max_tok, case.arena, case.survivors(False), case.best_row)
            hi = simulate(counts, case.T[c], sched, case.T, case.max_tok, case.arena, case.survivors(True), case.best_row)
            out.append((lo[0], hi[0], hi[2]))
        return out
