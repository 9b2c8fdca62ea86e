"""Cases aimed at the constants GetCutoff's radix selection is cut along (wfst_kernels.hip kth_smallest_t; plain numpy, no GPU), shared
by tests/test_selection_cases.py (CPU: the cases do what they claim under the order-free oracle) and tests/test_gpu_cutoff_selection.py.

kth_smallest_t has three instantiations; each keeps the first threads x kept costs in registers across its passes and reads the rest
in batches, the cold one from an LDS cache first:

  frame_boundary_fused -> kth_smallest_cold   512 x 4 = 2048 costs, then 3 * lds_slots cached ones, then HBM in strides of 4 x 512
  prep_frame<false>                            1024 x 8 = 8192 costs, then HBM in strides of 8 x 1024; bounds only on fused decoders
  prep_frame<true> (biglm)                     the same, never bounded

Every graph is geometry_util.frontier_of(N): utterances of 3 frames, so the frontier of frame 1 is exactly N tokens and the boundary
that closes it selects at n = N.  A multi-frame advance call of a two-launch decoder closes its inner frames in the insert launch (the
cold selection); a call's first frame is prepared by the closure launch (prep_frame), so a decoder fed frame by frame selects there."""
import collections
import os
import re
import zlib

import numpy as np

import geometry_util as U

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "asr-decoder_amd", "csrc")

# ---- the constants, restated (tests/test_selection_cases.py reads their definitions out of the sources and compares) -------------
COLD_THREADS, COLD_KEEP, COLD_BATCH = 512, 4, 4      # kInsertThreads, WFST_COLD_KEEP, kSelBatch under kSc1
WARM_THREADS, WARM_KEEP, WARM_BATCH = 1024, 8, 8     # kBT, kSelKeep, kSelBatch otherwise
CACHE_PER_SLOT = 3                                   # the cold selection's cache: SLmax * 3 costs
LOG2_LDS_SLOTS = 12                                  # wfst_options_default
COLD_REGS, WARM_REGS = COLD_THREADS * COLD_KEEP, WARM_THREADS * WARM_KEEP


def cold_cache(log2_lds_slots=LOG2_LDS_SLOTS):
    return CACHE_PER_SLOT << log2_lds_slots


def source_constants():
    """The same numbers, read out of wfst_kernels.hip and wfst_capi.cc as text: the lines that define them, and the two lines that
    tie each instantiation to its thread count and kept costs."""
    k = open(os.path.join(CSRC, "wfst_kernels.hip")).read()
    c = open(os.path.join(CSRC, "wfst_capi.cc")).read()

    def one(pattern, text=k):
        m = re.findall(pattern, text, flags=re.M)
        assert len(m) == 1, "%r matches %d times" % (pattern, len(m))
        return m[0]

    batch = one(r"^\s*constexpr int kSelBatch = kSc1 \? (\d+) : (\d+);")
    # (the instantiations: cold = <kT, sc1, BoundaryLite, WFST_COLD_KEEP> called with kInsertThreads; warm = <kBT, plain, .., kSelKeep>)
    one(r"kth_smallest_t<kT, true, BoundaryLite, WFST_COLD_KEEP>\(")
    one(r"kth_smallest_t<kBT, false, BoundaryShared, kSelKeep>\(")
    return dict(
        cold_threads=int(one(r"^constexpr int kInsertThreads = (\d+);")),
        cold_keep=int(one(r"^#define WFST_COLD_KEEP (\d+)\b")),
        cold_batch=int(batch[0]),
        warm_threads=int(one(r"^constexpr int kBT = (\d+);")),
        warm_keep=int(one(r"^constexpr int kSelKeep = (\d+);")),
        warm_batch=int(batch[1]),
        cache_per_slot=int(one(r"frame_boundary_fused<kInsertThreads>\(.*reinterpret_cast<uint32_t \*>\(smem\), SLmax \* (\d+)\);")),
        log2_lds_slots=int(one(r"^\s*o->log2_lds_slots = (\d+);", c)),
    )


RESTATED = dict(cold_threads=COLD_THREADS, cold_keep=COLD_KEEP, cold_batch=COLD_BATCH, warm_threads=WARM_THREADS, warm_keep=WARM_KEEP,
                warm_batch=WARM_BATCH, cache_per_slot=CACHE_PER_SLOT, log2_lds_slots=LOG2_LDS_SLOTS)


def gc_stride(max_tok, arena):
    """wfst_capi.cc: frames between two closure launches of a fused best-path decoder (0: none fits, every frame takes three launches).
    A restatement: the cases that name the two-launch or the three-launch path are sized by it, and assert dec.path_flags() on the GPU."""
    reserve = max(2 * max_tok, arena // 8)
    reserve = max(reserve, min(17 * max_tok, arena // 4))
    reserve = min(reserve, arena // 2)
    return min(reserve // max_tok - 1, 16)


def f2o(x):
    """wfst_kernels.hip f2o: float32 -> uint32 of the same order"""
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return np.where(u >> 31, u ^ 0xFFFFFFFF, u ^ 0x80000000).astype(np.uint64)


def range_bits(best, bound):
    """R of kth_smallest_t for a frame whose best token costs `best` and whose tokens were admitted below `bound` (the next_cutoff of
    the frame before): the low bits in which two costs of the frame can differ; 32 where the range is reset (hi <= lo)."""
    lo, hi = int(f2o(best)), int(f2o(bound))
    return 32 if hi <= lo else (lo ^ hi).bit_length()


# ---- legs: the decoder each case runs on ------------------------------------------------------------------------------------------
# bounded: the selection is handed (f2o(best), bound).  flags: what dec.path_flags() must report.
LEGS = {
    "cold": dict(bounded=True, flags=dict(staged=1, two_launch=1)),
    "cold_lds8": dict(bounded=True, opt=dict(log2_lds_slots=8), flags=dict(staged=1, two_launch=1)),
    "three_launch": dict(bounded=True, three=True, flags=dict(staged=1, two_launch=0, gc_stride=1)),
    "lattice": dict(bounded=True, lattice=True, flags=dict(staged=1, two_launch=0)),
    "plain": dict(bounded=False, gopt=dict(fuse_closures=0), flags=dict(staged=0, two_launch=0)),
    "biglm": dict(bounded=False, biglm=True, flags=dict(staged=0, two_launch=0)),
}
T_FRAMES = 3
BIGLM_MAX_TOK = 1 << 17   # a biglm token is a (state, LM state) pair: the frames behind frame 1 hold several per state


def frame_cap(case):
    """No frame of the case holds more tokens than this (frontier_of(N): N; the frame-0 graph has fewer than 256 states)"""
    return 256 if case.kind == "frame0" else case.n


def limits(case):
    """Decoder limits of a case: the per-frame limit just above N (a soft-limit case: below), the arena 1 << 18, or for the three-launch
    leg the power of two that holds the utterance and leaves no room for a collection stride."""
    leg = LEGS[case.leg]
    m = case.max_tok or (BIGLM_MAX_TOK if leg.get("biglm") else frame_cap(case) + 7)
    arena = 1 << 18
    if leg.get("three"):
        arena = 1 << int(T_FRAMES * frame_cap(case) + 1).bit_length()
    lim = dict(max_frames=8, max_tokens_per_frame=m, arena_tokens=arena)
    if leg.get("lattice"):
        lim["lattice_links"] = 1 << 20
    if leg.get("biglm"):
        lim["lm_pairs"] = 1 << 16
    return lim


# ---- graphs -------------------------------------------------------------------------------------------------------------------------
PLATEAU = 600      # tokens of bit-equal cost in the rank-edge graph
CLOSURE = (40, 4)  # the frame-0 graph: paths and depth of the start state's epsilon closure (41 tokens in frame 0)
SEEDS = {'p2049': 6, 'f8189': 57, 'f8191': 19, 'f2048': 6, 'f2049': 10, 'f14335': 6, 'f14336': 6, 'f2815': 8, 'f4865': 12, 'f8192': 11, 'f8193': 7}         # graph name (without a rung's suffix) -> seed, where the default (5) leaves a case short of its condition (tests/test_selection_cases.py)


def start_closure(synth, paths, depth, seed):
    """The start state has an epsilon closure of `paths` paths (frame 0 holds paths + 1 tokens) above a pool of plain states."""
    net = U._Net(synth, seed, 64)
    root = net.state()
    for _ in range(96):
        net.state()
    net.closure(root, paths, depth)
    g, f = net.finish(root)
    f.update(root=root, root_paths=int(f["paths"][root]), root_depth=int(f["depth"][root]))
    return g, f


def build_graph(synth, name):
    """f<N>[@e]: frontier_of(N) (the suffix names a ladder rung: the same graph); p<N>: with the plateau; closure: the frame-0 graph"""
    base = name.split("@")[0]
    seed = SEEDS.get(base, 5)
    if base == "closure":
        return start_closure(synth, CLOSURE[0], CLOSURE[1], seed)
    if base[0] == "p":
        return U.frontier_of(synth, int(base[1:]), plateau=PLATEAU, seed=seed)
    return U.frontier_of(synth, int(base[1:]), seed=seed)


# the pass-count ladder: graph f2049@<e> is decoded on log-likelihoods lowered by 1.3 * 2^e, so the path costs of frame f sit near
# f * 1.3 * 2^e: inside a binade and off the round mantissas in frames 1 and 2 (best cost and bound share their high bits: R falls with e)
LADDER_E = (0, 5, 9, 13, 17, 20)
LADDER_BEAM = 100.0


def offset_of(name):
    return 1.3 * 2.0 ** int(name.split("@")[1]) if "@" in name else 0.0


def utterances(name, n=2):
    """n matrices of 3 frames of N(-1.5, 1) log-likelihoods, lowered by the ladder rung's constant"""
    rng = np.random.default_rng(zlib.crc32(("selection " + name.split("@")[0]).encode()))
    return [(rng.normal(-1.5, 1.0, size=(T_FRAMES, 64)) - offset_of(name)).astype(np.float32) for _ in range(n)]


# ---- cases --------------------------------------------------------------------------------------------------------------------------
# id; leg; graph name; decoder configuration (beam, max_active, min_active, lattice_beam); kind: size / rank_max / rank_min / soft /
# ladder / frame0; n: the token count of frame 1 (frame0: of frame 0); limit: "max_active" / "min_active" (which one is moved
# by one in the sensitivity proof; the soft-limit case: the oracle's max_active, which stands for the per-frame limit); max_tok: a
# per-frame limit below n (the soft-limit case); moves: the directions in which a move of
# the limit by one changes the following frame (the other direction, if any, stays inside a run of equal costs and changes nothing)
Case = collections.namedtuple("Case", "id leg graph cfg kind n limit max_tok moves")
LATTICE_BEAM = dict(biglm=120.0)   # (biglm: see geometry_util.BIGLM)


def _cfg(leg, beam=100.0, max_active=1000000, min_active=0):
    return dict(beam=float(beam), max_active=int(max_active), min_active=int(min_active), lattice_beam=LATTICE_BEAM.get(leg, 8.0))


# biglm: frame 1 holds one token per fan state and one per LM state that reaches the super-final state: frontier_of(N - extra) gives N
BIGLM_GRAPH_N = {8191: 8191 - 2, 8193: 8193 - 2}
# the rank (0-based, by cost) of the plateau's first token in frame 1 of utterance 0 of p2049 (utterance 1, in the decoder's second
# channel, rides along at whatever rank the limit has there)
PLATEAU_RANK0 = 1001

MIN_MAX_ACTIVE = 2   # the least max_active a decoder takes (LatticeFasterDecoderConfig::Check, in the reference as here: max_active > 1)
SIZE_EDGES = [("cold", (COLD_REGS - 1, COLD_REGS, COLD_REGS + 1, COLD_REGS + cold_cache() - 1, COLD_REGS + cold_cache(), COLD_REGS + cold_cache() + 1)),
              ("cold_lds8", (COLD_REGS + cold_cache(8) - 1, COLD_REGS + cold_cache(8), COLD_REGS + cold_cache(8) + 1,
                             COLD_REGS + cold_cache(8) + COLD_BATCH * COLD_THREADS + 1)),
              ("three_launch", (WARM_REGS - 1, WARM_REGS, WARM_REGS + 1, WARM_REGS + WARM_BATCH * WARM_THREADS + 1)),
              ("lattice", (WARM_REGS - 1, WARM_REGS, WARM_REGS + 1, WARM_REGS + WARM_BATCH * WARM_THREADS + 1)),
              ("plain", (WARM_REGS - 1, WARM_REGS + 1)),
              ("biglm", (WARM_REGS - 1, WARM_REGS + 1))]
RANK_N = COLD_REGS + 1
RANK_LEGS = ("cold", "three_launch")
LADDER_LEGS = ("cold", "three_launch", "lattice")
FRAME0_LEGS = ("cold", "three_launch", "lattice", "plain")
FRAME0_MAX_ACTIVE = 20
SOFT_MAX_TOK = 1500


def cases():
    out = []

    def add(id, leg, graph, cfg, kind, n, limit, max_tok=0, moves=(-1, 1)):
        out.append(Case("%s-%s" % (leg, id), leg, graph, cfg, kind, n, limit, max_tok, moves))

    for leg, sizes in SIZE_EDGES:
        for n in sizes:
            gname = "f%d" % (BIGLM_GRAPH_N[n] if leg == "biglm" else n)
            for ma in (n - 1, n // 2, MIN_MAX_ACTIVE):
                add("n%d-max%d" % (n, ma), leg, gname, _cfg(leg, max_active=ma), "size", n, "max_active")
    n, r0 = RANK_N, PLATEAU_RANK0
    for leg in RANK_LEGS:
        # max_active on the plateau's first token, its last, and one past it (ranks in utterance 0; utterance 1 rides along)
        for what, ma, mv in (("first", r0, (-1,)), ("last", r0 + PLATEAU - 1, (1,)), ("past", r0 + PLATEAU, (-1, 1))):
            add("plateau-%s" % what, leg, "p%d" % n, _cfg(leg, max_active=ma), "rank_max", n, "max_active", moves=mv)
        # min_active sets the cutoff (beam 0.5; frame 0, one token below min_active, ends on an adaptive beam of +inf, so frame 1's
        # boundary is frame_boundary_fused's need_min): one below the frame's count, the count itself (the cutoff is +inf), and on the plateau's last token
        add("min-nm1", leg, "p%d" % n, _cfg(leg, beam=0.5, min_active=n - 1), "rank_min", n, "min_active")
        add("min-n", leg, "p%d" % n, _cfg(leg, beam=0.5, min_active=n), "rank_min", n, "min_active", moves=(-1,))   # (n + 1: +inf as well)
        add("min-plateau-last", leg, "p%d" % n, _cfg(leg, beam=0.5, min_active=r0 + PLATEAU - 1), "rank_min", n, "min_active", moves=(1,))
    # the per-frame limit below the frontier: it acts as a max_active (soft_limit decoders), the frames over it are counted
    add("soft%d" % SOFT_MAX_TOK, "cold", "f%d" % n, _cfg("cold"), "soft", n, "max_active", max_tok=SOFT_MAX_TOK)
    for e in LADDER_E:
        for leg in LADDER_LEGS:
            add("ladder-e%d" % e, leg, "f%d@%d" % (n, e), _cfg(leg, beam=LADDER_BEAM, max_active=n // 2), "ladder", n, "max_active")
    for leg in FRAME0_LEGS:
        add("frame0", leg, "closure", _cfg(leg, max_active=FRAME0_MAX_ACTIVE), "frame0", CLOSURE[0] + 1, "max_active")
    return out


def oracle_cfg(case, **moved):
    """The configuration the oracle decodes the case with: the decoder's own, a soft per-frame limit acting as max_active; moved:
    limit name -> what is added to it"""
    cd = dict(case.cfg)
    if case.max_tok:
        cd["max_active"] = min(cd["max_active"], case.max_tok)
    for k, by in moved.items():
        cd[k] += by
    return cd


def cfg_key(cd):
    return "b%g_x%d_n%d_l%g" % (cd["beam"], cd["max_active"], cd["min_active"], cd["lattice_beam"])


# ---- graphs, utterances and oracle results, made once -----------------------------------------------------------------------------
class World(U.World):
    """geometry_util.World over this module's graphs and utterances; a configuration is named by cfg_key(dict)"""

    def __init__(self, synth, oracle, tmp_dir):
        super().__init__(synth, oracle, tmp_dir)
        self._cfgs = {}

    def graph(self, name):
        if name not in self._g:
            g, f = build_graph(self.synth, name)
            p = "%s/%s.bin" % (self.dir, name.replace("@", "_at_"))
            g.write(p)
            self._g[name] = (g, f, p)
        return self._g[name][:2]

    def mats(self, name):
        if name not in self._mats:
            self._mats[name] = utterances(name)
        return self._mats[name]

    def key(self, cd):
        k = cfg_key(cd)
        self._cfgs[k] = dict(cd)
        return k

    def _cfg(self, cfg):
        import pyoracle

        return pyoracle.Config(**self._cfgs[cfg])

    def oracle_biglm_dump(self, name, cfg, ui, frame):
        """(graph states, costs, count) of the tokens of `frame` of the biglm decode: one entry per (state, LM state) pair"""
        import pyoracle

        self.oracle_biglm(name, cfg, ui)   # (loads the LM pair)
        o1, o2 = self._res["olm"]
        return self._cached(("biglm_dump", name, cfg, ui, frame),
                            lambda: pyoracle.biglm_decode(self.oracle, self.handle(name), self._cfg(cfg), o1, o2, self.mats(name)[ui], None, fixed=True,
                                                          dump_frame=frame, dump_cap=BIGLM_MAX_TOK).dump)

    def tie_rule_decode(self, name, cd, ui):
        """The order-free oracle under the decoders' tie rule (deviation 3): the reference of a tie-dense case"""
        def make():
            try:
                self.oracle.set_tie_rule(True)
                return self.oracle.decode(self.handle(name), self._cfg(self.key(cd)), self.mats(name)[ui], None)
            finally:
                self.oracle.set_tie_rule(False)
        return self._cached(("tie_rule", name, self.key(cd), ui), make)


def pair_multiset(states, costs):
    """The tokens of a frame as a sorted list of (graph state, cost bits): what identifies a biglm frontier, whose states repeat"""
    return sorted(zip(np.asarray(states).tolist(), np.asarray(costs, np.float32).view(np.int32).tolist()))


def frame_ranges(trace, cd):
    """{frame: R} of the max_active selection of a traced decode on a bounded decoder: the expanded frames that hold more than
    max_active tokens (frame 0 has no bound: its range is reset, 32)"""
    return {f: range_bits(trace.frame_best[f], trace.frame_next_cutoff[f - 1]) if f else 32
            for f in range(len(trace.frame_cutoff)) if trace.frame_ntoks[f] > cd["max_active"]}
