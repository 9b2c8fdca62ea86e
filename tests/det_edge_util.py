"""Raw lattices CONSTRUCTED for the branches of the one-wave-per-lattice determinizer (asr-decoder_amd/csrc/wfst_determinize_wave.h),
one named case per branch (plain numpy, no GPU), the constants and hashes of that header restated, and the writer of the file format
tools/det_bench.hip reads.

Raw-lattice convention (pyoracle.RawLattice): il = transition-id, ol = word; the determinizer inverts them.  An "epsilon arc" is a
word-less arc (ol == 0): the arcs an epsilon closure follows; its transition-id (if not 0) extends the element's string.  State 0 is
the start; every lattice ends in arc-less final states; every other state has an arc (the reference's LatticeCheckFormat).  Costs
are small multiples of 2^-4 (graph cost; the acoustic cost is 0 or 1/4), so every sum is exact and every tie is exact -- the two
"delta" cases alone use 2^-11 and 2^-9.

A case: name, lattice, `want` (counter name -> ("==", v) | (">=", v): what the counted build of the harness must report for the
lattice -- the branch it was built for MOVES, the branch it must keep away from stays 0), `facts` ((what, actual, claimed) triples
about the construction, computed here with the helpers below and asserted by tests/test_det_edge_lattices.py), `args` (options of
tools/det_bench for this file) and `refuse` (the error code host and device must both report, or None).

The wave's closure under test is, as a rule, that of state R = 1 behind one word arc 0 --word 1--> R: the start state's own closure
is {0}, and R's closure goes through everything a closure goes through (the start's is never normalized)."""
import numpy as np

import pyoracle

# ---- the header's constants and hashes, restated (tests/test_det_edge_lattices.py holds them to the sources) -----------------------
K_CUR = 1024        # kDwCur: closure elements in LDS
K_QUEUE = 1024      # kDwQueue
K_MAP = 2048        # kDwMap
K_ARCS = 4          # kDwArcs
K_WIN = 64 // K_ARCS  # kDwWin
K_LABS = 128        # kDwLabs
MAP_SHIFT = 11      # map word: state << 11 | index + 1
SORT_SHIFT = 10     # sort key: state << 10 | index
MAX_STATES = 1 << 21  # n_states >= this: the wave falls back on entry
TRIE_FIRST = 4096   # the trie's first table ...
TRIE_PER_STATE = 16  # ... doubled while < 16 * n_states
CLAIM = 256         # claim[s & 255]
DELTA = 1.0 / 1024
INF = float("inf")
_M = 0xFFFFFFFF


def mapslot(state):
    """detw_mapslot"""
    return ((state * 2654435761) & _M) >> (32 - MAP_SHIFT)


def hash2(a, b):
    """det_hash2"""
    h = (a * 2654435761) & _M
    h ^= (((b + 0x9E3779B9) & _M) * 0x85EBCA6B) & _M
    h ^= h >> 15
    return (h * 0x2C1B3C6D) & _M


def det_key(parent, label):
    return (parent & _M) | ((label & _M) << 32)


def first_table(n_states, full=1 << 20):
    """slots of the trie's table at the first attempt (determinize_kernel / detw_run_block)"""
    h = TRIE_FIRST
    while h < TRIE_PER_STATE * n_states and h < full:
        h <<= 1
    return min(h, full)


def map_probe_end(occupied, state):
    """the slot detw_map_find's probe for `state` (not in the index) ends at, `occupied` being the slots in use"""
    h = mapslot(state)
    while h in occupied:
        h = (h + 1) & (K_MAP - 1)
    return h


def map_insert_all(states):
    occ = set()
    for s in states:
        occ.add(map_probe_end(occ, s))
    return occ


# ---- builder ---------------------------------------------------------------------------------------------------------------------------
class Lat:
    def __init__(self):
        self.n = 0
        self.final = set()
        self.arcs = []   # (src, dst, tid, word, graph, acoustic)

    def state(self, k=None):
        """a new state's id; state(k): the ids of k new states"""
        s = self.n
        self.n += 1 if k is None else k
        return s if k is None else list(range(s, s + k))

    def eps(self, s, d, tid=0, g=0.0, ac=0.0):
        self.arcs.append((s, d, tid, 0, g, ac))

    def word(self, s, d, w, tid=0, g=0.0, ac=0.0):
        assert w > 0
        self.arcs.append((s, d, tid, w, g, ac))

    def raw(self):
        a = self.arcs
        fin = np.zeros(self.n, np.int32)
        fin[sorted(self.final)] = 1
        col = lambda i, t: np.asarray([x[i] for x in a], t)
        return pyoracle.RawLattice(True, self.n, 0, fin, col(0, np.int32), col(1, np.int32), col(2, np.int32), col(3, np.int32),
                                   col(4, np.float32), col(5, np.float32))


def as_dict(L):
    """what shard.lattice_to_bytes takes"""
    return dict(n_states=L.n_states, st_final=L.st_final, a_src=L.a_src, a_dst=L.a_dst, a_ilabel=L.a_il, a_olabel=L.a_ol,
                a_graph=L.a_graph, a_acoustic=L.a_ac)


def write_bin(path, L):
    """tools/det_bench.hip's file: int32 S, A; int32 is_final[S]; A x {int32 src, dst, il, ol; float graph, acoustic}"""
    with open(path, "wb") as f:
        np.asarray([L.n_states, len(L.a_src)], np.int32).tofile(f)
        np.asarray(L.st_final, np.int32).tofile(f)
        rec = np.zeros(len(L.a_src), dtype=[("src", "<i4"), ("dst", "<i4"), ("il", "<i4"), ("ol", "<i4"), ("g", "<f4"), ("ac", "<f4")])
        rec["src"], rec["dst"], rec["il"], rec["ol"], rec["g"], rec["ac"] = L.a_src, L.a_dst, L.a_il, L.a_ol, L.a_graph, L.a_ac
        rec.tofile(f)


# ---- facts -----------------------------------------------------------------------------------------------------------------------------
def _eps_rows(L):
    live = (L.a_ol == 0) & ~(np.isinf(L.a_graph) & np.isinf(L.a_ac))
    rows = {}
    for s, d in zip(L.a_src[live].tolist(), L.a_dst[live].tolist()):
        rows.setdefault(s, []).append(d)
    return rows


def closure(L, states):
    """BFS: the epsilon closure of a set of states (arcs of infinite cost are not followed)"""
    rows = _eps_rows(L)
    seen, todo = set(states), list(states)
    while todo:
        nxt = []
        for s in todo:
            for d in rows.get(s, ()):
                if d not in seen:
                    seen.add(d)
                    nxt.append(d)
        todo = nxt
    return seen


def minimal(L, states):
    """the states of a set that have a word arc of finite cost or are final (IsIsymbolOrFinal)"""
    live = (L.a_ol != 0) & ~(np.isinf(L.a_graph) & np.isinf(L.a_ac))
    has = set(L.a_src[live].tolist())
    return {s for s in states if s in has or L.st_final[s]}


def n_eps(L, s):
    """epsilon arcs in state s's row (of any cost: what the row's count of leading epsilons says)"""
    return int(np.sum((L.a_src == s) & (L.a_ol == 0)))


def n_word_arcs(L, states):
    return int(np.sum(np.isin(L.a_src, sorted(states)) & (L.a_ol != 0)))


def well_formed(L):
    out = np.bincount(L.a_src, minlength=L.n_states)
    return bool(np.all((out > 0) ^ (L.st_final == 1)) and L.a_dst.max() < L.n_states)


# ---- pieces ------------------------------------------------------------------------------------------------------------------------------
def _start(B):
    """0 --word 1--> R; returns R"""
    s0, R = B.state(), B.state()
    B.word(s0, R, 1)
    return R


def _end(B, states, F=None, word0=1000):
    """a word arc of its own (word = word0 + state) from every state of `states` to the final state"""
    if F is None:
        F = B.state()
        B.final.add(F)
    for s in states:
        B.word(s, F, word0 + s)
    return F


def _tree(B, root, n, cost=lambda i: (i % 5) / 16.0):
    """a fan of fans: n states (root included), state i's children 4 i + 1 .. 4 i + 4 -- no entry has more than kDwArcs arcs"""
    ids = [root] + B.state(n - 1)
    for i in range(1, n):
        B.eps(ids[(i - 1) // 4], ids[i], 0, cost(i))
    return ids


class Case:
    def __init__(self, name, B, want, facts, args=(), refuse=None):
        self.name, self.lat, self.want, self.facts, self.args, self.refuse = name, B.raw() if isinstance(B, Lat) else B, want, facts, list(args), refuse


NZ, Z = (">=", 1), ("==", 0)
ON_WAVE = dict(fallback=Z)


def _fan_case(k):
    B = Lat()
    R = _start(B)
    leaves = B.state(k)
    for i, s in enumerate(leaves):
        B.eps(R, s, 3 + i, (i % 3) / 16.0)
    _end(B, leaves)
    L = B.raw()
    rounds = (k + 63) // 64 if k > K_ARCS else 0
    want = dict(big_head=("==", 1 if k > K_ARCS else 0), big_round=("==", rounds), entry_arcs_full=NZ if k == K_ARCS else Z,
                entry_priced=NZ if k <= K_ARCS else Z, **ON_WAVE)
    return Case("eps_arcs_%d" % k, L, want, [("epsilon arcs of R", n_eps(L, R), k), ("closure of R", len(closure(L, [R])), k + 1)])


def _big_not_at_head():
    B = Lat()
    R = _start(B)
    a, b = B.state(), B.state()
    B.eps(R, a, 3, 1 / 16.0)
    B.eps(R, b, 4, 0.0)
    la = B.state()
    B.eps(a, la, 5, 0.25)
    lb = B.state(6)
    for i, s in enumerate(lb):
        B.eps(b, s, 6 + i, i / 16.0)
    _end(B, [la] + lb)
    L = B.raw()
    return Case("big_entry_behind_the_head", L, dict(win_cut=NZ, big_head=("==", 1), big_round=("==", 1), **ON_WAVE),
                [("epsilon arcs of a", n_eps(L, a), 1), ("epsilon arcs of b", n_eps(L, b), 6), ("closure", len(closure(L, [R])), 10)])


def _queue_of(n):
    """two hops behind R, n states are pushed by one window: the next window finds n live entries"""
    B = Lat()
    R = _start(B)
    p, q = B.state(), B.state()
    B.eps(R, p, 3)
    B.eps(R, q, 4, 1 / 16.0)
    mids = B.state(5)
    for i in range(4):
        B.eps(p, mids[i], 5 + i, i / 16.0)
    B.eps(q, mids[4], 9)
    per = {15: [4, 4, 4, 3, 0], 16: [4, 4, 4, 4, 0], 17: [4, 4, 4, 4, 1]}[n]
    leaves = []
    for m, k in zip(mids, per):
        for j in range(k):
            s = B.state()
            B.eps(m, s, 10 + j, j / 16.0)
            leaves.append(s)
    _end(B, leaves + ([mids[4]] if per[4] == 0 else []))
    L = B.raw()
    want = dict(win_peak=("==", min(n, K_WIN)), win_full=NZ if n >= K_WIN else Z, win_over=NZ if n > K_WIN else Z, big_head=Z, **ON_WAVE)
    return Case("queue_of_%d" % n, L, want, [("states pushed by the window of the five", len(leaves), n),
                                              ("most epsilon arcs of a state", max(n_eps(L, s) for s in range(L.n_states)), 4)])


def _zero_arcs():
    B = Lat()
    R = _start(B)
    a, b, c, d = B.state(4)
    B.eps(R, a, 3, 0.0)
    B.eps(R, b, 4, 1 / 16.0)
    B.eps(R, c, 5, 2 / 16.0)
    B.eps(R, d, 6, INF, INF)          # the last arc of a row
    t = B.state()
    B.eps(a, t, 7, INF, INF)          # the only arc of an entry
    big = B.state(6)
    for i, s in enumerate(big):        # a row of six priced alone, one of them zero
        B.eps(b, s, 8 + i, INF if i == 2 else i / 16.0, INF if i == 2 else 0.0)
    B.word(a, t, 7)
    _end(B, [c, d, t] + big)
    L = B.raw()
    return Case("zero_weight_arcs", L, dict(zero_arc=("==", 2), big_zero=("==", 1), **ON_WAVE),
                [("closure of R leaves out what only zero arcs reach", len(closure(L, [R])), 1 + 3 + 5), ("rows", [n_eps(L, R), n_eps(L, a), n_eps(L, b)], [4, 1, 6])])


def _rule1():
    B = Lat()
    R = _start(B)
    a, b = B.state(), B.state()
    B.eps(R, a, 3, 1 / 16.0)
    B.eps(R, b, 4, 1 / 16.0)
    B.eps(a, b, 5, 5 / 16.0)   # 6/16 against b's 1/16: loses
    _end(B, [a, b])
    return Case("rule1_offer_loses", B, dict(dropped=NZ, killed=Z, meet=Z, mixed=Z, **ON_WAVE), [])


def _rule2():
    B = Lat()
    R = _start(B)
    a, x, y = B.state(), B.state(), B.state()
    B.eps(R, a, 3, 0.0)
    B.eps(R, x, 4, 4 / 16.0)
    B.eps(a, x, 5, 1 / 16.0)   # x through a: 1/16, cheaper than its own 4/16 -- a and x sit in one window
    B.eps(x, y, 6, 1 / 16.0)   # y must come out at 2/16
    _end(B, [a, x, y])
    return Case("rule2_window_ends_in_front_of_x", B, dict(killed=NZ, stale_entry=NZ, mixed=Z, **ON_WAVE), [])


def _diamond(name, tids, costs, want):
    """R -> a, b -> n: the two offers to n sit in one window.  tids / costs: (R->a, R->b, a->n, b->n)"""
    B = Lat()
    R = _start(B)
    a, b, n = B.state(), B.state(), B.state()
    B.eps(R, a, tids[0], costs[0])
    B.eps(R, b, tids[1], costs[1])
    B.eps(a, n, tids[2], costs[2])
    B.eps(b, n, tids[3], costs[3])
    _end(B, [a, b, n])
    return Case(name, B, dict(meet=NZ, meet_new=NZ, mixed=Z, **want, **ON_WAVE), [])


def _rule3_existing():
    B = Lat()
    R = _start(B)
    e, a, b, y = B.state(), B.state(), B.state(), B.state()
    B.eps(R, e, 3, 9 / 16.0)
    B.eps(R, a, 4, 0.0)
    B.eps(R, b, 5, 0.0)
    B.eps(a, e, 6, 2 / 16.0)
    B.eps(b, e, 7, 1 / 16.0)
    B.eps(e, y, 8, 1 / 16.0)
    _end(B, [e, a, b, y])
    return Case("rule3_offers_meet_in_an_existing_state", B, dict(meet=NZ, meet_old=NZ, mixed=Z, **ON_WAVE), [])


def _mixed():
    """two states new to the closure, offered in one window, whose probes of the state index end in one empty slot (found by search)"""
    R, a, b = 1, 2, 3
    occ = map_insert_all([R, a, b])
    seen, pair = {}, None
    for s in range(4, 6000):
        h = map_probe_end(occ, s)
        if h in seen:
            pair = (seen[h], s)
            break
        seen[h] = s
    n1, n2 = pair
    B = Lat()
    B.state(n2 + 2)
    F = n2 + 1
    B.word(0, R, 1)
    B.eps(R, a, 3, 0.0)
    B.eps(R, b, 4, 1 / 16.0)
    B.eps(a, n1, 5, 1 / 16.0)
    B.eps(b, n2, 6, 2 / 16.0)
    B.eps(a, n2, 7, 5 / 16.0)   # (and a worse offer to n2 from the earlier entry: the in-order commit takes it first, then b's)
    for s in range(4, F + 1):
        if s not in (n1, n2):
            B.final.add(s)       # the ids between: unreachable, arc-less, final
    _end(B, [a, b, n1, n2], F=F)
    L = B.raw()
    return Case("two_new_states_after_one_slot", L, dict(mixed=NZ, fb_inorder=Z, **ON_WAVE),
                [("probe ends", map_probe_end(occ, n1), map_probe_end(occ, n2)), ("different states", n1 != n2, True),
                 ("closure", closure(L, [R]), {R, a, b, n1, n2})])


def _closure_of(n):
    B = Lat()
    R = _start(B)
    ids = _tree(B, R, n)
    _end(B, ids)
    L = B.raw()
    want = dict(fb_mid_cur=NZ, fallback=NZ, fb_entry_n=Z) if n > K_CUR else dict(fallback=Z, fb_mid_cur=Z, fb_mid_queue=Z, sort_pad=NZ if n & (n - 1) else Z,
                                                                                           cur_full=NZ if n == K_CUR else Z)
    return Case("closure_of_%d" % n, L, dict(big_head=Z, **want), [("closure of R", len(closure(L, [R])), n),
                                                                   ("most epsilon arcs of a state", max(np.bincount(L.a_src[L.a_ol == 0])), 4)])


def _subset_of(n, name=None, want=None):
    """one word from R to n states: an initial subset of n elements (the closure is entered with n)"""
    B = Lat()
    R = _start(B)
    t = B.state(n)
    for i, s in enumerate(t):
        B.word(R, s, 2, 3 + i % 7, (i % 4) / 16.0)
    _end(B, t)
    L = B.raw()
    return Case(name or "subset_of_%d" % n, L, want, [("arcs of R under word 2", int(np.sum((L.a_src == R) & (L.a_ol == 2))), n),
                                                       ("their targets", len(set(L.a_dst[(L.a_src == R)].tolist())), n)])


def _ring_wrap(K=24, Ln=64):
    """a ladder: K roots two hops apart, each with a cheaper arc to the head of a chain of Ln states -- every root sends another wave
    down the chain: far more than 1024 pushes in a closure of 1 + 2 K + Ln states"""
    B = Lat()
    R = _start(B)
    c = B.state(Ln)
    r = B.state(K)
    x = B.state(K - 1)
    B.eps(R, r[0], 3)
    for k in range(K):
        B.eps(r[k], c[0], 4, (K - k) / 16.0)
        if k + 1 < K:
            B.eps(r[k], x[k], 5)
            B.eps(x[k], r[k + 1], 6)
    for i in range(Ln - 1):
        B.eps(c[i], c[i + 1], 7, 0.0)
    _end(B, c)
    L = B.raw()
    return Case("ring_wraps", L, dict(ring_wrap=NZ, fb_mid_queue=Z, fb_mid_cur=Z, **ON_WAVE),
                [("closure of R", len(closure(L, [R])), 2 * K + Ln), ("pushes at the least", K * Ln > K_QUEUE, True)])


def _queue_trip():
    """a fan of fans down to 256 states, each with four arcs into one layer of 256: state p of the 256 reaches 4 (p % 64) + a at a
    cost that falls with p // 64 -- every state of the layer is pushed four times while the 256 leave the queue 16 at a time"""
    B = Lat()
    R = _start(B)
    ids = _tree(B, R, 341, cost=lambda i: 0.0)
    layer = B.state(256)
    for p in range(256):
        for a in range(4):
            B.eps(ids[85 + p], layer[4 * (p % 64) + a], 3 + a, (3 - p // 64) / 16.0)
    _end(B, layer)
    L = B.raw()
    return Case("queue_outgrown", L, dict(fb_mid_queue=NZ, fb_mid_cur=Z, fallback=NZ, fb_entry_n=Z),
                [("closure of R", len(closure(L, [R])), 341 + 256), ("queue at the last window", 256 + 15 * (64 - K_WIN) + 64 > K_QUEUE, True)])


def _minimal_of(m):
    """a closure whose minimal result has m elements: a chain of hubs, three leaves each; only the leaves have word arcs"""
    B = Lat()
    R = _start(B)
    leaves, hub = [], R
    while len(leaves) < m:
        for j in range(min(3, m - len(leaves))):
            s = B.state()
            B.eps(hub, s, 3 + j, j / 16.0)
            leaves.append(s)
        if len(leaves) < m:
            nh = B.state()
            B.eps(hub, nh, 9, 1 / 16.0)
            hub = nh
    _end(B, leaves)
    L = B.raw()
    C = closure(L, [R])
    want = dict(sort_pad=NZ, stage_over=NZ if m > 64 else Z, norm_lane0=NZ if m > 64 else Z, pairs_lane0_n=NZ if m > 64 else Z, **ON_WAVE)
    return Case("minimal_result_of_%d" % m, L, want, [("minimal result", len(minimal(L, C)), m), ("closure no power of two", len(C) & (len(C) - 1) != 0, True)])


def _pairs_total(tot):
    """sixteen elements with tot labelled arcs between them"""
    B = Lat()
    R = _start(B)
    el = B.state(16)
    F = B.state()
    B.final.add(F)
    for i, s in enumerate(el):
        B.eps(R, s, 3 + i, (i % 4) / 16.0)
        for a in range(4 + (1 if i == 7 and tot == 65 else 0)):
            B.word(s, F, 100 + (37 * (4 * i + a)) % 101, 0, a / 16.0)
    L = B.raw()
    want = dict(pairs_lane0_tot=NZ, pairs_shell40=NZ) if tot > 64 else dict(pairs_lane0_tot=Z, pairs_shell40=Z, pairs_wave=NZ)
    return Case("pairs_%d_of_16_elements" % tot, L, dict(pairs_lane0_n=Z, **want, **ON_WAVE), [("labelled arcs of the 16", n_word_arcs(L, el), tot)])


def _final_tie():
    B = Lat()
    R = _start(B)
    f1, f2, f3 = B.state(3)
    B.eps(R, f1, 0, 2 / 16.0)
    B.eps(R, f2, 0, 2 / 16.0)
    B.eps(R, f3, 0, 3 / 16.0)
    B.final.update([f1, f2, f3])
    return Case("final_elements_tie", B, dict(final_multi=NZ, final_tie=NZ, **ON_WAVE), [])


def _merge():
    B = Lat()
    R = _start(B)
    t, u = B.state(), B.state()
    B.word(R, t, 2, 3, 2 / 16.0)
    B.word(R, t, 2, 4, 1 / 16.0)
    B.word(R, t, 2, 5, 1 / 16.0)
    B.word(R, u, 2, 6, 0.0)
    _end(B, [t, u])
    return Case("equal_pairs_merge", B, dict(unique_merge=("==", 2), **ON_WAVE), [])


def _plen0():
    B = Lat()
    R = _start(B)
    a, b = B.state(), B.state()
    B.word(R, a, 2, 5, 1 / 16.0)
    B.word(R, b, 2, 6, 0.0)
    _end(B, [a, b])
    return Case("no_common_prefix", B, dict(norm_plen0=NZ, **ON_WAVE), [])


def _best_tie():
    B = Lat()
    R = _start(B)
    a, b, c = B.state(3)
    B.word(R, a, 2, 5, 1 / 16.0)
    B.word(R, b, 2, 5, 1 / 16.0)
    B.word(R, c, 2, 5, 2 / 16.0)
    _end(B, [a, b, c])
    return Case("best_weight_tied", B, dict(norm_best_tie=NZ, norm_prefix=NZ, **ON_WAVE), [])


def _strings(n_left, name=None):
    """R's closure holds a (string [5]), b (string [5, 20, 21, ...]: n_left labels more) and c (string [9]): no common prefix
    in the output state; word 2 leaves a and b only, so its subset's strings share [5] and the longest has n_left labels left"""
    B = Lat()
    R = _start(B)
    a, c = B.state(), B.state()
    B.eps(R, a, 5, 1 / 16.0)
    B.eps(R, c, 9, 0.0)
    prev = a
    for i in range(n_left):
        s = B.state()
        B.eps(prev, s, 20 + i, 0.0)
        prev = s
    b = prev
    x, y, z = B.state(3)
    B.word(a, x, 2, 0, 0.0)
    B.word(b, y, 2, 0, 1 / 16.0)
    B.word(c, z, 3, 0, 0.0)
    _end(B, [x, y, z])
    L = B.raw()
    want = dict(norm_prefix=NZ, norm_depths=NZ, norm_at_labs=NZ if n_left == K_LABS else Z, norm_long=NZ if n_left > K_LABS else Z, **ON_WAVE)
    return Case(name or "string_of_%d_left" % n_left, L, want, [("closure of R", len(closure(L, [R])), 3 + n_left), ("minimal", minimal(L, closure(L, [R])), {a, b, c})])


def _delta(exp):
    """the same subset {x, y} under word 3 from two states, y's weight 2^-exp apart"""
    B = Lat()
    s0 = B.state()
    r1, r2, x, y = B.state(4)
    B.word(s0, r1, 1)
    B.word(s0, r2, 2)
    B.word(r1, x, 3, 0, 0.0)
    B.word(r1, y, 3, 0, 1.0)
    B.word(r2, x, 3, 0, 0.0)
    B.word(r2, y, 3, 0, 1.0 + 2.0 ** -exp)
    _end(B, [x, y])
    # initial subsets made: {r1}, {r2}, {x, y}, {F} -- and {x, y} once more where the two are further apart than delta
    want = dict(init_found_approx=NZ, init_new=("==", 4)) if 2.0 ** -exp <= DELTA else dict(init_found_approx=Z, init_new=("==", 5))
    return Case("subsets_2p-%d_apart" % exp, B, dict(**want, **ON_WAVE), [("within delta", 2.0 ** -exp <= DELTA, exp == 11)])


def _trie_pair(kind):
    """R with two epsilon arcs whose labels, after the empty string, go for: the same node / one empty slot with two keys / two empty
    slots that share a claim word -- labels found by search against the first table of a lattice of this size"""
    n_states = 5
    mask = first_table(n_states) - 1
    slot = lambda l: hash2(0, l) & mask
    l1, l2 = 5, None
    if kind == "same_key":
        l2 = l1
    else:
        for l in range(6, 200000):
            if kind == "same_slot" and slot(l) == slot(l1) and slot(l) != 0:
                l2 = l
                break
            if kind == "alias" and slot(l) != slot(l1) and slot(l) % CLAIM == slot(l1) % CLAIM and slot(l) != 0:
                l2 = l
                break
    B = Lat()
    R = _start(B)
    a, b = B.state(), B.state()
    B.eps(R, a, l1, 0.0)
    B.eps(R, b, l2, 1 / 16.0)
    _end(B, [a, b])
    L = B.raw()
    want = dict(trie_lost_same_key=NZ if kind == "same_key" else Z, trie_lost_same_slot=NZ if kind == "same_slot" else Z,
                trie_lost_alias=NZ if kind == "alias" else Z, **ON_WAVE)
    facts = [("states", L.n_states, n_states), ("slot of the first label is free", slot(l1) != 0, True),
             ("same key", det_key(0, l1) == det_key(0, l2), kind == "same_key"), ("same slot", slot(l1) == slot(l2), kind != "alias"),
             ("same claim word", slot(l1) % CLAIM == slot(l2) % CLAIM, True)]
    return Case("trie_" + kind, L, want, facts)


def chain_lattice(hops=100, par=30):
    """a chain of `hops` hops with `par` parallel word-less arcs each, every one with another transition-id: every offer makes a
    trie node (the losers too): hops * par nodes in a lattice of hops + 3 states"""
    B = Lat()
    R = _start(B)
    prev = R
    for h in range(hops):
        s = B.state()
        for j in range(par):
            B.eps(prev, s, 1 + h * par + j, ((j * 7) % par) / 16.0)
        prev = s
    _end(B, [prev])
    return B.raw()


def _trie_retry():
    L = chain_lattice()
    return Case("trie_outgrows_the_first_table", L, dict(trie_retry=("==", 1), fb_entry_n=Z, fb_mid_cur=Z, fb_mid_queue=Z, big_head=NZ),   # (fallback counts the closure the first attempt's refusal ended, too)
                [("states", L.n_states <= 256, True), ("first table", first_table(L.n_states), TRIE_FIRST),
                 ("nodes against half the table", 100 * 30 > TRIE_FIRST // 2, True)])


def _top_ids(n_states):
    """n_states states; the closure under test on the highest ids, everything between unreachable, arc-less and final"""
    S = n_states
    R, a, b, c, F = S - 1, S - 2, S - 3, S - 4, S - 5
    fin = np.ones(S, np.int32)
    fin[[0, R, a, b, c]] = 0
    arcs = [(0, R, 0, 1, 0.0), (R, a, 3, 0, 1 / 16.0), (R, b, 4, 0, 0.0), (a, c, 5, 0, 1 / 16.0), (b, c, 6, 0, 3 / 16.0),
            (a, F, 0, 7, 0.0), (b, F, 0, 8, 0.0), (c, F, 0, 9, 0.0)]
    col = lambda i, t: np.asarray([x[i] for x in arcs], t)
    L = pyoracle.RawLattice(True, S, 0, fin, col(0, np.int32), col(1, np.int32), col(2, np.int32), col(3, np.int32), col(4, np.float32),
                            np.zeros(len(arcs), np.float32))
    on = S < MAX_STATES
    want = dict(fb_entry_states=Z if on else NZ, fallback=Z if on else NZ, meet_new=NZ if on else Z)   # (a and b's offers meet in c: on the wave)
    return Case("states_2p21" + ("_less_1" if on else ""), L, want, [("states", S, MAX_STATES - 1 if on else MAX_STATES),
                                                                       ("highest id of the closure", max(closure(L, [R])), S - 1),
                                                                       ("its map word and sort key fit 32 bits", max((S - 1) << MAP_SHIFT | K_CUR, (S - 1) << SORT_SHIFT | (K_CUR - 1)) <= _M, True)])


def _word_chain(name, args, code):
    B = Lat()
    prev = B.state()
    for i in range(10):
        s = B.state()
        B.word(prev, s, 1 + i, 3, i / 16.0)
        prev = s
    B.final.add(prev)
    return Case(name, B, {}, [], args=args, refuse=code)


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        c = [_fan_case(k) for k in (3, 4, 5, 63, 64, 65, 130)]
        c += [_big_not_at_head()] + [_queue_of(n) for n in (15, 16, 17)] + [_zero_arcs()]
        c += [_rule1(), _rule2(),
              _diamond("rule3_better_offer_wins", (0, 0, 0, 0), (0.0, 0.0, 2 / 16.0, 1 / 16.0), dict(meet_tie=Z)),
              _diamond("rule3_exact_tie", (5, 5, 7, 7), (0.0, 0.0, 1 / 16.0, 1 / 16.0), dict(meet_tie=NZ, trie_lost_same_key=NZ)),
              _diamond("rule3_strings_differ_in_a_label", (5, 5, 7, 8), (0.0, 0.0, 1 / 16.0, 1 / 16.0), dict(meet_str_label=NZ, meet_tie=Z)),
              _diamond("rule3_strings_differ_in_length", (5, 0, 7, 8), (0.0, 0.0, 1 / 16.0, 1 / 16.0), dict(meet_str_len=NZ, meet_tie=Z)),
              _rule3_existing(), _mixed()]
        c += [_closure_of(n) for n in (1023, 1024, 1025)]
        c += [_subset_of(1025, "closure_entered_with_1025", dict(fb_entry_n=NZ, fallback=NZ, run_te=NZ, subset_big=NZ))]
        c += [_ring_wrap(), _queue_trip()] + [_minimal_of(m) for m in (63, 64, 65, 200)]
        c += [_pairs_total(64), _pairs_total(65),
              _subset_of(64, "run_of_64_pairs", dict(run_te=Z, subset_64=NZ, subset_big=Z, pairs_lane0_tot=Z, **ON_WAVE)),
              _subset_of(65, "run_of_65_pairs", dict(run_te=NZ, subset_big=NZ, pairs_lane0_tot=NZ, pairs_shell40=NZ, **ON_WAVE)),
              _final_tie(), _merge()]
        c += [_subset_of(1, "subset_of_one", dict(norm_k1=NZ, **ON_WAVE)), _plen0(), _strings(3, "strings_of_different_depth"),
              _strings(127), _strings(128), _strings(129), _best_tie(), _delta(11), _delta(9)]
        c += [_trie_pair(k) for k in ("same_key", "same_slot", "alias")] + [_trie_retry()]
        c += [_top_ids(MAX_STATES - 1), _top_ids(MAX_STATES)]
        c += [_word_chain("refused_states", ["--cap-states", "4"], 3), _word_chain("refused_arcs", ["--cap-arcs", "4"], 5)]
        assert len({x.name for x in c}) == len(c)
        _CASES = c
    return _CASES


# ---- decoding graphs for the product kernel's own CSR build and retry loop (a real BatchDecoder; in the manner of gc_util.fan) --------
DECODER_CFG = dict(beam=64.0, max_active=1000000, min_active=0, lattice_beam=64.0)   # prunes nothing of these graphs
DECODER_SHAPES = ("fan_of_70", "strings_beyond_128", "chain_of_parallel_arcs")
FAN = 70
STRETCH = 135        # frames of "strings_beyond_128": the two strings keep STRETCH - 3 labels behind the one they share
HOPS, PAR = 100, 30


def decoder_shape(synth, name):
    """(graph, loglikes [T][1 + n_tid], facts(raw lattice) -> [(what, got, claimed)]): column = transition-id, no tid2pdf.
    fan_of_70: 0 --w--> h --70 word-less arcs--> u_i --w_i--> f: the lattice state of h has 70 word-less out-arcs.
    strings_beyond_128: 0 --w--> a --tid 2--> P | Q, each with a self-loop of its own transition-id, left for f on the last frame
      with one word: the minimal closure behind a holds two strings that share [2] and keep more than 128 labels each.
    chain_of_parallel_arcs: HOPS hops of PAR parallel word-less arcs, every one with another transition-id, a word at the end:
      at most 256 lattice states, HOPS * PAR trie nodes."""
    if name == "fan_of_70":
        h, f = 1, 2 + FAN
        arcs = {0: [(1, 1, 0.0, h)], h: [(2 + i, 0, (i % 5) / 16.0, 2 + i) for i in range(FAN)]}
        for i in range(FAN):
            arcs[2 + i] = [(1, 2 + i, 0.0, f)]
        g, T, n_tid = synth.graph_from_arc_lists(f + 1, 0, arcs, {f: 0.0}), 3, 1 + FAN
        facts = lambda L: [("most word-less arcs of a lattice state", int(np.bincount(L.a_src[L.a_ol == 0]).max()), FAN)]
    elif name == "strings_beyond_128":
        a, P, Q, f = 1, 2, 3, 4
        arcs = {0: [(1, 1, 0.0, a)], a: [(2, 0, 0.0, P), (2, 0, 1 / 16.0, Q)], P: [(3, 0, 0.0, P), (5, 2, 0.0, f)], Q: [(4, 0, 0.0, Q), (5, 2, 0.0, f)]}
        g, T, n_tid = synth.graph_from_arc_lists(5, 0, arcs, {f: 0.0}), STRETCH, 5
        facts = lambda L: [("arcs with the shared transition-id", int(np.sum(L.a_il == 2)), 2), ("they leave one state", len(set(L.a_src[L.a_il == 2].tolist())), 1),
                           ("labels behind it, P", int(np.sum(L.a_il == 3)), STRETCH - 3), ("labels behind it, Q", int(np.sum(L.a_il == 4)), STRETCH - 3),
                           ("more than kDwLabs", STRETCH - 3 > K_LABS, True), ("word arcs", int(np.sum(L.a_ol != 0)), 3)]
    else:
        arcs = {s: [(1 + PAR * s + j, 0, ((7 * j) % PAR) / 16.0, s + 1) for j in range(PAR)] for s in range(HOPS)}
        arcs[HOPS] = [(1 + PAR * HOPS, 1, 0.0, HOPS + 1)]
        g, T, n_tid = synth.graph_from_arc_lists(HOPS + 2, 0, arcs, {HOPS + 1: 0.0}), HOPS + 1, 1 + PAR * HOPS
        facts = lambda L: [("lattice states", L.n_states <= 256, True), ("first table", first_table(L.n_states), TRIE_FIRST),
                           ("word-less arcs with a transition-id of their own", len(set(L.a_il[(L.a_ol == 0) & (L.a_il != 0)].tolist())), HOPS * PAR),
                           ("more than half the first table", HOPS * PAR > TRIE_FIRST // 2, True)]
    t, c = np.meshgrid(np.arange(T), np.arange(n_tid + 1), indexing="ij")
    ll = -(((3 * c + t) % 4) / 4.0).astype(np.float32)
    return g, ll, facts
