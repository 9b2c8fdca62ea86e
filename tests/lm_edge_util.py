"""Edge LMs, script graphs and a counting LM walk for tests/test_lm_edge_models.py and tests/test_gpu_lm_edges.py.

The device walks a back-off LM through ONE open-addressed (state, word) table (LmDev::hash, wfst_device.h), the biglm kernels kLmProbe
= 4 slots per round trip with a probe offset carried across rounds and reset at a back-off (lm_step_pk, wfst_kernels.hip).  What that
walk can get wrong shows only where a probe sequence is longer than a round, ends right at a round's edge, wraps from the last slot to
slot 0, or where a back-off chain is long -- so the LMs here are BUILT to hold such places, with a numpy mirror of lm_hash and of the
host's insertion loop (wfst_lm_from_arrays), and the scripts are word sequences that ask for exactly those keys.  All LMs are
lmsynth.NgramLm tables over V = 300 real words: ARPA models the reference converter reads.  numpy only."""
import importlib

import numpy as np

lmsynth = importlib.import_module("asr-decoder_amd.lmsynth")
synth = importlib.import_module("asr-decoder_amd.synth")

V = 300
BOS, EOS, UNK = V + 1, V + 2, V + 3
K_PROBE = 4                      # slots per round trip of the biglm kernels (kLmProbe)
RUN_LENGTHS = (4, 5, 8, 9)       # isolated runs: a probe ends at a round's last slot (4, 8) or in the first slot of the next (5, 9)
WRAP_LENGTH = 14                 # the run over slot 1023 and slot 0: displacements up to 13, a fourth round
N_WORDS = 6                      # words (= frames) of a script
TAIL = (298, 299)                # the two words of the shared tail
PADS = tuple(range(260, 298))    # filler words of the scripts (no edge LM gives them a higher-order line of its own)
f32 = np.float32


# ---------------------------------------------------------------- the mirror of the device table
def lm_hash(state, word):
    """lm_hash (wfst_device.h) on scalars or arrays: uint32 arithmetic carried out in uint64."""
    M = np.uint64(0xFFFFFFFF)
    s = np.asarray(state, np.int64).astype(np.uint64) & M
    w = np.asarray(word, np.int64).astype(np.uint64) & M
    h = ((s * np.uint64(0x9E3779B1)) & M) ^ ((((w + np.uint64(0x7F4A7C15)) & M) * np.uint64(0x85EBCA77)) & M)
    h = h ^ (h >> np.uint64(15))
    return ((h * np.uint64(0x2C1B3C6D)) & M).astype(np.int64)


class MirrorTable:
    """The (state, word) table as wfst_lm_from_arrays fills it: every arc of every state but the empty history, state by state, a
    state's arcs in word order, linear probing from lm_hash & (size - 1); size = the power of two >= max(1024, 4 * entries)."""

    def __init__(self, fsa):
        off = fsa.arc_offsets()
        n = fsa.n_arcs - int(off[1])
        size = 1024
        while size < 4 * max(1, n):
            size <<= 1
        self.size, self.mask = size, size - 1
        self.state = np.full(size, -1, np.int64)
        self.word = np.full(size, -1, np.int64)
        self.arc = np.full(size, -1, np.int64)
        self.disp = {}                                   # (state, word) -> slots past its home slot
        words = fsa.arcs["wordid"]
        for s in range(1, fsa.n_states):
            for a in range(int(off[s]), int(off[s + 1])):
                w = int(words[a])
                slot, d = int(lm_hash(s, w)) & self.mask, 0
                while self.state[slot] >= 0:
                    slot, d = (slot + 1) & self.mask, d + 1
                self.state[slot], self.word[slot], self.arc[slot] = s, w, a
                self.disp[(s, w)] = d

    def runs(self):
        """[(first slot, length)] of the cyclic runs of occupied slots"""
        occ = self.state >= 0
        if not occ.any():
            return []
        e = int(np.flatnonzero(~occ)[0])
        out, first, n = [], -1, 0
        for k in range(1, self.size + 1):
            slot = (e + k) & self.mask
            if occ[slot]:
                if n == 0:
                    first = slot
                n += 1
            elif n:
                out.append((first, n))
                n = 0
        return out

    def stats(self):
        """the figures of wfstdec.Lm.table_stats()"""
        r = self.runs()
        return dict(table_size=self.size, used=int((self.state >= 0).sum()), longest_run=max([n for _, n in r] + [0]),
                    max_displacement=max(list(self.disp.values()) + [0]), wraps=bool(self.state[self.size - 1] >= 0 and self.state[0] >= 0))

    def probe(self, s, w):
        """(arc index or -1, slots looked at, the empty one that ends a miss included) -- fsa_getarc's loop"""
        slot, n = int(lm_hash(s, w)) & self.mask, 1
        while True:
            if self.state[slot] == s and self.word[slot] == w:
                return int(self.arc[slot]), n
            if self.state[slot] < 0:
                return -1, n
            slot, n = (slot + 1) & self.mask, n + 1


# ---------------------------------------------------------------- the counting walk
def get_arc(fsa, tab, s, word):
    """ComposeArpaLm::GetArc (newlm/compose-arpalm.cc:52-70) over the Fsa arrays and the mirror table: (next state, Value1 cost,
    probes, depth).  probes = [(state, slots looked at, found)] level by level (the empty history is indexed, 0 slots); depth = the
    back-offs taken.  The cost is minus the float32 sum of the back-off weights and the arc weight, in that order."""
    weight, probes = f32(0.0), []
    while True:
        if s == 0:
            a = int(word)
            probes.append((0, 0, True))
        else:
            a, n = tab.probe(s, word)
            probes.append((s, n, a >= 0))
        if a >= 0:
            break
        weight = f32(weight + fsa.states["backoff_prob"][s])
        s = int(fsa.states["backoff_id"][s])
    weight = f32(weight + fsa.arcs["weight"][a])
    return int(fsa.arcs["tostateid"][a]), f32(f32(-1.0) * weight), probes, len(probes) - 1


def walk_records(fsa, scripts, tab=None):
    """Every look-up a decode of the scripts asks of this LM, from ComposeArpaLm::Start (the state after <s>): one per word and the
    final cost's look-up of </s> (pos = N_WORDS).  dict(script, pos, state, word, next, cost, probes, depth)."""
    tab = tab or MirrorTable(fsa)
    out = []
    for i, sc in enumerate(scripts):
        s = int(fsa.arcs["tostateid"][fsa.bos])
        for pos, w in enumerate(list(sc["words"]) + [fsa.eos]):
            nx, cost, probes, depth = get_arc(fsa, tab, s, int(w))
            out.append(dict(script=i, pos=pos, state=s, word=int(w), next=nx, cost=cost, probes=probes, depth=depth))
            if pos < len(sc["words"]):
                s = nx
    return out


def rounds(slots):
    """round trips of K_PROBE slots a probe sequence of `slots` slots takes"""
    return -(-int(slots) // K_PROBE)


def walk_profile(fsa, scripts):
    """The set of (rounds, depth) the scripts' look-ups meet in this LM: rounds = ceil(probe length / K_PROBE) with the look-up's
    probe length = its longest probe sequence over the levels of its back-off chain, depth = its back-offs."""
    return {(rounds(max(n for _, n, _ in r["probes"])), r["depth"]) for r in walk_records(fsa, scripts)}


def end_states(fsa, scripts):
    """the LM state every script ends in"""
    last = {}
    for r in walk_records(fsa, scripts):
        if r["pos"] == N_WORDS:
            last[r["script"]] = r["state"]
    return [last[i] for i in range(len(scripts))]


# ---------------------------------------------------------------- weights
class _Weights:
    """log10 weights from a seeded generator, no two equal (as float32, and as the natural-log float32 the converter makes of them):
    a sum taken in another order, or a weight taken from a neighbouring arc, changes bits."""

    def __init__(self, rng):
        self.rng, self.seen = rng, set()

    def __call__(self, lo, hi):
        while True:
            x = f32(self.rng.uniform(lo, hi))
            k = (x.tobytes(), lmsynth._ln(x).tobytes())
            if x != 0 and not (set(k) & self.seen):
                self.seen.update(k)
                return x


def _unigrams(W, order, skip=(), with_unk=False):
    uni = []
    for w in list(range(1, V + 1)) + [BOS, EOS] + ([UNK] if with_unk else []):
        if w in skip:
            continue
        lp = f32(-99.0) if w == BOS else W(-5.0, -1.0)
        uni.append(((w,), lp, f32(0) if (w == EOS or order == 1) else W(-1.0, -0.05)))
    return uni


def _sorted_lines(d):
    """ARPA lines of one order, a context's lines contiguous and in word order (the converter's arc pool needs the first, its
    insertion sort makes the second immaterial)"""
    return [(k, d[k][0], d[k][1]) for k in sorted(d)]


# ---------------------------------------------------------------- the edge LMs
def unigram_lm(seed):
    """order 1: every look-up is the empty history's indexed arc -- in lockstep it is done in one round while the other LM probes on"""
    W = _Weights(np.random.default_rng([int(seed), 0x01]))
    lm = lmsynth.NgramLm(V, [_unigrams(W, 1)])
    lm.edge = dict(kind="unigram")
    return lm


def cluster_lm(seed):
    """order 2, at most 256 bigram lines (a table of 1 024 slots), the bigrams chosen with the mirror: a bigram (a, b) is the key
    (state a + 1, b).  Isolated runs of exactly 4, 5, 8 and 9 occupied slots and one of WRAP_LENGTH over slot 1023 and slot 0, the
    keys of a run all at home in its first slot (displacements 0 .. length - 1); 150 filler lines, <s> contexts and </s> words among
    them, on even slots away from those runs (and three more for the resets, below).  lm.edge: runs = [dict(first, length, keys [(a, b)], absent (a, b))] -- absent: a
    bigram the LM does not have whose home slot is the run's first, so that its look-up crosses the whole run; resets = [dict(words
    [x, y, w], leaf, crossed)] (below)."""
    rng = np.random.default_rng([int(seed), 0xC1])
    W = _Weights(rng)
    a = np.repeat(np.arange(1, V + 1), V)
    b = np.tile(np.arange(1, V + 1), V)
    home = lm_hash(a + 1, b) & 1023
    wrap_first = 1024 - int(rng.integers(5, 10))
    taken = {(wrap_first + k) & 1023 for k in range(-2, WRAP_LENGTH + 2)}
    firsts = []
    for L in RUN_LENGTHS:
        while True:
            s = int(rng.integers(16, 1000 - L))
            zone = set(range(s - 2, s + L + 2))
            if not (zone & taken):
                break
        taken |= zone
        firsts.append(s)
    runs, bi = [], {}
    for s, L in zip(firsts + [wrap_first], RUN_LENGTHS + (WRAP_LENGTH,)):
        idx = np.flatnonzero(home == s)
        assert len(idx) > L
        pick = rng.choice(idx, L + 1, replace=False)
        keys = sorted((int(a[i]), int(b[i])) for i in pick[:L])
        runs.append(dict(first=s, length=L, keys=keys, absent=(int(a[pick[L]]), int(b[pick[L]]))))
        for k in keys:
            bi[k] = None
    never = {r["absent"] for r in runs}
    used = set()

    def fill(x, y):
        h = int(lm_hash(x + 1, y)) & 1023
        if h % 2 or h in taken or h in used or (x, y) in bi or (x, y) in never:
            return False
        used.add(h)
        bi[(x, y)] = None
        return True

    n = 0
    while n < 12:      # ... </s> as an explicit bigram at some states
        n += fill(int(rng.integers(1, V + 1)), EOS)
    n = 0
    while n < 8:       # ... and some bigrams of the sentence start
        n += fill(BOS, int(rng.integers(1, V + 1)))
    n = 0
    while n < 130:
        n += fill(int(rng.integers(1, V + 1)), int(rng.integers(1, V + 1)))
    # RESETS: a look-up that has probed past its first round when it misses, and then backs off to a state whose own look-up is a
    # table probe that must start at ITS home slot again.  The unigram states back off to the empty history (indexed, no probe), so
    # the miss is a leaf's: the state of a bigram line (x, y) -- number 1 + (EOS + 1) + the line's place in the file, no arcs -- asked
    # for a word w whose key (leaf, w) is at home in the first slot of a run of 8 or more; it backs off to (y), where the bigram
    # (y, w) -- a filler line added here, behind (x, y) in the file so that the leaf keeps its number -- sits in its home slot.
    resets = []
    long_first = {r["first"]: r["length"] for r in runs if r["length"] >= 8}
    guard = (0, 0)                                  # the last chosen (x, y): a line added behind it moves no chosen leaf
    while len(resets) < 3:
        n = len(resets)
        for i, (x, y) in enumerate(sorted(bi)):
            if x > V or y > V or any(r["words"][:2] == [x, y] for r in resets):
                continue
            leaf = 1 + (EOS + 1) + i
            for w in range(1, V + 1):
                h = int(lm_hash(leaf, w)) & 1023
                if h in long_first and (y, w) > max(guard, (x, y)) and fill(y, w):
                    resets.append(dict(words=[x, y, w], leaf=leaf, crossed=long_first[h]))
                    guard = max(guard, (x, y))
                    break
            if len(resets) > n:
                break                                # (the file order has changed: number the lines again)
        assert len(resets) > n
    for k in bi:
        bi[k] = (W(-4.0, -0.2), f32(0))
    lm = lmsynth.NgramLm(V, [_unigrams(W, 2), _sorted_lines(bi)])
    lm.edge = dict(kind="cluster", runs=runs, resets=resets)
    return lm


# words of the deep LM's cases
DEEP_FAMILIES = [dict(ctx=(20 + 10 * f, 21 + 10 * f, 22 + 10 * f, 23 + 10 * f), x=24 + 10 * f, word_depth=f, eos_depth=(f + 2) % 5) for f in range(5)]
SKIP = dict(ctx=(80, 81, 82), bigram_word=83, unigram_word=84)    # 80 81 82 without a bigram 81 82: its state backs off to (82)
DROPPED = (90, 91, 92)                                            # "no A B, but have A B C" (arpa2fsa.cc:558-565)
NO_UNIGRAM = 57                                                   # a word without a unigram line: the on-demand start arc, weight 0


def deep_lm(seed):
    """order 5.  Five families of a four-word context (a b c d) whose suffix states (b c d), (c d), (d) all exist, so that a word
    missing at the top k levels is found after exactly k back-offs: family f has its word x at depth f and </s> at depth (f + 2) % 5
    (depth 0: a 5-gram; depth 4: the unigram alone).  SKIP: a trigram state whose suffix bigram is absent -- its back-off skips a
    level.  DROPPED: a trigram without its bigram, which the converter does not add.  NO_UNIGRAM: a word id below V with no unigram
    line.  An <unk> unigram line, which the converter refuses (every unknown word maps to that id).  A few dozen random lines per
    order on top, most of them with suffixes missing, many of them leaves.  Every back-off weight non-zero and distinct."""
    rng = np.random.default_rng([int(seed), 0xDE])
    W = _Weights(rng)
    g = [dict() for _ in range(5)]

    def add(t):
        """the n-gram t and, so that the converter finds its context, every prefix of it"""
        t = tuple(int(x) for x in t)
        if len(t) == 1 or t in g[len(t) - 1]:
            return
        add(t[:-1])
        g[len(t) - 1][t] = (W(-3.0, -0.1), f32(0) if (len(t) == 5 or t[-1] == EOS) else W(-1.2, -0.05))

    for fam in DEEP_FAMILIES:
        c = fam["ctx"]
        add(c)
        add(c[1:])
        add(c[2:])
        for word, depth in ((fam["x"], fam["word_depth"]), (EOS, fam["eos_depth"])):
            if depth < 4:
                add(c[depth:] + (word,))
    add(SKIP["ctx"])
    add((SKIP["ctx"][2], SKIP["bigram_word"]))
    for k in range(1, 5):                                  # random lines: words 100 .. 239, some ending in </s>, some after <s>
        for _ in range(24):
            t = [int(x) for x in rng.integers(100, 240, k + 1)]
            if rng.random() < 0.15:
                t[-1] = EOS
            if rng.random() < 0.15:
                t[0] = BOS
            add(t)
    g[2][DROPPED] = (W(-3.0, -0.1), W(-1.2, -0.05))
    assert DROPPED[:2] not in g[1] and SKIP["ctx"][1:] not in g[1]
    lm = lmsynth.NgramLm(V, [_unigrams(W, 5, skip=(NO_UNIGRAM,), with_unk=True)] + [_sorted_lines(d) for d in g[1:]])
    lm.edge = dict(kind="deep")
    return lm


# ---------------------------------------------------------------- scripts and their graph
def edge_scripts(cluster_a, cluster_b, seed=0):
    """The word sequences (N_WORDS each) that ask the edge LMs for their edges, as dict(words, tail, eps):
    every key of a required run of either cluster LM as [a, b] (a from a state that backs off to the unigram), every run's absent
    bigram, the cluster LMs' reset cases, the deep LM's families (the word case, and the context as the script's END for the </s> case), its skip-level state, its
    dropped line, the word without a unigram.  tail: the script ends in the two TAIL words, on graph states it shares with the
    other tail scripts; eps = (position, "before" | "after"): that word sits on an input-epsilon arc before / behind an emitting arc
    without a word.  (The <unk> id is no script word: the converter gives it no arc from the empty history, so a graph with that
    label is one the biglm decoder refuses -- rightly.)"""
    rng = np.random.default_rng([int(seed), 0x5C])
    pad = lambda: int(rng.choice(PADS))
    whole = []
    for fam in DEEP_FAMILIES:
        whole.append(list(fam["ctx"]) + [fam["x"], pad()])
        whole.append([pad(), pad()] + list(fam["ctx"]))
    whole.append(list(SKIP["ctx"]) + [SKIP["bigram_word"], pad(), pad()])
    whole.append(list(SKIP["ctx"]) + [SKIP["unigram_word"], pad(), pad()])
    whole.append(list(DROPPED) + [pad(), NO_UNIGRAM, pad()])
    whole.append([NO_UNIGRAM, pad(), pad(), NO_UNIGRAM, NO_UNIGRAM, pad()])
    for ra, rb in zip(cluster_a.edge["resets"], cluster_b.edge["resets"]):
        whole.append(ra["words"] + rb["words"])
    pairs = []
    for lm in (cluster_a, cluster_b):
        for r in lm.edge["runs"]:
            pairs += [list(k) for k in r["keys"]] + [list(r["absent"])]
    order = rng.permutation(len(pairs))
    pairs = [pairs[i] for i in order]
    n_tail = 32
    scripts = []
    for i in range(n_tail):                                # two pairs and the tail
        scripts.append(dict(words=pairs[2 * i] + pairs[2 * i + 1] + list(TAIL), tail=True))
    rest = pairs[2 * n_tail:]
    while len(rest) % 3:
        rest.append([pad(), pad()])
    for i in range(0, len(rest), 3):
        scripts.append(dict(words=rest[i] + rest[i + 1] + rest[i + 2], tail=False))
    scripts += [dict(words=w, tail=False) for w in whole]
    for i, sc in enumerate(scripts):
        sc["eps"] = None
        if i % 4 == 0:                                     # a quarter: one word on an input-epsilon arc
            sc["eps"] = (int(rng.integers(0, 4 if sc["tail"] else N_WORDS)), "before" if i % 8 == 0 else "after")
    assert all(len(sc["words"]) == N_WORDS for sc in scripts) and len({tuple(sc["words"]) for sc in scripts}) == len(scripts)
    return scripts


def script_graph(scripts, seed=0):
    """One chain per script from ONE start state, an arc per word: olabel the word, ilabel a transition id of its own (n_tid of
    them: every emitting arc has its own log-likelihood column, tid2pdf = identity).  The tail scripts join shared states for
    their last two words.  Every chain is N_WORDS emitting arcs long, so all end on frame N_WORDS.
    Returns (synth.Graph, n_tid, the graph state every script ends in)."""
    rng = np.random.default_rng([int(seed), 0x6A])
    wt = lambda: float(f32(rng.uniform(0.05, 2.0)))
    arcs, finals = {0: []}, {}
    n_states, n_tid = 1, 0

    def new_state():
        nonlocal n_states
        arcs[n_states] = []
        n_states += 1
        return n_states - 1

    def new_tid():
        nonlocal n_tid
        n_tid += 1
        return n_tid

    def word_arc(u, v, word, eps):
        """the word from u to v: on an emitting arc, or split over an epsilon arc and a wordless emitting arc through a state m"""
        if eps is None:
            arcs[u].append((new_tid(), word, wt(), v))
            return
        m = new_state()
        if eps == "before":
            arcs[u].append((0, word, wt(), m))
            arcs[m].append((new_tid(), 0, wt(), v))
        else:
            arcs[u].append((new_tid(), 0, wt(), m))
            arcs[m].append((0, word, wt(), v))

    tail0, tail1, tail2 = new_state(), new_state(), new_state()
    word_arc(tail0, tail1, TAIL[0], None)
    word_arc(tail1, tail2, TAIL[1], None)
    finals[tail2] = wt()
    ends = []
    for sc in scripts:
        own = N_WORDS - 2 if sc["tail"] else N_WORDS
        u = 0
        for j in range(own):
            v = tail0 if (sc["tail"] and j == own - 1) else new_state()
            word_arc(u, v, int(sc["words"][j]), sc["eps"][1] if (sc["eps"] and sc["eps"][0] == j) else None)
            u = v
        if sc["tail"]:
            assert tuple(sc["words"][own:]) == TAIL
            u = tail2
        else:
            finals[u] = wt()
        ends.append(u)
    return synth.graph_from_arc_lists(n_states, 0, arcs, finals), n_tid, ends


def make_loglikes(n_tid, seed):
    """float32[N_WORDS][n_tid + 1]: a column per transition id (no tid2pdf), continuous values -- exact ties do not happen, and the
    tests assert that they did not"""
    return np.random.default_rng([int(seed), 0x11]).normal(-1.5, 1.0, size=(N_WORDS, n_tid + 1)).astype(np.float32)


WIDE = dict(beam=400.0, max_active=1000000, min_active=0, lattice_beam=400.0)   # nothing is pruned: every script stays in the lattice


def write_models(d, seed=0):
    """The edge LMs and the script graph as files under directory d (a pathlib.Path): dict(lms {name: NgramLm}, fsa {name: Fsa},
    paths {name: str}, scripts, graph, gpath, n_tid, ends).  LM names: clusterA, clusterB, deep, unigram."""
    lms = dict(clusterA=cluster_lm(10 + seed), clusterB=cluster_lm(20 + seed), deep=deep_lm(30 + seed), unigram=unigram_lm(40 + seed))
    fsa = {k: lm.to_fsa() for k, lm in lms.items()}
    paths = {}
    for k, f in fsa.items():
        paths[k] = str(d / (k + ".lm"))
        f.write(paths[k])
    scripts = edge_scripts(lms["clusterA"], lms["clusterB"], seed)
    graph, n_tid, ends = script_graph(scripts, seed)
    gpath = str(d / "scripts.graph")
    graph.write(gpath)
    return dict(lms=lms, fsa=fsa, paths=paths, scripts=scripts, graph=graph, gpath=gpath, n_tid=n_tid, ends=ends)


PAIRS = [("clusterA", "deep"), ("deep", "clusterB"), ("unigram", "clusterA"), ("clusterA", "clusterB")]   # (old at -1, new at 1)
