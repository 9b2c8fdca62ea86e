"""The tie rule stated a second time, in numpy float32, straight from its definition (deviation 3) -- no
hash list, no queue, no visiting order.  tests/test_oracle_ties.py holds the C oracle's tie mode to it.

Beam-only pruning (max_active unbounded, min_active 0) and a lattice beam so wide that no forward link is ever pruned:
  frame loop   a token is expanded if its cost <= best + beam; an emitting arrival costs (cost + (-loglike)) + graph cost;
               next_cutoff = min over all arrivals of (arrival + beam); arrivals below it are admitted; a token's cost is the
               minimum of its admitted arrivals;
  closure      to a fixpoint: from every token below the cutoff, every epsilon arc whose arrival cost + graph cost is below the
               cutoff; a token's cost is the minimum over all its arrivals;
  post-pass    every token's backpointer is recomputed as the arg-min, over ALL arrivals (from the final costs) that equal the
               token's final cost, of (emitting before epsilon, arc index, biglm: source pair key old | new << 32);
  end          the cheapest (final, if asked for and there is one) token, then the lowest graph state, then the lowest pair key;
  report       a hop bp -> tok is reported with the LAST of bp's admitted arcs of that kind into tok (GetBestPath takes the first
               forward link, links are prepended in arc order).
biglm: graph cost = arc weight + LM score of the pair's two components (the fixed DiffArpaLm), keys are (state, pair)."""
import numpy as np

f32 = np.float32
INF = f32(np.inf)


class Rule:
    def __init__(self, g, beam, lm1=None, lm2=None):
        self.g, self.beam, self.lm1, self.lm2 = g, f32(beam), lm1, lm2
        n = np.asarray([int(x[0]) for x in g.state_info], np.int64)
        self.off = np.concatenate([[0], np.cumsum(n)])
        self.cache = {}
        self.pair0 = (lm1.start(), lm2.start()) if lm1 else (0, 0)

    def arcs_of(self, s):
        return range(int(self.off[s]), int(self.off[s + 1]))

    def step(self, pair, ol):
        """(next pair, LM score) of DiffArpaLm::GetArc on the pair's components"""
        if self.lm1 is None or ol == 0:
            return pair, f32(0.0)
        k = (pair, ol)
        if k not in self.cache:
            n1, w1 = self.lm1.getarc_many([pair[0]], [ol])
            n2, w2 = self.lm2.getarc_many([pair[1]], [ol])
            self.cache[k] = ((int(n1[0]), int(n2[0])), f32(f32(w1[0]) + f32(w2[0])))
        return self.cache[k]

    def gcost(self, a, pair):
        A = self.g.arcs[a]
        npair, ls = self.step(pair, int(A["olabel"]))
        return npair, (f32(A["w"]) if self.lm1 is None else f32(f32(A["w"]) + ls))

    @staticmethod
    def pk(pair):
        return pair[0] | (pair[1] << 32)

    def closure(self, cost, arr, cutoff):
        """cost: {key: f32}; appends the epsilon arrivals from the FINAL costs to arr: {key: [(cost, class, arc, source key)]}"""
        changed = True
        while changed:
            changed = False
            for (s, pair), c in list(cost.items()):
                if not c < cutoff:
                    continue
                for a in self.arcs_of(s):
                    if int(self.g.arcs[a]["ilabel"]) != 0:
                        continue
                    npair, gc = self.gcost(a, pair)
                    tot = f32(c + gc)
                    k = (int(self.g.arcs[a]["to"]), npair)
                    if tot < cutoff and tot < cost.get(k, INF):
                        cost[k] = tot
                        changed = True
        for (s, pair), c in cost.items():
            if not c < cutoff:
                continue
            for a in self.arcs_of(s):
                if int(self.g.arcs[a]["ilabel"]) != 0:
                    continue
                npair, gc = self.gcost(a, pair)
                tot = f32(c + gc)
                if tot < cutoff:
                    arr.setdefault((int(self.g.arcs[a]["to"]), npair), []).append((tot, 1, a, (s, pair), True))

    def backpointers(self, cost, arr):
        bp = {}
        for k, c in cost.items():
            eq = [x for x in arr.get(k, []) if x[0] == c]
            if eq:
                w = min(eq, key=lambda x: (x[1], x[2], self.pk(x[3][1])))
                bp[k] = (w[3], w[1])
        return bp

    def decode(self, ll, tid2pdf=None, use_final=True):
        """hops [(ilabel, olabel, graph cost, acoustic cost)] start -> final (hop 0: the root's) and (tot, lm) as LatticeToVector
        sums them; None: no path"""
        g = self.g
        frames = []   # per frame: (cost, arrivals, backpointers)
        cost, arr = {(int(g.start), self.pair0): f32(0.0)}, {}
        self.closure(cost, arr, self.beam)
        frames.append((cost, arr, self.backpointers(cost, arr)))
        for t in range(len(ll)):
            prev = frames[-1][0]
            if not prev:
                return None
            cur_cutoff = f32(min(prev.values()) + self.beam)
            cand = []
            for (s, pair), c in prev.items():
                if not c <= cur_cutoff:
                    continue
                for a in self.arcs_of(s):
                    il = int(g.arcs[a]["ilabel"])
                    if il == 0:
                        continue
                    npair, gc = self.gcost(a, pair)
                    ac = f32(-ll[t, il if tid2pdf is None else tid2pdf[il]])
                    cand.append((f32(f32(c + ac) + gc), 0, a, (s, pair), (int(g.arcs[a]["to"]), npair)))
            next_cutoff = min([f32(x[0] + self.beam) for x in cand], default=INF)
            cost, arr = {}, {}
            for tot, cl, a, src, k in cand:
                if tot < next_cutoff:
                    arr.setdefault(k, []).append((tot, cl, a, src, True))
                    cost[k] = min(cost.get(k, INF), tot)
            self.closure(cost, arr, next_cutoff)
            frames.append((cost, arr, self.backpointers(cost, arr)))
        cost = frames[-1][0]
        if not cost or len(ll) == 0:
            return None
        fin = {k: c for k, c in cost.items() if k[0] == int(g.final_state)}
        if use_final and fin:
            score = {k: (f32(c + f32(0.0)) if self.lm1 is None else f32(c + f32(f32(self.lm1.final(k[1][0])) + f32(self.lm2.final(k[1][1])))))
                     for k, c in fin.items()}
        else:
            score = dict(cost)
        end = min(score, key=lambda k: (score[k], k[0], self.pk(k[1])))
        hops, k, f = [], end, len(frames) - 1
        while True:
            cost, arr, bp = frames[f]
            if k not in bp:
                hops.append((0, 0, f32(0.0), f32(0.0)))
                break
            src, cl = bp[k]
            a = max(x[2] for x in arr[k] if x[3] == src and x[1] == cl)   # the first forward link src -> k: the last such arc
            A = g.arcs[a]
            _, gc = self.gcost(a, src[1])
            ac = f32(0.0) if cl else f32(-ll[f - 1, int(A["ilabel"]) if tid2pdf is None else tid2pdf[int(A["ilabel"])]])
            hops.append((int(A["ilabel"]), int(A["olabel"]), gc, ac))
            k = src
            f -= 0 if cl else 1
        hops.reverse()
        tot = lm = f32(0.0)
        for il, ol, gc, ac in hops:
            lm = f32(lm + gc)
            tot = f32(tot + f32(gc + ac))
        return hops, tot, lm
