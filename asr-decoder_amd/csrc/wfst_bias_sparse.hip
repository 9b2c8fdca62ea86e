// Phrase boosting for large lists (wfst_decoder_biased_words_sparse): bias_kernel's sweep (wfst_bias.hip) over the cells a path can
// actually reach.  Along one path the phrase automaton is in exactly one node and most lattice words are in no phrase, so of the
// states x nodes cells of the dense table all but a small multiple of the states are +inf.  R(t), the nodes a path into lattice
// state t can be in, does not depend on the settings:  R(0) = {0};  over an in-arc s -> t that is an arc R(t) takes R(s) where the
// arc has no word and {delta(i, olabel) : i in R(s)} where it has one;  R is the least such family (the lattice is a DAG).  v[t][j]
// finite implies j in R(t), so the table restricted to R holds the dense table's bits under the same recurrence.
//
// bias_reach_kernel, one workgroup per slot, once per call and shared by the settings: frames in ascending order over the in-arc
// index (align_index_kernel's, AlignDev::idx).  Per frame: the in-arcs' edge counts |R(source)| by a scan (that is the upper bound of
// the frame's candidates, and the edges' CSR), the candidates delta(i, word) written where the edges will stand, per state the
// candidates sorted and made unique, the sets packed behind the earlier frames' (so cell ids run in (state, node) order), the
// candidates replaced by their local index in the destination's set.  A frame with arcs between its own states repeats this with
// all its in-arcs until no set grows -- sets only grow, so an equal size is an equal set -- with rescale_kernel's bound: more rounds
// than the frame has states is a cycle.  A region that is too small ends the pass with kReachOverCells / kReachOverEdges; the host
// launches again with a larger one.  Integer work only; every loop is bounded by the lattice's, the book's and the regions' sizes.
//
// bias_sparse_kernel, one workgroup per (slot, setting): bias_kernel's shape.  The cells of a frame are one contiguous range; a cell
// PULLS its minimum over its state's in-arcs, from the source cells whose stored edge is the cell's local index.  No atomic on a
// cost, no backpointers, delta is never evaluated in the sweep.  Wave 0 picks the end, walks back by exact equality (the first
// qualifying source cell of an arc is the least node: sets ascend) and reads the path forwards as bias_kernel does, recomputing the
// node track from the automaton itself (goto / fail): a hop whose node differs from the traced cell's is kAlnInternal, which ties the
// reach pass to the definition on every call.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wfst_align_index.h"   // AlnIndex / aln_carve, aln_wave_min_64
#include "wfst_device.h"

namespace wfst {
namespace {

typedef unsigned long long u64;
constexpr int kSpThreads = 256;
constexpr int kSpSmallSet = 16;   // candidates of a state one lane sorts alone; above, the workgroup ranks them together

__device__ __forceinline__ double sp_load(const double *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void sp_store(double *p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ int32_t sp_iload(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void sp_istore(int32_t *p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// the cost expressions: bias_kernel's, word for word (wfst_bias.hip)
__device__ __forceinline__ double sp_arc_cost(double gs, double as, double wip, int32_t graph_bits, int32_t ac_bits, int32_t olabel) {
#pragma clang fp contract(off)
  const double g = gs * (double)__int_as_float(graph_bits);
  const double a = as * (double)__int_as_float(ac_bits);
  const double scaled = g + a;
  return scaled + (olabel != 0 ? wip : 0.0);
}
__device__ __forceinline__ double sp_bonus(double bs, double beta, int32_t olabel) {
#pragma clang fp contract(off)
  const double r = bs * beta;
  return olabel != 0 ? r : 0.0;
}
__device__ __forceinline__ double sp_biased(double c, double r) {
#pragma clang fp contract(off)
  const double d = c - r;
  return d;
}
__device__ __forceinline__ bool sp_is_arc(int32_t graph_bits, int32_t ac_bits) {
  const float s = __int_as_float(graph_bits) + __int_as_float(ac_bits);
  return s - s == 0.0f;
}
__device__ __forceinline__ bool sp_extend(double src, double d, double *out) {
#pragma clang fp contract(off)
  const double sum = src + d;
  const double v = sum + 0.0;   // (+ 0.0: a zero total is +0)
  *out = v;
  return v - v == 0.0;
}

// ---- a slot's book ----------------------------------------------------------------------------------------------------------------
struct Book {
  int J, W;   // J = 1, W = 0: no book
  const int32_t *word, *fail, *phrase, *first_child, *n_child, *words;
  const double *beta;
};
__device__ __forceinline__ Book sp_book(const BiasBooksDev &B, int book) {
  Book K = {1, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  if (book < 0) return K;
  const int32_t *H = B.hdr + (size_t)book * kBookHdr;
  K.J = H[0];
  K.W = H[1];
  const int32_t *I = B.ints + H[2];
  K.word = I; K.fail = I + K.J; K.phrase = I + 2 * (size_t)K.J; K.first_child = I + 3 * (size_t)K.J; K.n_child = I + 4 * (size_t)K.J;
  K.words = I + 5 * (size_t)K.J;
  K.beta = B.beta + H[3];
  return K;
}
__device__ __forceinline__ double sp_beta(const Book &K, int j) { return K.W ? K.beta[j] : 0.0; }
// the first index of a[lo, hi) that is not below w (ascending)
__device__ __forceinline__ int sp_lower(const int32_t *a, int lo, int hi, int32_t w) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < w) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// the last index x of a[lo, hi] with a[x] <= v (a ascending, a[lo] <= v)
__device__ __forceinline__ int sp_owner(const int32_t *a, int lo, int hi, int32_t v) {
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (a[mid] <= v) lo = mid; else hi = mid - 1;
  }
  return lo;
}
// delta(i, w), w != 0: the child over w of the first of i, fail(i), ... that has one, the root if none has (at most 16 links: a
// failure link is shallower than its node).  A word in no phrase leads to the root from every node.
__device__ __forceinline__ int sp_delta(const Book &K, int i, int32_t w) {
  if (K.W == 0) return 0;
  const int at = sp_lower(K.words, 0, K.W, w);
  if (at >= K.W || K.words[at] != w) return 0;
  for (int hop = 0; hop <= 16; ++hop) {
    const int c0 = K.first_child[i], c1 = c0 + K.n_child[i];
    const int c = sp_lower(K.word, c0, c1, w);
    if (c < c1 && K.word[c] == w) return c;
    if (i == 0) return 0;
    i = K.fail[i];
  }
  return 0;
}

// exclusive scan of one value per lane over the workgroup, and the total; s_w: 4 words of LDS
__device__ __forceinline__ long long sp_scan(long long v, long long *total, long long *s_w) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long long incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const long long o = __shfl_up(incl, d, 64);
    if (lane >= d) incl += o;
  }
  if (lane == 63) s_w[wave] = incl;
  __syncthreads();
  long long before = 0, all = 0;
  for (int w = 0; w < kSpThreads / 64; ++w) {
    if (w < wave) before += s_w[w];
    all += s_w[w];
  }
  __syncthreads();
  *total = all;
  return before + incl - v;
}

struct Region {
  int32_t *roff, *ncnt, *eoff, *rnode, *rstate, *edge, *stage;
  int64_t cell_cap, edge_cap;
};
__device__ __forceinline__ Region sp_region(const BiasReachDev &Q, const AlignDev &A, int slot) {
  Region G;
  G.cell_cap = Q.reg[4 * slot + 1];
  G.edge_cap = Q.reg[4 * slot + 2];
  G.roff = Q.ints + Q.reg[4 * slot];
  G.ncnt = G.roff + A.ns_cap + 1;
  G.eoff = G.ncnt + A.ns_cap;
  G.rnode = G.eoff + A.na_cap + 1;
  G.rstate = G.rnode + G.cell_cap;
  G.edge = G.rstate + G.cell_cap;
  G.stage = G.edge + G.edge_cap;
  return G;
}

}  // namespace

__global__ __launch_bounds__(kSpThreads) void bias_reach_kernel(AlignDev A, BiasReachDev Q) {
  const int slot = blockIdx.x, tid = threadIdx.x;
  int4 *wa, *wb;
  const AlnIndex X = aln_carve(A, slot, &wa, &wb);
  const Region G = sp_region(Q, A, slot);
  int32_t *head = Q.head + (size_t)slot * kReachHead;
  __shared__ long long s_w[kSpThreads / 64];
  __shared__ int s_max;
  const int status = X.head[0];
  if (status || G.cell_cap <= 0 || G.edge_cap <= 0) {   // no lattice to look at (the sweep reports it), or not asked for
    if (tid < kReachHead) head[tid] = tid == 0 ? (status ? status : kReachSkipped) : 0;
    return;
  }
  if (tid == 0) s_max = 0;
  const Book K = sp_book(Q.B, Q.book_of[slot]);
  const int nd = X.head[3];
  long long cbase = 0, ebase = 0;   // the cells and the edges of the finished frames
  int err = 0;
  for (int f = 0; f <= nd && !err; ++f) {
    const int b = X.fbeg[f], e = X.fend[f];
    if (e <= b) continue;
    const int a_lo = X.off[b], a_hi = X.off[e];
    const bool eps_frame = X.feps[f] != 0;
    long long cend = cbase, eend = ebase;
    for (int round = 0;; ++round) {
      // ---- 1. the arcs' edge counts and where their edges stand: round 0 takes the emitting in-arcs, whose sources are finished;
      //         the later rounds every in-arc, the sources inside the frame as the round before left them
      long long run = ebase;
      for (int base = a_lo; base < a_hi; base += kSpThreads) {
        const int a = base + tid;
        long long n = 0;
        if (a < a_hi) {
          const int4 R = X.recA[a];
          if (sp_is_arc(R.z, R.w) && (R.x >= 0 || round > 0)) {
            const int src = R.x & 0x7FFFFFFF;
            n = G.roff[src + 1] - G.roff[src];
          }
        }
        long long total;
        const long long at = sp_scan(n, &total, s_w);
        if (run + total > G.edge_cap) { err = kReachOverEdges; break; }
        if (a < a_hi) G.eoff[a] = (int32_t)(run + at);
        run += total;
      }
      if (err) break;
      if (tid == 0) G.eoff[a_hi] = (int32_t)run;
      eend = run;
      __syncthreads();
      // ---- 2. the candidates: the node every source cell goes to over its arc, where the edge will stand -----------------------------
      for (long long x = ebase + tid; x < eend; x += kSpThreads) {
        const int a = sp_owner(G.eoff, a_lo, a_hi - 1, (int32_t)x);
        const int4 R = X.recA[a];
        const int src = R.x & 0x7FFFFFFF;
        const int i = G.rnode[G.roff[src] + (int)(x - G.eoff[a])];
        G.edge[x] = R.y == 0 ? i : sp_delta(K, i, R.y);
      }
      __syncthreads();
      // ---- 3. per state the candidates sorted and made unique, into the state's place of the stage (its candidates + one) -----------
      bool large = false;
      for (int t = b + tid; t < e; t += kSpThreads) {
        const int lo = G.eoff[X.off[t]], hi = G.eoff[X.off[t + 1]];
        int32_t *out = G.stage + (lo - ebase) + (t - b);
        int m = 0;
        if (t == 0) out[m++] = 0;   // R(0) holds the root (every arc goes to a higher state: state 0 has no in-arc)
        if (hi - lo > kSpSmallSet) {
          large = true;
        } else {
          for (int x = lo; x < hi; ++x) {   // insertion into the ascending set
            const int32_t c = G.edge[x];
            int at = m;
            while (at > 0 && out[at - 1] > c) --at;
            if (at > 0 && out[at - 1] == c) continue;
            for (int y = m; y > at; --y) out[y] = out[y - 1];
            out[at] = c;
            ++m;
          }
          G.ncnt[t] = m;
        }
      }
      if (__syncthreads_or(large)) {
        for (int t = b; t < e; ++t) {   // (uniform: every lane reads the same bounds)
          const int lo = G.eoff[X.off[t]], hi = G.eoff[X.off[t + 1]];
          if (hi - lo <= kSpSmallSet) continue;
          int32_t *out = G.stage + (lo - ebase) + (t - b);
          // a candidate that has an equal one before it is marked (bit 31; a node id has 16 bits) ...
          for (int x = lo + tid; x < hi; x += kSpThreads) {
            const int32_t c = sp_iload(&G.edge[x]) & 0x7FFFFFFF;
            bool dup = false;
            for (int y = lo; y < x && !dup; ++y) dup = (sp_iload(&G.edge[y]) & 0x7FFFFFFF) == c;
            if (dup) sp_istore(&G.edge[x], c | (int32_t)0x80000000);
          }
          __syncthreads();
          // ... and the others go to their rank among themselves
          int mine = 0;
          for (int x = lo + tid; x < hi; x += kSpThreads) {
            const int32_t c = G.edge[x];
            if (c < 0) continue;
            int rank = t == 0 ? 1 : 0;
            for (int y = lo; y < hi; ++y) {
              const int32_t o = G.edge[y];
              rank += o >= 0 && o < c;
            }
            out[rank] = c;
            ++mine;
          }
          long long total;
          sp_scan(mine, &total, s_w);   // (its barriers also stand between the states' passes)
          if (tid == 0) G.ncnt[t] = (int)total + (t == 0 ? 1 : 0);
        }
      }
      __syncthreads();
      // ---- 4. the frame's sets packed behind the finished frames' ------------------------------------------------------------------
      int grew = 0;
      long long crun = cbase;
      for (int base = b; base < e; base += kSpThreads) {
        const int t = base + tid;
        const int n = t < e ? G.ncnt[t] : 0;
        if (t < e && round > 0 && n != G.roff[t + 1] - G.roff[t]) grew = 1;
        long long total;
        const long long at = sp_scan(n, &total, s_w);   // (its barriers stand between the old sizes' loads and the stores)
        if (crun + total > G.cell_cap) { err = kReachOverCells; cend = crun + total; break; }
        if (t < e) G.roff[t] = (int32_t)(crun + at);
        crun += total;
      }
      if (err) break;
      if (tid == 0) G.roff[e] = (int32_t)crun;
      cend = crun;
      __syncthreads();
      int most = 0;
      for (int t = b + tid; t < e; t += kSpThreads) {
        const int32_t *in = G.stage + (G.eoff[X.off[t]] - ebase) + (t - b);
        const int c0 = G.roff[t], n = G.ncnt[t];
        for (int k = 0; k < n; ++k) { G.rnode[c0 + k] = in[k]; G.rstate[c0 + k] = t; }
        most = max(most, n);
      }
      if (most) atomicMax(&s_max, most);
      grew = __syncthreads_or(grew);
      if (!eps_frame || (round > 0 && !grew)) break;
      if (round > e - b) { err = kAlnCycle; break; }   // a path inside the frame visits a state once
    }
    if (err) { cbase = cend; break; }
    // ---- 5. the candidates become the local index of their cell in the destination's set ------------------------------------------
    for (long long x = ebase + tid; x < eend; x += kSpThreads) {
      const int a = sp_owner(G.eoff, a_lo, a_hi - 1, (int32_t)x);
      const int t = sp_owner(X.off, b, e - 1, a);
      const int32_t c = G.edge[x] & 0x7FFFFFFF;
      const int c0 = G.roff[t], c1 = G.roff[t + 1];
      const int at = sp_lower(G.rnode, c0, c1, c);
      G.edge[x] = at < c1 && G.rnode[at] == c ? at - c0 : -1;   // (-1: never expected; the sweep then finds no source)
    }
    cbase = cend;
    ebase = eend;
    __syncthreads();
  }
  __syncthreads();
  if (tid == 0) {
    head[0] = err;
    head[1] = (int32_t)min(cbase, (long long)INT32_MAX);
    head[2] = (int32_t)ebase;
    head[3] = s_max;
    head[4] = 0; head[5] = 0; head[6] = 0; head[7] = 0;
  }
}

__global__ __launch_bounds__(kSpThreads) void bias_sparse_kernel(AlignDev A, BiasSparseDev Q, BiasSet S, const int32_t *chans) {
  const int pair = blockIdx.x, pos = pair / Q.n_set, q = pair % Q.n_set, slot = Q.slot_of[pos], c = chans[slot];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int4 *wa, *wb;
  const AlnIndex X = aln_carve(A, slot, &wa, &wb);
  const Region G = sp_region(Q.R, A, slot);
  const int cap = Q.cap_words, cap_hits = Q.cap_hits;
  int32_t *o = Q.out + (size_t)pair * bias_out_ints(cap, cap_hits);
  int32_t *o_words = o + kBiasHead, *o_begin = o_words + cap, *o_end = o_begin + cap, *o_hit_phrase = o_end + cap, *o_hit_word = o_hit_phrase + cap_hits;
  const int64_t cell0 = Q.cell_off[pair];
  const int status = X.head[0], reach = Q.R.head[(size_t)slot * kReachHead];
  if (cell0 < 0 || status || reach) {   // not asked for, no lattice to look at, or no sets
    if (tid < kBiasHead) o[tid] = tid == 4 && cell0 >= 0 && status != kAlnNoLattice ? (status ? status : reach) : 0;
    return;
  }
  __shared__ int s_err;
  if (tid == 0) s_err = 0;
  __syncthreads();
  const Book K = sp_book(Q.R.B, Q.R.book_of[slot]);
  const double gs = S.v[4 * q], as = S.v[4 * q + 1], wip = S.v[4 * q + 2], bs = S.v[4 * q + 3];
  const double unreached = __longlong_as_double(0x7FF0000000000000ll);
  const int nt = X.head[1], nd = X.head[3];
  double *v = Q.cells + cell0;
  const int4 *toks = Q.lat_toks + (size_t)c * Q.lat_tok_cap;
  // ---- the cells, frame by frame -------------------------------------------------------------------------------------------
  for (int f = 0; f <= nd; ++f) {
    const int b = X.fbeg[f], e = X.fend[f];
    if (e <= b) continue;
    const int c_lo = G.roff[b], c_hi = G.roff[e];
    const bool eps_frame = X.feps[f] != 0;
    for (int round = 0;; ++round) {
      int moved = 0;
      for (int x = c_lo + tid; x < c_hi; x += kSpThreads) {
        const int t = G.rstate[x], j = G.rnode[x], local = x - G.roff[t];
        const double old = round ? sp_load(&v[x]) : (x == 0 ? 0.0 : unreached);   // (cell 0 is (state 0, the root))
        double best = old;
        const double beta = sp_beta(K, j);
        const int a1 = X.off[t + 1];
        for (int a = X.off[t]; a < a1; ++a) {
          const int4 R = X.recA[a];
          if ((R.x < 0) != (round > 0)) continue;   // round 0: the emitting in-arcs; later rounds: the arcs inside the frame
          if (!sp_is_arc(R.z, R.w)) continue;
          const int src = R.x & 0x7FFFFFFF;
          const int s0 = G.roff[src], n = G.roff[src + 1] - s0;
          const int32_t *edge = G.edge + G.eoff[a];
          const double d = sp_biased(sp_arc_cost(gs, as, wip, R.z, R.w, R.y), sp_bonus(bs, beta, R.y));
          for (int k = 0; k < n; ++k) {
            if (edge[k] != local) continue;
            double y;
            if (sp_extend(sp_load(&v[s0 + k]), d, &y)) best = y < best ? y : best;
          }
        }
        if (round == 0 || best < old) { sp_store(&v[x], best); moved = 1; }
      }
      moved = __syncthreads_or(moved);   // (the barrier also orders this round's stores before the next round's loads)
      if (!eps_frame || (round > 0 && !moved)) break;
      if (round > e - b) {
        if (tid == 0) s_err = kAlnCycle;
        break;
      }
    }
  }
  __syncthreads();
  if (wave != 0) return;
  if (s_err) {
    if (lane < kBiasHead) o[lane] = lane == 4 ? s_err : 0;
    return;
  }
  // ---- the end: the (final state, node) with the least v, then the least graph state, then the least node, then the state ---------
  int t = -1, j = 0, x_at = 0;
  {
    double mine = unreached;
    u64 mine1 = ~0ull, mine2 = ~0ull;
    for (int i = X.fbeg[nd] + lane; i < X.fend[nd]; i += 64) {
      const int4 tk = toks[i];
      if (!((tk.w >> 30) & 1)) continue;
      for (int k = G.roff[i]; k < G.roff[i + 1]; ++k) {
        const double x = v[k];
        if (!(x < unreached)) continue;
        const u64 x1 = ((u64)(uint32_t)tk.y << 32) | (uint32_t)G.rnode[k], x2 = ((u64)(uint32_t)i << 32) | (uint32_t)k;
        if (x < mine || (x == mine && (x1 < mine1 || (x1 == mine1 && x2 < mine2)))) { mine = x; mine1 = x1; mine2 = x2; }
      }
    }
    double best = mine;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const double other = __shfl_xor(best, m, 64);
      best = other < best ? other : best;
    }
    if (best < unreached) {
      const u64 m1 = aln_wave_min_64(mine == best ? mine1 : ~0ull);
      const u64 m2 = aln_wave_min_64(mine == best && mine1 == m1 ? mine2 : ~0ull);
      t = (int)(uint32_t)(m2 >> 32);
      x_at = (int)(uint32_t)m2;
      j = (int)(uint32_t)m1;
    }
  }
  if (t < 0) {   // no final state is reached
    if (lane < kBiasHead) o[lane] = 0;
    return;
  }
  const double end_cost = v[x_at];
  const int end_node = j;
  // ---- the walk back: exact equality, the tie rule ---------------------------------------------------------------------------
  int32_t *path = Q.path + (size_t)pair * 2 * Q.path_cap, *pnode = path + Q.path_cap;
  int n = 0, err = 0;
  while (t != 0) {
    if (n >= nt || n >= Q.path_cap) { err = kAlnInternal; break; }
    const double here = v[x_at];
    const int local = x_at - G.roff[t];
    const double beta = sp_beta(K, j);
    const int a0 = X.off[t], a1 = X.off[t + 1];
    u64 k1 = ~0ull, k2 = ~0ull;
    uint32_t k3 = 0xFFFFFFFFu;
    int my_a = -1, my_src = 0, my_node = 0, my_x = 0;
    for (int a = a0 + lane; a < a1; a += 64) {
      const int4 R = X.recA[a];
      if (!sp_is_arc(R.z, R.w)) continue;
      const int src = R.x & 0x7FFFFFFF;
      const int s0 = G.roff[src], ns = G.roff[src + 1] - s0;
      const int32_t *edge = G.edge + G.eoff[a];
      const double d = sp_biased(sp_arc_cost(gs, as, wip, R.z, R.w, R.y), sp_bonus(bs, beta, R.y));
      // the least source node that qualifies over this arc: the first, the sets ascend
      int at = -1;
      double y;
      for (int k = 0; k < ns && at < 0; ++k)
        if (edge[k] == local && sp_extend(v[s0 + k], d, &y) && y == here) at = s0 + k;
      if (at < 0) continue;
      const int node = G.rnode[at];
      const int4 B = X.recB[a];
      const u64 c1 = ((u64)(R.x < 0 ? 1 : 0) << 63) | ((u64)(uint32_t)B.x << 32) | (uint32_t)B.y;
      const u64 c2 = ((u64)(uint32_t)R.y << 32) | (uint32_t)R.z;
      const uint32_t c3 = (uint32_t)R.w;
      if (my_a < 0 || c1 < k1 || (c1 == k1 && (c2 < k2 || (c2 == k2 && (c3 < k3 || (c3 == k3 && node < my_node)))))) {
        k1 = c1; k2 = c2; k3 = c3; my_a = a; my_src = src; my_node = node; my_x = at;
      }
    }
    u64 cand = __ballot(my_a >= 0);
    if (!cand) { err = kAlnInternal; break; }   // (a reached cell without the arrival that made it: never expected)
    if (__popcll(cand) > 1) {
      const u64 m1 = aln_wave_min_64(my_a >= 0 ? k1 : ~0ull);
      const bool at1 = my_a >= 0 && k1 == m1;
      const u64 m2 = aln_wave_min_64(at1 ? k2 : ~0ull);
      const bool at2 = at1 && k2 == m2;
      const u64 m3 = aln_wave_min_64(at2 ? ((u64)k3 << 32) | (uint32_t)my_node : ~0ull);
      cand = __ballot(at2 && (((u64)k3 << 32) | (uint32_t)my_node) == m3);
    }
    const int win = __ffsll((long long)cand) - 1;
    const int a = __shfl(my_a, win, 64);
    if (lane == 0) { path[n] = a; pnode[n] = j; }
    ++n;
    t = __shfl(my_src, win, 64);
    j = __shfl(my_node, win, 64);
    x_at = __shfl(my_x, win, 64);
  }
  if (!err && j != 0) err = kAlnInternal;   // (state 0 is reached at the root alone)
  if (err) {
    if (lane < kBiasHead) o[lane] = lane == 4 ? err : 0;
    return;
  }
  // ---- front to back: the node track from the automaton itself, the sums in hop order, the words, their times and the hits ----------
  // (lane 0's stores to path[] are read back by the other lanes: one wave, in program order behind the stores' completion)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  float lm = 0.0f, tot = 0.0f;
  double cost = 0.0, bonus = 0.0;
  int kw = 0, n_hits = 0, node = 0, end_c = 0, begin_c = 0;
  for (int base = 0; base < n; base += 64) {
    const int m = min(64, n - base);
    int4 R = make_int4(0, 0, 0, 0), B = make_int4(0, 0, 0, 0);
    int traced = 0;
    if (lane < m) {
      const int a = path[n - 1 - (base + lane)];
      traced = pnode[n - 1 - (base + lane)];
      R = X.recA[a];
      B = X.recB[a];
    }
    const bool eps = R.x < 0;
    const bool sil = Q.sil_bits && B.y > 0 && B.y <= Q.n_tid && ((Q.sil_bits[B.y >> 5] >> (B.y & 31)) & 1u);
    const int endv = (lane < m && !eps && !sil) ? B.z + 1 : 0;
    for (int h = 0; h < m; ++h) {
      const int word = __shfl(R.y, h, 64), F = __shfl(B.z, h, 64), ev = __shfl(endv, h, 64);
      const int gb = __shfl(R.z, h, 64), ab = __shfl(R.w, h, 64);
      const float g = __int_as_float(gb);
      lm += g;
      tot = (tot + (g + __int_as_float(ab))) + 0.0f;
      if (word != 0) node = sp_delta(K, node, word);
      if (node != __shfl(traced, h, 64)) err = kAlnInternal;   // (the sets and edges must follow the automaton)
      const double r = sp_bonus(bs, sp_beta(K, node), word);
      sp_extend(cost, sp_biased(sp_arc_cost(gs, as, wip, gb, ab, word), r), &cost);
      bonus = bonus + r;
      if (word != 0) {
        if (lane == 0 && kw >= 1 && kw <= cap) o_end[kw - 1] = max(end_c, begin_c);
        if (lane == 0 && kw < cap) { o_words[kw] = word; o_begin[kw] = F; }
        begin_c = F;
        for (int x = node; x != 0; x = K.fail[x]) {   // every phrase that ends here, the longest first
          const int p = K.phrase[x];
          if (p < 0) continue;
          if (lane == 0 && n_hits < cap_hits) { o_hit_phrase[n_hits] = p; o_hit_word[n_hits] = kw; }
          ++n_hits;
        }
        ++kw;
      }
      end_c = max(end_c, ev);
    }
  }
  // (the path read forwards must reproduce the cell it was traced from)
  if (cost != end_cost || node != end_node) err = kAlnInternal;
  if (lane == 0) {
    if (!err && kw >= 1 && kw <= cap) o_end[kw - 1] = max(end_c, begin_c);
    const long long cb = __double_as_longlong(end_cost), bb = __double_as_longlong(bonus);
    o[0] = err ? 0 : 1; o[1] = n; o[2] = __float_as_int(tot); o[3] = __float_as_int(lm); o[4] = err;
    o[5] = kw; o[6] = n_hits; o[7] = 0; o[8] = (int32_t)(uint32_t)cb; o[9] = (int32_t)(uint32_t)((u64)cb >> 32);
    o[10] = (int32_t)(uint32_t)bb; o[11] = (int32_t)(uint32_t)((u64)bb >> 32); o[12] = 0; o[13] = 0; o[14] = 0; o[15] = 0;
  }
}

void launch_bias_reach(const AlignDev &A, const BiasReachDev &Q, int cnt, hipStream_t s) {
  hipLaunchKernelGGL(bias_reach_kernel, dim3(cnt), dim3(kSpThreads), 0, s, A, Q);
}

void launch_bias_sparse(const AlignDev &A, const BiasSparseDev &Q, const BiasSet &S, const int32_t *chans, int cnt, hipStream_t s) {
  hipLaunchKernelGGL(bias_sparse_kernel, dim3(cnt * Q.n_set), dim3(kSpThreads), 0, s, A, Q, S, chans);
}

}  // namespace wfst
