// Phrase boosting (wfst_decoder_biased_words): the best path of a channel's raw lattice picked again under new scales, a word penalty
// and a per-channel list of boosted phrases, for n_set settings per listed channel, without decoding again.  rescale_kernel's sweep
// (wfst_rescale.hip) over the product of the lattice and the list's phrase automaton, over the same in-arc index
// (align_index_kernel's, AlignDev::idx).
//
// A cell is (lattice state t, node j of the automaton), v[t][j] float64.  Along a path the node starts at the root and moves by
// delta(node, olabel) on a word arc (olabel != 0); an arc costs d = c_q(a) - r with c_q(a) rescale_kernel's and r = bs * beta(node
// reached) on a word arc, 0.0 otherwise -- the product and the difference rounded one by one (#pragma clang fp contract(off)).
// v[0][0] = +0; v[t][j] = the minimum over the in-arcs s -> t and the source nodes i whose step over the arc gives j of
// (v[s][i] + d) + 0.0.  A minimum does not depend on the order it is taken in: the cells are bit for bit whatever the order of the
// index.
//
// bias_kernel, one workgroup per (channel, setting):
//  - the list's automaton is staged in LDS (a node's last word, beta, the offsets of its predecessor lists, the distinct words); the
//    predecessor lists, the failure links and the byte table delta(i, word) stay in global memory, read-only and shared by the pairs.
//  - frames in ascending order, one lane per cell of the frame, strided.  A cell PULLS its minimum: over an arc without a word from
//    (s, j); over a word arc into j != 0 only where the word is j's last, from the host-built list {i : delta(i, word(j)) = j}; into
//    the root from every i the table sends to the root.  The emitting in-arcs leave finished frames: one pass and a barrier, no
//    atomic on a cost, no backpointers.
//  - a frame with arcs between its own states repeats the pass over those arcs until nothing moves, as rescale_kernel does and
//    with its bound: a path inside the frame visits a lattice state once.
//  - wave 0 picks the end, walks back by exact equality under align_kernel's arc tuple and then the least source node, and reads
//    the path front to back: words, times, the sums in hop order and the hits along the chains node, fail(node), ...
// The cells other lanes may be writing in the same pass are read and written by relaxed 64-bit atomics: plain vector loads and
// stores that cannot tear; either value is a valid bound.  Every loop is bounded by the lattice's and the list's own sizes; nothing
// waits for another workgroup.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wfst_align_index.h"   // AlnIndex / aln_carve, aln_wave_min_64
#include "wfst_device.h"

namespace wfst {
namespace {

typedef unsigned long long u64;
constexpr int kBsThreads = 256;

__device__ __forceinline__ double bs_load(const double *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void bs_store(double *p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// c_q(a), as rescale_kernel takes it: the products and sums rounded one by one
__device__ __forceinline__ double bs_arc_cost(double gs, double as, double wip, int32_t graph_bits, int32_t ac_bits, int32_t olabel) {
#pragma clang fp contract(off)
  const double g = gs * (double)__int_as_float(graph_bits);
  const double a = as * (double)__int_as_float(ac_bits);
  const double scaled = g + a;
  return scaled + (olabel != 0 ? wip : 0.0);
}
// r of an arc that reaches a node of this beta: the product is rounded before it is subtracted
__device__ __forceinline__ double bs_bonus(double bs, double beta, int32_t olabel) {
#pragma clang fp contract(off)
  const double r = bs * beta;
  return olabel != 0 ? r : 0.0;
}
__device__ __forceinline__ double bs_biased(double c, double r) {
#pragma clang fp contract(off)
  const double d = c - r;
  return d;
}
// an arc whose float32 graph + acoustic is not finite is no arc
__device__ __forceinline__ bool bs_is_arc(int32_t graph_bits, int32_t ac_bits) {
  const float s = __int_as_float(graph_bits) + __int_as_float(ac_bits);
  return s - s == 0.0f;
}
// the cell reached over an arc of cost d from a source cell src: false where that is no transition
__device__ __forceinline__ bool bs_extend(double src, double d, double *out) {
#pragma clang fp contract(off)
  const double sum = src + d;
  const double v = sum + 0.0;   // (+ 0.0: a zero total is +0)
  *out = v;
  return v - v == 0.0;   // finite (an unreached source is +inf)
}
// the column of a word in the list's table, -1: the word is in no phrase (it leads to the root from every node)
__device__ __forceinline__ int bs_col(const int32_t *words, int W, int32_t w) {
  int lo = 0, hi = W;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (words[mid] < w) lo = mid + 1; else hi = mid;
  }
  return lo < W && words[lo] == w ? lo : -1;
}

}  // namespace

__global__ __launch_bounds__(kBsThreads) void bias_kernel(AlignDev A, BiasDev Q, BiasSet S, const int32_t *chans) {
  const int pair = blockIdx.x, slot = pair / Q.n_set, q = pair % Q.n_set, c = chans[slot];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int4 *wa, *wb;
  const AlnIndex X = aln_carve(A, slot, &wa, &wb);
  const int cap = Q.cap_words, cap_hits = Q.cap_hits;
  int32_t *o = Q.out + (size_t)pair * bias_out_ints(cap, cap_hits);
  int32_t *o_words = o + kBiasHead, *o_begin = o_words + cap, *o_end = o_begin + cap, *o_hit_phrase = o_end + cap, *o_hit_word = o_hit_phrase + cap_hits;
  const int64_t cell0 = Q.cell_off[pair];
  const int status = X.head[0];
  if (cell0 < 0 || status) {   // not asked for, or no lattice to look at
    if (tid < kBiasHead) o[tid] = tid == 4 && cell0 >= 0 && status != kAlnNoLattice ? status : 0;
    return;
  }
  // ---- the slot's automaton ------------------------------------------------------------------------------------------------
  __shared__ int32_t s_word[kBiasMaxNodes], s_poff[kBiasMaxNodes + 1], s_words[kBiasMaxNodes];
  __shared__ double s_beta[kBiasMaxNodes];
  __shared__ int s_err;
  const int list = Q.list_of[slot];
  int J = 1, W = 0;
  const int32_t *g_fail = nullptr, *g_phrase = nullptr, *g_pred = nullptr;
  const uint8_t *g_tab = nullptr;
  if (list >= 0) {
    const int32_t *H = Q.L.hdr + (size_t)list * kBiasHdr;
    J = H[0];
    W = H[1];
    const int32_t *I = Q.L.ints + H[2];
    g_fail = I + J;
    g_phrase = I + 2 * J;
    g_pred = I + 4 * J + 1 + W;
    g_tab = Q.L.table + H[4];
    const double *beta = Q.L.beta + H[3];
    for (int k = tid; k < J; k += kBsThreads) { s_word[k] = I[k]; s_beta[k] = beta[k]; }
    for (int k = tid; k <= J; k += kBsThreads) s_poff[k] = I[3 * J + k];
    for (int k = tid; k < W; k += kBsThreads) s_words[k] = I[4 * J + 1 + k];
  } else if (tid == 0) {
    s_word[0] = 0; s_beta[0] = 0.0; s_poff[0] = 0; s_poff[1] = 0;
  }
  if (tid == 0) s_err = 0;
  __syncthreads();
  const double gs = S.v[4 * q], as = S.v[4 * q + 1], wip = S.v[4 * q + 2], bs = S.v[4 * q + 3];
  const double unreached = __longlong_as_double(0x7FF0000000000000ll);
  const int nt = X.head[1], nd = X.head[3];
  double *v = Q.cells + cell0;
  const int4 *toks = Q.lat_toks + (size_t)c * Q.lat_tok_cap;
  // ---- the cells, frame by frame ---------------------------------------------------------------------------------------
  for (int f = 0; f <= nd; ++f) {
    const int b = X.fbeg[f], e = X.fend[f];
    const int64_t n_cells = (int64_t)(e - b) * J;
    const bool eps_frame = X.feps[f] != 0;
    for (int round = 0;; ++round) {
      int moved = 0;
      for (int64_t x = tid; x < n_cells; x += kBsThreads) {
        const int t = b + (int)(x / J), j = (int)(x % J);
        double *cell = &v[(size_t)t * J + j];
        const double old = round ? bs_load(cell) : (t == 0 && j == 0 ? 0.0 : unreached);
        double best = old;
        const int32_t wj = s_word[j];
        const int a1 = X.off[t + 1];
        for (int a = X.off[t]; a < a1; ++a) {
          const int4 R = X.recA[a];
          if ((R.x < 0) != (round > 0)) continue;   // round 0: the emitting in-arcs; later rounds: the arcs inside the frame
          if (!bs_is_arc(R.z, R.w)) continue;
          const double *src = v + (size_t)(R.x & 0x7FFFFFFF) * J;
          const double d = bs_biased(bs_arc_cost(gs, as, wip, R.z, R.w, R.y), bs_bonus(bs, s_beta[j], R.y));
          double y;
          if (R.y == 0) {   // no word: the node stays
            if (bs_extend(bs_load(src + j), d, &y)) best = y < best ? y : best;
          } else if (j != 0) {   // a word arc into j: only j's last word gets there, from j's predecessors
            if (R.y != wj) continue;
            for (int k = s_poff[j]; k < s_poff[j + 1]; ++k)
              if (bs_extend(bs_load(src + g_pred[k]), d, &y)) best = y < best ? y : best;
          } else {   // into the root: from every node the word sends there
            const int col = bs_col(s_words, W, R.y);
            for (int i = 0; i < J; ++i) {
              if (col >= 0 && g_tab[(size_t)i * W + col] != 0) continue;
              if (bs_extend(bs_load(src + i), d, &y)) best = y < best ? y : best;
            }
          }
        }
        if (round == 0 || best < old) { bs_store(cell, best); moved = 1; }
      }
      moved = __syncthreads_or(moved);   // (the barrier also orders this round's stores before the next round's loads)
      if (!eps_frame || (round > 0 && !moved)) break;
      if (round > e - b) {   // a path inside the frame visits a state once: more rounds than states is a cycle
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
  // ---- the end: the (final state, node) with the least v, then the least graph state, then the least node ---------------------
  int t = -1, j = 0;
  {
    double mine = unreached;
    u64 mine1 = ~0ull, mine2 = ~0ull;
    for (int i = X.fbeg[nd] + lane; i < X.fend[nd]; i += 64) {
      const int4 tk = toks[i];
      if (!((tk.w >> 30) & 1)) continue;
      for (int k = 0; k < J; ++k) {
        const double x = v[(size_t)i * J + k];
        if (!(x < unreached)) continue;
        const u64 x1 = ((u64)(uint32_t)tk.y << 32) | (uint32_t)k, x2 = (uint32_t)i;
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
      t = (int)(uint32_t)m2;
      j = (int)(uint32_t)m1;
    }
  }
  if (t < 0) {   // no final state is reached
    if (lane < kBiasHead) o[lane] = 0;
    return;
  }
  const double end_cost = v[(size_t)t * J + j];
  const int end_node = j;
  // ---- the walk back: exact equality, the tie rule -----------------------------------------------------------------------
  int32_t *path = Q.path + (size_t)pair * Q.path_cap;
  int n = 0, err = 0;
  while (t != 0) {
    if (n >= nt || n >= Q.path_cap) { err = kAlnInternal; break; }
    const double here = v[(size_t)t * J + j];
    const int32_t wj = s_word[j];
    const int a0 = X.off[t], a1 = X.off[t + 1];
    u64 k1 = ~0ull, k2 = ~0ull;
    uint32_t k3 = 0xFFFFFFFFu;
    int my_a = -1, my_src = 0, my_node = 0;
    for (int a = a0 + lane; a < a1; a += 64) {
      const int4 R = X.recA[a];
      if (!bs_is_arc(R.z, R.w)) continue;
      const int src = R.x & 0x7FFFFFFF;
      const double *from = v + (size_t)src * J;
      const double d = bs_biased(bs_arc_cost(gs, as, wip, R.z, R.w, R.y), bs_bonus(bs, s_beta[j], R.y));
      // the least source node that qualifies over this arc
      int node = -1;
      double y;
      if (R.y == 0) {
        if (bs_extend(from[j], d, &y) && y == here) node = j;
      } else if (j != 0) {
        if (R.y != wj) continue;
        for (int k = s_poff[j]; k < s_poff[j + 1] && node < 0; ++k)
          if (bs_extend(from[g_pred[k]], d, &y) && y == here) node = g_pred[k];
      } else {
        const int col = bs_col(s_words, W, R.y);
        for (int i = 0; i < J && node < 0; ++i) {
          if (col >= 0 && g_tab[(size_t)i * W + col] != 0) continue;
          if (bs_extend(from[i], d, &y) && y == here) node = i;
        }
      }
      if (node < 0) continue;
      const int4 B = X.recB[a];
      const u64 c1 = ((u64)(R.x < 0 ? 1 : 0) << 63) | ((u64)(uint32_t)B.x << 32) | (uint32_t)B.y;
      const u64 c2 = ((u64)(uint32_t)R.y << 32) | (uint32_t)R.z;
      const uint32_t c3 = (uint32_t)R.w;
      if (my_a < 0 || c1 < k1 || (c1 == k1 && (c2 < k2 || (c2 == k2 && (c3 < k3 || (c3 == k3 && node < my_node)))))) {
        k1 = c1; k2 = c2; k3 = c3; my_a = a; my_src = src; my_node = node;
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
    if (lane == 0) path[n] = a;
    ++n;
    t = __shfl(my_src, win, 64);
    j = __shfl(my_node, win, 64);
  }
  if (!err && j != 0) err = kAlnInternal;   // (state 0 is reached at the root alone)
  if (err) {
    if (lane < kBiasHead) o[lane] = lane == 4 ? err : 0;
    return;
  }
  // ---- front to back: the node track, the sums in hop order, the words, their times and the hits ------------------------------
  // (lane 0's stores to path[] are read back by the other lanes: one wave, in program order behind the stores' completion)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  float lm = 0.0f, tot = 0.0f;
  double cost = 0.0, bonus = 0.0;
  int kw = 0, n_hits = 0, node = 0, end_c = 0, begin_c = 0;   // words and hits so far, the node, one past the newest non-silence emitting hop, the newest word's begin
  for (int base = 0; base < n; base += 64) {
    const int m = min(64, n - base);
    int4 R = make_int4(0, 0, 0, 0), B = make_int4(0, 0, 0, 0);
    if (lane < m) {
      const int a = path[n - 1 - (base + lane)];
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
      if (word != 0) {
        const int col = bs_col(s_words, W, word);
        node = col < 0 ? 0 : (int)g_tab[(size_t)node * W + col];
      }
      const double r = bs_bonus(bs, s_beta[node], word);
      bs_extend(cost, bs_biased(bs_arc_cost(gs, as, wip, gb, ab, word), r), &cost);
      bonus = bonus + r;
      if (word != 0) {
        if (lane == 0 && kw >= 1 && kw <= cap) o_end[kw - 1] = max(end_c, begin_c);
        if (lane == 0 && kw < cap) { o_words[kw] = word; o_begin[kw] = F; }
        begin_c = F;
        for (int x = node; x != 0; x = g_fail[x]) {   // every phrase that ends here, the longest first
          const int p = g_phrase[x];
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
    if (!err && kw >= 1 && kw <= cap) o_end[kw - 1] = max(end_c, begin_c);   // (no silence list: the frames the path consumed = the end state's frame)
    const long long cb = __double_as_longlong(end_cost), bb = __double_as_longlong(bonus);
    o[0] = err ? 0 : 1; o[1] = n; o[2] = __float_as_int(tot); o[3] = __float_as_int(lm); o[4] = err;
    o[5] = kw; o[6] = n_hits; o[7] = 0; o[8] = (int32_t)(uint32_t)cb; o[9] = (int32_t)(uint32_t)((u64)cb >> 32);
    o[10] = (int32_t)(uint32_t)bb; o[11] = (int32_t)(uint32_t)((u64)bb >> 32); o[12] = 0; o[13] = 0; o[14] = 0; o[15] = 0;
  }
}

void launch_bias(const AlignDev &A, const BiasDev &Q, const BiasSet &S, const int32_t *chans, int cnt, hipStream_t s) {
  hipLaunchKernelGGL(bias_kernel, dim3(cnt * Q.n_set), dim3(kBsThreads), 0, s, A, Q, S, chans);
}

}  // namespace wfst
