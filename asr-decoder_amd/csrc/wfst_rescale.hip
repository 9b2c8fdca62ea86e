// Best paths under new scales (wfst_decoder_rescaled_words): the 1-best of a channel's raw lattice picked again under another LM
// weight, another acoustic scale and a word insertion penalty -- Kaldi's lattice-best-path-score (ScaleLattice, then the shortest path),
// the step every scoring script sweeps over LMWT x penalty -- for n_set settings per listed channel, without decoding again.  The
// min-plus twin of posterior_kernel (wfst_posterior.hip) over the same lattice and in-arc index (align_index_kernel's, AlignDev::idx).
//
// An arc costs c_q(a) = (gs * graph + as * acoustic) + (olabel != 0 ? wip : 0) in float64, every product and sum rounded on its own
// (no fused multiply-add: #pragma clang fp contract(off) around the expression).  v[0] = +0; v[t] = the minimum over the in-arcs
// s -> t of (v[s] + c_q(a)) + 0.0, a sum that is not finite being no transition, an arc whose float32 graph + acoustic is not finite
// being no arc.  A minimum does not depend on the order it is taken in: the cells are bit for bit whatever the order of the index.
//
// rescale_kernel, one workgroup per (channel, setting):
//  - frames in ascending order, one lane per state of the frame, strided where the frame has more states than the workgroup lanes.  A
//    state PULLS its minimum over its in-arc records: the emitting ones leave finished frames, so a frame is one pass and a barrier,
//    with no atomic on a cost and no backpointers -- 8 bytes per state and setting.
//  - a frame with arcs between its own states repeats the pass over those arcs until nothing moves, as align_kernel does: float
//    addition is monotone and the minimum idempotent, so the fixed point is the minimum over the paths whatever the order, reached
//    in at most one pass per state of the frame.  (posterior_kernel's level rule is what a SUM needs, which must take every arc
//    once; it costs 4 bytes per state and a counting pass that a minimum has no use for.)
//  - wave 0 picks the end, walks back by exact equality under align_kernel's arc tuple, and reads the path front to back: every lane
//    adds the costs in hop order (no tree) while lane 0 places words and frames by nearest_kernel's definitions; the transition-ids
//    of 64 hops are placed at once by a ballot.
// The cells other lanes may be writing in the same pass (the sources of arcs inside a frame) are read and written by relaxed 64-bit
// atomics: plain vector loads and stores that cannot tear; either value is a valid bound.
// Every loop is bounded by the lattice's own sizes; nothing waits for another workgroup.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wfst_align_index.h"   // AlnIndex / aln_carve, aln_wave_min_64
#include "wfst_device.h"

namespace wfst {
namespace {

typedef unsigned long long u64;
constexpr int kRsThreads = 256;

__device__ __forceinline__ double rs_load(const double *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void rs_store(double *p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// c_q(a): the products and sums rounded one by one.  hipcc contracts a * b + c into a fused multiply-add by default, and its
// __dmul_rn / __dadd_rn are plain operators that it contracts all the same: the pragma is what keeps the five roundings apart.
__device__ __forceinline__ double rs_arc_cost(double gs, double as, double wip, int32_t graph_bits, int32_t ac_bits, int32_t olabel) {
#pragma clang fp contract(off)
  const double g = gs * (double)__int_as_float(graph_bits);
  const double a = as * (double)__int_as_float(ac_bits);
  const double scaled = g + a;
  return scaled + (olabel != 0 ? wip : 0.0);
}
// an arc whose float32 graph + acoustic is not finite is no arc
__device__ __forceinline__ bool rs_is_arc(int32_t graph_bits, int32_t ac_bits) {
  const float s = __int_as_float(graph_bits) + __int_as_float(ac_bits);
  return s - s == 0.0f;
}
// the cell reached over an arc of cost c from a source cell src: false where that is no transition
__device__ __forceinline__ bool rs_extend(double src, double c, double *out) {
#pragma clang fp contract(off)
  const double sum = src + c;
  const double v = sum + 0.0;   // (+ 0.0: a zero total is +0)
  *out = v;
  return v - v == 0.0;   // finite (an unreached source is +inf)
}

}  // namespace

__global__ __launch_bounds__(kRsThreads) void rescale_kernel(AlignDev A, RescaleDev Q, RescaleSet S, const int32_t *chans) {
  const int pair = blockIdx.x, slot = pair / Q.n_set, q = pair % Q.n_set, c = chans[slot];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int4 *wa, *wb;
  const AlnIndex X = aln_carve(A, slot, &wa, &wb);
  const int cap = Q.cap_words, cap_tids = Q.cap_tids;
  int32_t *o = Q.out + (size_t)pair * rescale_out_ints(cap, cap_tids);
  int32_t *o_words = o + kRescaleHead, *o_begin = o_words + cap, *o_end = o_begin + cap, *o_tids = o_end + cap;
  const int64_t cell0 = Q.cell_off[pair];
  const int status = X.head[0];
  if (cell0 < 0 || status) {   // not asked for, or no lattice to look at
    if (tid < kRescaleHead) o[tid] = tid == 4 && cell0 >= 0 && status != kAlnNoLattice ? status : 0;
    return;
  }
  const double gs = S.v[3 * q], as = S.v[3 * q + 1], wip = S.v[3 * q + 2];
  const double unreached = __longlong_as_double(0x7FF0000000000000ll);
  const int nt = X.head[1], nd = X.head[3];
  double *v = Q.cells + cell0;
  const int4 *toks = Q.lat_toks + (size_t)c * Q.lat_tok_cap;
  __shared__ int s_err;
  if (tid == 0) s_err = 0;
  // ---- the cells, frame by frame ---------------------------------------------------------------------------------------
  for (int f = 0; f <= nd; ++f) {
    const int b = X.fbeg[f], e = X.fend[f];
    const bool eps_frame = X.feps[f] != 0;
    for (int round = 0;; ++round) {
      int moved = 0;
      for (int t = b + tid; t < e; t += kRsThreads) {
        const double old = round ? rs_load(&v[t]) : (t == 0 ? 0.0 : unreached);
        double best = old;
        const int a1 = X.off[t + 1];
        for (int a = X.off[t]; a < a1; ++a) {
          const int4 R = X.recA[a];
          if ((R.x < 0) != (round > 0)) continue;   // round 0: the emitting in-arcs; later rounds: the arcs inside the frame
          if (!rs_is_arc(R.z, R.w)) continue;
          double x;
          if (!rs_extend(rs_load(&v[R.x & 0x7FFFFFFF]), rs_arc_cost(gs, as, wip, R.z, R.w, R.y), &x)) continue;
          best = x < best ? x : best;
        }
        if (round == 0 || best < old) { rs_store(&v[t], best); moved = 1; }
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
    if (lane < kRescaleHead) o[lane] = lane == 4 ? s_err : 0;
    return;
  }
  // ---- the end: the final state with the least v, the least graph state among equals ----------------------------------------
  int t = -1;
  {
    double mine = unreached;
    u64 mine2 = ~0ull;
    for (int i = X.fbeg[nd] + lane; i < X.fend[nd]; i += 64) {
      const int4 tk = toks[i];
      if (!((tk.w >> 30) & 1)) continue;
      const double x = v[i];
      if (!(x < unreached)) continue;
      const u64 x2 = ((u64)(uint32_t)tk.y << 32) | (uint32_t)i;
      if (x < mine || (x == mine && x2 < mine2)) { mine = x; mine2 = x2; }
    }
    double best = mine;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const double other = __shfl_xor(best, m, 64);
      best = other < best ? other : best;
    }
    if (best < unreached) t = (int)(uint32_t)aln_wave_min_64(mine == best ? mine2 : ~0ull);
  }
  if (t < 0) {   // no final state is reached
    if (lane < kRescaleHead) o[lane] = 0;
    return;
  }
  const double end_cost = v[t];
  // ---- the walk back: exact equality, the tie rule -----------------------------------------------------------------------
  int32_t *path = Q.path + (size_t)pair * Q.path_cap;
  int n = 0, err = 0;
  while (t != 0) {
    if (n >= nt || n >= Q.path_cap) { err = kAlnInternal; break; }
    const double here = v[t];
    const int a0 = X.off[t], a1 = X.off[t + 1];
    u64 k1 = ~0ull, k2 = ~0ull;
    uint32_t k3 = 0xFFFFFFFFu;
    int my_a = -1, my_src = 0;
    for (int a = a0 + lane; a < a1; a += 64) {
      const int4 R = X.recA[a];
      if (!rs_is_arc(R.z, R.w)) continue;
      const int src = R.x & 0x7FFFFFFF;
      double x;
      if (!rs_extend(v[src], rs_arc_cost(gs, as, wip, R.z, R.w, R.y), &x) || x != here) continue;
      const int4 B = X.recB[a];
      const u64 c1 = ((u64)(R.x < 0 ? 1 : 0) << 63) | ((u64)(uint32_t)B.x << 32) | (uint32_t)B.y;
      const u64 c2 = ((u64)(uint32_t)R.y << 32) | (uint32_t)R.z;
      const uint32_t c3 = (uint32_t)R.w;
      if (my_a < 0 || c1 < k1 || (c1 == k1 && (c2 < k2 || (c2 == k2 && c3 < k3)))) {
        k1 = c1; k2 = c2; k3 = c3; my_a = a; my_src = src;
      }
    }
    u64 cand = __ballot(my_a >= 0);
    if (!cand) { err = kAlnInternal; break; }   // (a reached cell without the arrival that made it: never expected)
    if (__popcll(cand) > 1) {
      const u64 m1 = aln_wave_min_64(my_a >= 0 ? k1 : ~0ull);
      const bool at1 = my_a >= 0 && k1 == m1;
      const u64 m2 = aln_wave_min_64(at1 ? k2 : ~0ull);
      const bool at2 = at1 && k2 == m2;
      const u64 m3 = aln_wave_min_64(at2 ? (u64)k3 : ~0ull);
      cand = __ballot(at2 && (u64)k3 == m3);
    }
    const int win = __ffsll((long long)cand) - 1;
    const int a = __shfl(my_a, win, 64);
    if (lane == 0) path[n] = a;
    ++n;
    t = __shfl(my_src, win, 64);
  }
  if (err) {
    if (lane < kRescaleHead) o[lane] = lane == 4 ? err : 0;
    return;
  }
  // ---- front to back: the sums in hop order, the words and their times, the transition-ids --------------------------------
  // (lane 0's stores to path[] are read back by the other lanes: one wave, in program order behind the stores' completion)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  float lm = 0.0f, tot = 0.0f;
  double cost = 0.0;
  int kw = 0, n_tids = 0, end_c = 0, begin_c = 0;   // words and transition-ids so far, one past the newest non-silence emitting hop, the newest word's begin
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
    // the alignment: the non-zero ilabels, in path order
    const u64 has_tid = __ballot(lane < m && B.y != 0);
    if (lane < m && B.y != 0) {
      const int at = n_tids + __popcll(has_tid & ((1ull << lane) - 1ull));
      if (at < cap_tids) o_tids[at] = B.y;
    }
    n_tids += __popcll(has_tid);
    for (int j = 0; j < m; ++j) {
      const int word = __shfl(R.y, j, 64), F = __shfl(B.z, j, 64), ev = __shfl(endv, j, 64);
      const int gb = __shfl(R.z, j, 64), ab = __shfl(R.w, j, 64);
      const float g = __int_as_float(gb);
      lm += g;
      tot = (tot + (g + __int_as_float(ab))) + 0.0f;
      rs_extend(cost, rs_arc_cost(gs, as, wip, gb, ab, word), &cost);
      if (word != 0) {
        if (lane == 0 && kw >= 1 && kw <= cap) o_end[kw - 1] = max(end_c, begin_c);
        if (lane == 0 && kw < cap) { o_words[kw] = word; o_begin[kw] = F; }
        begin_c = F;
        ++kw;
      }
      end_c = max(end_c, ev);
    }
  }
  // (the path read forwards must reproduce the cell it was traced from)
  if (cost != end_cost) err = kAlnInternal;
  if (lane == 0) {
    if (!err && kw >= 1 && kw <= cap) o_end[kw - 1] = max(end_c, begin_c);   // (no silence list: the frames the path consumed = the end state's frame)
    const long long cb = __double_as_longlong(end_cost);
    o[0] = err ? 0 : 1; o[1] = n; o[2] = __float_as_int(tot); o[3] = __float_as_int(lm); o[4] = err;
    o[5] = kw; o[6] = n_tids; o[7] = 0; o[8] = (int32_t)(uint32_t)cb; o[9] = (int32_t)(uint32_t)((u64)cb >> 32); o[10] = 0; o[11] = 0;
  }
}

void launch_rescale(const AlignDev &A, const RescaleDev &Q, const RescaleSet &S, const int32_t *chans, int cnt, hipStream_t s) {
  hipLaunchKernelGGL(rescale_kernel, dim3(cnt * Q.n_set), dim3(kRsThreads), 0, s, A, Q, S, chans);
}

}  // namespace wfst
