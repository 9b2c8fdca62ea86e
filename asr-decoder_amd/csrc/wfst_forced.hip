// Forced alignment against per-utterance graphs (wfst_decoder_force_align): exact float32 Viterbi of a channel's scores against that
// utterance's own small graph -- a compiled training graph, a transcript acceptor -- with the table V[f][s] of include/wfst_decoder.h:
// an emitting arc offers (V[f][s] + (-ll(f, ilabel))) + w to V[f + 1][t], an epsilon arc V[f][s] + w to V[f][t], a candidate that is
// not finite is none, every sum rounded on its own.  Nothing here reads the search's tokens: the scores only.
//
// forced_align_kernel, one workgroup per list entry, the frames in order:
//  - a lane per DESTINATION state, strided beyond the block, pulls the state's minimum over its in-arc records (ForcedGraphsDev):
//    the emitting records read the finished row of frame f, so that part of a frame is one pass; the epsilon records read the row
//    being made, level by level of the graph's epsilon DAG (the levels are the graph set's, computed once on the host), one barrier
//    per level and no iteration to a fixed point.  No atomic on a cost; nothing waits for another workgroup.
//  - the first exact minimum in record order wins (strict <), emitting records before epsilon ones: the tie rule does not depend on
//    the order the lanes run in.  The winner's record goes into the (frame, state) backpointer cell, 4 bytes.
//  - the two cost rows live in LDS for a graph of up to kFalignLdsStates states and in the workspace beyond; the same code either way.
//  - the scores a frame needs are the graph's distinct ilabels': where there are at most kFalignLdsLabels of them, frame f + 1's are
//    loaded into registers before frame f's pass and stored into the other half of an LDS row behind it, so that the pass's only HBM
//    accesses are the in-arc records (L2 hits after the first frame).  -DWFST_FALIGN_NO_STAGING (tools/force_align_probe.py's
//    variant build) gathers every score from the frame's row instead.
//  - wave 0 then walks the backpointers from (T, final state) to the seed (lane 0: a dependent chain) and reads the path front to
//    back 64 hops at a time: the hop list, the alignment, the words and their frames by ballots, the two LatticeToVector sums in
//    hop order.  -DWFST_FALIGN_NO_TRACEBACK (the probe's other variant) stops before the walk.
// Every loop is bounded by the graph's and the utterance's own sizes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wfst_device.h"

namespace wfst {
namespace {

typedef unsigned long long u64;
constexpr int kFaThreads = 256;
constexpr int kFaPre = kFalignLdsLabels / kFaThreads;   // scores a lane fetches ahead

__device__ __forceinline__ float fa_inf() { return __int_as_float(0x7F800000); }
__device__ __forceinline__ bool fa_finite(float x) { return x - x == 0.0f; }
// the two candidates, every sum rounded on its own (there is no product to fuse with; the pragma keeps it so)
__device__ __forceinline__ float fa_emit(float v, float ll, float w) {
#pragma clang fp contract(off)
  const float ac = -ll;
  const float with_ac = v + ac;
  return with_ac + w;
}
__device__ __forceinline__ float fa_eps(float v, float w) {
#pragma clang fp contract(off)
  return v + w;
}

template <bool kLds>
__device__ __forceinline__ void forced_run(const ForcedDev &Q, const ForcedChan &C, const int32_t *H, float *s_rows, float *s_sc) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int start = H[0], fin = H[1], S = H[2], depth = H[4], NL = H[5];
  const int2 *in_off = Q.G.in_off + H[6];
  const int4 *rec = Q.G.rec + H[7];
  const int32_t *lvl_state = Q.G.lvl_state + H[8], *lvl_off = Q.G.lvl_off + H[9], *labels = Q.G.labels + H[10];
  const int4 *arcs = Q.G.arcs + H[11];
  const int T = C.T;
  const int64_t stride = C.stride;
  const float *ll = C.ll;
  int32_t *bp = Q.bp + C.bp_off;
  float *rows = kLds ? s_rows : Q.rows + C.row_off;
  const int RS = kLds ? kFalignLdsStates : S;
#ifdef WFST_FALIGN_NO_STAGING
  const bool staged = false;
#else
  const bool staged = NL <= kFalignLdsLabels;
#endif
  // the columns of the labels this lane stages
  int col[kFaPre];
#pragma unroll
  for (int k = 0; k < kFaPre; ++k) {
    const int j = tid + k * kFaThreads;
    col[k] = 0;
    if (staged && j < NL) { const int il = labels[j]; col[k] = Q.col_map ? Q.col_map[il] : il; }
  }
  // ---- frame 0: the seed, then the epsilon arcs out of it ----------------------------------------------------------------------
  {
    float *cur = rows;
    for (int t = tid; t < S; t += kFaThreads) { cur[t] = t == start ? 0.0f : fa_inf(); bp[t] = 0; }
    if (staged && T > 0) {
#pragma unroll
      for (int k = 0; k < kFaPre; ++k) {
        const int j = tid + k * kFaThreads;
        if (j < NL) s_sc[j] = ll[col[k]];
      }
    }
  }
  __syncthreads();
  for (int f = 0;; ++f) {
    // the epsilon arcs inside frame f (row f & 1), level by level
    {
      float *cur = rows + (f & 1) * RS;
      int32_t *bpf = bp + (int64_t)f * S;
      for (int L = 1; L <= depth; ++L) {
        for (int i = lvl_off[L - 1] + tid; i < lvl_off[L]; i += kFaThreads) {
          const int t = lvl_state[i];
          float best = cur[t];
          int b = 0;
          const int a1 = in_off[t + 1].x;
          for (int a = in_off[t].y; a < a1; ++a) {
            const int4 R = rec[a];
            const float x = fa_eps(cur[R.x], __int_as_float(R.z));
            if (fa_finite(x) && x < best) { best = x; b = a + 1; }
          }
          if (b) { cur[t] = best; bpf[t] = b; }
        }
        __syncthreads();
      }
    }
    if (f == T) break;
    // the emitting arcs out of frame f into frame f + 1
    const float *prev = rows + (f & 1) * RS;
    float *cur = rows + ((f + 1) & 1) * RS;
    const float *sc = s_sc + (f & 1) * kFalignLdsLabels;
    float *scn = s_sc + ((f + 1) & 1) * kFalignLdsLabels;
    const float *row = ll + (int64_t)f * stride;
    float pre[kFaPre];
    const bool ahead = staged && f + 1 < T;
    if (ahead) {
#pragma unroll
      for (int k = 0; k < kFaPre; ++k)
        if (tid + k * kFaThreads < NL) pre[k] = row[stride + col[k]];
    }
    int32_t *bpn = bp + (int64_t)(f + 1) * S;
    for (int t = tid; t < S; t += kFaThreads) {
      float best = fa_inf();
      int b = 0;
      const int2 o = in_off[t];
      for (int a = o.x; a < o.y; ++a) {
        const int4 R = rec[a];
        float s;
        if (staged) {
          s = sc[R.y];
        } else {
          const int il = labels[R.y];
          s = row[Q.col_map ? Q.col_map[il] : il];
        }
        const float x = fa_emit(prev[R.x], s, __int_as_float(R.z));
        if (fa_finite(x) && x < best) { best = x; b = a + 1; }
      }
      cur[t] = best;
      bpn[t] = b;
    }
    if (ahead) {
#pragma unroll
      for (int k = 0; k < kFaPre; ++k)
        if (tid + k * kFaThreads < NL) scn[tid + k * kFaThreads] = pre[k];
    }
    __syncthreads();
  }
  // ---- the result: wave 0 ---------------------------------------------------------------------------------------------------------
  if (wave != 0) return;
  int32_t *o = Q.out + (int64_t)blockIdx.x * falign_out_ints(Q.cap_frames, Q.cap_hops, Q.cap_words);
  const float cost = rows[(T & 1) * RS + fin];
  if (!fa_finite(cost)) return;   // not found: the zeros the host filled in stand
#ifdef WFST_FALIGN_NO_TRACEBACK
  if (lane == 0) { o[0] = 1; o[1] = T; o[2] = __float_as_int(cost); }
  return;
#endif
  int32_t *o_hops = o + kFalignHead, *o_ali = o_hops + Q.cap_hops, *o_words = o_ali + Q.cap_frames, *o_wf = o_words + Q.cap_words;
  int32_t *path = Q.path + C.path_off;
  // the walk back (lane 0; every lane follows it: the loads are uniform)
  int n = 0, err = 0;
  {
    int f = T, t = fin;
    for (;;) {
      const int b = bp[(int64_t)f * S + t];
      if (!b) break;
      if (n >= C.path_cap) { err = 1; break; }
      const int4 R = rec[b - 1];
      if (lane == 0) path[n] = b - 1;
      ++n;
      if (R.y >= 0) --f;
      t = R.x;
    }
    if (!err && (f != 0 || t != start)) err = 1;   // (a reached cell whose chain does not end in the seed: never expected)
  }
  if (err) {
    if (lane == 0) o[7] = 1;
    return;
  }
  // (lane 0's stores to path[] are read back by the other lanes: one wave, in program order behind the stores' completion)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  float tot = 0.0f, lm = 0.0f;
  int f0 = 0, nw = 0;   // frames and words before this batch of hops
  for (int base = 0; base < n; base += 64) {
    const int m = min(64, n - base);
    int4 A = make_int4(0, 0, 0, 0);
    int arc = 0;
    if (lane < m) {
      const int4 R = rec[path[n - 1 - (base + lane)]];
      arc = R.w;
      A = arcs[arc];
    }
    const u64 below = (1ull << lane) - 1ull;
    const u64 emit = __ballot(lane < m && A.x != 0), word = __ballot(lane < m && A.y != 0);
    const int f = f0 + __popcll(emit & below), k = nw + __popcll(word & below);
    float ac = 0.0f;
    if (lane < m) {
      if (base + lane < Q.cap_hops) o_hops[base + lane] = arc;
      if (A.x != 0) {
        ac = -ll[(int64_t)f * stride + (Q.col_map ? Q.col_map[A.x] : A.x)];
        if (f < Q.cap_frames) o_ali[f] = Q.label_map ? Q.label_map[A.x] : A.x;
      }
      if (A.y != 0 && k < Q.cap_words) { o_words[k] = A.y; o_wf[k] = f; }
    }
    for (int j = 0; j < m; ++j) {   // LatticeToVector's sums, in hop order
#pragma clang fp contract(off)
      const float g = __int_as_float(__shfl(A.z, j, 64)), a = __shfl(ac, j, 64);
      lm += g;
      tot += g + a;
    }
    f0 += __popcll(emit);
    nw += __popcll(word);
  }
  if (lane == 0) {
    o[0] = 1; o[1] = T; o[2] = __float_as_int(cost); o[3] = __float_as_int(tot); o[4] = __float_as_int(lm); o[5] = n; o[6] = nw; o[7] = 0;
  }
}

}  // namespace

__global__ __launch_bounds__(kFaThreads) void forced_align_kernel(ForcedDev Q) {
  __shared__ float s_rows[2 * kFalignLdsStates];
  __shared__ float s_sc[2 * kFalignLdsLabels];
  const ForcedChan C = Q.chan[blockIdx.x];
  const int32_t *H = Q.G.hdr + (int64_t)C.graph * kFalignHdr;
  if (H[2] <= kFalignLdsStates) forced_run<true>(Q, C, H, s_rows, s_sc);
  else forced_run<false>(Q, C, H, s_rows, s_sc);
}

void launch_forced_align(const ForcedDev &Q, int cnt, hipStream_t s) {
  hipLaunchKernelGGL(forced_align_kernel, dim3(cnt), dim3(kFaThreads), 0, s, Q);
}

}  // namespace wfst
