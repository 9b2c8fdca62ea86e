// What the log-semiring kernels over the in-arc index share (posterior_kernel / confidence_kernel: wfst_posterior.hip; seqpost_kernel:
// wfst_seqpost.hip; slot_mass_kernel / slot_none_kernel: wfst_altern.hip; frame_post_kernel / frame_pack_kernel: wfst_framepost.hip;
// acc_kernel / seqstat_frame_kernel / seqstat_pack_kernel: wfst_seqstat.hip).  DESIGN.md 6o describes each piece once.
//  - the float64 arithmetic: +inf, "is finite", an in-arc record's cost c(a) with the "no arc" rule, the two-pass log-sum;
//  - the block primitives, templates over the block size NT (every lane of the block calls them; each takes its barrier on entry);
//  - the levelled frame sweep, by in-arc records and by the by-source table;
//  - the cut points of a hypothesis' cells;
//  - the per-frame class reduction and the two steps the pack kernels share.
// Device code only: included by the .hip files.
#ifndef WFST_LATTICE_SWEEP_H_
#define WFST_LATTICE_SWEEP_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wfst_align_index.h"
#include "wfst_device.h"

namespace wfst {
namespace {

// ---- float64 arithmetic ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double post_inf() { return __longlong_as_double(0x7FF0000000000000ll); }
__device__ __forceinline__ bool post_finite(double x) { return x - x == 0.0; }
// c(a), false where the arc is no arc
__device__ __forceinline__ bool post_cost(const PostDev &P, const int4 &R, double *c) {
  const float g = __int_as_float(R.z), a = __int_as_float(R.w), v = g + a;
  *c = P.graph_scale * (double)g + P.acoustic_scale * (double)a;
  return v - v == 0.0f;
}

// -log of the sum of exp(-x) over the seed (where seeded) and the terms i0 <= i < i1 for which term(i, &x) says true (a true term is
// finite): the least term m, then m - log(sum exp(-(x - m))), the seed first and the range ascending in both passes; +inf where
// there is no term at all.
template <class Term>
__device__ __forceinline__ double post_logsum(int i0, int i1, Term term, bool seeded = false, double seed = 0.0) {
  double m = seeded ? seed : post_inf();
  for (int i = i0; i < i1; ++i) {
    double x;
    if (term(i, &x) && x < m) m = x;
  }
  if (!post_finite(m)) return post_inf();
  double sum = seeded ? exp(-(seed - m)) : 0.0;
  for (int i = i0; i < i1; ++i) {
    double x;
    if (term(i, &x)) sum += exp(-(x - m));
  }
  return m - log(sum);
}

// ---- block primitives ------------------------------------------------------------------------------------------------------------
// lane tid's contiguous slice [*b, *e) of n items
template <int NT>
__device__ __forceinline__ void blk_slice(int n, int tid, int *b, int *e) {
  const int per = (n + NT - 1) / NT;
  *b = min(n, tid * per);
  *e = min(n, *b + per);
}
// inclusive scan of one int per lane (s: NT entries, reusable at once; s[NT - 1] is the total)
template <int NT>
__device__ __forceinline__ int blk_scan_int(int v, int *s, int tid) {
  __syncthreads();
  s[tid] = v;
  __syncthreads();
  for (int d = 1; d < NT; d <<= 1) {
    const int o = tid >= d ? s[tid - d] : 0;
    __syncthreads();
    s[tid] += o;
    __syncthreads();
  }
  return s[tid];
}
template <int NT>
__device__ __forceinline__ int blk_total_int(int v, int *s, int tid) {
  blk_scan_int<NT>(v, s, tid);
  return s[NT - 1];
}
// segmented inclusive scan of NV doubles per lane, left in s[c * NT + lane]: flag = "a run head lies in the lane's slice"; a lane's
// values then stop the sums from its left
template <int NT, int NV>
__device__ __forceinline__ void blk_scan_seg(const double (&v)[NV], int flag, double *s, int *sf, int tid) {
  __syncthreads();
#pragma unroll
  for (int c = 0; c < NV; ++c) s[c * NT + tid] = v[c];
  sf[tid] = flag;
  __syncthreads();
  for (int d = 1; d < NT; d <<= 1) {
    double o[NV] = {};
    int of = 0;
    if (tid >= d) {
#pragma unroll
      for (int c = 0; c < NV; ++c) o[c] = s[c * NT + tid - d];
      of = sf[tid - d];
    }
    const int mine = sf[tid];
    __syncthreads();
    if (tid >= d && !mine) {
#pragma unroll
      for (int c = 0; c < NV; ++c) s[c * NT + tid] += o[c];
      sf[tid] = of;
    }
    __syncthreads();
  }
}
// the block's sum / minimum of one double per lane, in every lane: a tree (s: NT doubles)
template <int NT>
__device__ __forceinline__ double blk_sum(double v, double *s, int tid) {
  __syncthreads();   // (s may still be read from the reduction before)
  s[tid] = v;
  __syncthreads();
  for (int step = NT / 2; step >= 1; step >>= 1) {
    if (tid < step) s[tid] += s[tid + step];
    __syncthreads();
  }
  return s[0];
}
template <int NT>
__device__ __forceinline__ double blk_min(double v, double *s, int tid) {
  __syncthreads();
  s[tid] = v;
  __syncthreads();
  for (int step = NT / 2; step >= 1; step >>= 1) {
    if (tid < step) { const double o = s[tid + step]; if (o < s[tid]) s[tid] = o; }
    __syncthreads();
  }
  return s[0];
}
// the last k of [0, n) with at(k) <= x (at ascending, at(0) <= x)
template <class At>
__device__ __forceinline__ int last_at_most(int n, int x, At at) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (at(mid) <= x) lo = mid; else hi = mid;
  }
  return lo;
}

// ---- the levelled frame sweep ------------------------------------------------------------------------------------------------------
// visit(t) once for every state t of the frame [b, e), a lane per state (strided beyond NT), after every state of the same frame that
// t depends on.  A frame without epsilon arcs between its own states (!eps) is one pass and a barrier.  Otherwise it goes by LEVELS:
// a sum may not iterate to a fixpoint, so a state is visited in the round after the last of its dependencies was.  done[] holds
// 1 + that round: a flag written in this round reads as "not yet" whether or not the store has landed.  One barrier per round, which
// also orders the round's stores before the next round's loads; as many rounds as the frame's longest epsilon chain (*rounds);
// more rounds than states is a cycle: kAlnCycle, 0 otherwise (the same in every lane).
// dep(t, ok) calls ok(state) for the dependencies of t inside the frame until one says false.
template <int NT, class Dep, class Visit>
__device__ __forceinline__ int sweep_frame(int b, int e, bool eps, int32_t *done, Dep dep, Visit visit, int *rounds) {
  const int tid = threadIdx.x;
  if (rounds) *rounds = 0;
  if (!eps) {
    for (int t = b + tid; t < e; t += NT) visit(t);
    __syncthreads();
    return 0;
  }
  for (int t = b + tid; t < e; t += NT) done[t] = 0;
  __syncthreads();
  for (int round = 0;; ++round) {
    int pending = 0;
    for (int t = b + tid; t < e; t += NT) {
      if (done[t]) continue;
      const bool ready = dep(t, [&](int s) { const int dn = done[s]; return dn != 0 && dn <= round; });
      if (!ready) { pending = 1; continue; }
      visit(t);
      done[t] = round + 1;
    }
    pending = __syncthreads_or(pending);
    if (rounds) *rounds = round + 1;
    if (!pending) return 0;
    if (round > e - b) return kAlnCycle;   // an epsilon path visits a state of the frame once
  }
}
// forward: t depends on the sources of its in-arc records inside the frame (recA.x < 0)
template <int NT, class Visit>
__device__ __forceinline__ int sweep_in(const AlnIndex &X, int b, int e, bool eps, int32_t *done, Visit visit, int *rounds = nullptr) {
  return sweep_frame<NT>(b, e, eps, done, [&](int t, auto ok) {
    bool ready = true;
    const int a1 = X.off[t + 1];
    for (int a = X.off[t]; a < a1 && ready; ++a) {
      const int src = X.recA[a].x;
      if (src < 0) ready = ok(src & 0x7FFFFFFF);   // (src >= 0: an emitting arc)
    }
    return ready;
  }, visit, rounds);
}
// backward: s depends on the destinations of its out-arcs inside the frame, over posterior_kernel's by-source table
template <int NT, class Visit>
__device__ __forceinline__ int sweep_out(const AlnIndex &X, const int2 *sarc, const int32_t *soff, int b, int e, bool eps, int32_t *done,
                                         Visit visit, int *rounds = nullptr) {
  return sweep_frame<NT>(b, e, eps, done, [&](int s, auto ok) {
    bool ready = true;
    const int p1 = soff[s];
    for (int p = s ? soff[s - 1] : 0; p < p1 && ready; ++p) {
      const int2 E = sarc[p];
      if (X.recA[E.x].x < 0) ready = ok(E.y);
    }
    return ready;
  }, visit, rounds);
}

// ---- the cut points of a hypothesis' cells -----------------------------------------------------------------------------------------
// m[0] = 0, m[k] = (b[k - 1] + b[k] + 1) >> 1 over the aligned words' begin frames: cell k is the frames m[k] <= f < m[k + 1]
struct AltCuts {
  const int32_t *s_m, *begin;   // s_m: the points in LDS (filled from raw()), or nullptr
  __device__ __forceinline__ int raw(int k) const { return k ? (begin[k - 1] + begin[k] + 1) >> 1 : 0; }
  __device__ __forceinline__ int at(int k) const { return s_m ? s_m[k] : raw(k); }
  // the last k with m[k] <= f
  __device__ __forceinline__ int cell_of(int f, int L) const {
    return last_at_most(L, f, [&](int k) { return at(k); });
  }
};

// ---- the per-frame class reduction -------------------------------------------------------------------------------------------------
constexpr uint32_t kClassNone = 0xFFFFFFFFu;   // the key of an arc in no class, above every class (a class is a non-negative int32)
// the class of transition-id il: itself, or what the map makes of it (a transition-id the map does not have: in no class)
__device__ __forceinline__ uint32_t class_of(const int32_t *label_map, int n_tid, int il) {
  if (!label_map) return (uint32_t)il;
  return il >= 0 && il <= n_tid ? (uint32_t)label_map[il] : kClassNone;
}
// is record i of the sorted keys the last of a run of a class?
__device__ __forceinline__ bool class_run_end(const uint32_t *key, int i, int m) {
  return key[i] != kClassNone && !(i + 1 < m && key[i + 1] == key[i]);
}
// the emitting arcs among a frame's records rec0 + [0, recs), a contiguous slice [*r0, *r1) of the records per lane: returns their
// number m (which decides between LDS and the workspace before anything is loaded); *first = where this lane's go among them
template <int NT>
__device__ __forceinline__ int class_count(const AlnIndex &X, int rec0, int recs, int *s_i, int *r0, int *r1, int *first) {
  const int tid = threadIdx.x;
  blk_slice<NT>(recs, tid, r0, r1);
  int mine = 0;
  for (int i = *r0; i < *r1; ++i) mine += X.recA[rec0 + i].x >= 0;
  *first = blk_scan_int<NT>(mine, s_i, tid) - mine;
  return s_i[NT - 1];
}
template <int NV>
__device__ __forceinline__ void class_exchange(uint32_t *key, double *const (&val)[NV], int lo, int hi) {
  const uint32_t a = key[lo], b = key[hi];
  if (a > b) {
    key[lo] = b; key[hi] = a;
#pragma unroll
    for (int c = 0; c < NV; ++c) { const double x = val[c][lo]; val[c][lo] = val[c][hi]; val[c][hi] = x; }
  }
}
// One frame, after class_count: the lane's emitting records go to key / val[c][first ..) (LDS or the workspace) in record order, column c
// from src[c] (nullptr: zeros; an arc in no class: zeros); then the block leaves key[0..m) sorted ascending and val[c][i] = the sum of
// column c over i's run of equal keys up to i, so that a run's sum stands at its last record.  s_d: NV * NT doubles, s_i: NT ints.
//  - the sort is the bitonic network in the form whose every exchange is ascending (the first step of a merge mirrors its block, the
//    others stride): the positions beyond m then behave as keys above all and never move, so the network of the next power of two
//    runs over exactly the records, in place, whatever their number;
//  - the sums are a segmented scan: every lane scans its slice [*b, *e) of the sorted records, the slices' open sums are scanned across
//    the lanes, and a slice takes what is carried into it up to its first run head -- a run of hundreds of records is summed by as many
//    lanes as it spans, never by one.
template <int NT, int NV>
__device__ __forceinline__ void class_reduce(const AlnIndex &X, const int32_t *label_map, int n_tid, const double *const (&src)[NV], int rec0,
                                             int r0, int r1, int first, int m, uint32_t *key, double *const (&val)[NV], double *s_d,
                                             int *s_i, int *b, int *e) {
  const int tid = threadIdx.x;
  for (int i = r0, at = first; i < r1; ++i) {
    if (X.recA[rec0 + i].x < 0) continue;   // an arc inside the next frame
    const uint32_t k = class_of(label_map, n_tid, X.recB[rec0 + i].y);
    key[at] = k;
#pragma unroll
    for (int c = 0; c < NV; ++c) val[c][at] = k != kClassNone && src[c] ? src[c][rec0 + i] : 0.0;
    ++at;
  }
  __syncthreads();
  int P = 1;
  while (P < m) P <<= 1;
  for (int k = 2; k <= P; k <<= 1) {
    const int half = k >> 1;
    for (int t = tid; t < (P >> 1); t += NT) {   // the block of k mirrored
      const int base = (t / half) * k, j = t % half, hi = base + k - 1 - j;
      if (hi < m) class_exchange<NV>(key, val, base + j, hi);
    }
    __syncthreads();
    for (int j = half >> 1; j >= 1; j >>= 1) {
      for (int t = tid; t < (P >> 1); t += NT) {
        const int lo = (t / j) * 2 * j + t % j, hi = lo + j;
        if (hi < m) class_exchange<NV>(key, val, lo, hi);
      }
      __syncthreads();
    }
  }
  blk_slice<NT>(m, tid, b, e);
  double run[NV];
#pragma unroll
  for (int c = 0; c < NV; ++c) run[c] = 0.0;
  int has_head = 0;
  for (int i = *b; i < *e; ++i) {
    const bool head = i == 0 || key[i] != key[i - 1];
    has_head |= head;
#pragma unroll
    for (int c = 0; c < NV; ++c) {
      if (head) run[c] = 0.0;
      run[c] += val[c][i];
      val[c][i] = run[c];
    }
  }
  blk_scan_seg<NT, NV>(run, has_head, s_d, s_i, tid);
  double carry[NV];   // what the lanes to the left leave open
#pragma unroll
  for (int c = 0; c < NV; ++c) carry[c] = tid ? s_d[c * NT + tid - 1] : 0.0;
  for (int i = *b; i < *e; ++i) {
    if (i == 0 || key[i] != key[i - 1]) break;
#pragma unroll
    for (int c = 0; c < NV; ++c) val[c][i] = carry[c] + val[c][i];
  }
  __syncthreads();   // (s_d is read above and may be reused at once; val[] is final)
}

// ---- what the pack kernels share -----------------------------------------------------------------------------------------------------
// the exclusive scan of cnt[0..nf) (one contiguous slice per lane), written with its total into off[0..nf] where `rows`; the total
template <int NT>
__device__ __forceinline__ int pack_frame_off(const int32_t *cnt, int nf, bool rows, int32_t *off, int *s_i, int tid) {
  int b, e, sum = 0;
  blk_slice<NT>(nf, tid, &b, &e);
  for (int f = b; f < e; ++f) sum += cnt[f];
  int run = blk_scan_int<NT>(sum, s_i, tid) - sum;
  const int total = s_i[NT - 1];
  if (rows) {
    for (int f = b; f < e; ++f) {
      off[f] = run;
      run += cnt[f];
    }
    if (tid == 0) off[nf] = total;
  }
  return total;
}
// the frame of packed entry i: the last with off[f] <= i (an empty frame before it has the same offset)
__device__ __forceinline__ int pack_frame_of(const int32_t *off, int nf, int i) {
  return last_at_most(nf, i, [&](int f) { return off[f]; });
}

}  // namespace
}  // namespace wfst
#endif
