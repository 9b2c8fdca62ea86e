// Frame posteriors (wfst_decoder_frame_posteriors): per frame of a channel's raw lattice the posterior mass of every class -- the
// transition-id of an emitting arc, or what a caller's map makes of it (pdf, phone) -- Kaldi's lattice-to-post, behind
// align_index_kernel (wfst_align.hip) and posterior_kernel (wfst_posterior.hip), whose index and gamma these kernels read.
//   post(f, v)    = the sum of gamma(a) over the emitting arcs a (ilabel > 0) whose source state's frame is f and whose class is v
//   frame_mass[f] = the sum over all v;  n_distinct[f] = the classes with post(f, v) > 0
//   the list of f = the classes with post(f, v) > 0 and post(f, v) >= min_post, by class id ascending
// The index is by destination and the states are in frame order, so the in-arc records of the states of frame f + 1
// (off[fbeg[f + 1]] .. off[fend[f + 1]]) hold exactly frame f's emitting arcs, beside the epsilon arcs inside frame f + 1: one
// contiguous range per frame, the frames independent of each other.  No table across frames, no atomic.
//
// frame_post_kernel, one workgroup of 256 lanes per (channel, frame); the workgroups beyond a channel's frames leave at once:
//  - the range's emitting arcs counted (a slice of the records per lane, the counts scanned), then their (class, gamma) pairs loaded
//    side by side in record order, the map applied on load;
//  - a bitonic sort by class in the form whose every exchange is ascending (the first step of a merge mirrors its block, the others
//    stride): the positions beyond the records then behave as keys above all and never move, so the network of the next power of
//    two runs over exactly the records, in place, whatever their number;
//  - a segmented inclusive scan of gamma over the runs of equal class: every lane scans a contiguous slice, the slices' open sums are
//    scanned across the lanes, and a slice takes what is carried into it up to its first run head -- a run of hundreds of records (a
//    phone map) is summed by as many lanes as it spans, never by one;
//  - a run's sum stands at its last record: the runs that pass (> 0, >= min_post on this very sum) are counted per slice, the counts
//    scanned, and the list goes out by class ascending to the staging area at the frame's record offset, its length, n_distinct and
//    frame_mass beside it.
//    Up to kFramePostLdsRecs emitting arcs the pairs live in LDS; a frame with more runs the same code over the workspace, at the
//    frame's record offset.  Which of the two is decided from the count before anything is loaded.
// frame_pack_kernel, one workgroup per channel: the frames' counts scanned into frame_off, the staged lists copied into the packed
// rows (an entry finds its frame by a binary search in frame_off), n_entries and the capacity flag.
// The order of a run's sum is the sort's, which follows the index's: results are reproducible to rounding, not bit for bit.
// Every loop is bounded by the lattice's own sizes; nothing waits for another workgroup.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wfst_align_index.h"
#include "wfst_device.h"

namespace wfst {
namespace {

constexpr int kFpThreads = 256;
constexpr uint32_t kFpNone = 0xFFFFFFFFu;   // the key of an arc in no class, above every class (a class is a non-negative int32)

// inclusive scans of one value per lane across the block (s: kFpThreads entries; a barrier on entry, so s may be reused at once)
__device__ __forceinline__ int fp_scan_int(int v, int *s, int tid) {
  __syncthreads();
  s[tid] = v;
  __syncthreads();
  for (int d = 1; d < kFpThreads; d <<= 1) {
    const int o = tid >= d ? s[tid - d] : 0;
    __syncthreads();
    s[tid] += o;
    __syncthreads();
  }
  return s[tid];
}
// ... segmented: flag = "a run head lies in the lane's slice"; a lane's value then stops the sum from its left
__device__ __forceinline__ double fp_scan_seg(double v, int flag, double *s, int *sf, int tid) {
  __syncthreads();
  s[tid] = v;
  sf[tid] = flag;
  __syncthreads();
  for (int d = 1; d < kFpThreads; d <<= 1) {
    double o = 0.0;
    int of = 0;
    if (tid >= d) { o = s[tid - d]; of = sf[tid - d]; }
    const int mine = sf[tid];
    __syncthreads();
    if (tid >= d && !mine) { s[tid] += o; sf[tid] = of; }
    __syncthreads();
  }
  return s[tid];
}
__device__ __forceinline__ double fp_sum(double v, double *s, int tid) {
  __syncthreads();
  s[tid] = v;
  __syncthreads();
  for (int step = kFpThreads / 2; step >= 1; step >>= 1) {
    if (tid < step) s[tid] += s[tid + step];
    __syncthreads();
  }
  return s[0];
}

__device__ __forceinline__ void fp_exchange(uint32_t *key, double *val, int lo, int hi) {
  const uint32_t a = key[lo], b = key[hi];
  if (a > b) {
    key[lo] = b; key[hi] = a;
    const double x = val[lo];
    val[lo] = val[hi]; val[hi] = x;
  }
}

// One frame: the m emitting arcs among the records rec0 + [r0, r1) of this lane's slice go to key / val[first ..) (LDS or the
// workspace), in record order; then the block works on key[0..m) / val[0..m).
__device__ __forceinline__ void fp_frame(const AlnIndex &X, const double *gamma, const FramePostDev &Q, int rec0, int r0, int r1, int first,
                                         int m, uint32_t *key, double *val, double *s_d, int *s_i, int32_t *st_class, double *st_post,
                                         int *n_listed, int *n_distinct, double *mass) {
  const int tid = threadIdx.x;
  for (int i = r0, at = first; i < r1; ++i) {
    if (X.recA[rec0 + i].x < 0) continue;   // an arc inside the next frame
    const int il = X.recB[rec0 + i].y;
    uint32_t k = kFpNone;                   // (a transition-id the map does not have: in no class)
    if (!Q.label_map) k = (uint32_t)il;
    else if (il >= 0 && il <= Q.n_tid) k = (uint32_t)Q.label_map[il];
    key[at] = k;
    val[at] = k != kFpNone ? gamma[rec0 + i] : 0.0;
    ++at;
  }
  __syncthreads();
  // ---- the sort --------------------------------------------------------------------------------------------------------------
  int P = 1;
  while (P < m) P <<= 1;
  for (int k = 2; k <= P; k <<= 1) {
    const int half = k >> 1;
    for (int t = tid; t < (P >> 1); t += kFpThreads) {   // the block of k mirrored
      const int base = (t / half) * k, j = t % half, hi = base + k - 1 - j;
      if (hi < m) fp_exchange(key, val, base + j, hi);
    }
    __syncthreads();
    for (int j = half >> 1; j >= 1; j >>= 1) {
      for (int t = tid; t < (P >> 1); t += kFpThreads) {
        const int lo = (t / j) * 2 * j + t % j, hi = lo + j;
        if (hi < m) fp_exchange(key, val, lo, hi);
      }
      __syncthreads();
    }
  }
  // ---- the runs' sums: val[i] = the sum of its run up to i ---------------------------------------------------------------------
  const int per = (m + kFpThreads - 1) / kFpThreads, b = min(m, tid * per), e = min(m, b + per);
  double run = 0.0;
  int has_head = 0;
  for (int i = b; i < e; ++i) {
    if (i == 0 || key[i] != key[i - 1]) { run = 0.0; has_head = 1; }
    run += val[i];
    val[i] = run;
  }
  const double incl = fp_scan_seg(run, has_head, s_d, s_i, tid);
  (void)incl;
  const double carry = tid ? s_d[tid - 1] : 0.0;   // what the lanes to the left leave open
  for (int i = b; i < e; ++i) {
    if (i == 0 || key[i] != key[i - 1]) break;
    val[i] = carry + val[i];
  }
  __syncthreads();   // (s_d is read above and reused below; val[] is final)
  // ---- the runs that are listed ------------------------------------------------------------------------------------------------
  int mine = 0, distinct = 0;
  double total = 0.0;
  for (int i = b; i < e; ++i) {
    if (key[i] == kFpNone || (i + 1 < m && key[i + 1] == key[i])) continue;   // not a run's last record
    const double x = val[i];
    if (!(x > 0.0)) continue;
    ++distinct;
    total += x;
    if (x >= Q.min_post) ++mine;
  }
  const int upto = fp_scan_int(mine, s_i, tid);
  int pos = upto - mine;
  const int listed = s_i[kFpThreads - 1];
  for (int i = b; i < e; ++i) {
    if (key[i] == kFpNone || (i + 1 < m && key[i + 1] == key[i])) continue;
    const double x = val[i];
    if (!(x > 0.0) || !(x >= Q.min_post)) continue;
    st_class[rec0 + pos] = (int32_t)key[i];
    st_post[rec0 + pos] = x;
    ++pos;
  }
  const int inc = fp_scan_int(distinct, s_i, tid);
  (void)inc;
  *n_distinct = s_i[kFpThreads - 1];
  *n_listed = listed;
  *mass = fp_sum(total, s_d, tid);
}

}  // namespace

__global__ __launch_bounds__(kFpThreads) void frame_post_kernel(AlignDev A, PostDev P, FramePostDev Q) {
  const int slot = blockIdx.x / A.fr_cap, f = blockIdx.x % A.fr_cap, tid = threadIdx.x;
  int4 *wa, *wb;
  const AlnIndex X = aln_carve(A, slot, &wa, &wb);
  // no lattice to look at, a lattice whose posteriors do not stand, or a frame the lattice does not have
  if (X.head[0] || P.chan_err[slot] || f >= X.head[3]) return;
  const int rec0 = X.off[X.fbeg[f + 1]], recs = X.off[X.fend[f + 1]] - rec0;
  __shared__ uint32_t s_key[kFramePostLdsRecs];
  __shared__ double s_val[kFramePostLdsRecs];
  __shared__ double s_d[kFpThreads];
  __shared__ int s_i[kFpThreads];
  const size_t arcs0 = (size_t)slot * A.na_cap;
  int listed = 0, distinct = 0;
  double mass = 0.0;
  if (recs > 0 && rec0 >= 0 && rec0 + recs <= A.na_cap) {
    // the frame's emitting arcs counted, a contiguous slice of the records per lane: where each lane's go, and which path is taken
    const int per = (recs + kFpThreads - 1) / kFpThreads, r0 = min(recs, tid * per), r1 = min(recs, r0 + per);
    int mine = 0;
    for (int i = r0; i < r1; ++i) mine += X.recA[rec0 + i].x >= 0;
    const int first = fp_scan_int(mine, s_i, tid) - mine, m = s_i[kFpThreads - 1];
    if (m > 0 && m <= kFramePostLdsRecs)
      fp_frame(X, P.gamma + arcs0, Q, rec0, r0, r1, first, m, s_key, s_val, s_d, s_i, Q.st_class + arcs0, Q.st_post + arcs0, &listed, &distinct,
               &mass);
    else if (m > 0)
      fp_frame(X, P.gamma + arcs0, Q, rec0, r0, r1, first, m, Q.ws_key + arcs0 + rec0, Q.ws_val + arcs0 + rec0, s_d, s_i, Q.st_class + arcs0,
               Q.st_post + arcs0, &listed, &distinct, &mass);
  }
  if (tid == 0) {
    const size_t at = (size_t)slot * A.fr_cap + f;
    Q.st_cnt[at] = listed;
    Q.st_distinct[at] = distinct;
    Q.st_mass[at] = mass;
  }
}

__global__ __launch_bounds__(kFpThreads) void frame_pack_kernel(AlignDev A, PostDev P, FramePostDev Q) {
  const int slot = blockIdx.x, tid = threadIdx.x;
  int4 *wa, *wb;
  const AlnIndex X = aln_carve(A, slot, &wa, &wb);
  const size_t capf = (size_t)Q.cap_frames, cape = (size_t)Q.cap_entries;
  int32_t *o = Q.out + (size_t)slot * (kFramePostHead + 2 * capf + 1 + cape);
  int32_t *o_off = o + kFramePostHead, *o_distinct = o_off + capf + 1, *o_class = o_distinct + capf;
  double *d_mass = Q.dout + (size_t)slot * (capf + cape), *d_post = d_mass + capf;
  const int status = X.head[0];
  if (status || P.chan_err[slot]) {
    if (tid < kFramePostHead) o[tid] = tid == 4 && status != kAlnNoLattice ? status : 0;
    return;
  }
  const int nf = X.head[3];
  const bool rows = nf <= Q.cap_frames;
  const int32_t *cnt = Q.st_cnt + (size_t)slot * A.fr_cap;
  __shared__ int s_i[kFpThreads];
  // exclusive scan of cnt[0..nf) into frame_off (one contiguous slice per lane)
  const int per = (nf + kFpThreads - 1) / kFpThreads, b = min(nf, tid * per), e = min(nf, b + per);
  int sum = 0;
  for (int f = b; f < e; ++f) sum += cnt[f];
  int run = fp_scan_int(sum, s_i, tid) - sum;
  const int total = s_i[kFpThreads - 1];
  if (rows) {
    for (int f = b; f < e; ++f) {
      o_off[f] = run;
      run += cnt[f];
      o_distinct[f] = Q.st_distinct[(size_t)slot * A.fr_cap + f];
      d_mass[f] = Q.st_mass[(size_t)slot * A.fr_cap + f];
    }
    if (tid == 0) o_off[nf] = total;
  }
  const bool fits = rows && total <= Q.cap_entries;
  if (tid < kFramePostHead) o[tid] = tid == 0 ? nf : (tid == 1 ? total : (tid == 2 ? !fits : 0));
  if (!fits) return;
  __syncthreads();   // frame_off is read by every lane
  const size_t arcs0 = (size_t)slot * A.na_cap;
  for (int i = tid; i < total; i += kFpThreads) {
    int lo = 0, hi = nf;   // the last frame with frame_off[f] <= i: the entry's own (an empty frame before it has the same offset)
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (o_off[mid] <= i) lo = mid; else hi = mid;
    }
    const size_t src = arcs0 + X.off[X.fbeg[lo + 1]] + (i - o_off[lo]);
    o_class[i] = Q.st_class[src];
    d_post[i] = Q.st_post[src];
  }
}

void launch_frame_post(const AlignDev &A, const PostDev &P, const FramePostDev &Q, int cnt, hipStream_t s) {
  hipLaunchKernelGGL(frame_post_kernel, dim3(cnt * A.fr_cap), dim3(kFpThreads), 0, s, A, P, Q);
  hipLaunchKernelGGL(frame_pack_kernel, dim3(cnt), dim3(kFpThreads), 0, s, A, P, Q);
}

}  // namespace wfst
