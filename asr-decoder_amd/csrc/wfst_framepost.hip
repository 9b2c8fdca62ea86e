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
//  - the frame-class reduction of wfst_lattice_sweep.h over one value column: the range's emitting arcs counted, their (class, gamma)
//    pairs loaded side by side in record order, the map applied on load, sorted by class, gamma summed over the runs of equal class;
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
#include "wfst_lattice_sweep.h"   // class_count / class_reduce, the block primitives, pack_frame_off / pack_frame_of

namespace wfst {
namespace {

constexpr int kFpThreads = 256;

// One frame's list from what class_reduce left in key / val[0, m), [b, e) this lane's slice of it: the runs that pass (> 0, >= min_post
// on the run's very sum) by class ascending to st_*[0 ..), its length, the classes with a sum > 0 and their mass.
__device__ __forceinline__ void fp_list(const FramePostDev &Q, int m, int b, int e, const uint32_t *key, const double *val, double *s_d,
                                        int *s_i, int32_t *st_class, double *st_post, int *n_listed, int *n_distinct, double *mass) {
  const int tid = threadIdx.x;
  int mine = 0, distinct = 0;
  double total = 0.0;
  for (int i = b; i < e; ++i) {
    if (!class_run_end(key, i, m)) continue;
    const double x = val[i];
    if (!(x > 0.0)) continue;
    ++distinct;
    total += x;
    if (x >= Q.min_post) ++mine;
  }
  int pos = blk_scan_int<kFpThreads>(mine, s_i, tid) - mine;
  *n_listed = s_i[kFpThreads - 1];
  for (int i = b; i < e; ++i) {
    if (!class_run_end(key, i, m)) continue;
    const double x = val[i];
    if (!(x > 0.0) || !(x >= Q.min_post)) continue;
    st_class[pos] = (int32_t)key[i];
    st_post[pos] = x;
    ++pos;
  }
  *n_distinct = blk_total_int<kFpThreads>(distinct, s_i, tid);
  *mass = blk_sum<kFpThreads>(total, s_d, tid);
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
    int r0, r1, first;
    const int m = class_count<kFpThreads>(X, rec0, recs, s_i, &r0, &r1, &first);
    const double *const src[1] = {P.gamma + arcs0};
    const auto frame = [&](uint32_t *key, double *val) {   // the (class, gamma) pairs: sorted, summed, listed
      double *const cols[1] = {val};
      int b, e;
      class_reduce<kFpThreads, 1>(X, Q.label_map, Q.n_tid, src, rec0, r0, r1, first, m, key, cols, s_d, s_i, &b, &e);
      fp_list(Q, m, b, e, key, val, s_d, s_i, Q.st_class + arcs0 + rec0, Q.st_post + arcs0 + rec0, &listed, &distinct, &mass);
    };
    if (m > 0 && m <= kFramePostLdsRecs) frame(s_key, s_val);
    else if (m > 0) frame(Q.ws_key + arcs0 + rec0, Q.ws_val + arcs0 + rec0);
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
  const int total = pack_frame_off<kFpThreads>(cnt, nf, rows, o_off, s_i, tid);
  if (rows)
    for (int f = tid; f < nf; f += kFpThreads) {
      o_distinct[f] = Q.st_distinct[(size_t)slot * A.fr_cap + f];
      d_mass[f] = Q.st_mass[(size_t)slot * A.fr_cap + f];
    }
  const bool fits = rows && total <= Q.cap_entries;
  if (tid < kFramePostHead) o[tid] = tid == 0 ? nf : (tid == 1 ? total : (tid == 2 ? !fits : 0));
  if (!fits) return;
  __syncthreads();   // frame_off is read by every lane
  const size_t arcs0 = (size_t)slot * A.na_cap;
  for (int i = tid; i < total; i += kFpThreads) {
    const int lo = pack_frame_of(o_off, nf, i);
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
