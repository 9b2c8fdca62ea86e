// Sequence-training statistics (wfst_decoder_sequence_stats): the expectation-semiring pass of Kaldi's
// LatticeForwardBackwardMpeVariants (sMBR) and the occupation difference of LatticeForwardBackwardMmi, per frame of a channel's raw
// lattice, behind align_index_kernel (wfst_align.hip) and posterior_kernel (wfst_posterior.hip), whose index, alpha, beta, gamma and
// by-source table these kernels read.  Everything is float64.
//   acc(a)  = 1 where an emitting arc's class is its frame's reference class and no silence class, 0 otherwise
//   p_in(a) = exp(-(alpha[s] + c(a) - alpha[t])),  p_out(a) = exp(-(c(a) + beta[t] - beta[s]))      (0 where not finite)
//   fa[0] = 0, fa[t] = sum over in-arcs p_in(a) (fa[s] + acc(a));  fb[s] = sum over out-arcs p_out(a) (fb[t] + acc(a))
//   tot_acc = fb[0];  w(a) = gamma(a) (fa[s] + acc(a) + fb[t] - tot_acc)
//   per frame f and class v:  post = sum gamma(a);  value = sum w(a) (sMBR) or [v == ref[f]] - post (MMI)
//
// acc_kernel, one workgroup of 1024 lanes per listed channel (sMBR only): forward, frames ascending, a lane per state of the frame
// (strided beyond 1024) PULLS fa over its in-arc records from finished values; a frame with epsilon arcs between its own states goes
// by posterior_kernel's levels (done[] holds 1 + the round that summed the state).  Backward, frames descending, the same over the
// by-source table posterior_kernel built: it is still resident (soff / sarc are not touched after that kernel's fill), so it is read,
// not built again; done[] is that kernel's scratch and is taken over.  Then w(a) per in-arc record.  The reference classes of up to
// kAccLdsFrames frames and the silence list sit in LDS.
// seqstat_frame_kernel, one workgroup of 256 lanes per (channel, frame): frame_post_kernel's scheme (wfst_framepost.hip) over
// (class, gamma, w) triples -- the frame-class reduction of wfst_lattice_sweep.h over two value columns, then the runs with post > 0
// listed by class ascending -- with MMI's values, its extra entry (ref[f], 0, 1) at its place in the order and the drop rule applied
// as the list is staged.  Up to kSeqStatLdsRecs emitting arcs the triples live in LDS, more in the workspace at the frame's record offset.
// seqstat_pack_kernel, one workgroup per channel: the frames' counts scanned into frame_off, the staged triples copied into the
// packed rows, n_ref_frames, n_dropped, tot_acc, n_entries and the capacity flag.
// seqstat_dense_kernel, one workgroup per (channel, frame row): n_cols zeros, a barrier, then float32(grad_scale * value) at the
// column of every staged entry.  A frame's entries have distinct classes: plain stores.
// The order of every sum is the index's, which the emit launch decides: results are reproducible to rounding, not bit for bit.
// Every loop is bounded by the lattice's own sizes; nothing waits for another workgroup; no atomic on a float.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wfst_align_index.h"
#include "wfst_device.h"
#include "wfst_lattice_sweep.h"

namespace wfst {
namespace {

constexpr int kAccThreads = 1024;
constexpr int kAccLdsFrames = 4096;   // reference classes kept in LDS (16 KB)
constexpr int kSsThreads = 256;

// acc(a) of in-arc record a (ref: the slot's row, in LDS or not; sil: the silence list, ascending)
__device__ __forceinline__ double ss_acc(const AlnIndex &X, const SeqStatDev &Q, const int32_t *ref, const int32_t *sil, int a) {
  if (X.recA[a].x < 0) return 0.0;   // an arc inside a frame
  const int4 B = X.recB[a];
  const int32_t r = ref[B.z];
  if (r < 0 || class_of(Q.label_map, Q.n_tid, B.y) != (uint32_t)r) return 0.0;
  for (int i = 0; i < Q.n_sil; ++i)
    if (sil[i] == r) return 0.0;
  return 1.0;
}

__device__ double ss_forward(const PostDev &P, const AlnIndex &X, const SeqStatDev &Q, const int32_t *ref, const int32_t *sil,
                             const double *alpha, const double *fa, int t) {
  const int a1 = X.off[t + 1];
  const double at = alpha[t];
  double sum = 0.0;
  for (int a = X.off[t]; a < a1; ++a) {
    const int4 R = X.recA[a];
    double c;
    if (!post_cost(P, R, &c)) continue;
    const int s = R.x & 0x7FFFFFFF;
    const double x = alpha[s] + c - at;
    if (post_finite(x)) sum += exp(-x) * (fa[s] + ss_acc(X, Q, ref, sil, a));
  }
  return sum;
}

__device__ double ss_backward(const PostDev &P, const AlnIndex &X, const SeqStatDev &Q, const int32_t *ref, const int32_t *sil,
                              const int2 *sarc, const int32_t *soff, const double *beta, const double *fb, int s) {
  const int p1 = soff[s];
  const double bs = beta[s];
  double sum = 0.0;
  for (int p = s ? soff[s - 1] : 0; p < p1; ++p) {
    const int2 E = sarc[p];
    double c;
    if (!post_cost(P, X.recA[E.x], &c)) continue;
    const double y = c + beta[E.y] - bs;
    if (post_finite(y)) sum += exp(-y) * (fb[E.y] + ss_acc(X, Q, ref, sil, E.x));
  }
  return sum;
}

// is record i of the sorted triples the last of a run that is listed (post > 0)?
__device__ __forceinline__ bool ss_listed(const uint32_t *key, const double *val, int i, int m) {
  return class_run_end(key, i, m) && val[i] > 0.0;
}

// One frame's list from what class_reduce left in key / val / wv[0, m), [b, e) this lane's slice of it: the runs with post > 0 by class
// ascending, with sMBR's or MMI's value.  r: the frame's reference class (-1: unlabelled).  The list goes to st_*[0 ..); returns its
// length, *dropped = the drop rule applied.
__device__ __forceinline__ int ss_list(const SeqStatDev &Q, int m, int b, int e, int32_t r, const uint32_t *key, const double *val,
                                       const double *wv, int *s_i, int32_t *st_class, double *st_post, double *st_value, int *dropped) {
  const int tid = threadIdx.x;
  const bool smbr = Q.criterion == kSeqSmbr;
  int mine = 0, less = 0, hit = 0;
  for (int i = b; i < e; ++i) {
    if (!ss_listed(key, val, i, m)) continue;
    ++mine;
    if (r >= 0 && key[i] < (uint32_t)r) ++less;
    if (r >= 0 && key[i] == (uint32_t)r) hit = 1;
  }
  const int upto = blk_scan_int<kSsThreads>(mine, s_i, tid);
  const int listed = s_i[kSsThreads - 1];
  const int below = blk_total_int<kSsThreads>(less, s_i, tid);
  const bool has_ref = blk_total_int<kSsThreads>(hit, s_i, tid) != 0;
  // MMI on a labelled frame whose reference class the lattice does not have: the frame is dropped, or the class gets an entry
  const bool absent = !smbr && r >= 0 && !has_ref, drop = absent && Q.drop_frames, extra = absent && !Q.drop_frames;
  int pos = upto - mine;
  for (int i = b; i < e; ++i) {
    if (!ss_listed(key, val, i, m)) continue;
    const double x = val[i];
    double v;
    if (smbr) v = wv[i];
    else if (r < 0 || drop) v = 0.0;
    else v = (key[i] == (uint32_t)r ? 1.0 : 0.0) - x;
    const int at = pos + (extra && key[i] > (uint32_t)r ? 1 : 0);
    st_class[at] = (int32_t)key[i];
    st_post[at] = x;
    st_value[at] = v;
    ++pos;
  }
  if (extra && tid == 0) {
    st_class[below] = r;
    st_post[below] = 0.0;
    st_value[below] = 1.0;
  }
  *dropped = drop;
  return listed + (extra ? 1 : 0);
}

}  // namespace

__global__ __launch_bounds__(kAccThreads) void acc_kernel(AlignDev A, PostDev P, SeqStatDev Q, SeqStatSil sil) {
  const int slot = blockIdx.x, tid = threadIdx.x;
  int4 *wa, *wb;
  const AlnIndex X = aln_carve(A, slot, &wa, &wb);
  if (X.head[0] || P.chan_err[slot]) {   // no lattice to look at, or one whose posteriors do not stand
    if (tid == 0) Q.tot[slot] = 0.0;
    return;
  }
  const int nt = X.head[1], nd = X.head[3];
  const double *alpha = P.alpha + (size_t)slot * A.ns_cap, *beta = P.beta + (size_t)slot * A.ns_cap, *gamma = P.gamma + (size_t)slot * A.na_cap;
  int32_t *done = P.done + (size_t)slot * A.ns_cap;
  const int32_t *soff = P.soff + (size_t)slot * A.ns_cap;
  const int2 *sarc = P.sarc + (size_t)slot * A.na_cap;
  double *fa = Q.fa + (size_t)slot * A.ns_cap, *fb = Q.fb + (size_t)slot * A.ns_cap, *w = Q.w + (size_t)slot * A.na_cap;
  __shared__ int32_t s_ref[kAccLdsFrames];
  __shared__ int32_t s_sil[kSeqStatMaxSil];
  const int32_t *ref = Q.ref + (size_t)slot * A.fr_cap;
  if (A.fr_cap <= kAccLdsFrames) {
    for (int f = tid; f < A.fr_cap; f += kAccThreads) s_ref[f] = ref[f];
    ref = s_ref;
  }
  if (tid < kSeqStatMaxSil) s_sil[tid] = sil.v[tid];
  __syncthreads();
  // ---- forward, backward: frame by frame, by levels inside a frame (a cycle: posterior_kernel has passed this lattice, not reached)
  int err = 0;
  for (int f = 0; f <= nd && !err; ++f)
    err = sweep_in<kAccThreads>(X, X.fbeg[f], X.fend[f], X.feps[f], done,
                                [&](int t) { fa[t] = ss_forward(P, X, Q, ref, s_sil, alpha, fa, t); });
  for (int f = nd; f >= 0 && !err; --f)
    err = sweep_out<kAccThreads>(X, sarc, soff, X.fbeg[f], X.fend[f], X.feps[f], done,
                                 [&](int s) { fb[s] = ss_backward(P, X, Q, ref, s_sil, sarc, soff, beta, fb, s); });
  if (err) {
    if (tid == 0) { Q.tot[slot] = 0.0; P.chan_err[slot] = err; }
    return;
  }
  // ---- the arcs' signed weights --------------------------------------------------------------------------------------------------
  const double tot = fb[0];
  for (int t = tid; t < nt; t += kAccThreads) {
    const double ft = fb[t];
    const int a1 = X.off[t + 1];
    for (int a = X.off[t]; a < a1; ++a)
      w[a] = gamma[a] * (fa[X.recA[a].x & 0x7FFFFFFF] + ss_acc(X, Q, ref, s_sil, a) + ft - tot);
  }
  if (tid == 0) Q.tot[slot] = tot;
}

__global__ __launch_bounds__(kSsThreads) void seqstat_frame_kernel(AlignDev A, PostDev P, SeqStatDev Q) {
  const int slot = blockIdx.x / A.fr_cap, f = blockIdx.x % A.fr_cap, tid = threadIdx.x;
  int4 *wa, *wb;
  const AlnIndex X = aln_carve(A, slot, &wa, &wb);
  // no lattice to look at, a lattice whose posteriors do not stand, or a frame the lattice does not have (f + 1 < fr_cap below)
  if (X.head[0] || P.chan_err[slot] || f >= X.head[3] || f + 1 >= A.fr_cap) return;
  const int rec0 = X.off[X.fbeg[f + 1]], recs = X.off[X.fend[f + 1]] - rec0;
  __shared__ uint32_t s_key[kSeqStatLdsRecs];
  __shared__ double s_val[kSeqStatLdsRecs];
  __shared__ double s_w[kSeqStatLdsRecs];
  __shared__ double s_d[2 * kSsThreads];
  __shared__ int s_i[kSsThreads];
  const size_t arcs0 = (size_t)slot * A.na_cap, st0 = (size_t)slot * ((size_t)A.na_cap + A.fr_cap);
  const int32_t r = Q.ref[(size_t)slot * A.fr_cap + f];
  int listed = 0, dropped = 0;
  const bool sane = rec0 >= 0 && recs >= 0 && rec0 + recs <= A.na_cap;   // (then the list's place, rec0 + f + [0, recs], is in the staging rows)
  if (sane) {
    int32_t *st_class = Q.st_class + st0 + rec0 + f;
    double *st_post = Q.st_post + st0 + rec0 + f, *st_value = Q.st_value + st0 + rec0 + f;
    int r0, r1, first;
    const int m = class_count<kSsThreads>(X, rec0, recs, s_i, &r0, &r1, &first);
    const double *const src[2] = {P.gamma + arcs0, Q.criterion == kSeqSmbr ? Q.w + arcs0 : nullptr};
    const auto frame = [&](uint32_t *key, double *val, double *wv) {   // the (class, gamma, w) triples: sorted, summed, listed
      double *const cols[2] = {val, wv};
      int b, e;
      class_reduce<kSsThreads, 2>(X, Q.label_map, Q.n_tid, src, rec0, r0, r1, first, m, key, cols, s_d, s_i, &b, &e);
      return ss_list(Q, m, b, e, r, key, val, wv, s_i, st_class, st_post, st_value, &dropped);
    };
    if (m <= kSeqStatLdsRecs) listed = frame(s_key, s_val, s_w);   // (m == 0: nothing is sorted, and MMI's rules still hold)
    else listed = frame(Q.ws_key + arcs0 + rec0, Q.ws_val + arcs0 + rec0, Q.ws_w + arcs0 + rec0);
  }
  if (tid == 0) {
    const size_t at = (size_t)slot * A.fr_cap + f;
    Q.st_cnt[at] = listed;
    Q.st_flag[at] = (r >= 0 ? 1 : 0) | (dropped ? 2 : 0);
  }
}

__global__ __launch_bounds__(kSsThreads) void seqstat_pack_kernel(AlignDev A, PostDev P, SeqStatDev Q) {
  const int slot = blockIdx.x, tid = threadIdx.x;
  int4 *wa, *wb;
  const AlnIndex X = aln_carve(A, slot, &wa, &wb);
  const size_t capf = (size_t)Q.cap_frames, cape = (size_t)Q.cap_entries;
  int32_t *o = Q.out + (size_t)slot * (kSeqStatHead + capf + 1 + cape);
  int32_t *o_off = o + kSeqStatHead, *o_class = o_off + capf + 1;
  double *d_tot = Q.dout + (size_t)slot * (1 + 2 * cape), *d_post = d_tot + 1, *d_value = d_post + cape;
  const int status = X.head[0];
  if (status || P.chan_err[slot]) {
    if (tid < kSeqStatHead) o[tid] = tid == 4 && status != kAlnNoLattice ? status : 0;
    if (tid == 0) *d_tot = 0.0;
    return;
  }
  const int nf = min(X.head[3], A.fr_cap - 1);
  const bool lists = Q.cap_frames > 0 || Q.cap_entries > 0, rows = lists && nf <= Q.cap_frames;
  const int32_t *cnt = Q.st_cnt + (size_t)slot * A.fr_cap, *flag = Q.st_flag + (size_t)slot * A.fr_cap;
  __shared__ int s_i[kSsThreads];
  int lab = 0, drp = 0;   // the labelled and the dropped frames counted (before the scan's barriers: the loads go out with its own)
  for (int f = tid; f < nf; f += kSsThreads) {
    lab += flag[f] & 1;
    drp += (flag[f] >> 1) & 1;
  }
  const int total = pack_frame_off<kSsThreads>(cnt, nf, rows, o_off, s_i, tid);
  const int n_lab = blk_total_int<kSsThreads>(lab, s_i, tid), n_drp = blk_total_int<kSsThreads>(drp, s_i, tid);
  const bool fits = !lists || (rows && total <= Q.cap_entries);
  if (tid < kSeqStatHead) o[tid] = tid == 0 ? nf : (tid == 1 ? total : (tid == 2 ? !fits : (tid == 3 ? n_lab : (tid == 5 ? n_drp : 0))));
  if (tid == 0) *d_tot = Q.criterion == kSeqSmbr ? Q.tot[slot] : 0.0;
  if (!fits || !lists) return;
  __syncthreads();   // frame_off is read by every lane
  const size_t st0 = (size_t)slot * ((size_t)A.na_cap + A.fr_cap);
  for (int i = tid; i < total; i += kSsThreads) {
    const int lo = pack_frame_of(o_off, nf, i);
    const size_t src = st0 + X.off[X.fbeg[lo + 1]] + lo + (i - o_off[lo]);
    o_class[i] = Q.st_class[src];
    d_post[i] = Q.st_post[src];
    d_value[i] = Q.st_value[src];
  }
}

__global__ __launch_bounds__(kSsThreads) void seqstat_dense_kernel(AlignDev A, PostDev P, SeqStatDev Q) {
  const int slot = blockIdx.x / A.fr_cap, f = blockIdx.x % A.fr_cap, tid = threadIdx.x;
  int4 *wa, *wb;
  const AlnIndex X = aln_carve(A, slot, &wa, &wb);
  float *base = Q.grad[slot];
  if (!base || X.head[0] || P.chan_err[slot] || f + 1 >= A.fr_cap || f >= X.head[3] || f >= Q.grad_rows[slot]) return;
  float *row = base + (size_t)f * (size_t)Q.grad_pitch[slot];
  for (int c = tid; c < Q.n_cols; c += kSsThreads) row[c] = 0.0f;
  __syncthreads();   // the zeros stand before an entry's store to the same column
  const int rec0 = X.off[X.fbeg[f + 1]], n = Q.st_cnt[(size_t)slot * A.fr_cap + f];
  if (rec0 < 0 || rec0 > A.na_cap) return;   // (the frame kernel staged nothing: n == 0)
  const size_t src = (size_t)slot * ((size_t)A.na_cap + A.fr_cap) + rec0 + f;
  for (int i = tid; i < n; i += kSsThreads) {
    const int32_t c = Q.st_class[src + i];
    if (c >= 0 && c < Q.n_cols) row[c] = (float)(Q.grad_scale * Q.st_value[src + i]);   // (the host refused a class beyond n_cols)
  }
}

void launch_seq_stat(const AlignDev &A, const PostDev &P, const SeqStatDev &Q, const SeqStatSil &sil, int cnt, bool dense, hipStream_t s) {
  if (Q.criterion == kSeqSmbr) hipLaunchKernelGGL(acc_kernel, dim3(cnt), dim3(kAccThreads), 0, s, A, P, Q, sil);
  hipLaunchKernelGGL(seqstat_frame_kernel, dim3(cnt * A.fr_cap), dim3(kSsThreads), 0, s, A, P, Q);
  hipLaunchKernelGGL(seqstat_pack_kernel, dim3(cnt), dim3(kSsThreads), 0, s, A, P, Q);
  if (dense) hipLaunchKernelGGL(seqstat_dense_kernel, dim3(cnt * A.fr_cap), dim3(kSsThreads), 0, s, A, P, Q);
}

}  // namespace wfst
