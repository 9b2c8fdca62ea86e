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
// (class, gamma, w) triples -- the frame's emitting records compacted in record order, a bitonic sort by class whose every exchange
// is ascending, a segmented scan of BOTH sums, the runs with post > 0 listed by class ascending -- with MMI's values, its extra
// entry (ref[f], 0, 1) at its place in the order and the drop rule applied as the list is staged.  Up to kSeqStatLdsRecs emitting
// arcs the triples live in LDS, more in the workspace at the frame's record offset.
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
#include "wfst_post_math.h"

namespace wfst {
namespace {

constexpr int kAccThreads = 1024;
constexpr int kAccLdsFrames = 4096;   // reference classes kept in LDS (16 KB)
constexpr int kSsThreads = 256;
constexpr uint32_t kSsNone = 0xFFFFFFFFu;   // the key of an arc in no class, above every class

__device__ __forceinline__ uint32_t ss_class(const SeqStatDev &Q, int il) {
  if (!Q.label_map) return (uint32_t)il;
  return il >= 0 && il <= Q.n_tid ? (uint32_t)Q.label_map[il] : kSsNone;
}

// acc(a) of in-arc record a (ref: the slot's row, in LDS or not; sil: the silence list, ascending)
__device__ __forceinline__ double ss_acc(const AlnIndex &X, const SeqStatDev &Q, const int32_t *ref, const int32_t *sil, int a) {
  if (X.recA[a].x < 0) return 0.0;   // an arc inside a frame
  const int4 B = X.recB[a];
  const int32_t r = ref[B.z];
  if (r < 0 || ss_class(Q, B.y) != (uint32_t)r) return 0.0;
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

// inclusive scans of one value per lane across the block (s: kSsThreads entries; a barrier on entry, so s may be reused at once)
__device__ __forceinline__ int ss_scan_int(int v, int *s, int tid) {
  __syncthreads();
  s[tid] = v;
  __syncthreads();
  for (int d = 1; d < kSsThreads; d <<= 1) {
    const int o = tid >= d ? s[tid - d] : 0;
    __syncthreads();
    s[tid] += o;
    __syncthreads();
  }
  return s[tid];
}
// ... segmented, two sums at once: flag = "a run head lies in the lane's slice"; a lane's values then stop the sums from its left
__device__ __forceinline__ void ss_scan_seg2(double v, double u, int flag, double *s, double *s2, int *sf, int tid) {
  __syncthreads();
  s[tid] = v;
  s2[tid] = u;
  sf[tid] = flag;
  __syncthreads();
  for (int d = 1; d < kSsThreads; d <<= 1) {
    double o = 0.0, o2 = 0.0;
    int of = 0;
    if (tid >= d) { o = s[tid - d]; o2 = s2[tid - d]; of = sf[tid - d]; }
    const int mine = sf[tid];
    __syncthreads();
    if (tid >= d && !mine) { s[tid] += o; s2[tid] += o2; sf[tid] = of; }
    __syncthreads();
  }
}

__device__ __forceinline__ void ss_exchange(uint32_t *key, double *val, double *wv, int lo, int hi) {
  const uint32_t a = key[lo], b = key[hi];
  if (a > b) {
    key[lo] = b; key[hi] = a;
    const double x = val[lo];
    val[lo] = val[hi]; val[hi] = x;
    const double y = wv[lo];
    wv[lo] = wv[hi]; wv[hi] = y;
  }
}

// is record i of the sorted triples the last of a run that is listed (post > 0)?
__device__ __forceinline__ bool ss_listed(const uint32_t *key, const double *val, int i, int m) {
  if (key[i] == kSsNone || (i + 1 < m && key[i + 1] == key[i])) return false;
  return val[i] > 0.0;
}

// One frame: the m emitting arcs among the records rec0 + [r0, r1) of this lane's slice go to key / val / wv[first ..) (LDS or the
// workspace), in record order; then the block works on [0, m).  r: the frame's reference class (-1: unlabelled).  The list goes to
// st_*[0 ..); returns its length, *dropped = the drop rule applied.
__device__ __forceinline__ int ss_frame(const AlnIndex &X, const double *gamma, const double *w, const SeqStatDev &Q, int rec0, int r0, int r1,
                                        int first, int m, int32_t r, uint32_t *key, double *val, double *wv, double *s_d, double *s_d2,
                                        int *s_i, int32_t *st_class, double *st_post, double *st_value, int *dropped) {
  const int tid = threadIdx.x;
  const bool smbr = Q.criterion == kSeqSmbr;
  for (int i = r0, at = first; i < r1; ++i) {
    if (X.recA[rec0 + i].x < 0) continue;   // an arc inside the next frame
    const uint32_t k = ss_class(Q, X.recB[rec0 + i].y);
    key[at] = k;
    val[at] = k != kSsNone ? gamma[rec0 + i] : 0.0;
    wv[at] = k != kSsNone && smbr ? w[rec0 + i] : 0.0;
    ++at;
  }
  __syncthreads();
  // ---- the sort --------------------------------------------------------------------------------------------------------------
  int Pw = 1;
  while (Pw < m) Pw <<= 1;
  for (int k = 2; k <= Pw; k <<= 1) {
    const int half = k >> 1;
    for (int t = tid; t < (Pw >> 1); t += kSsThreads) {   // the block of k mirrored
      const int base = (t / half) * k, j = t % half, hi = base + k - 1 - j;
      if (hi < m) ss_exchange(key, val, wv, base + j, hi);
    }
    __syncthreads();
    for (int j = half >> 1; j >= 1; j >>= 1) {
      for (int t = tid; t < (Pw >> 1); t += kSsThreads) {
        const int lo = (t / j) * 2 * j + t % j, hi = lo + j;
        if (hi < m) ss_exchange(key, val, wv, lo, hi);
      }
      __syncthreads();
    }
  }
  // ---- the runs' sums: val[i] / wv[i] = the sums of its run up to i ------------------------------------------------------------
  const int per = (m + kSsThreads - 1) / kSsThreads, b = min(m, tid * per), e = min(m, b + per);
  double run = 0.0, run2 = 0.0;
  int has_head = 0;
  for (int i = b; i < e; ++i) {
    if (i == 0 || key[i] != key[i - 1]) { run = 0.0; run2 = 0.0; has_head = 1; }
    run += val[i];
    run2 += wv[i];
    val[i] = run;
    wv[i] = run2;
  }
  ss_scan_seg2(run, run2, has_head, s_d, s_d2, s_i, tid);
  const double carry = tid ? s_d[tid - 1] : 0.0, carry2 = tid ? s_d2[tid - 1] : 0.0;   // what the lanes to the left leave open
  for (int i = b; i < e; ++i) {
    if (i == 0 || key[i] != key[i - 1]) break;
    val[i] = carry + val[i];
    wv[i] = carry2 + wv[i];
  }
  __syncthreads();   // (s_d is read above and reused below; val[] and wv[] are final)
  // ---- the list ------------------------------------------------------------------------------------------------------------------
  int mine = 0, less = 0, hit = 0;
  for (int i = b; i < e; ++i) {
    if (!ss_listed(key, val, i, m)) continue;
    ++mine;
    if (r >= 0 && key[i] < (uint32_t)r) ++less;
    if (r >= 0 && key[i] == (uint32_t)r) hit = 1;
  }
  const int upto = ss_scan_int(mine, s_i, tid);
  const int listed = s_i[kSsThreads - 1];
  const int below_upto = ss_scan_int(less, s_i, tid);
  (void)below_upto;
  const int below = s_i[kSsThreads - 1];
  (void)ss_scan_int(hit, s_i, tid);
  const bool has_ref = s_i[kSsThreads - 1] != 0;
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
  // ---- forward ---------------------------------------------------------------------------------------------------------------
  int err = 0;
  for (int f = 0; f <= nd && !err; ++f) {
    const int b = X.fbeg[f], e = X.fend[f];
    if (!X.feps[f]) {   // every in-arc leaves an earlier frame
      for (int t = b + tid; t < e; t += kAccThreads) fa[t] = ss_forward(P, X, Q, ref, s_sil, alpha, fa, t);
      __syncthreads();
      continue;
    }
    for (int t = b + tid; t < e; t += kAccThreads) done[t] = 0;
    __syncthreads();
    for (int round = 0;; ++round) {
      int pending = 0;
      for (int t = b + tid; t < e; t += kAccThreads) {
        if (done[t]) continue;
        bool ready = true;
        const int a1 = X.off[t + 1];
        for (int a = X.off[t]; a < a1 && ready; ++a) {
          const int src = X.recA[a].x;
          if (src >= 0) continue;   // an emitting arc
          const int dn = done[src & 0x7FFFFFFF];
          ready = dn != 0 && dn <= round;
        }
        if (!ready) { pending = 1; continue; }
        fa[t] = ss_forward(P, X, Q, ref, s_sil, alpha, fa, t);
        done[t] = round + 1;
      }
      pending = __syncthreads_or(pending);   // (the barrier also orders this round's stores before the next round's loads)
      if (!pending) break;
      if (round > e - b) { err = kAlnCycle; break; }   // (posterior_kernel has passed this lattice: not reached)
    }
  }
  // ---- backward --------------------------------------------------------------------------------------------------------------
  for (int f = nd; f >= 0 && !err; --f) {
    const int b = X.fbeg[f], e = X.fend[f];
    if (!X.feps[f]) {
      for (int s = b + tid; s < e; s += kAccThreads) fb[s] = ss_backward(P, X, Q, ref, s_sil, sarc, soff, beta, fb, s);
      __syncthreads();
      continue;
    }
    for (int s = b + tid; s < e; s += kAccThreads) done[s] = 0;
    __syncthreads();
    for (int round = 0;; ++round) {
      int pending = 0;
      for (int s = b + tid; s < e; s += kAccThreads) {
        if (done[s]) continue;
        bool ready = true;
        const int p1 = soff[s];
        for (int p = s ? soff[s - 1] : 0; p < p1 && ready; ++p) {
          const int2 E = sarc[p];
          if (X.recA[E.x].x >= 0) continue;
          const int dn = done[E.y];
          ready = dn != 0 && dn <= round;
        }
        if (!ready) { pending = 1; continue; }
        fb[s] = ss_backward(P, X, Q, ref, s_sil, sarc, soff, beta, fb, s);
        done[s] = round + 1;
      }
      pending = __syncthreads_or(pending);
      if (!pending) break;
      if (round > e - b) { err = kAlnCycle; break; }
    }
  }
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
  __shared__ double s_d[kSsThreads];
  __shared__ double s_d2[kSsThreads];
  __shared__ int s_i[kSsThreads];
  const size_t arcs0 = (size_t)slot * A.na_cap, st0 = (size_t)slot * ((size_t)A.na_cap + A.fr_cap);
  const int32_t r = Q.ref[(size_t)slot * A.fr_cap + f];
  int listed = 0, dropped = 0;
  const bool sane = rec0 >= 0 && recs >= 0 && rec0 + recs <= A.na_cap;   // (then the list's place, rec0 + f + [0, recs], is in the staging rows)
  if (sane) {
    int32_t *st_class = Q.st_class + st0 + rec0 + f;
    double *st_post = Q.st_post + st0 + rec0 + f, *st_value = Q.st_value + st0 + rec0 + f;
    // the frame's emitting arcs counted, a contiguous slice of the records per lane: where each lane's go, and which path is taken
    const int per = (recs + kSsThreads - 1) / kSsThreads, r0 = min(recs, tid * per), r1 = min(recs, r0 + per);
    int mine = 0;
    for (int i = r0; i < r1; ++i) mine += X.recA[rec0 + i].x >= 0;
    const int first = ss_scan_int(mine, s_i, tid) - mine, m = s_i[kSsThreads - 1];
    if (m <= kSeqStatLdsRecs)   // (m == 0: nothing is sorted, and MMI's rules still hold)
      listed = ss_frame(X, P.gamma + arcs0, Q.w + arcs0, Q, rec0, r0, r1, first, m, r, s_key, s_val, s_w, s_d, s_d2, s_i, st_class, st_post,
                        st_value, &dropped);
    else
      listed = ss_frame(X, P.gamma + arcs0, Q.w + arcs0, Q, rec0, r0, r1, first, m, r, Q.ws_key + arcs0 + rec0, Q.ws_val + arcs0 + rec0,
                        Q.ws_w + arcs0 + rec0, s_d, s_d2, s_i, st_class, st_post, st_value, &dropped);
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
  // exclusive scan of cnt[0..nf) into frame_off (one contiguous slice per lane); the labelled and the dropped frames counted
  const int per = (nf + kSsThreads - 1) / kSsThreads, b = min(nf, tid * per), e = min(nf, b + per);
  int sum = 0, lab = 0, drp = 0;
  for (int f = b; f < e; ++f) {
    sum += cnt[f];
    lab += flag[f] & 1;
    drp += (flag[f] >> 1) & 1;
  }
  int run = ss_scan_int(sum, s_i, tid) - sum;
  const int total = s_i[kSsThreads - 1];
  (void)ss_scan_int(lab, s_i, tid);
  const int n_lab = s_i[kSsThreads - 1];
  (void)ss_scan_int(drp, s_i, tid);
  const int n_drp = s_i[kSsThreads - 1];
  if (rows) {
    for (int f = b; f < e; ++f) {
      o_off[f] = run;
      run += cnt[f];
    }
    if (tid == 0) o_off[nf] = total;
  }
  const bool fits = !lists || (rows && total <= Q.cap_entries);
  if (tid < kSeqStatHead) o[tid] = tid == 0 ? nf : (tid == 1 ? total : (tid == 2 ? !fits : (tid == 3 ? n_lab : (tid == 5 ? n_drp : 0))));
  if (tid == 0) *d_tot = Q.criterion == kSeqSmbr ? Q.tot[slot] : 0.0;
  if (!fits || !lists) return;
  __syncthreads();   // frame_off is read by every lane
  const size_t st0 = (size_t)slot * ((size_t)A.na_cap + A.fr_cap);
  for (int i = tid; i < total; i += kSsThreads) {
    int lo = 0, hi = nf;   // the last frame with frame_off[f] <= i: the entry's own (an empty frame before it has the same offset)
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (o_off[mid] <= i) lo = mid; else hi = mid;
    }
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
