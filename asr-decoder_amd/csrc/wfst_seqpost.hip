// Sentence and phrase posteriors (wfst_decoder_sequence_posterior): the log-semiring twin of align_kernel (wfst_align.hip) and
// nearest_kernel (wfst_nearest.hip).  The same lattice, in-arc index (align_index_kernel's, AlignDev::idx) and frame-ordered table of
// states x (L + 1) cells -- but a cell is the float64 cost of the SUM over the paths that reach it, where align_kernel keeps the
// minimum.  Arc costs, the "no arc" rule and the way a sum is taken are posterior_kernel's (wfst_posterior.hip, wfst_lattice_sweep.h),
// whose alpha, beta and log_z this kernel reads.
//   mode 0, sentence:  S[0][0] = 0;  S[t][k] = -log( sum over a: s -> t, olabel 0           of exp(-(S[s][k]     + c(a)))
//                                                  + sum over a: s -> t, olabel == w[k - 1] of exp(-(S[s][k - 1] + c(a))) )
//                      seq_cost = -log sum over the final states s of exp(-S[s][L]);  seq_logpost = -log_z - seq_cost
//   mode 1, phrase:    P[s][0] = alpha[s];  P[t][k], 1 <= k < L, by the recurrence above;  an arc a: s -> t with olabel == w[L - 1]
//                      completes an occurrence, occ(a) = exp(-(P[s][L - 1] + c(a) + beta[t] + log_z));  count = sum occ(a),
//                      hit[f] = sum of occ(a) over the arcs whose source state's frame is f;  seq_logpost = log(count)
//
// seqpost_kernel, one workgroup per (channel, sequence):
//  - frames in ascending order, a lane per cell (state of the frame, k), strided where the frame has more cells than lanes.  A cell
//    PULLS over its state's in-arcs from finished cells in two passes, the least term and then the sum: no atomic on a cost.
//  - a frame with arcs between its own states goes by LEVELS, posterior_kernel's rule: a sum may not iterate to a fixpoint, so a
//    state's row is summed in the round after the last of its same-frame sources.  The level of a state does not depend on k: it is
//    worked out first, a lane per state (the sweep of wfst_lattice_sweep.h with nothing to compute: lvl[] = 1 + the round, more rounds
//    than states is a cycle); then one pass over the frame's cells per level, a barrier between.
//    A word on an arc inside a frame moves k - 1 -> k at the destination's higher level of the same frame.
//  - the end, mode 0: a block reduction over the final states' S[s][L], the least term and then the sum.  Mode 1: the lanes stride over
//    the states' in-arcs, add occ(a) to the frame's entry of hit_mass with a float64 atomic add -- to LDS where the row fits, to the
//    global row otherwise, as confidence_kernel does -- and reduce their own totals across the block.
// The order of every sum is the index's, which the emit launch decides: results are reproducible to rounding, not bit for bit.
// Every loop is bounded by the lattice's or the sequence's own sizes; nothing waits for another workgroup.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wfst_align_index.h"
#include "wfst_device.h"
#include "wfst_lattice_sweep.h"

namespace wfst {
namespace {

constexpr int kSpThreads = 1024;
constexpr int kSpFrames = 4096;   // hit_mass rows up to this many frames are added up in LDS

struct SpTable {
  double *cell;             // the pair's table, W cells per state
  int W, mode;
  const int32_t *w;         // the sequence
  const double *alpha;
};

// the term an in-arc record contributes to cell (., k) of its destination; false: none
__device__ __forceinline__ bool sp_term(const PostDev &P, const SpTable &T, const int4 &R, int k, double *x) {
  double c;
  if (!post_cost(P, R, &c)) return false;
  const double *row = T.cell + (size_t)(R.x & 0x7FFFFFFF) * T.W;
  if (R.y == 0) *x = row[k] + c;
  else if (k >= 1 && R.y == T.w[k - 1]) *x = row[k - 1] + c;
  else return false;
  return post_finite(*x);
}

// cell (t, k) from the finished cells of t's sources
__device__ double sp_cell(const PostDev &P, const AlnIndex &X, const SpTable &T, int t, int k) {
  if (T.mode && k == 0) return T.alpha[t];
  if (t == 0) return k == 0 ? 0.0 : post_inf();
  return post_logsum(X.off[t], X.off[t + 1], [&](int a, double *x) { return sp_term(P, T, X.recA[a], k, x); });
}

}  // namespace

__global__ __launch_bounds__(kSpThreads) void seqpost_kernel(AlignDev A, PostDev P, SeqPostDev Q, const int32_t *chans) {
  const int pair = blockIdx.x, slot = pair / A.n_seqs, c = chans[slot], tid = threadIdx.x;
  int4 *wa, *wb;
  const AlnIndex X = aln_carve(A, slot, &wa, &wb);
  int32_t *o = A.out + (size_t)pair * kSeqPostHead;
  const int64_t cell0 = A.cell_off[pair];
  const int L = A.seq_len[pair], cap = A.cap_words, status = X.head[0], mode = Q.mode;
  const int nf = status ? 0 : X.head[3] + 1;   // the state frames 0 .. frames decoded
  double *hit = Q.hit ? Q.hit + (size_t)pair * Q.cap_frames : nullptr;
  if (hit)
    for (int f = tid; f < Q.cap_frames; f += kSpThreads) hit[f] = 0.0;
  if (tid == 0) Q.out[pair] = 0.0;
  // not asked for, no lattice to look at, or a lattice whose posteriors do not stand (posterior_kernel reports why)
  if (cell0 < 0 || L < 0 || L > cap || (mode && L == 0) || status || P.chan_err[slot]) {
    if (tid < kSeqPostHead) o[tid] = tid == 1 ? nf : (tid == 4 && cell0 >= 0 && status != kAlnNoLattice ? status : 0);
    return;
  }
  const int nt = X.head[1], nd = X.head[3];
  SpTable T;
  T.cell = reinterpret_cast<double *>(A.cells) + cell0;
  T.W = mode ? L : L + 1;
  T.mode = mode;
  T.w = A.seq_words + (size_t)pair * cap;
  T.alpha = P.alpha + (size_t)slot * A.ns_cap;
  const int W = T.W;
  int32_t *lvl = A.path + (size_t)pair * A.ns_cap;
  __shared__ double s_red[kSpThreads];
  __shared__ double s_hit[kSpFrames];
  // ---- the table, frame by frame ---------------------------------------------------------------------------------------------
  int err = 0;
  for (int f = 0; f <= nd && !err; ++f) {
    const int b = X.fbeg[f], e = X.fend[f];
    const int64_t ncell = (int64_t)(e - b) * W;
    double *tf = T.cell + (size_t)b * W;   // the frame's cells: consecutive, a row per state
    if (!X.feps[f]) {   // every in-arc leaves an earlier frame
      for (int64_t cell = tid; cell < ncell; cell += kSpThreads) {
        const int i = (int)(cell / W);
        tf[cell] = sp_cell(P, X, T, b + i, (int)(cell - (int64_t)i * W));
      }
      __syncthreads();
      continue;
    }
    // the states' levels inside the frame: the sweep with nothing to compute leaves lvl[] = 1 + the round; then the rows, level by level
    int rounds = 0;
    err = sweep_in<kSpThreads>(X, b, e, true, lvl, [](int) {}, &rounds);
    for (int r = 1; r <= rounds && !err; ++r) {
      for (int64_t cell = tid; cell < ncell; cell += kSpThreads) {
        const int i = (int)(cell / W);
        if (lvl[b + i] != r) continue;
        tf[cell] = sp_cell(P, X, T, b + i, (int)(cell - (int64_t)i * W));
      }
      __syncthreads();
    }
  }
  if (err) {
    if (tid < kSeqPostHead) o[tid] = tid == 1 ? nf : (tid == 4 ? err : 0);
    return;
  }
  const double log_z = P.log_z[slot];
  double answer = 0.0;
  int found = 0;
  if (!mode) {
    // ---- the final states' S[s][L]: the least, then the sum ------------------------------------------------------------------
    const int4 *toks = Q.lat_toks + (size_t)c * Q.lat_tok_cap;
    double m = post_inf();
    for (int s = tid; s < nt; s += kSpThreads) {
      if (!((toks[s].w >> 30) & 1)) continue;
      const double x = T.cell[(size_t)s * W + L];
      if (post_finite(x) && x < m) m = x;
    }
    m = blk_min<kSpThreads>(m, s_red, tid);
    if (post_finite(m)) {   // (the same m in every lane)
      double sum = 0.0;
      for (int s = tid; s < nt; s += kSpThreads) {
        if (!((toks[s].w >> 30) & 1)) continue;
        const double x = T.cell[(size_t)s * W + L];
        if (post_finite(x)) sum += exp(-(x - m));
      }
      sum = blk_sum<kSpThreads>(sum, s_red, tid);
      answer = -log_z - (m - log(sum));
      found = 1;
    }
  } else {
    // ---- the arcs that complete the phrase ---------------------------------------------------------------------------------------
    const double *beta = P.beta + (size_t)slot * A.ns_cap;
    const bool rows = hit != nullptr && nf <= Q.cap_frames, in_lds = rows && nf <= kSpFrames;
    if (in_lds)
      for (int f = tid; f < nf; f += kSpThreads) s_hit[f] = 0.0;
    __syncthreads();   // (orders the zeroes of hit[] and s_hit[] before the additions of the other lanes)
    double *acc = in_lds ? s_hit : hit;
    const int last = T.w[L - 1];
    double mine = 0.0;
    for (int t = tid; t < nt; t += kSpThreads) {
      const double bt = beta[t];
      const int a1 = X.off[t + 1];
      for (int a = X.off[t]; a < a1; ++a) {
        const int4 R = X.recA[a];
        double cst;
        if (R.y != last || !post_cost(P, R, &cst)) continue;
        const double x = T.cell[(size_t)(R.x & 0x7FFFFFFF) * W + (L - 1)] + cst + bt + log_z;
        if (!post_finite(x)) continue;
        const double occ = exp(-x);
        mine += occ;
        if (rows) atomicAdd(&acc[X.recB[a].z], occ);
      }
    }
    const double count = blk_sum<kSpThreads>(mine, s_red, tid);   // (its barriers also finish the additions to s_hit[])
    if (in_lds)
      for (int f = tid; f < nf; f += kSpThreads) hit[f] = s_hit[f];
    if (count > 0.0) { answer = log(count); found = 1; }
  }
  if (tid == 0) Q.out[pair] = answer;
  if (tid < kSeqPostHead) o[tid] = tid == 0 ? found : (tid == 1 ? nf : 0);
}

void launch_seqpost(const AlignDev &A, const PostDev &P, const SeqPostDev &Q, const int32_t *chans, int cnt, hipStream_t s) {
  hipLaunchKernelGGL(seqpost_kernel, dim3(cnt * A.n_seqs), dim3(kSpThreads), 0, s, A, P, Q, chans);
}

}  // namespace wfst
