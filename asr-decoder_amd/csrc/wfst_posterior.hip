// Lattice posteriors and word confidences (wfst_decoder_word_confidence): the sum over ALL paths of a channel's raw lattice where
// wfst_align.hip takes the minimum over the paths that spell one sequence.  Everything is float64; an arc costs
// c(a) = graph_scale * graph + acoustic_scale * acoustic, and an arc whose float32 graph + acoustic is not finite is no arc
// (align_kernel's rule, so that both see the same paths).
//   alpha[0] = 0, alpha[t] = -log sum over in-arcs  exp(-(alpha[s] + c(a)))
//   beta[s]  = -log([s final] + sum over out-arcs exp(-(c(a) + beta[t]))),   log_z = -beta[0]
//   gamma(a) = exp(-(alpha[s] + c(a) + beta[t] + log_z))
// every sum as m - log(sum exp(-(x - m))) with m the least term; a state without a finite term is +inf and its arcs have gamma 0.
//
// posterior_kernel, one workgroup per listed channel, over the in-arc index align_index_kernel left (wfst_align_index.h):
//  - the by-source table (a counting pass, a scan, a fill) the backward pass needs: the index is by destination, and
//    lattice_emit_kernel appends a channel's arcs in whatever order its waves retire, not grouped by source;
//  - forward, frames ascending, a lane per state of the frame (strided beyond 1024): a state PULLS the sum over its in-arcs from
//    finished values, no atomic on a cost.  A frame with epsilon arcs between its own states goes by LEVELS: a minimum may iterate
//    to a fixpoint, a sum may not, so a state is summed in the round after the last of its same-frame sources was (the sweep of
//    wfst_lattice_sweep.h over done[]);
//  - backward, frames descending, the same over the out-arcs;
//  - gamma per in-arc record.
// confidence_kernel, one workgroup per (channel, sequence): the cut points m[] of the aligned words' begin frames, a binary search
// of every word-carrying record's source frame in them, the records' gamma added up per cell; the aligned path's own cost.
// The order of every sum is the index's, which the emit launch decides: results are reproducible to rounding, not bit for bit.
// Every loop is bounded by the lattice's or the sequence's own sizes; nothing waits for another workgroup.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wfst_align_index.h"   // AlnIndex / aln_carve
#include "wfst_device.h"
#include "wfst_lattice_sweep.h"   // post_cost / post_logsum, sweep_in / sweep_out, AltCuts

namespace wfst {
namespace {

constexpr int kPostThreads = 1024;
constexpr int kConfWords = 4096;   // sequences up to this many words keep their cut points and sums in LDS

// alpha of state t from the finished values of its sources
__device__ double post_forward(const PostDev &P, const AlnIndex &X, const double *alpha, int t) {
  if (t == 0) return 0.0;
  return post_logsum(X.off[t], X.off[t + 1], [&](int a, double *x) {
    const int4 R = X.recA[a];
    double c;
    if (!post_cost(P, R, &c)) return false;
    *x = alpha[R.x & 0x7FFFFFFF] + c;
    return post_finite(*x);
  });
}

// beta of state s from the finished values of its destinations, and its final weight 0 where it is final
__device__ double post_backward(const PostDev &P, const AlnIndex &X, const int2 *sarc, const int32_t *soff, const double *beta, int s,
                                bool is_final) {
  return post_logsum(s ? soff[s - 1] : 0, soff[s], [&](int p, double *x) {
    const int2 E = sarc[p];
    double c;
    if (!post_cost(P, X.recA[E.x], &c)) return false;
    *x = c + beta[E.y];
    return post_finite(*x);
  }, is_final, 0.0);
}

}  // namespace

__global__ __launch_bounds__(kPostThreads) void posterior_kernel(DecoderDev D, AlignDev A, PostDev P, const int32_t *chans) {
  const int slot = blockIdx.x, c = chans[slot], tid = threadIdx.x;
  int4 *wa, *wb;
  const AlnIndex X = aln_carve(A, slot, &wa, &wb);
  if (X.head[0]) {   // no lattice to look at: align_kernel reports why
    if (tid == 0) { P.log_z[slot] = 0.0; P.chan_err[slot] = 0; }
    return;
  }
  const int nt = X.head[1], na = X.head[2], nd = X.head[3];
  const int4 *toks = D.lat_toks + (size_t)c * D.lat_tok_cap;
  double *alpha = P.alpha + (size_t)slot * A.ns_cap, *beta = P.beta + (size_t)slot * A.ns_cap, *gamma = P.gamma + (size_t)slot * A.na_cap;
  int32_t *done = P.done + (size_t)slot * A.ns_cap, *soff = P.soff + (size_t)slot * A.ns_cap;
  int2 *sarc = P.sarc + (size_t)slot * A.na_cap;
  __shared__ int s_part[kPostThreads];
  // ---- the by-source table ---------------------------------------------------------------------------------------------------
  for (int i = tid; i < nt; i += kPostThreads) soff[i] = 0;
  __syncthreads();
  for (int a = tid; a < na; a += kPostThreads) atomicAdd(&soff[X.recA[a].x & 0x7FFFFFFF], 1);
  __syncthreads();
  {  // exclusive scan of soff[0..nt) (one contiguous slice per thread)
    const int per = (nt + kPostThreads - 1) / kPostThreads, b = min(nt, tid * per), e = min(nt, b + per);
    int sum = 0;
    for (int i = b; i < e; ++i) sum += soff[i];
    s_part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
      int run = 0;
      for (int i = 0; i < kPostThreads; ++i) { const int v = s_part[i]; s_part[i] = run; run += v; }
    }
    __syncthreads();
    int run = s_part[tid];
    for (int i = b; i < e; ++i) { const int v = soff[i]; soff[i] = run; run += v; }
  }
  __syncthreads();
  // (the fill moves soff[s] from the first out-arc of s to one past its last: the first out-arc of s + 1)
  for (int t = tid; t < nt; t += kPostThreads) {
    const int a1 = X.off[t + 1];
    for (int a = X.off[t]; a < a1; ++a) sarc[atomicAdd(&soff[X.recA[a].x & 0x7FFFFFFF], 1)] = make_int2(a, t);
  }
  __syncthreads();
  // ---- forward, backward: frame by frame, by levels inside a frame (wfst_lattice_sweep.h) --------------------------------------
  int err = 0;
  for (int f = 0; f <= nd && !err; ++f)
    err = sweep_in<kPostThreads>(X, X.fbeg[f], X.fend[f], X.feps[f], done, [&](int t) { alpha[t] = post_forward(P, X, alpha, t); });
  for (int f = nd; f >= 0 && !err; --f)
    err = sweep_out<kPostThreads>(X, sarc, soff, X.fbeg[f], X.fend[f], X.feps[f], done,
                                  [&](int s) { beta[s] = post_backward(P, X, sarc, soff, beta, s, (toks[s].w >> 30) & 1); });
  if (err) {
    if (tid == 0) { P.log_z[slot] = 0.0; P.chan_err[slot] = err; }
    return;
  }
  // ---- the arcs' posteriors ----------------------------------------------------------------------------------------------------
  const double log_z = -beta[0];
  for (int t = tid; t < nt; t += kPostThreads) {
    const double bt = beta[t];
    const int a1 = X.off[t + 1];
    for (int a = X.off[t]; a < a1; ++a) {
      const int4 R = X.recA[a];
      double cst, g = 0.0;
      if (post_cost(P, R, &cst)) {
        const double x = alpha[R.x & 0x7FFFFFFF] + cst + bt + log_z;
        if (post_finite(x)) g = exp(-x);
      }
      gamma[a] = g;
    }
  }
  if (tid == 0) { P.log_z[slot] = log_z; P.chan_err[slot] = 0; }
}

__global__ __launch_bounds__(kPostThreads) void confidence_kernel(AlignDev A, PostDev P) {
  const int pair = blockIdx.x, slot = pair / A.n_seqs, tid = threadIdx.x;
  int4 *wa, *wb;
  const AlnIndex X = aln_carve(A, slot, &wa, &wb);
  const int cap = A.cap_words;
  const int32_t *o = A.out + (size_t)pair * (kAlignHead + 2 * (size_t)cap), *o_begin = o + kAlignHead;
  double *out = P.out + (size_t)pair * (1 + (size_t)cap);
  for (int k = tid; k <= cap; k += kPostThreads) out[k] = 0.0;
  // found, without an error word of its own, on a lattice whose posteriors stand
  if (!o[0] || o[4] || X.head[0] || P.chan_err[slot]) return;
  const int L = A.seq_len[pair], na = X.head[2];
  const int32_t *w = A.seq_words + (size_t)pair * cap;
  __shared__ int32_t s_m[kConfWords + 1];
  __shared__ double s_acc[kConfWords];
  const bool in_lds = L <= kConfWords;
  const AltCuts C = {in_lds ? s_m : nullptr, o_begin};   // cell k is the frames m[k] <= f < m[k + 1], m[L] = +inf
  if (in_lds)
    for (int k = tid; k < L; k += kPostThreads) {
      s_m[k] = C.raw(k);
      s_acc[k] = 0.0;
    }
  __syncthreads();   // (orders the zeroes of out[] before the additions of the other lanes as well)
  double *acc = in_lds ? s_acc : out + 1;
  if (tid == kPostThreads - 1) {   // the aligned path's own cost, in arc order (align_kernel left the path last arc first)
    const int32_t *path = A.path + (size_t)pair * A.ns_cap;
    double sum = 0.0;
    for (int j = o[1] - 1; j >= 0; --j) {
      double c;
      post_cost(P, X.recA[path[j]], &c);
      sum += c;
    }
    out[0] = -P.log_z[slot] - sum;
  }
  if (L > 0) {
    const double *gamma = P.gamma + (size_t)slot * A.na_cap;
    for (int a = tid; a < na; a += kPostThreads) {
      const int word = X.recA[a].y;
      if (word == 0) continue;
      const int lo = C.cell_of(X.recB[a].z, L);
      if (w[lo] == word) atomicAdd(&acc[lo], gamma[a]);
    }
  }
  __syncthreads();
  if (in_lds)
    for (int k = tid; k < L; k += kPostThreads) out[1 + k] = s_acc[k];
}

void launch_posterior(const DecoderDev &D, const AlignDev &A, const PostDev &P, const int32_t *chans, int cnt, hipStream_t s) {
  hipLaunchKernelGGL(posterior_kernel, dim3(cnt), dim3(kPostThreads), 0, s, D, A, P, chans);
}
void launch_confidence(const AlignDev &A, const PostDev &P, int cnt, hipStream_t s) {
  hipLaunchKernelGGL(confidence_kernel, dim3(cnt * A.n_seqs), dim3(kPostThreads), 0, s, A, P);
}

}  // namespace wfst
