// Word alternatives per slot (wfst_decoder_word_alternatives): a confusion network pinned to a hypothesis.  The hypothesis is the
// pivot, confidence_kernel's cells (wfst_posterior.hip) are the slots, and every other word of the lattice falls into the slot its
// arc's source frame lies in.  Both kernels run behind align_index_kernel, align_kernel, posterior_kernel and confidence_kernel, one
// workgroup per (channel, sequence), over the in-arc index (wfst_align_index.h) and posterior_kernel's alpha, beta, gamma and log_z.
// Arc costs, the "no arc" rule and the way a sum is taken are posterior_kernel's (wfst_lattice_sweep.h).
//
// slot_mass_kernel: mass(k, v) = the sum of gamma(a) over the arcs with olabel v > 0 whose source frame lies in cell k.
//  - the lanes stride over the in-arc records; a word-carrying record with gamma > 0 finds its cell by a binary search of the cut
//    points and adds its gamma to the entry of key (cell, word) in an open-addressed table: the key claimed by compare-and-swap, the
//    mass added by a float64 atomic add.  The table is in LDS (kAltLdsSlots slots, at most WFST_ALTERN_LDS_KEYS distinct keys: half
//    full at the most).  A sequence with more distinct keys starts again in its table in the workspace, which has a slot for every arc
//    of the lattice and one more, so it never fills.
//  - the table is then SORTED in place by (cell ascending, mass descending, word ascending), empty slots last (a bitonic network: the
//    table's size is a power of two).  An entry's rank inside its cell is its position minus the cell's first, found by a binary
//    search; the first n_alts ranks are written out, the last rank of a cell is n_distinct.  The order is taken on the kernel's OWN
//    sums, so a list is strictly ordered by construction.
// slot_none_kernel: none_post[k] = the share of the lattice's weight on the complete paths without a word-carrying arc whose source
// frame lies in cell k.  ONE pass over the frames in ascending order serves all cells, which partition the time axis:
//   A[t] = -log( sum over a: s -> t, frame(s) < lo              of exp(-(alpha[s] + c(a)))
//              + sum over a: s -> t, frame(s) >= lo, olabel 0   of exp(-(A[s]     + c(a))) ),   lo = the first frame of t's cell
//  - a lane per state of the frame, strided beyond the block; a state PULLS its sum over its in-arcs in two passes, the least term and
//    then the sum; a frame with arcs between its own states goes by levels, posterior_kernel's rule (the flags sit in AlignDev::path,
//    which confidence_kernel has finished with);
//  - at a frame that begins a cell the wordless emitting in-arcs are also the LEAVING arcs of the cell before: exp(-(A[s] + c(a) +
//    beta[t] + log_z)) is added to that cell; a final state adds exp(-(A[s] + log_z)) to its own cell and exp(-(alpha[s] + log_z)) to
//    the "ended early" mass of its cell, which every LATER cell receives (a running sum over the cells at the end);
//  - these additions are order-free float64 atomic adds, to LDS where the sequence's cells fit, to the global rows otherwise.
// The order of every sum is the index's, which the emit launch decides: results are reproducible to rounding, not bit for bit.
// Every loop is bounded by the lattice's or the sequence's own sizes; nothing waits for another workgroup.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wfst_decoder.h"   // WFST_ALTERN_LDS_KEYS
#include "wfst_align_index.h"
#include "wfst_device.h"
#include "wfst_lattice_sweep.h"

namespace wfst {
namespace {

constexpr int kAltThreads = 1024;
constexpr int kAltLdsKeys = WFST_ALTERN_LDS_KEYS;
constexpr int kAltLdsSlots = 2 * kAltLdsKeys;   // a power of two
constexpr int kAltCells = 2048;                 // sequences up to this many words keep their cut points (and none sums) in LDS
constexpr unsigned long long kAltEmpty = ~0ull;
static_assert((kAltLdsSlots & (kAltLdsSlots - 1)) == 0, "the LDS table's size is a power of two");

__device__ __forceinline__ uint32_t alt_hash(unsigned long long key) {
  key *= 0x9E3779B97F4A7C15ull;
  return (uint32_t)(key >> 32);
}

// gamma added up by (cell, word) in the table tk / tm of T slots (a power of two).  key_room: the distinct keys the table may take;
// *over is set when one more is claimed (the lanes then stop: the caller starts again elsewhere).
__device__ __forceinline__ void alt_accumulate(const AlnIndex &X, const double *gamma, int na, const AltCuts &C, int L, unsigned long long *tk,
                                               double *tm, int T, int key_room, int *count, volatile int *over, int tid) {
  for (int a = tid; a < na; a += kAltThreads) {
    const int word = X.recA[a].y;
    if (word == 0) continue;
    const double g = gamma[a];
    if (!(g > 0.0)) continue;
    if (*over) break;
    const unsigned long long key = (unsigned long long)(uint32_t)C.cell_of(X.recB[a].z, L) << 32 | (uint32_t)word;
    uint32_t h = alt_hash(key) & (uint32_t)(T - 1);
    for (int probe = 0; probe < T; ++probe, h = (h + 1) & (uint32_t)(T - 1)) {
      unsigned long long cur = tk[h];
      if (cur == kAltEmpty) {
        cur = atomicCAS(&tk[h], kAltEmpty, key);
        if (cur == kAltEmpty) {
          if (atomicAdd(count, 1) >= key_room) *over = 1;
          cur = key;
        }
      }
      if (cur == key) { atomicAdd(&tm[h], g); break; }
    }
  }
}

// entry (ka, ma) comes before (kb, mb): cell ascending (the empty key's is the largest), mass descending, word ascending
__device__ __forceinline__ bool alt_before(unsigned long long ka, double ma, unsigned long long kb, double mb) {
  const uint32_t ca = (uint32_t)(ka >> 32), cb = (uint32_t)(kb >> 32);
  if (ca != cb) return ca < cb;
  if (ma != mb) return ma > mb;
  return (uint32_t)ka < (uint32_t)kb;
}

// the table sorted in place, then the first n_alts entries of every cell and the cells' counts written out
__device__ __forceinline__ void alt_select(unsigned long long *tk, double *tm, int T, int n_alts, int32_t *alt_word, double *alt_post,
                                           int32_t *n_distinct, int tid) {
  for (int k = 2; k <= T; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < T; i += kAltThreads) {
        const int o = i ^ j;
        if (o <= i) continue;
        const unsigned long long ki = tk[i], ko = tk[o];
        const double mi = tm[i], mo = tm[o];
        const bool up = (i & k) == 0;
        if (up ? alt_before(ko, mo, ki, mi) : alt_before(ki, mi, ko, mo)) { tk[i] = ko; tm[i] = mo; tk[o] = ki; tm[o] = mi; }
      }
      __syncthreads();
    }
  for (int i = tid; i < T; i += kAltThreads) {
    const unsigned long long key = tk[i];
    if (key == kAltEmpty) continue;
    const uint32_t cell = (uint32_t)(key >> 32);
    int lo = -1, hi = i;   // the first entry of the cell: the least index whose cell is not below this one's
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if ((uint32_t)(tk[mid] >> 32) < cell) lo = mid; else hi = mid;
    }
    const int rank = i - hi;
    if (rank < n_alts) {
      alt_word[(size_t)cell * n_alts + rank] = (int32_t)(uint32_t)key;
      alt_post[(size_t)cell * n_alts + rank] = tm[i];
    }
    if (i + 1 == T || (uint32_t)(tk[i + 1] >> 32) != cell) n_distinct[cell] = rank + 1;
  }
}

// the term an in-arc record contributes to A of its destination, a state of frame f in a cell that begins at lo; false: none
__device__ __forceinline__ bool none_term(const PostDev &P, const AlnIndex &X, const double *alpha, const double *acost, int a, int f, int lo,
                                          double *x) {
  const int4 R = X.recA[a];
  double c;
  if (!post_cost(P, R, &c)) return false;
  const int s = R.x & 0x7FFFFFFF;
  const int sf = R.x < 0 ? f : X.recB[a].z;
  if (sf < lo) *x = alpha[s] + c;          // the arc ENTERS the cell: its word belongs to the cell before
  else if (R.y == 0) *x = acost[s] + c;
  else return false;
  return post_finite(*x);
}

__device__ double none_forward(const PostDev &P, const AlnIndex &X, const double *alpha, const double *acost, int t, int f, int lo) {
  if (t == 0) return 0.0;
  return post_logsum(X.off[t], X.off[t + 1], [&](int a, double *x) { return none_term(P, X, alpha, acost, a, f, lo, x); });
}

// what a finished state of cell k adds where it is final: its wordless mass to the cell, its whole mass to the cell's "ended early"
__device__ __forceinline__ void none_final(double a_t, double alpha_t, double log_z, double *none, double *early, int k) {
  const double x = a_t + log_z, y = alpha_t + log_z;
  if (post_finite(x)) atomicAdd(&none[k], exp(-x));
  if (post_finite(y)) atomicAdd(&early[k], exp(-y));
}

// found, without an error word of its own, on a lattice whose posteriors stand: the pair has slots
__device__ __forceinline__ bool alt_runs(const int32_t *o, const AlnIndex &X, const PostDev &P, int slot) {
  return o[0] && !o[4] && !X.head[0] && !P.chan_err[slot];
}

}  // namespace

__global__ __launch_bounds__(kAltThreads) void slot_mass_kernel(AlignDev A, PostDev P, AltDev Q) {
  const int pair = blockIdx.x, slot = pair / A.n_seqs, tid = threadIdx.x;
  int4 *wa, *wb;
  const AlnIndex X = aln_carve(A, slot, &wa, &wb);
  const int cap = A.cap_words, K = Q.n_alts;
  const int32_t *o = A.out + (size_t)pair * (kAlignHead + 2 * (size_t)cap), *o_begin = o + kAlignHead;
  int32_t *alt_word = Q.alt_word + (size_t)pair * cap * K, *n_distinct = Q.n_distinct + (size_t)pair * cap;
  double *alt_post = Q.alt_post + (size_t)pair * cap * K;
  for (int i = tid; i < cap * K; i += kAltThreads) { alt_word[i] = 0; alt_post[i] = 0.0; }
  for (int k = tid; k < cap; k += kAltThreads) n_distinct[k] = 0;
  const int L = A.seq_len[pair];
  if (!alt_runs(o, X, P, slot) || L <= 0) return;
  const int na = X.head[2];
  const double *gamma = P.gamma + (size_t)slot * A.na_cap;
  __shared__ int32_t s_m[kAltCells];
  __shared__ unsigned long long s_key[kAltLdsSlots];
  __shared__ double s_mass[kAltLdsSlots];
  __shared__ int s_count, s_over;
  const AltCuts C = {L <= kAltCells ? s_m : nullptr, o_begin};
  if (C.s_m)
    for (int k = tid; k < L; k += kAltThreads) s_m[k] = C.raw(k);
  for (int i = tid; i < kAltLdsSlots; i += kAltThreads) { s_key[i] = kAltEmpty; s_mass[i] = 0.0; }
  if (tid == 0) { s_count = 0; s_over = 0; }
  __syncthreads();   // (orders the zeroes of the outputs before the stores of the other lanes as well)
  alt_accumulate(X, gamma, na, C, L, s_key, s_mass, kAltLdsSlots, kAltLdsKeys, &s_count, &s_over, tid);
  __syncthreads();
  if (!s_over) {   // (the same in every lane)
    alt_select(s_key, s_mass, kAltLdsSlots, K, alt_word, alt_post, n_distinct, tid);
    return;
  }
  // more distinct keys than the LDS table takes: once more, in the pair's table in the workspace
  const int T = (int)Q.tab_slots;
  unsigned long long *tk = Q.tab_key + (size_t)pair * Q.tab_slots;
  double *tm = Q.tab_mass + (size_t)pair * Q.tab_slots;
  for (int i = tid; i < T; i += kAltThreads) { tk[i] = kAltEmpty; tm[i] = 0.0; }
  __syncthreads();
  if (tid == 0) { s_count = 0; s_over = 0; }
  __syncthreads();
  alt_accumulate(X, gamma, na, C, L, tk, tm, T, T, &s_count, &s_over, tid);   // (T > the lattice's arcs: never over)
  __syncthreads();
  alt_select(tk, tm, T, K, alt_word, alt_post, n_distinct, tid);
}

__global__ __launch_bounds__(kAltThreads) void slot_none_kernel(AlignDev A, PostDev P, AltDev Q, const int32_t *chans) {
  const int pair = blockIdx.x, slot = pair / A.n_seqs, c = chans[slot], tid = threadIdx.x;
  int4 *wa, *wb;
  const AlnIndex X = aln_carve(A, slot, &wa, &wb);
  const int cap = A.cap_words;
  const int32_t *o = A.out + (size_t)pair * (kAlignHead + 2 * (size_t)cap), *o_begin = o + kAlignHead;
  double *out = Q.none + (size_t)pair * cap, *g_early = Q.early + (size_t)pair * cap;
  for (int k = tid; k < cap; k += kAltThreads) { out[k] = 0.0; g_early[k] = 0.0; }
  const int L = A.seq_len[pair];
  if (!alt_runs(o, X, P, slot) || L <= 0) return;
  const int nd = X.head[3];
  const int4 *toks = Q.lat_toks + (size_t)c * Q.lat_tok_cap;
  const double *alpha = P.alpha + (size_t)slot * A.ns_cap, *beta = P.beta + (size_t)slot * A.ns_cap;
  const double log_z = P.log_z[slot];
  double *acost = Q.acost + (size_t)pair * A.ns_cap;
  int32_t *done = A.path + (size_t)pair * A.ns_cap;   // (confidence_kernel has read the aligned path)
  __shared__ int32_t s_m[kAltCells];
  __shared__ double s_none[kAltCells], s_early[kAltCells];
  const bool in_lds = L <= kAltCells;
  const AltCuts C = {in_lds ? s_m : nullptr, o_begin};
  if (in_lds)
    for (int k = tid; k < L; k += kAltThreads) {
      s_m[k] = C.raw(k);
      s_none[k] = 0.0;
      s_early[k] = 0.0;
    }
  __syncthreads();   // (orders the zeroes of the global rows before the additions of the other lanes as well)
  double *none = in_lds ? s_none : out, *early = in_lds ? s_early : g_early;
  int err = 0, k = 0;   // k: the cell of frame f, the last with m[k] <= f (the same in every lane)
  for (int f = 0; f <= nd && !err; ++f) {
    const int kprev = k;
    while (k + 1 < L && C.at(k + 1) <= f) ++k;
    const int lo = C.at(k), b = X.fbeg[f], e = X.fend[f];
    if (k != kprev)   // the frame begins a cell: its wordless in-arcs from earlier frames LEAVE the cell of the frame before
      for (int t = b + tid; t < e; t += kAltThreads) {
        const double tail = beta[t] + log_z;
        const int a1 = X.off[t + 1];
        for (int a = X.off[t]; a < a1; ++a) {
          const int4 R = X.recA[a];
          double cst;
          if (R.x < 0 || R.y != 0 || !post_cost(P, R, &cst)) continue;
          const double x = acost[R.x] + cst + tail;
          if (post_finite(x)) atomicAdd(&none[kprev], exp(-x));
        }
      }
    err = sweep_in<kAltThreads>(X, b, e, X.feps[f], done, [&](int t) {   // (a cycle: posterior_kernel has reported it, not reached)
      const double v = none_forward(P, X, alpha, acost, t, f, lo);
      acost[t] = v;
      if ((toks[t].w >> 30) & 1) none_final(v, alpha[t], log_z, none, early, k);
    });
  }
  __syncthreads();
  if (tid != 0) return;
  // the paths that ended before a cell began reach every later cell; a cell without a frame says nothing on every path
  double run = 0.0;
  for (int j = 0; j < L; ++j) {
    const bool empty = j + 1 < L && C.at(j) >= C.at(j + 1);
    const double here = none[j], ended = early[j];
    out[j] = err ? 0.0 : (empty ? 1.0 : here + run);
    run += ended;
  }
}

void launch_slot_mass(const AlignDev &A, const PostDev &P, const AltDev &Q, int cnt, hipStream_t s) {
  hipLaunchKernelGGL(slot_mass_kernel, dim3(cnt * A.n_seqs), dim3(kAltThreads), 0, s, A, P, Q);
}
void launch_slot_none(const AlignDev &A, const PostDev &P, const AltDev &Q, const int32_t *chans, int cnt, hipStream_t s) {
  hipLaunchKernelGGL(slot_none_kernel, dim3(cnt * A.n_seqs), dim3(kAltThreads), 0, s, A, P, Q, chans);
}

}  // namespace wfst
