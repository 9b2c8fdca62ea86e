// Lattice edit distance (wfst_decoder_nearest_words): given a reference r[0..L), the path of a channel's raw lattice nearest it -- the
// least word edit distance, the cheapest among those -- with the edit counts, the path's words, their times and scores.  The least
// distance over a lattice is its oracle error, Kaldi's lattice-oracle figure beside the 1-best WER kaldi-bin/bin/nbest-compute-wer.cc:
// 111-167 counts; the path, its operations and times are a lightly supervised alignment.  The generalisation of align_kernel
// (wfst_align.hip): the same lattice, in-arc index (align_index_kernel's, AlignDev::idx) and frame-ordered dynamic program.
//
// A cell v[s][k] is (errors, cost) in one 64-bit word, errors high, the cost's orderable float bits low: the lexicographic minimum is
// one unsigned minimum.  v[root][0] = (0, +0); over an arc s -> t at d' = (d + (graph + acoustic)) + 0.0f, finite: olabel 0 takes
// (s, k) to (t, k); a word takes (s, k) to (t, k + 1) with an error if it is not r[k], and (s, k) to (t, k) with one (an
// insertion); (s, k) goes to (s, k + 1) with one (a deletion) at d.
//
// nearest_kernel, one workgroup per (channel, reference):
//  - frames in ascending order, one lane per cell (state of the frame, k).  A cell PULLS its minimum over its state's in-arcs, up to
//    two candidates per arc (columns k and k - 1 of the finished source): no atomic read-modify-write, no backpointers.
//  - the deletion step is a prefix minimum along k, v[s][k] = k 2^32 + min_{j <= k} (v[s][j] - j 2^32): consecutive lanes hold
//    consecutive cells, so it is a segmented log-step scan inside the wave (six shuffles, on the value just pulled, before it is
//    stored), and behind a barrier a cell whose row began in an earlier 64-cell chunk takes the carry from those chunks' last
//    cells -- (L + 1) / 64 of them at the most, each already the prefix minimum of its own chunk's part of the row.
//  - a frame with arcs between its own states repeats "pull over those arcs, scan" until nothing moves (every step is monotone in
//    the cell order, so the fixpoint is the minimum over paths whatever the order), at most once per state of the frame.
//  - wave 0 picks the end, walks back by exact equality of the whole cell under the kind order and align_kernel's arc tuple, and
//    reads the steps front to back: every lane adds the costs in hop order (no tree) while lane 0 places counts, words, frames
//    and ref_hyp.
// The loads and stores of cells other lanes may be writing in the same pass (the sources of arcs inside a frame, the chunk ends of
// the carry) are relaxed 64-bit atomics: plain vector loads and stores that cannot tear; either value is a valid bound.
// Every loop is bounded by the lattice's or the reference's own sizes; nothing waits for another workgroup.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wfst_align_index.h"
#include "wfst_device.h"

namespace wfst {
namespace {

typedef unsigned long long u64;
constexpr int kNrThreads = 1024;
constexpr u64 kNrOne = 1ull << 32;   // one error

__device__ __forceinline__ u64 nr_load(const u64 *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void nr_store(u64 *p, u64 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// the cell reached over an arc of cost `arc` from a source cell `src`, `err` errors added: kNrUnreached where that is no transition
__device__ __forceinline__ u64 nr_extend(u64 src, float arc, uint32_t err) {
  if (src == kNrUnreached) return kNrUnreached;
  const float v = (aln_o2f((uint32_t)src) + arc) + 0.0f;   // (+ 0.0f: a zero total is +0)
  if (!(v - v == 0.0f)) return kNrUnreached;               // not finite
  return ((u64)((uint32_t)(src >> 32) + err) << 32) | aln_f2o(v);
}
__device__ __forceinline__ u64 nr_min(u64 a, u64 b) { return a < b ? a : b; }

}  // namespace

__global__ __launch_bounds__(kNrThreads) void nearest_kernel(AlignDev A, NearestDev N, const int32_t *chans) {
  const int pair = blockIdx.x, slot = pair / N.n_refs, c = chans[slot];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int4 *wa, *wb;
  const AlnIndex X = aln_carve(A, slot, &wa, &wb);
  const int cap = N.cap_words, cap_hyp = N.cap_hyp;
  int32_t *o = N.out + (size_t)pair * nearest_out_ints(cap, cap_hyp);
  int32_t *o_words = o + kNearestHead, *o_begin = o_words + cap_hyp, *o_end = o_begin + cap_hyp, *o_ref = o_end + cap_hyp;
  const int64_t cell0 = N.cell_off[pair];
  const int L = N.ref_len[pair];
  const int status = X.head[0];
  if (cell0 < 0 || L < 0 || L > cap || status) {   // not asked for, or no lattice to look at
    if (tid < kNearestHead) o[tid] = tid == 4 && cell0 >= 0 && status != kAlnNoLattice ? status : 0;
    return;
  }
  const int nd = X.head[3], W = L + 1;
  const int32_t *r = N.ref_words + (size_t)pair * cap;
  u64 *v = N.cells + cell0;
  const int4 *toks = N.lat_toks + (size_t)c * N.lat_tok_cap;
  __shared__ int s_err;
  if (tid == 0) s_err = 0;
  // ---- the table, frame by frame -------------------------------------------------------------------------------------
  for (int f = 0; f <= nd; ++f) {
    const int b = X.fbeg[f], e = X.fend[f], ncell = (e - b) * W;
    const bool eps_frame = X.feps[f] != 0;
    u64 *vf = v + (size_t)b * W;   // the frame's cells: consecutive, a row per state
    for (int round = 0;; ++round) {
      int moved = 0;
      // (the trip count is the workgroup's, not the lane's: the shuffles below need whole waves)
      for (int base = 0; base < ncell; base += kNrThreads) {
        const int cell = base + tid;
        const bool active = cell < ncell;
        const int t = b + cell / W, k = cell % W;
        u64 old = kNrUnreached, best = kNrUnreached;
        if (active) {
          old = round ? nr_load(&vf[cell]) : (t == 0 && k == 0 ? (u64)aln_f2o(0.0f) : kNrUnreached);
          best = old;
          const int a1 = X.off[t + 1];
          for (int a = X.off[t]; a < a1; ++a) {
            const int4 R = X.recA[a];
            if ((R.x < 0) != (round > 0)) continue;   // round 0: the emitting in-arcs; later rounds: the arcs inside the frame
            const u64 *row = v + (size_t)(R.x & 0x7FFFFFFF) * W;
            const float arc = __int_as_float(R.z) + __int_as_float(R.w);   // (rounded first: tot += graph + acoustic)
            best = nr_min(best, nr_extend(nr_load(&row[k]), arc, R.y != 0));   // a free arc, or an insertion
            if (R.y != 0 && k > 0) best = nr_min(best, nr_extend(nr_load(&row[k - 1]), arc, R.y != r[k - 1]));   // match / substitution
          }
        }
        // the deletion step inside the wave: lane - step holds cell - step, which is of this row iff k >= step
#pragma unroll
        for (int step = 1; step < 64; step <<= 1) {
          const u64 up = __shfl_up(best, step, 64);
          if (lane >= step && k >= step && up != kNrUnreached) best = nr_min(best, up + (u64)step * kNrOne);
        }
        if (active && (round == 0 || best < old)) { nr_store(&vf[cell], best); moved = 1; }
      }
      if (W > 1) {
        __syncthreads();   // (this round's stores before the carry's loads)
        for (int cell = tid; cell < ncell; cell += kNrThreads) {
          const int k = cell % W;
          if (k <= lane) continue;   // the row begins in this cell's own 64-cell chunk
          const int row0 = cell - k;
          const u64 cur = nr_load(&vf[cell]);
          u64 best = cur;
          for (int m = cell - lane - 1; m >= row0; m -= 64) {   // the last cells of the row's earlier chunks
            const u64 up = nr_load(&vf[m]);
            if (up != kNrUnreached) best = nr_min(best, up + (u64)(cell - m) * kNrOne);
          }
          if (best < cur) { nr_store(&vf[cell], best); moved = 1; }
        }
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
    if (lane < kNearestHead) o[lane] = lane == 4 ? s_err : 0;
    return;
  }
  // ---- the end: the final state with the least v[.][L], the least graph state among equals -------------------------------
  int t = -1;
  {
    u64 mine = kNrUnreached, mine2 = ~0ull;
    for (int i = X.fbeg[nd] + lane; i < X.fend[nd]; i += 64) {
      const int4 tk = toks[i];
      if (!((tk.w >> 30) & 1)) continue;
      const u64 x = v[(size_t)i * W + L];
      if (x == kNrUnreached) continue;
      const u64 x2 = ((u64)(uint32_t)tk.y << 32) | (uint32_t)i;
      if (x < mine || (x == mine && x2 < mine2)) { mine = x; mine2 = x2; }
    }
    const u64 best = aln_wave_min_64(mine);
    if (best != kNrUnreached) t = (int)(uint32_t)aln_wave_min_64(mine == best ? mine2 : ~0ull);
  }
  if (t < 0) {   // no final state is reached
    if (lane < kNearestHead) o[lane] = 0;
    return;
  }
  const u64 end_cell = v[(size_t)t * W + L];
  // ---- the walk back: exact equality of the cell, the kind order, the arc tuple ------------------------------------------
  int32_t *path = N.path + (size_t)pair * N.path_cap;
  int n = 0, k = L, err = 0;
  while (t != 0 || k != 0) {
    if (n >= N.path_cap) { err = kAlnInternal; break; }
    const u64 here = v[(size_t)t * W + k];
    const int a0 = X.off[t], a1 = X.off[t + 1];
    u64 k0 = ~0ull, k1 = ~0ull, k2 = ~0ull;
    uint32_t k3 = 0xFFFFFFFFu;
    int my_a = -1, my_src = 0;
    for (int a = a0 + lane; a < a1; a += 64) {
      const int4 R = X.recA[a];
      const int src = R.x & 0x7FFFFFFF;
      const u64 *row = v + (size_t)src * W;
      const float arc = __int_as_float(R.z) + __int_as_float(R.w);
      int kind = -1;   // (the arc's own candidates: a match / substitution comes before its insertion)
      if (R.y != 0 && k > 0 && nr_extend(row[k - 1], arc, R.y != r[k - 1]) == here) kind = 0;
      else if (nr_extend(row[k], arc, R.y != 0) == here) kind = R.y != 0 ? 2 : 1;
      if (kind < 0) continue;   // (here is a reached cell: kNrUnreached never equals it)
      const int4 S = X.recB[a];
      const u64 c1 = ((u64)(R.x < 0 ? 1 : 0) << 63) | ((u64)(uint32_t)S.x << 32) | (uint32_t)S.y;
      const u64 c2 = ((u64)(uint32_t)R.y << 32) | (uint32_t)R.z;
      const uint32_t c3 = (uint32_t)R.w;
      if (my_a < 0 || (u64)kind < k0 || ((u64)kind == k0 && (c1 < k1 || (c1 == k1 && (c2 < k2 || (c2 == k2 && c3 < k3)))))) {
        k0 = (u64)kind; k1 = c1; k2 = c2; k3 = c3; my_a = a; my_src = src;
      }
    }
    u64 cand = __ballot(my_a >= 0);
    if (!cand) {   // no arc arrives here exactly: the deletion step, the last kind
      const u64 left = k > 0 ? v[(size_t)t * W + k - 1] : kNrUnreached;
      if (left == kNrUnreached || left + kNrOne != here) { err = kAlnInternal; break; }   // (a reached cell without its arrival)
      if (lane == 0) path[n] = (int32_t)(3u << 30);
      ++n;
      --k;
      continue;
    }
    if (__popcll(cand) > 1) {
      const u64 m0 = aln_wave_min_64(my_a >= 0 ? k0 : ~0ull);
      const bool at0 = my_a >= 0 && k0 == m0;
      const u64 m1 = aln_wave_min_64(at0 ? k1 : ~0ull);
      const bool at1 = at0 && k1 == m1;
      const u64 m2 = aln_wave_min_64(at1 ? k2 : ~0ull);
      const bool at2 = at1 && k2 == m2;
      const u64 m3 = aln_wave_min_64(at2 ? (u64)k3 : ~0ull);
      cand = __ballot(at2 && (u64)k3 == m3);
    }
    const int win = __ffsll((long long)cand) - 1;
    const int a = __shfl(my_a, win, 64), kind = (int)__shfl((int)k0, win, 64);
    if (lane == 0) path[n] = (int32_t)(((uint32_t)kind << 30) | (uint32_t)a);
    ++n;
    t = __shfl(my_src, win, 64);
    if (kind == 0) --k;
  }
  if (err) {
    if (lane < kNearestHead) o[lane] = lane == 4 ? err : 0;
    return;
  }
  // ---- front to back: the sums in hop order, the counts, the words and their times ---------------------------------------
  // (lane 0's stores to path[] are read back by the other lanes: one wave, in program order behind the stores' completion)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  float lm = 0.0f, tot = 0.0f;
  int kw = 0, kr = 0, end_c = 0, begin_c = 0;   // hypothesis words and reference words so far, one past the newest non-silence emitting hop, the newest word's begin
  int n_arcs = 0, n_cor = 0, n_sub = 0, n_ins = 0, n_del = 0;
  for (int base = 0; base < n; base += 64) {
    const int m = min(64, n - base);
    int4 R = make_int4(0, 0, 0, 0), S = make_int4(0, 0, 0, 0);
    int kind = 1;
    if (lane < m) {
      const uint32_t p = (uint32_t)path[n - 1 - (base + lane)];
      kind = (int)(p >> 30);
      if (kind != 3) {
        R = X.recA[p & 0x3FFFFFFFu];
        S = X.recB[p & 0x3FFFFFFFu];
      }
    }
    const bool eps = R.x < 0;
    const bool sil = N.sil_bits && S.y > 0 && S.y <= N.n_tid && ((N.sil_bits[S.y >> 5] >> (S.y & 31)) & 1u);
    const int endv = (lane < m && kind != 3 && !eps && !sil) ? S.z + 1 : 0;
    for (int j = 0; j < m; ++j) {
      const int kd = __shfl(kind, j, 64);
      if (kd == 3) {
        if (kr >= L) { err = kAlnInternal; break; }
        if (lane == 0) o_ref[kr] = -1;
        ++kr;
        ++n_del;
        continue;
      }
      const int word = __shfl(R.y, j, 64), F = __shfl(S.z, j, 64), ev = __shfl(endv, j, 64);
      const float g = __int_as_float(__shfl(R.z, j, 64));
      lm += g;
      tot = (tot + (g + __int_as_float(__shfl(R.w, j, 64)))) + 0.0f;
      ++n_arcs;
      if (word != 0) {
        if (lane == 0 && kw >= 1 && kw <= cap_hyp) o_end[kw - 1] = max(end_c, begin_c);
        if (lane == 0 && kw < cap_hyp) { o_words[kw] = word; o_begin[kw] = F; }
        begin_c = F;
        if (kd == 0) {
          if (kr >= L) { err = kAlnInternal; break; }
          if (word == r[kr]) ++n_cor; else ++n_sub;
          if (lane == 0) o_ref[kr] = kw;
          ++kr;
        } else {
          ++n_ins;
        }
        ++kw;
      }
      end_c = max(end_c, ev);
    }
    if (err) break;
  }
  // (the path read forwards must reproduce the cell it was traced from: its errors and, added up in hop order, its cost)
  if (!err && (kr != L || aln_f2o(tot) != (uint32_t)end_cell || (uint32_t)(n_sub + n_ins + n_del) != (uint32_t)(end_cell >> 32))) err = kAlnInternal;
  if (lane == 0) {
    if (!err && kw >= 1 && kw <= cap_hyp) o_end[kw - 1] = max(end_c, begin_c);   // (no silence list: the frames the path consumed = the end state's frame)
    o[0] = err ? 0 : 1; o[1] = n_arcs; o[2] = __float_as_int(tot); o[3] = __float_as_int(lm); o[4] = err;
    o[5] = n_sub + n_ins + n_del; o[6] = n_cor; o[7] = n_sub; o[8] = n_ins; o[9] = n_del; o[10] = kw; o[11] = 0;
  }
}

void launch_nearest(const AlignDev &A, const NearestDev &N, const int32_t *chans, int cnt, hipStream_t s) {
  hipLaunchKernelGGL(nearest_kernel, dim3(cnt * N.n_refs), dim3(kNrThreads), 0, s, A, N, chans);
}

}  // namespace wfst
