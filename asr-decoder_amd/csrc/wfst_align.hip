// Lattice-constrained word alignment (wfst_decoder_align_words): given a word sequence w[0..L), the cheapest path of a channel's
// raw lattice that spells it, with that path's word times and scores -- what gives an n-best path, a rescored 1-best
// (kaldi-nnet3/kaldi-online-nnet3-my-decoder.cc:122-130) or an outside transcript the (start, end) per word that the services'
// AlignStruct carries for the first-pass best path (gpu-asr/gpu-worker-pool-itf.h:85-97); the determinizer drops the input labels
// (OutputNoolabel), so the times have to come from the raw lattice.
//
// The recurrence, over the lattice lat_toks[] / lat_arcs[] hold (state = position in lat_toks[], arena order: frames ascending, the
// root token first): d[root][0] = 0; an arc s -> t with olabel 0 takes (s, k) to (t, k), one with olabel == w[k] takes (s, k) to
// (t, k + 1), at d[s][k] + (graph + acoustic) in float32, the arc's own sum rounded first (LatticeToVector's order); a zero total
// is +0; a total that is not finite is no path.  The answer ends in the final state with the least d[.][L], the least graph
// state among equals.
//
// align_index_kernel, one workgroup per listed channel: the by-destination in-arc index nbest_kernel builds for itself
// (wfst_nbest.hip), kept in the workspace for all of the channel's sequences.
// align_kernel, one workgroup per (channel, sequence):
//  - frames in ascending order, one lane per cell (state of the frame, k).  A cell PULLS its minimum over the state's in-arcs: the
//    emitting ones leave the finished previous frame, so a frame is one pass and a barrier, with no atomic (an HBM atomic costs
//    about 17 plain stores here: tools/ubench_atomics.hip); a frame with epsilon arcs between its own states repeats the pass over
//    those arcs until nothing moves (float addition is monotone, so the fixpoint is the minimum over the sources' final values
//    whatever the order), at most once per state of the frame.  Only d[states][L + 1] is kept: no backpointers.
//  - wave 0 then walks back from the end: at (t, k) the in-arcs whose source cell plus the arc's cost equal d[t][k] exactly are
//    the candidates, the least under THE ALIGNMENT'S TIE RULE (emitting before epsilon, graph state of the source token, ilabel,
//    olabel, graph bits, acoustic bits -- nothing that depends on the order the device listed the arcs in) is taken.  The hops go
//    to the workspace last first; the same wave then reads them front to back, 64 at a time, and every lane adds the costs up in
//    hop order (no tree: lm_score must round as the host's loop does) while it places the words' begin and end frames by
//    words_kernel's definition (wfst_kernels.hip).
// Every loop is bounded by the lattice's own sizes; nothing waits for another workgroup.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wfst_align_index.h"   // AlnIndex / aln_carve, aln_f2o / aln_o2f, aln_wave_min_64
#include "wfst_device.h"

namespace wfst {
namespace {

typedef unsigned long long u64;
constexpr int kAlnThreads = 1024;

// the cost of arriving over an in-arc from a source cell that holds `src` (orderable bits): false where that is no path
__device__ __forceinline__ bool aln_extend(uint32_t src, int32_t graph_bits, int32_t ac_bits, float *out) {
  if (src == kAlnUnreached) return false;
  const float arc = __int_as_float(graph_bits) + __int_as_float(ac_bits);   // (rounded first: tot += graph + acoustic)
  const float v = (aln_o2f(src) + arc) + 0.0f;                              // (+ 0.0f: a zero total is +0)
  *out = v;
  return v - v == 0.0f;   // finite
}

}  // namespace

__global__ __launch_bounds__(kAlnThreads) void align_index_kernel(DecoderDev D, AlignDev A, const int32_t *chans) {
  const int slot = blockIdx.x, c = chans[slot], tid = threadIdx.x;
  const ChanCtl *ctl = D.ctl + c;
  const int nd = ctl->n_decoded, nt = ctl->lat_toks, na = ctl->lat_arcs;
  const int4 *toks = D.lat_toks + (size_t)c * D.lat_tok_cap;
  const LatArc *arcs = D.lat_arcs + (size_t)c * D.lat_arc_cap;
  int32_t *state_of = D.remap + (size_t)c * D.arena_cap;   // arena index -> lattice state (scratch between pruning passes, as determinize_kernel's)
  int4 *recA, *recB;
  const AlnIndex X = aln_carve(A, slot, &recA, &recB);
  __shared__ int s_part[kAlnThreads];
  __shared__ int s_gap;
  int status = 0;
  if (ctl->error) status = kAlnChannelError;
  else if (nt <= 0 || nd <= 0) status = kAlnNoLattice;
  else if (nt > A.ns_cap || na > A.na_cap || nd + 1 > A.fr_cap || na < 0) status = kAlnTooLarge;
  else if (toks[0].x != 0) status = kAlnInternal;   // the root token is arena entry 0 and lat_toks[] is in arena order
  if (tid == 0) { X.head[0] = status; X.head[1] = nt; X.head[2] = na; X.head[3] = nd; s_gap = 0; }
  if (status) return;
  for (int f = tid; f <= nd; f += kAlnThreads) { X.fbeg[f] = 0; X.fend[f] = 0; X.feps[f] = 0; }
  __syncthreads();
  for (int i = tid; i < nt; i += kAlnThreads) {
    const int4 t = toks[i];
    state_of[t.x] = i;
    X.off[i] = 0;
    const int f = t.w & 0x3FFFFFFF;
    if (f > nd) { s_gap = 1; continue; }
    if (i == 0 || (toks[i - 1].w & 0x3FFFFFFF) != f) X.fbeg[f] = i;
    if (i == nt - 1 || (toks[i + 1].w & 0x3FFFFFFF) != f) X.fend[f] = i + 1;
  }
  __syncthreads();
  // GetRawLattice returns false when a frame has no token left (base-inl.h:906-911)
  for (int f = tid; f <= nd; f += kAlnThreads)
    if (X.fend[f] <= X.fbeg[f]) s_gap = 1;
  __syncthreads();
  if (s_gap) {
    if (tid == 0) X.head[0] = kAlnNoLattice;
    return;
  }
  for (int a = tid; a < na; a += kAlnThreads) {
    const LatArc L = arcs[a];
    atomicAdd(&X.off[state_of[L.dst_tok]], 1);
    if (L.is_eps) X.feps[L.src_frame] = 1;   // (an epsilon arc stays inside its frame)
  }
  __syncthreads();
  {  // exclusive scan of off[0..nt) (one contiguous slice per thread)
    const int per = (nt + kAlnThreads - 1) / kAlnThreads, b = min(nt, tid * per), e = min(nt, b + per);
    int sum = 0;
    for (int i = b; i < e; ++i) sum += X.off[i];
    s_part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
      int run = 0;
      for (int i = 0; i < kAlnThreads; ++i) { const int v = s_part[i]; s_part[i] = run; run += v; }
    }
    __syncthreads();
    int run = s_part[tid];
    for (int i = b; i < e; ++i) { const int v = X.off[i]; X.off[i] = run; X.cur[i] = run; run += v; }
    if (tid == 0) X.off[nt] = na;
  }
  __syncthreads();
  for (int a = tid; a < na; a += kAlnThreads) {
    const LatArc L = arcs[a];
    const int src = state_of[L.src_tok];
    const int p = atomicAdd(&X.cur[state_of[L.dst_tok]], 1);
    recA[p] = make_int4(src | (L.is_eps ? (int)0x80000000 : 0), L.olabel, __float_as_int(L.graph), __float_as_int(L.acoustic));
    recB[p] = make_int4(toks[src].y, L.ilabel, L.src_frame, 0);
  }
}

__global__ __launch_bounds__(kAlnThreads) void align_kernel(DecoderDev D, AlignDev A, const int32_t *chans) {
  const int pair = blockIdx.x, slot = pair / A.n_seqs, c = chans[slot];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int4 *wa, *wb;
  const AlnIndex X = aln_carve(A, slot, &wa, &wb);
  const int cap = A.cap_words;
  int32_t *o = A.out + (size_t)pair * (kAlignHead + 2 * (size_t)cap);
  int32_t *o_begin = o + kAlignHead, *o_end = o_begin + cap;
  const int64_t cell0 = A.cell_off[pair];
  const int L = A.seq_len[pair];
  const int status = X.head[0];
  if (cell0 < 0 || L < 0 || L > cap || status) {   // not asked for, or no lattice to look at
    if (tid < kAlignHead) o[tid] = tid == 4 && cell0 >= 0 && status != kAlnNoLattice ? status : 0;
    return;
  }
  const int nt = X.head[1], nd = X.head[3], W = L + 1;
  const int32_t *w = A.seq_words + (size_t)pair * cap;
  uint32_t *d = A.cells + cell0;
  const int4 *toks = D.lat_toks + (size_t)c * D.lat_tok_cap;
  __shared__ int s_err;
  if (tid == 0) s_err = 0;
  // ---- the table, frame by frame -------------------------------------------------------------------------------------
  for (int f = 0; f <= nd; ++f) {
    const int b = X.fbeg[f], e = X.fend[f], ncell = (e - b) * W;
    const bool eps_frame = X.feps[f] != 0;
    for (int round = 0;; ++round) {
      int moved = 0;
      for (int cell = tid; cell < ncell; cell += kAlnThreads) {
        const int t = b + cell / W, k = cell % W;
        const uint32_t old = round ? d[(size_t)t * W + k] : (t == 0 && k == 0 ? aln_f2o(0.0f) : kAlnUnreached);
        uint32_t best = old;
        const int a1 = X.off[t + 1];
        for (int a = X.off[t]; a < a1; ++a) {
          const int4 R = X.recA[a];
          if ((R.x < 0) != (round > 0)) continue;   // round 0: the emitting in-arcs; later rounds: the epsilon in-arcs
          int kk = k;
          if (R.y != 0) {
            if (k == 0 || R.y != w[k - 1]) continue;
            kk = k - 1;
          }
          float v;
          if (!aln_extend(d[(size_t)(R.x & 0x7FFFFFFF) * W + kk], R.z, R.w, &v)) continue;
          best = min(best, aln_f2o(v));
        }
        if (round == 0 || best < old) { d[(size_t)t * W + k] = best; moved = 1; }
      }
      moved = __syncthreads_or(moved);   // (the barrier also orders this round's stores before the next round's loads)
      if (!eps_frame || (round > 0 && !moved)) break;
      if (round > e - b) {   // an epsilon path visits a state of the frame once: more rounds than states is a cycle
        if (tid == 0) s_err = kAlnCycle;
        break;
      }
    }
  }
  __syncthreads();
  if (wave != 0) return;
  if (s_err) {
    if (lane < kAlignHead) o[lane] = lane == 4 ? s_err : 0;
    return;
  }
  // ---- the end: the final state with the least d[.][L], the least graph state among equals -------------------------------
  int t = -1;
  {
    u64 mine = ~0ull;
    int my_t = -1;
    for (int i = X.fbeg[nd] + lane; i < X.fend[nd]; i += 64) {
      const int4 tk = toks[i];
      if (!((tk.w >> 30) & 1)) continue;
      const uint32_t v = d[(size_t)i * W + L];
      if (v == kAlnUnreached) continue;
      const u64 key = ((u64)v << 32) | (uint32_t)tk.y;
      if (key < mine) { mine = key; my_t = i; }
    }
    const u64 best = aln_wave_min_64(mine);
    if (best != ~0ull) t = __shfl(my_t, __ffsll((long long)__ballot(mine == best)) - 1, 64);
  }
  if (t < 0) {   // the sequence is not in the lattice
    if (lane < kAlignHead) o[lane] = 0;
    return;
  }
  const uint32_t tot_bits = __float_as_uint(aln_o2f(d[(size_t)t * W + L]));
  // ---- the walk back: exact equality, the tie rule ---------------------------------------------------------------------
  int32_t *path = A.path + (size_t)pair * A.ns_cap;
  int n = 0, k = L, err = 0;
  while (t != 0) {
    if (n >= nt) { err = kAlnInternal; break; }
    const float here = aln_o2f(d[(size_t)t * W + k]);
    const int a0 = X.off[t], a1 = X.off[t + 1];
    u64 k1 = ~0ull, k2 = ~0ull;
    uint32_t k3 = 0xFFFFFFFFu;
    int my_a = -1, my_src = 0, my_k = 0;
    for (int a = a0 + lane; a < a1; a += 64) {
      const int4 R = X.recA[a];
      int kk = k;
      if (R.y != 0) {
        if (k == 0 || R.y != w[k - 1]) continue;
        kk = k - 1;
      }
      const int src = R.x & 0x7FFFFFFF;
      float v;
      if (!aln_extend(d[(size_t)src * W + kk], R.z, R.w, &v) || v != here) continue;
      const int4 S = X.recB[a];
      const u64 c1 = ((u64)(R.x < 0 ? 1 : 0) << 63) | ((u64)(uint32_t)S.x << 32) | (uint32_t)S.y;
      const u64 c2 = ((u64)(uint32_t)R.y << 32) | (uint32_t)R.z;
      const uint32_t c3 = (uint32_t)R.w;
      if (my_a < 0 || c1 < k1 || (c1 == k1 && (c2 < k2 || (c2 == k2 && c3 < k3)))) {
        k1 = c1; k2 = c2; k3 = c3; my_a = a; my_src = src; my_k = kk;
      }
    }
    u64 cand = __ballot(my_a >= 0);
    if (!cand) { err = kAlnInternal; break; }   // (a reached cell without the arrival that made it: never expected)
    if (__popcll(cand) > 1) {
      const u64 m1 = aln_wave_min_64(my_a >= 0 ? k1 : ~0ull);
      const bool at1 = my_a >= 0 && k1 == m1;
      const u64 m2 = aln_wave_min_64(at1 ? k2 : ~0ull);
      const bool at2 = at1 && k2 == m2;
      const u64 m3 = aln_wave_min_64(at2 ? (u64)k3 : ~0ull);
      cand = __ballot(at2 && (u64)k3 == m3);
    }
    const int win = __ffsll((long long)cand) - 1;
    const int a = __shfl(my_a, win, 64);
    if (lane == 0) path[n] = a;
    ++n;
    t = __shfl(my_src, win, 64);
    k = __shfl(my_k, win, 64);
  }
  if (!err && k != 0) err = kAlnInternal;
  if (err) {
    if (lane < kAlignHead) o[lane] = lane == 4 ? err : 0;
    return;
  }
  // ---- front to back: the two sums in hop order, the words' times ------------------------------------------------------
  // (lane 0's stores to path[] are read back by the other lanes: one wave, in program order behind the stores' completion)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  float lm = 0.0f;
  int kw = 0, end_c = 0, begin_c = 0;   // words so far, one past the newest non-silence emitting hop, the newest word's begin
  for (int base = 0; base < n; base += 64) {
    const int m = min(64, n - base);
    int4 R = make_int4(0, 0, 0, 0), S = make_int4(0, 0, 0, 0);
    if (lane < m) {
      const int a = path[n - 1 - (base + lane)];
      R = X.recA[a];
      S = X.recB[a];
    }
    const bool eps = R.x < 0;
    const bool sil = A.sil_bits && S.y > 0 && S.y <= A.n_tid && ((A.sil_bits[S.y >> 5] >> (S.y & 31)) & 1u);
    const int endv = (lane < m && !eps && !sil) ? S.z + 1 : 0;
    for (int j = 0; j < m; ++j) {
      const int word = __shfl(R.y, j, 64), F = __shfl(S.z, j, 64), ev = __shfl(endv, j, 64);
      lm += __int_as_float(__shfl(R.z, j, 64));
      if (word != 0) {
        if (lane == 0 && kw >= 1 && kw <= L) o_end[kw - 1] = max(end_c, begin_c);
        if (lane == 0 && kw < L) o_begin[kw] = F;
        begin_c = F;
        ++kw;
      }
      end_c = max(end_c, ev);
    }
  }
  if (lane == 0) {
    if (kw >= 1 && kw <= L) o_end[kw - 1] = max(end_c, begin_c);   // (no silence list: the frames the path consumed = the end state's frame)
    o[0] = 1; o[1] = n; o[2] = (int32_t)tot_bits; o[3] = __float_as_int(lm);
    o[4] = kw == L ? 0 : kAlnInternal; o[5] = 0; o[6] = 0; o[7] = 0;
  }
}

void launch_align_index(const DecoderDev &D, const AlignDev &A, const int32_t *chans, int cnt, hipStream_t s) {
  hipLaunchKernelGGL(align_index_kernel, dim3(cnt), dim3(kAlnThreads), 0, s, D, A, chans);
}
void launch_align(const DecoderDev &D, const AlignDev &A, const int32_t *chans, int cnt, hipStream_t s) {
  hipLaunchKernelGGL(align_kernel, dim3(cnt * A.n_seqs), dim3(kAlnThreads), 0, s, D, A, chans);
}

}  // namespace wfst
