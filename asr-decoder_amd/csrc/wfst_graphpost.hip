// Graph posteriors (wfst_decoder_graph_posteriors): the forward-backward pass, in the log semiring and in float64, of a channel's scores
// against that utterance's own small graph -- the sum over the paths wfst_decoder_force_align takes the best of -- with the tables
// alpha[f][s] and beta[f][s] of include/wfst_decoder.h.  Nothing here reads the search's tokens: the scores only.
//
// graphpost_kernel, one workgroup per list entry, no atomic on a float, nothing waits for another workgroup:
//  - forward, the frames in order: a lane per DESTINATION state takes ONE two-pass log-sum (post_logsum) over the state's in-arc records
//    (ForcedGraphsDev) -- the emitting records read the finished row of frame f - 1, the epsilon records the row being made.  The
//    states without an epsilon in-arc go first, then level by level of the graph's epsilon DAG, one barrier each.  Every cell goes
//    to the (T + 1) x S table in the workspace as well.
//  - backward, the frames in reverse: a lane per SOURCE state takes the same sum over its out-arcs (GpostGraphsDev), the states by
//    the longest epsilon path OUT of them, ascending: a state reads beta of the frame behind it through its emitting arcs and beta
//    of lower levels of its own frame through its epsilon arcs.  The same lane then computes gamma of its own out-arcs against the
//    stored alpha cell, stores the emitting arcs' into gamma[] of the frame and adds every arc's into the arc's occupancy: an arc has
//    one source state and a state one lane, so no atomic is needed.
//  - behind a frame's last level a lane per class slot sums the gammas of the slot's arcs in the order of the host's CSR into the
//    [T][slots] table.  gamma[] is double buffered by frame parity, so that this pass needs no barrier of its own.
//  - the two live rows are in LDS for a graph of up to kGpostLdsStates states and in the workspace beyond; the same code either way.
//  - the scores of a frame are staged in LDS one frame ahead (forward) or behind (backward) where the graph has at most
//    kFalignLdsLabels distinct ilabels, as forced_align_kernel stages them; beyond that they are gathered from the frame's row.
// graphpost_pack_kernel, one workgroup per entry: per frame the list's length, n_distinct and frame_mass, the scan of the lengths
// (pack_frame_off), the lists by class ascending, the occupancies.  graphpost_dense_kernel, one workgroup per (entry, frame row):
// n_cols zeros, a barrier, then float32(grad_scale * post) at the column of every class with post > 0, plain stores.
// Every loop is bounded by the graph's and the utterance's own sizes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wfst_device.h"
#include "wfst_lattice_sweep.h"   // post_inf / post_finite / post_logsum, pack_frame_off

namespace wfst {
namespace {

constexpr int kGpThreads = 256;
constexpr int kGpPre = kFalignLdsLabels / kGpThreads;   // scores a lane fetches ahead

// c(f, a) and c(a), operation by operation as the header states them; false where the arc is no arc
__device__ __forceinline__ bool gp_emit_cost(const GpostDev &Q, float ll, float w, double *c) {
#pragma clang fp contract(off)
  const float x = -ll;
  const double ac = Q.acoustic_scale * (double)x;
  const double gc = Q.graph_scale * (double)w;
  *c = ac + gc;
  return x - x == 0.0f && w - w == 0.0f;
}
__device__ __forceinline__ bool gp_eps_cost(const GpostDev &Q, float w, double *c) {
#pragma clang fp contract(off)
  *c = Q.graph_scale * (double)w;
  return w - w == 0.0f;
}

template <bool kLds>
__device__ __forceinline__ void gpost_run(const GpostDev &Q, const GpostChan &C, const int32_t *H, double *s_rows, float *s_sc) {
  const int tid = threadIdx.x;
  const int start = H[0], fin = H[1], S = H[2], A = H[3], depth = H[4], NL = H[5];
  const int2 *in_off = Q.G.in_off + H[6];
  const int4 *rec = Q.G.rec + H[7];
  const int32_t *lvl_state = Q.G.lvl_state + H[8], *lvl_off = Q.G.lvl_off + H[9], *labels = Q.G.labels + H[10];
  const int32_t *BH = Q.B.bhdr + (int64_t)C.graph * kGpostHdr;
  const int2 *out_off = Q.B.out_off + BH[0];
  const int4 *orec = Q.B.orec + BH[1];
  const int32_t *blvl_state = Q.B.blvl_state + BH[2], *blvl_off = Q.B.blvl_off + BH[3];
  const int bdepth = BH[4];
  const int T = C.T, NS = C.n_slots;
  const int64_t stride = C.stride;
  const float *ll = C.ll;
  double *tab = Q.tab + C.tab_off;
  double *rows = kLds ? s_rows : Q.rows + C.row_off;
  const int RS = kLds ? kGpostLdsStates : S;
  double *gam = Q.gam + C.gam_off, *occ = gam + 2 * (int64_t)A;
  double *post = Q.post + C.post_off;
  const int32_t *slot_off = Q.cls + C.cls_off + NS, *slot_arc = slot_off + NS + 1;
  const bool staged = NL <= kFalignLdsLabels;
  // the columns of the labels this lane stages
  int col[kGpPre];
#pragma unroll
  for (int k = 0; k < kGpPre; ++k) {
    const int j = tid + k * kGpThreads;
    col[k] = 0;
    if (staged && j < NL) { const int il = labels[j]; col[k] = Q.col_map ? Q.col_map[il] : il; }
  }
  // the scores of frame g (0 <= g < T) into the staging half g & 1, behind the pass that runs meanwhile
  float pre[kGpPre];
  auto fetch = [&](int g) {
#pragma unroll
    for (int k = 0; k < kGpPre; ++k)
      if (tid + k * kGpThreads < NL) pre[k] = ll[(int64_t)g * stride + col[k]];
  };
  auto stash = [&](int g) {
#pragma unroll
    for (int k = 0; k < kGpPre; ++k)
      if (tid + k * kGpThreads < NL) s_sc[(g & 1) * kFalignLdsLabels + tid + k * kGpThreads] = pre[k];
  };
  // the score of label slot j at frame g, whose staged half is sc
  auto score = [&](const float *sc, int g, int j) -> float {
    if (staged) return sc[j];
    const int il = labels[j];
    return ll[(int64_t)g * stride + (Q.col_map ? Q.col_map[il] : il)];
  };

  // ---- forward ---------------------------------------------------------------------------------------------------------------------
  for (int f = 0; f <= T; ++f) {
    const double *prev = rows + ((f + 1) & 1) * RS;   // frame f - 1
    double *cur = rows + (f & 1) * RS;
    const float *sc = s_sc + ((f + 1) & 1) * kFalignLdsLabels;
    double *tabf = tab + (int64_t)f * S;
    const bool ahead = staged && f < T;
    if (ahead) fetch(f);
    auto cell = [&](int t) {
      const int2 o = in_off[t];
      const double v = post_logsum(f > 0 ? o.x : o.y, in_off[t + 1].x, [&](int a, double *x) {
        const int4 R = rec[a];
        double c;
        if (R.y >= 0) {
          if (!gp_emit_cost(Q, score(sc, f - 1, R.y), __int_as_float(R.z), &c)) return false;
          *x = prev[R.x] + c;
        } else {
          if (!gp_eps_cost(Q, __int_as_float(R.z), &c)) return false;
          *x = cur[R.x] + c;
        }
        return post_finite(*x);
      }, f == 0 && t == start, 0.0);
      cur[t] = v;
      tabf[t] = v;
    };
    for (int t = tid; t < S; t += kGpThreads)
      if (in_off[t].y == in_off[t + 1].x) cell(t);   // no epsilon in-arc: level 0
    if (ahead) stash(f);
    __syncthreads();
    for (int L = 1; L <= depth; ++L) {
      for (int i = lvl_off[L - 1] + tid; i < lvl_off[L]; i += kGpThreads) cell(lvl_state[i]);
      __syncthreads();
    }
  }
  const double tot = rows[(T & 1) * RS + fin];
  if (!post_finite(tot)) return;   // not found: the zeros the host filled in stand
  __syncthreads();                 // every lane has read tot: the rows are free for beta

  // ---- backward, gamma, the class sums ------------------------------------------------------------------------------------------------
  for (int f = T; f >= 0; --f) {
    const double *nxt = rows + ((f + 1) & 1) * RS;   // frame f + 1
    double *cur = rows + (f & 1) * RS;
    const float *sc = s_sc + (f & 1) * kFalignLdsLabels;
    const double *tabf = tab + (int64_t)f * S;
    double *gamf = gam + (int64_t)(f & 1) * A;
    const bool ahead = staged && f > 0 && f < T;   // (frame T - 1's scores lie in their half since the forward pass staged them)
    if (ahead) fetch(f - 1);
    for (int L = 0; L <= bdepth; ++L) {
      for (int i = blvl_off[L] + tid; i < blvl_off[L + 1]; i += kGpThreads) {
        const int s = blvl_state[i];
        const int2 o = out_off[s];
        const int a_end = out_off[s + 1].x, a1 = f < T ? a_end : o.y;   // (no emitting arc leaves frame T)
        auto term = [&](int a, double *x) {
          const int4 R = orec[a];
          double c;
          if (R.y >= 0) {
            if (!gp_emit_cost(Q, score(sc, f, R.y), __int_as_float(R.z), &c)) return false;
            *x = c + nxt[R.x];
          } else {
            if (!gp_eps_cost(Q, __int_as_float(R.z), &c)) return false;
            *x = c + cur[R.x];
          }
          return post_finite(*x);
        };
        cur[s] = post_logsum(o.x, a1, term, f == T && s == fin, 0.0);
        const double al = tabf[s];
        for (int a = o.x; a < a_end; ++a) {
          double g = 0.0;
          if (a < a1) {
            const int4 R = orec[a];
            double c;
            bool ok;
            double bt;
            if (R.y >= 0) { ok = gp_emit_cost(Q, score(sc, f, R.y), __int_as_float(R.z), &c); bt = nxt[R.x]; }
            else { ok = gp_eps_cost(Q, __int_as_float(R.z), &c); bt = cur[R.x]; }
            const double e = ((al + c) + bt) - tot;
            if (ok && post_finite(e)) g = exp(-e);
          }
          if (a >= o.y && f < T) gamf[a] = g;
          if (C.want_occ) occ[a] = f == T ? g : occ[a] + g;
        }
      }
      if (L == 0 && ahead) stash(f - 1);
      __syncthreads();
    }
    if (f < T) {
      double *pf = post + (int64_t)f * NS;
      for (int j = tid; j < NS; j += kGpThreads) {
        double sum = 0.0;
        for (int k = slot_off[j]; k < slot_off[j + 1]; ++k) sum += gamf[slot_arc[k]];
        pf[j] = sum;
      }
    }
  }
  if (tid == 0) {
    int32_t *o = Q.out + (int64_t)blockIdx.x * gpost_out_ints(Q.cap_frames, Q.cap_entries);
    o[0] = 1;
    o[1] = T;
    Q.dout[(int64_t)blockIdx.x * gpost_out_doubles(Q.cap_frames, Q.cap_entries, Q.cap_arcs)] = -tot;
  }
}

}  // namespace

__global__ __launch_bounds__(kGpThreads) void graphpost_kernel(GpostDev Q) {
  __shared__ double s_rows[2 * kGpostLdsStates];
  __shared__ float s_sc[2 * kFalignLdsLabels];
  const GpostChan C = Q.chan[blockIdx.x];
  const int32_t *H = Q.G.hdr + (int64_t)C.graph * kFalignHdr;
  if (H[2] <= kGpostLdsStates) gpost_run<true>(Q, C, H, s_rows, s_sc);
  else gpost_run<false>(Q, C, H, s_rows, s_sc);
}

__global__ __launch_bounds__(kGpThreads) void graphpost_pack_kernel(GpostDev Q) {
  const int tid = threadIdx.x;
  const GpostChan C = Q.chan[blockIdx.x];
  const size_t capf = (size_t)Q.cap_frames, cape = (size_t)Q.cap_entries;
  int32_t *o = Q.out + (int64_t)blockIdx.x * gpost_out_ints(Q.cap_frames, Q.cap_entries);
  int32_t *o_off = o + kGpostHead, *o_nd = o_off + capf + 1, *o_class = o_nd + capf;
  double *d = Q.dout + (int64_t)blockIdx.x * gpost_out_doubles(Q.cap_frames, Q.cap_entries, Q.cap_arcs);
  double *d_mass = d + 1, *d_post = d_mass + capf, *d_occ = d_post + cape;
  if (!o[0]) return;   // not found: every output stays zero
  const int T = C.T, NS = C.n_slots, A = Q.G.hdr[(int64_t)C.graph * kFalignHdr + 3];
  const double *post = Q.post + C.post_off;
  const int32_t *slot_class = Q.cls + C.cls_off;
  int32_t *cnt = Q.cnt + C.cnt_off;
  const bool lists = Q.cap_frames > 0 || Q.cap_entries > 0, rows = lists && T <= Q.cap_frames;
  __shared__ int s_i[kGpThreads];
  for (int f = tid; f < T; f += kGpThreads) {
    const double *pf = post + (int64_t)f * NS;
    int n = 0, nd = 0;
    double mass = 0.0;
    for (int j = 0; j < NS; ++j) {
      const double p = pf[j];
      if (p > 0.0) {
        ++nd;
        mass += p;
        n += p >= Q.min_post;
      }
    }
    cnt[f] = n;
    if (rows) { o_nd[f] = nd; d_mass[f] = mass; }
  }
  __syncthreads();   // cnt[] is summed by other lanes than wrote it
  const int total = pack_frame_off<kGpThreads>(cnt, T, rows, o_off, s_i, tid);
  const bool fits = !lists || (rows && total <= Q.cap_entries);
  if (tid == 0) { o[2] = total; o[3] = !fits; }
  if (C.want_occ && A <= Q.cap_arcs) {
    const double *occ = Q.gam + C.gam_off + 2 * (int64_t)A;
    for (int a = tid; a < A; a += kGpThreads) d_occ[a] = occ[a];
  }
  if (!fits || !lists) return;
  __syncthreads();   // frame_off is read by other lanes than wrote it
  for (int f = tid; f < T; f += kGpThreads) {
    const double *pf = post + (int64_t)f * NS;
    int k = o_off[f];
    for (int j = 0; j < NS; ++j) {
      const double p = pf[j];
      if (p > 0.0 && p >= Q.min_post) { o_class[k] = slot_class[j]; d_post[k] = p; ++k; }
    }
  }
}

__global__ __launch_bounds__(kGpThreads) void graphpost_dense_kernel(GpostDev Q, int max_T) {
  const int e = blockIdx.x / max_T, f = blockIdx.x % max_T, tid = threadIdx.x;
  const GpostChan C = Q.chan[e];
  if (!C.grad || f >= C.T || f >= C.grad_rows || !Q.out[(int64_t)e * gpost_out_ints(Q.cap_frames, Q.cap_entries)]) return;
  float *row = C.grad + (int64_t)f * C.grad_pitch;
  for (int c = tid; c < Q.n_cols; c += kGpThreads) row[c] = 0.0f;
  __syncthreads();   // the zeros stand before a class' store to the same column
  const double *pf = Q.post + C.post_off + (int64_t)f * C.n_slots;
  const int32_t *slot_class = Q.cls + C.cls_off;
  for (int j = tid; j < C.n_slots; j += kGpThreads) {
    const double p = pf[j];
    const int32_t c = slot_class[j];
    if (p > 0.0 && c >= 0 && c < Q.n_cols) row[c] = (float)(Q.grad_scale * p);   // (the host refused a class beyond n_cols)
  }
}

void launch_graph_post(const GpostDev &Q, int cnt, int max_T, bool dense, hipStream_t s) {
  hipLaunchKernelGGL(graphpost_kernel, dim3(cnt), dim3(kGpThreads), 0, s, Q);
  hipLaunchKernelGGL(graphpost_pack_kernel, dim3(cnt), dim3(kGpThreads), 0, s, Q);
  if (dense && max_T > 0) hipLaunchKernelGGL(graphpost_dense_kernel, dim3(cnt * max_T), dim3(kGpThreads), 0, s, Q, max_T);
}

}  // namespace wfst
