// wfst_decoder_word_confidence: the posteriors of a channel's raw lattice (forward-backward in the log semiring, float64) and, for
// every word of a sequence wfst_decoder_align_words places in time, the posterior mass of the arcs that say the word at about that
// time -- for a channel list (live and finalized channels mixed) and several sequences per channel, one launch per stage
// (lattice_emit_kernel for the live channels, align_index_kernel, align_kernel, posterior_kernel, confidence_kernel:
// wfst_align.hip, wfst_posterior.hip).  A translation unit of its own -- see wfst_capi_posterior.h.
#include "wfst_capi_posterior.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "wfst_capi_words.h"   // capi_fail, capi_fail_ctl

using namespace wfst;

#define P_TRY(expr)                                                                                   \
  do {                                                                                                \
    hipError_t e_ = (expr);                                                                           \
    if (e_ != hipSuccess) return capi_fail(WFST_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

namespace {
template <class B>
hipError_t grow(B &buf, size_t need) { return buf.n >= need ? hipSuccess : buf.alloc(need); }
template <class T>
void zero(T *p, size_t n) { if (p) std::fill(p, p + n, (T)0); }
}  // namespace

int wfst_decoder_word_confidence(wfst_decoder *d, const int32_t *channels, int32_t n, int32_t use_final_probs, double graph_scale,
                                 double acoustic_scale, int32_t n_seqs, int32_t cap_words, const int32_t *seq_words, const int32_t *seq_len,
                                 int64_t max_cells, int32_t *status, double *log_z, int32_t *found, int32_t *n_arcs, int32_t *begin_frame,
                                 int32_t *end_frame, double *word_post, double *path_logpost, float *tot_score, float *lm_score) {
  if (!d || !channels) return capi_fail(WFST_E_ARG, "NULL decoder / channel list");
  if (!std::isfinite(graph_scale) || !std::isfinite(acoustic_scale) || graph_scale < 0.0 || acoustic_scale < 0.0)
    return capi_fail(WFST_E_ARG, "graph_scale / acoustic_scale must be finite and >= 0");
  if (n_seqs < 1 || n_seqs > 64) return capi_fail(WFST_E_ARG, "1 <= n_seqs <= 64 sequences per channel");
  if (cap_words <= 0) return capi_fail(WFST_E_ARG, "cap_words <= 0");
  if (!seq_words || !seq_len) return capi_fail(WFST_E_ARG, "NULL sequences");
  if (max_cells < 0) return capi_fail(WFST_E_ARG, "max_cells < 0");
  AlignView V;
  int rc = align_begin(d, channels, n, &V);
  if (rc != WFST_OK) return rc;
  const size_t ns = (size_t)n_seqs, cap = (size_t)cap_words, np = (size_t)n * ns;
  for (size_t p = 0; p < np; ++p) {
    if (seq_len[p] > cap_words) return capi_fail(WFST_E_ARG, "a seq_len above cap_words");
    for (int k = 0; k < seq_len[p]; ++k)
      if (seq_words[p * cap + (size_t)k] <= 0) return capi_fail(WFST_E_ARG, "a word id <= 0 inside a sequence");
  }
  if (status) std::fill(status, status + n, (int32_t)WFST_OK);
  zero(log_z, (size_t)n); zero(found, np); zero(n_arcs, np); zero(begin_frame, np * cap); zero(end_frame, np * cap);
  zero(word_post, np * cap); zero(path_logpost, np); zero(tot_score, np); zero(lm_score, np);
  // the channels with a lattice to look at (a finalized channel without final-probs has none: GetRawLattice, base-inl.h:879-884),
  // by their position in the caller's list
  std::vector<int32_t> pos, list;
  for (int i = 0; i < n; ++i)
    if (align_channel_state(d, channels[i]) == 1 || use_final_probs) { pos.push_back(i); list.push_back(channels[i]); }
  if (pos.empty()) return WFST_OK;
  std::vector<int32_t> sizes;
  rc = align_emit(d, list, use_final_probs, &sizes);
  if (rc != WFST_OK) return rc;
  hipStream_t st = V.stream;
  AlignState &S = *V.as;
  const int64_t limit = max_cells > 0 ? max_cells : kPosteriorDefaultCells;
  // per listed channel: its own failure (reported in status[], the call goes on) or the cells its sequences' tables take
  std::vector<int64_t> need(pos.size(), 0);
  std::vector<char> run(pos.size(), 0);
  for (size_t i = 0; i < pos.size(); ++i) {
    const int32_t *z = &sizes[4 * i];
    const size_t o = (size_t)pos[i];
    if (z[3]) {   // a device error of THIS channel's utterance
      const int code = capi_fail_ctl(list[i], z[3]);
      if (status) status[o] = code;
      continue;
    }
    bool over = false;
    for (size_t q = 0; q < ns; ++q) {
      const int32_t len = seq_len[o * ns + q];
      if (len < 0) continue;
      const int64_t cells = (int64_t)std::max(z[0], 0) * (len + 1);
      if (cells > limit) over = true;
      need[i] += cells;
    }
    if (over) {
      const int code = capi_fail(WFST_E_CAPACITY, "channel " + std::to_string(list[i]) + ": word confidence: a table of " + std::to_string(z[0]) +
                                                      " lattice states x (words + 1) is beyond max_cells (" + std::to_string(limit) + ")");
      if (status) status[o] = code;
      continue;
    }
    run[i] = 1;
  }
  const size_t per = (size_t)kAlignHead + 2 * cap, dper = 1 + cap;
  for (size_t first = 0; first < pos.size();) {
    // a round: the next channels whose tables fit the round's budget together (at least one)
    std::vector<size_t> rnd;
    int64_t cells = 0;
    size_t next = first;
    for (; next < pos.size(); ++next) {
      if (!run[next]) continue;
      if (!rnd.empty() && cells + need[next] > kPosteriorRoundCells) break;
      rnd.push_back(next);
      cells += need[next];
    }
    first = next;
    if (rnd.empty()) break;
    const size_t cnt = rnd.size(), pairs = cnt * ns;
    AlignDev A = {};
    A.ns_cap = 1; A.na_cap = 1; A.fr_cap = 2;
    for (size_t i : rnd) {
      A.ns_cap = std::max(A.ns_cap, sizes[4 * i]);
      A.na_cap = std::max(A.na_cap, sizes[4 * i + 1]);
      A.fr_cap = std::max(A.fr_cap, sizes[4 * i + 2] + 2);
    }
    A.idx_ints = align_idx_ints(A.ns_cap, A.na_cap, A.fr_cap);
    A.n_seqs = n_seqs;
    A.cap_words = cap_words;
    A.sil_bits = V.sil_bits;
    A.n_tid = V.sil_ntid;
    const size_t nsc = (size_t)A.ns_cap, nac = (size_t)A.na_cap;
    // staged inputs: the pairs' table offsets (64-bit, first: aligned), the round's channels, the lengths, the words;
    // packed results: align_kernel's, then posterior_kernel's error word per channel
    const size_t in_ints = 2 * pairs + cnt + pairs + pairs * cap, out_ints = pairs * per + cnt;
    // the posterior workspace: alpha, beta [cnt][ns_cap], gamma [cnt][na_cap], then what comes back: log_z [cnt], the pairs' results;
    // sarc [cnt][na_cap], then done and soff [cnt][ns_cap] as int2 halves
    const size_t res_at = cnt * (2 * nsc + nac), res_n = cnt + pairs * dper, post_n = res_at + res_n;
    const size_t pidx_n = cnt * nac + cnt * nsc;
    const size_t idx_need = (size_t)A.idx_ints * cnt, path_need = pairs * nsc, cell_need = (size_t)std::max<int64_t>(cells, 1);
    if (S.idx.n < idx_need || S.path.n < path_need || S.in.n < in_ints || S.out.n < out_ints || S.cells.n < cell_need || S.post.n < post_n ||
        S.post_idx.n < pidx_n) {
      P_TRY(hipStreamSynchronize(st));
      if (grow(S.idx, idx_need) != hipSuccess || grow(S.path, path_need) != hipSuccess || grow(S.in, in_ints) != hipSuccess ||
          grow(S.out, out_ints) != hipSuccess || grow(S.cells, cell_need) != hipSuccess || grow(S.post, post_n) != hipSuccess ||
          grow(S.post_idx, pidx_n) != hipSuccess) {
        (void)hipGetLastError();
        return capi_fail(WFST_E_CAPACITY, "word confidence: no device memory for the workspace of " + std::to_string(cnt) + " lattice(s), " +
                                              std::to_string(n_seqs) + " sequences each (" + std::to_string(cells) + " cells, " +
                                              std::to_string(cnt * post_slot_bytes(A.ns_cap, A.na_cap)) +
                                              " bytes of posteriors): lower max_cells or ask for fewer channels at a time");
      }
    }
    P_TRY(S.pin.reserve(std::max(in_ints, out_ints)));
    P_TRY(S.post_pin.reserve(res_n));
    int64_t *h_off = reinterpret_cast<int64_t *>(S.pin.p);
    int32_t *h_chan = S.pin.p + 2 * pairs, *h_len = h_chan + cnt, *h_words = h_len + pairs;
    int64_t at = 0;
    for (size_t j = 0; j < cnt; ++j) {
      const size_t i = rnd[j], o = (size_t)pos[i];
      h_chan[j] = list[i];
      memcpy(h_len + j * ns, seq_len + o * ns, ns * 4);
      memcpy(h_words + j * ns * cap, seq_words + o * ns * cap, ns * cap * 4);
      for (size_t q = 0; q < ns; ++q) {
        const int32_t len = seq_len[o * ns + q];
        h_off[j * ns + q] = len < 0 ? -1 : at;
        if (len >= 0) at += (int64_t)std::max(sizes[4 * i], 0) * (len + 1);
      }
    }
    P_TRY(hipMemcpyAsync(S.in.p, S.pin.p, in_ints * 4, hipMemcpyHostToDevice, st));
    A.idx = S.idx.p;
    A.cell_off = reinterpret_cast<const int64_t *>(S.in.p);
    const int32_t *dev_chan = S.in.p + 2 * pairs;
    A.seq_len = dev_chan + cnt;
    A.seq_words = A.seq_len + pairs;
    A.cells = S.cells.p;
    A.path = S.path.p;
    A.out = S.out.p;
    PostDev P = {};
    P.alpha = S.post.p;
    P.beta = P.alpha + cnt * nsc;
    P.gamma = P.beta + cnt * nsc;
    P.log_z = S.post.p + res_at;
    P.out = P.log_z + cnt;
    P.sarc = S.post_idx.p;
    P.done = reinterpret_cast<int32_t *>(S.post_idx.p + cnt * nac);
    P.soff = P.done + cnt * nsc;
    P.chan_err = S.out.p + pairs * per;
    P.graph_scale = graph_scale;
    P.acoustic_scale = acoustic_scale;
    launch_align_index(*V.D, A, dev_chan, (int)cnt, st);
    P_TRY(hipGetLastError());
    launch_align(*V.D, A, dev_chan, (int)cnt, st);
    P_TRY(hipGetLastError());
    launch_posterior(*V.D, A, P, dev_chan, (int)cnt, st);
    P_TRY(hipGetLastError());
    launch_confidence(A, P, (int)cnt, st);
    P_TRY(hipGetLastError());
    // (the staged inputs share the landing place of the results: in stream order the upload has read it before the kernels run)
    P_TRY(hipMemcpyAsync(S.pin.p, S.out.p, out_ints * 4, hipMemcpyDeviceToHost, st));
    P_TRY(hipMemcpyAsync(S.post_pin.p, P.log_z, res_n * 8, hipMemcpyDeviceToHost, st));
    P_TRY(hipStreamSynchronize(st));
    for (size_t j = 0; j < cnt; ++j) {
      const size_t i = rnd[j], o = (size_t)pos[i];
      int code = WFST_OK;
      if (S.pin.p[pairs * per + j] == kAlnCycle)
        code = capi_fail(WFST_E_DEVICE, "channel " + std::to_string(list[i]) + ": word confidence: the lattice has an epsilon cycle");
      for (size_t q = 0; q < ns && code == WFST_OK; ++q) {
        const int32_t e = S.pin.p[(j * ns + q) * per + 4];
        if (e == kAlnCycle) code = capi_fail(WFST_E_DEVICE, "channel " + std::to_string(list[i]) + ": word confidence: the lattice has an epsilon cycle");
        else if (e == kAlnTooLarge) code = capi_fail(WFST_E_CAPACITY, "channel " + std::to_string(list[i]) + ": word confidence: the lattice outgrew the round's index");
        else if (e) code = capi_fail(WFST_E_DEVICE, "channel " + std::to_string(list[i]) + ": word confidence: internal invariant violated on the device (a reached cell without its arrival)");
      }
      if (status) status[o] = code;
      if (code != WFST_OK) continue;
      if (log_z) log_z[o] = S.post_pin.p[j];
      for (size_t q = 0; q < ns; ++q) {
        const int32_t *r = S.pin.p + (j * ns + q) * per;
        if (!r[0]) continue;
        const double *x = S.post_pin.p + cnt + (j * ns + q) * dper;
        const size_t p = o * ns + q;
        const size_t len = (size_t)std::max(seq_len[p], 0);
        if (found) found[p] = 1;
        if (n_arcs) n_arcs[p] = r[1];
        if (tot_score) memcpy(&tot_score[p], &r[2], 4);
        if (lm_score) memcpy(&lm_score[p], &r[3], 4);
        if (begin_frame) memcpy(begin_frame + p * cap, r + kAlignHead, len * 4);
        if (end_frame) memcpy(end_frame + p * cap, r + kAlignHead + cap, len * 4);
        if (path_logpost) path_logpost[p] = x[0];
        if (word_post) memcpy(word_post + p * cap, x + 1, len * 8);
      }
    }
  }
  return WFST_OK;
}
