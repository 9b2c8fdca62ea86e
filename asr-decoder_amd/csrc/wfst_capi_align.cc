// wfst_decoder_align_words: the cheapest path of a channel's raw lattice that spells a given word sequence, with its word times and
// scores, for a channel list (live and finalized channels mixed) and several sequences per channel -- one launch per stage
// (lattice_emit_kernel for the live channels, align_index_kernel, align_kernel: wfst_align.hip).  A translation unit of its own -- see
// wfst_capi_align.h.
#include "wfst_capi_align.h"

#include <algorithm>
#include <cstring>
#include <string>

#include "wfst_capi_words.h"   // capi_fail, capi_fail_ctl

using namespace wfst;

#define A_TRY(expr)                                                                                   \
  do {                                                                                                \
    hipError_t e_ = (expr);                                                                           \
    if (e_ != hipSuccess) return capi_fail(WFST_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

namespace {
// max_cells = 0: a lattice of 65 536 states (the determinizer's own default bound, wfst_limits.det_raw_states) against 64 words.
// A sequence's table takes 4 bytes per cell and its path scratch 4 bytes per state: 16.25 MiB + 0.25 MiB at this bound.
constexpr int64_t kAlignDefaultCells = 65536ll * 65;
// cells of one round's tables (256 MiB); a channel whose own sequences need more runs in a round of its own
constexpr int64_t kAlignRoundCells = 64ll << 20;

template <class B>
hipError_t grow(B &buf, size_t need) { return buf.n >= need ? hipSuccess : buf.alloc(need); }
}  // namespace

int wfst_decoder_align_words(wfst_decoder *d, const int32_t *channels, int32_t n, int32_t use_final_probs, int32_t n_seqs, int32_t cap_words,
                             const int32_t *seq_words, const int32_t *seq_len, int64_t max_cells, int32_t *status, int32_t *found,
                             int32_t *n_arcs, int32_t *begin_frame, int32_t *end_frame, float *tot_score, float *lm_score) {
  if (!d || !channels) return capi_fail(WFST_E_ARG, "NULL decoder / channel list");
  if (n_seqs < 1 || n_seqs > 64) return capi_fail(WFST_E_ARG, "1 <= n_seqs <= 64 sequences per channel");
  if (cap_words <= 0) return capi_fail(WFST_E_ARG, "cap_words <= 0");
  if (!seq_words || !seq_len) return capi_fail(WFST_E_ARG, "NULL sequences");
  if (max_cells < 0) return capi_fail(WFST_E_ARG, "max_cells < 0");
  AlignView V;
  int rc = align_begin(d, channels, n, &V);
  if (rc != WFST_OK) return rc;
  const size_t ns = (size_t)n_seqs, cap = (size_t)cap_words;
  for (size_t p = 0; p < (size_t)n * ns; ++p) {
    if (seq_len[p] > cap_words) return capi_fail(WFST_E_ARG, "a seq_len above cap_words");
    for (int k = 0; k < seq_len[p]; ++k)
      if (seq_words[p * cap + (size_t)k] <= 0) return capi_fail(WFST_E_ARG, "a word id <= 0 inside a sequence");
  }
  if (status) std::fill(status, status + n, (int32_t)WFST_OK);
  if (found) std::fill(found, found + (size_t)n * ns, 0);
  if (n_arcs) std::fill(n_arcs, n_arcs + (size_t)n * ns, 0);
  if (begin_frame) std::fill(begin_frame, begin_frame + (size_t)n * ns * cap, 0);
  if (end_frame) std::fill(end_frame, end_frame + (size_t)n * ns * cap, 0);
  if (tot_score) std::fill(tot_score, tot_score + (size_t)n * ns, 0.0f);
  if (lm_score) std::fill(lm_score, lm_score + (size_t)n * ns, 0.0f);
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
  const int64_t limit = max_cells > 0 ? max_cells : kAlignDefaultCells;
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
      const int code = capi_fail(WFST_E_CAPACITY, "channel " + std::to_string(list[i]) + ": align: a table of " + std::to_string(z[0]) +
                                                      " lattice states x (words + 1) is beyond max_cells (" + std::to_string(limit) + ")");
      if (status) status[o] = code;
      continue;
    }
    run[i] = 1;
  }
  const size_t per = (size_t)kAlignHead + 2 * cap;
  for (size_t first = 0; first < pos.size();) {
    // a round: the next channels whose tables fit the round's budget together (at least one)
    std::vector<size_t> rnd;
    int64_t cells = 0;
    size_t next = first;
    for (; next < pos.size(); ++next) {
      if (!run[next]) continue;
      if (!rnd.empty() && cells + need[next] > kAlignRoundCells) break;
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
    // staged inputs: the pairs' table offsets (64-bit, first: aligned), the round's channels, the lengths, the words
    const size_t in_ints = 2 * pairs + cnt + pairs + pairs * cap, out_ints = pairs * per;
    if (S.idx.n < (size_t)A.idx_ints * cnt || S.path.n < pairs * (size_t)A.ns_cap || S.in.n < in_ints || S.out.n < out_ints ||
        S.cells.n < (size_t)std::max<int64_t>(cells, 1)) {
      A_TRY(hipStreamSynchronize(st));
      if (grow(S.idx, (size_t)A.idx_ints * cnt) != hipSuccess || grow(S.path, pairs * (size_t)A.ns_cap) != hipSuccess ||
          grow(S.in, in_ints) != hipSuccess || grow(S.out, out_ints) != hipSuccess ||
          grow(S.cells, (size_t)std::max<int64_t>(cells, 1)) != hipSuccess) {
        (void)hipGetLastError();
        return capi_fail(WFST_E_CAPACITY, "align: no device memory for the workspace of " + std::to_string(cnt) + " lattice(s), " +
                                              std::to_string(n_seqs) + " sequences each (" + std::to_string(cells) + " cells): lower max_cells or ask for fewer channels at a time");
      }
    }
    A_TRY(S.pin.reserve(std::max(in_ints, out_ints)));
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
    A_TRY(hipMemcpyAsync(S.in.p, S.pin.p, in_ints * 4, hipMemcpyHostToDevice, st));
    A.idx = S.idx.p;
    A.cell_off = reinterpret_cast<const int64_t *>(S.in.p);
    const int32_t *dev_chan = S.in.p + 2 * pairs;
    A.seq_len = dev_chan + cnt;
    A.seq_words = A.seq_len + pairs;
    A.cells = S.cells.p;
    A.path = S.path.p;
    A.out = S.out.p;
    launch_align_index(*V.D, A, dev_chan, (int)cnt, st);
    A_TRY(hipGetLastError());
    launch_align(*V.D, A, dev_chan, (int)cnt, st);
    A_TRY(hipGetLastError());
    // (the staged inputs share the landing place of the results: in stream order the upload has read it before the kernels run)
    A_TRY(hipMemcpyAsync(S.pin.p, S.out.p, out_ints * 4, hipMemcpyDeviceToHost, st));
    A_TRY(hipStreamSynchronize(st));
    for (size_t j = 0; j < cnt; ++j) {
      const size_t i = rnd[j], o = (size_t)pos[i];
      int code = WFST_OK;
      for (size_t q = 0; q < ns && code == WFST_OK; ++q) {
        const int32_t e = S.pin.p[(j * ns + q) * per + 4];
        if (e == kAlnCycle) code = capi_fail(WFST_E_DEVICE, "channel " + std::to_string(list[i]) + ": align: the lattice has an epsilon cycle");
        else if (e == kAlnTooLarge) code = capi_fail(WFST_E_CAPACITY, "channel " + std::to_string(list[i]) + ": align: the lattice outgrew the round's index");
        else if (e) code = capi_fail(WFST_E_DEVICE, "channel " + std::to_string(list[i]) + ": align: internal invariant violated on the device (a reached cell without its arrival)");
      }
      if (status) status[o] = code;
      if (code != WFST_OK) continue;
      for (size_t q = 0; q < ns; ++q) {
        const int32_t *r = S.pin.p + (j * ns + q) * per;
        if (!r[0]) continue;
        const size_t p = o * ns + q;
        const size_t len = (size_t)std::max(seq_len[p], 0);
        if (found) found[p] = 1;
        if (n_arcs) n_arcs[p] = r[1];
        if (tot_score) memcpy(&tot_score[p], &r[2], 4);
        if (lm_score) memcpy(&lm_score[p], &r[3], 4);
        if (begin_frame) memcpy(begin_frame + p * cap, r + kAlignHead, len * 4);
        if (end_frame) memcpy(end_frame + p * cap, r + kAlignHead + cap, len * 4);
      }
    }
  }
  return WFST_OK;
}
