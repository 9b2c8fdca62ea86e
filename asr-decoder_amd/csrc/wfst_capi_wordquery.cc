// word_query_run: what wfst_decoder_align_words, wfst_decoder_nearest_words, wfst_decoder_word_confidence,
// wfst_decoder_sequence_posterior, wfst_decoder_word_alternatives, wfst_decoder_frame_posteriors, wfst_decoder_rescaled_words,
// wfst_decoder_sequence_stats and wfst_decoder_biased_words do
// alike -- see
// wfst_capi_align.h.  It launches nothing: the entry points' own units do, in their launch() hooks.
#include "wfst_capi_align.h"

namespace wfst {

int word_query_no_memory(const WordQuery &q, const WordRound &R) {
  return capi_fail(WFST_E_CAPACITY, std::string(q.name) + ": no device memory for the workspace of " + std::to_string(R.cnt) + " lattice(s), " +
                                        std::to_string(R.n_seqs) + " " + q.item + "s each (" + std::to_string(R.cells) + " cells" +
                                        q.workspace_note(R) + "): lower max_cells or ask for fewer channels at a time");
}

int word_query_run(WordQuery &q, wfst_decoder *d, const int32_t *channels, int32_t n, int32_t use_final_probs, int32_t n_seqs,
                   int32_t cap_words, const int32_t *seq_words, const int32_t *seq_len, int64_t max_cells, int32_t *status) {
  const std::string item = q.item, abbr = q.abbr;
  if (!d || !channels) return capi_fail(WFST_E_ARG, "NULL decoder / channel list");
  if (q.arg_error) return capi_fail(WFST_E_ARG, q.arg_error);
  if (n_seqs < 1 || n_seqs > 64) return capi_fail(WFST_E_ARG, "1 <= n_" + abbr + "s <= 64 " + item + "s per channel");
  if (cap_words <= 0 || q.cap_extra <= 0) return capi_fail(WFST_E_ARG, std::string(q.caps) + " <= 0");
  if (!seq_words || !seq_len) return capi_fail(WFST_E_ARG, "NULL " + item + "s");
  if (max_cells < 0) return capi_fail(WFST_E_ARG, "max_cells < 0");
  AlignView V;
  int rc = align_begin(d, channels, n, &V);
  if (rc != WFST_OK) return rc;
  const size_t ns = (size_t)n_seqs, cap = (size_t)cap_words;
  for (size_t p = 0; p < (size_t)n * ns; ++p) {
    if (seq_len[p] > cap_words) return capi_fail(WFST_E_ARG, "a " + abbr + "_len above cap_words");
    if (seq_len[p] >= 0 && seq_len[p] < q.min_len) return capi_fail(WFST_E_ARG, "a " + abbr + "_len below " + std::to_string(q.min_len));
    for (int k = 0; k < seq_len[p]; ++k)
      if (seq_words[p * cap + (size_t)k] <= 0) return capi_fail(WFST_E_ARG, "a word id <= 0 inside a " + item);
  }
  if (status) std::fill(status, status + n, (int32_t)WFST_OK);
  q.clear();
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
  const int64_t limit = max_cells > 0 ? max_cells : q.default_cells;
  // a pair's table: states x (words + 1) cells
  auto table = [&](size_t i, int32_t len) { return (int64_t)std::max(sizes[4 * i], 0) * (len + 1); };
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
    bool over = q.arc_limit > 0 && z[1] >= q.arc_limit;
    for (size_t s = 0; s < ns; ++s) {
      const int32_t len = seq_len[o * ns + s];
      if (len < 0) continue;
      if (table(i, len) > limit) over = true;
      need[i] += table(i, len);
    }
    if (over) {
      const int code = capi_fail(WFST_E_CAPACITY, "channel " + std::to_string(list[i]) + ": " + q.name + ": a table of " + std::to_string(z[0]) +
                                                      " lattice states x " + q.table_cols + " is beyond max_cells (" + std::to_string(limit) + ")");
      if (status) status[o] = code;
      continue;
    }
    run[i] = 1;
  }
  for (size_t first = 0; first < pos.size();) {
    // a round: the next channels whose tables fit the round's budget together (at least one)
    const RoundCut cut = cut_round(need, run, first, q.round_cells);
    first = cut.next;
    if (cut.members.empty()) break;
    const std::vector<size_t> &rnd = cut.members;
    const size_t cnt = rnd.size(), pairs = cnt * ns;
    WordRound R = {};
    R.V = &V; R.cnt = cnt; R.pairs = pairs; R.cells = cut.cells;
    R.n_seqs = n_seqs; R.cap_words = cap_words; R.seq_len = seq_len;
    for (size_t i : rnd) R.caller_pos.push_back(pos[i]);
    AlignDev &A = R.A;
    A.ns_cap = 1; A.na_cap = 1; A.fr_cap = 2;
    for (size_t i : rnd) {
      A.ns_cap = std::max(A.ns_cap, sizes[4 * i]);
      A.na_cap = std::max(A.na_cap, sizes[4 * i + 1]);
      A.fr_cap = std::max(A.fr_cap, sizes[4 * i + 2] + 2);
    }
    A.idx_ints = align_idx_ints(A.ns_cap, A.na_cap, A.fr_cap);
    // staged inputs: the pairs' table offsets (64-bit, first: aligned), the round's channels, the lengths, the words
    const size_t in_ints = 2 * pairs + cnt + pairs + pairs * cap, out_ints = pairs * q.pair_ints + cnt * q.chan_ints;
    const size_t idx_need = (size_t)A.idx_ints * cnt, path_need = pairs * ((size_t)A.ns_cap + (size_t)q.path_extra);
    const size_t cell_words = (size_t)q.cell_words * (size_t)std::max<int64_t>(cut.cells, 1);   // (AlignState::cells counts 32-bit words)
    if (S.idx.n < idx_need || S.path.n < path_need || S.in.n < in_ints || S.out.n < out_ints || S.cells.n < cell_words) {
      ALIGN_TRY(hipStreamSynchronize(st));
      if (align_grow(S.idx, idx_need) != hipSuccess || align_grow(S.path, path_need) != hipSuccess || align_grow(S.in, in_ints) != hipSuccess ||
          align_grow(S.out, out_ints) != hipSuccess || align_grow(S.cells, cell_words) != hipSuccess) {
        (void)hipGetLastError();
        return word_query_no_memory(q, R);
      }
    }
    ALIGN_TRY(S.pin.reserve(std::max(in_ints, out_ints)));
    int64_t *h_off = reinterpret_cast<int64_t *>(S.pin.p);
    int32_t *h_chan = S.pin.p + 2 * pairs, *h_len = h_chan + cnt, *h_words = h_len + pairs;
    int64_t at = 0;
    for (size_t j = 0; j < cnt; ++j) {
      const size_t i = rnd[j], o = (size_t)pos[i];
      h_chan[j] = list[i];
      memcpy(h_len + j * ns, seq_len + o * ns, ns * 4);
      memcpy(h_words + j * ns * cap, seq_words + o * ns * cap, ns * cap * 4);
      for (size_t s = 0; s < ns; ++s) {
        const int32_t len = seq_len[o * ns + s];
        h_off[j * ns + s] = len < 0 ? -1 : at;
        if (len >= 0) at += table(i, len);
      }
    }
    ALIGN_TRY(hipMemcpyAsync(S.in.p, S.pin.p, in_ints * 4, hipMemcpyHostToDevice, st));
    A.idx = S.idx.p;
    R.cell_off = reinterpret_cast<const int64_t *>(S.in.p);
    R.chan = S.in.p + 2 * pairs;
    R.len = R.chan + cnt;
    R.words = R.len + pairs;
    rc = q.launch(R);
    if (rc != WFST_OK) return rc;
    // (the staged inputs share the landing place of the results: in stream order the upload has read it before the kernels run)
    ALIGN_TRY(hipMemcpyAsync(S.pin.p, S.out.p, out_ints * 4, hipMemcpyDeviceToHost, st));
    if (R.more_bytes) ALIGN_TRY(hipMemcpyAsync(R.more_dst, R.more_src, R.more_bytes, hipMemcpyDeviceToHost, st));
    ALIGN_TRY(hipStreamSynchronize(st));
    R.landed = S.pin.p;
    for (size_t j = 0; j < cnt; ++j) {
      const size_t i = rnd[j], o = (size_t)pos[i];
      const std::string who = "channel " + std::to_string(list[i]) + ": " + q.name;
      int code = WFST_OK;
      if (q.chan_ints && R.landed[pairs * q.pair_ints + j * q.chan_ints] == kAlnCycle)
        code = capi_fail(WFST_E_DEVICE, who + ": the lattice has an epsilon cycle");
      for (size_t s = 0; s < ns && code == WFST_OK; ++s) {
        const int32_t e = R.landed[(j * ns + s) * q.pair_ints + 4];
        if (e == kAlnCycle) code = capi_fail(WFST_E_DEVICE, who + ": the lattice has an epsilon cycle");
        else if (e == kAlnTooLarge) code = capi_fail(WFST_E_CAPACITY, who + ": the lattice outgrew the round's index");
        else if (e) code = capi_fail(WFST_E_DEVICE, who + ": internal invariant violated on the device (" + q.invariant + ")");
      }
      if (code == WFST_OK) code = q.unpack(R, j, o, list[i]);
      if (status) status[o] = code;
    }
  }
  return WFST_OK;
}

}  // namespace wfst
