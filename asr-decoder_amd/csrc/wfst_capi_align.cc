// wfst_decoder_align_words: the cheapest path of a channel's raw lattice that spells a given word sequence, with its word times and
// scores, for a channel list (live and finalized channels mixed) and several sequences per channel -- one launch per stage
// (lattice_emit_kernel for the live channels, align_index_kernel, align_kernel: wfst_align.hip).  A translation unit of its own -- see
// wfst_capi_align.h.
#include "wfst_capi_align.h"

using namespace wfst;

namespace {
// max_cells = 0: a lattice of 65 536 states (the determinizer's own default bound, wfst_limits.det_raw_states) against 64 words.
// A sequence's table takes 4 bytes per cell and its path scratch 4 bytes per state: 16.25 MiB + 0.25 MiB at this bound.
constexpr int64_t kAlignDefaultCells = 65536ll * 65;
// cells of one round's tables (256 MiB); a channel whose own sequences need more runs in a round of its own
constexpr int64_t kAlignRoundCells = 64ll << 20;

struct AlignQuery : WordQuery {
  size_t np, cap;
  AlignOutputs out;
  AlignQuery(size_t np_, size_t cap_, const AlignOutputs &out_) : np(np_), cap(cap_), out(out_) {
    name = "align"; item = "sequence"; abbr = "seq";
    default_cells = kAlignDefaultCells; round_cells = kAlignRoundCells;
    pair_ints = (size_t)kAlignHead + 2 * cap;
    invariant = "a reached cell without its arrival";
  }
  void clear() override { out.clear(np, cap); }
  int launch(WordRound &R) override {
    const AlignDev A = R.align_dev();
    launch_align_index(*R.V->D, A, R.chan, (int)R.cnt, R.V->stream);
    ALIGN_TRY(hipGetLastError());
    launch_align(*R.V->D, A, R.chan, (int)R.cnt, R.V->stream);
    ALIGN_TRY(hipGetLastError());
    return WFST_OK;
  }
  int unpack(const WordRound &R, size_t j, size_t o, int32_t) override {
    const size_t ns = (size_t)R.n_seqs;
    for (size_t q = 0; q < ns; ++q) {
      const int32_t *r = R.landed + (j * ns + q) * pair_ints;
      if (r[0]) out.take(r, o * ns + q, (size_t)std::max(R.seq_len[o * ns + q], 0), cap);
    }
    return WFST_OK;
  }
};
}  // namespace

int wfst_decoder_align_words(wfst_decoder *d, const int32_t *channels, int32_t n, int32_t use_final_probs, int32_t n_seqs, int32_t cap_words,
                             const int32_t *seq_words, const int32_t *seq_len, int64_t max_cells, int32_t *status, int32_t *found,
                             int32_t *n_arcs, int32_t *begin_frame, int32_t *end_frame, float *tot_score, float *lm_score) {
  // (np, cap are used only behind the driver's checks of n, n_seqs and cap_words)
  AlignQuery q((size_t)n * (size_t)n_seqs, (size_t)cap_words, AlignOutputs{found, n_arcs, begin_frame, end_frame, tot_score, lm_score});
  return word_query_run(q, d, channels, n, use_final_probs, n_seqs, cap_words, seq_words, seq_len, max_cells, status);
}
