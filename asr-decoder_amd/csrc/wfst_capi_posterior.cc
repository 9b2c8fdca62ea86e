// wfst_decoder_word_confidence: the posteriors of a channel's raw lattice (forward-backward in the log semiring, float64) and, for
// every word of a sequence wfst_decoder_align_words places in time, the posterior mass of the arcs that say the word at about that
// time -- for a channel list (live and finalized channels mixed) and several sequences per channel, one launch per stage
// (lattice_emit_kernel for the live channels, align_index_kernel, align_kernel, posterior_kernel, confidence_kernel:
// wfst_align.hip, wfst_posterior.hip).  A translation unit of its own -- see wfst_capi_posterior.h.
#include "wfst_capi_posterior.h"

#include <cmath>

using namespace wfst;

namespace {
struct ConfidenceQuery : WordQuery {
  size_t n, np, cap, dper;
  double graph_scale, acoustic_scale;
  AlignOutputs out;
  double *log_z, *word_post, *path_logpost;
  ConfidenceQuery(size_t n_, size_t np_, size_t cap_, const AlignOutputs &out_) : n(n_), np(np_), cap(cap_), dper(1 + cap_), out(out_) {
    name = "word confidence"; item = "sequence"; abbr = "seq";
    default_cells = kPosteriorDefaultCells; round_cells = kPosteriorRoundCells;
    pair_ints = (size_t)kAlignHead + 2 * cap;
    chan_ints = 1;   // posterior_kernel's error word
    invariant = "a reached cell without its arrival";
  }
  std::string workspace_note(const WordRound &R) const override {
    return ", " + std::to_string(R.cnt * post_slot_bytes(R.A.ns_cap, R.A.na_cap)) + " bytes of posteriors";
  }
  void clear() override {
    align_zero(log_z, n); out.clear(np, cap); align_zero(word_post, np * cap); align_zero(path_logpost, np);
  }
  int launch(WordRound &R) override {
    const AlignView &V = *R.V;
    const AlignDev A = R.align_dev();
    const size_t cnt = R.cnt, res_n = cnt + R.pairs * dper;
    // what comes back: log_z [cnt], the pairs' results
    PostDev P;
    const int rc = post_workspace(*this, R, R.pairs * dper, graph_scale, acoustic_scale, &P);
    if (rc != WFST_OK) return rc;
    launch_align_index(*V.D, A, R.chan, (int)cnt, V.stream);
    ALIGN_TRY(hipGetLastError());
    launch_align(*V.D, A, R.chan, (int)cnt, V.stream);
    ALIGN_TRY(hipGetLastError());
    launch_posterior(*V.D, A, P, R.chan, (int)cnt, V.stream);
    ALIGN_TRY(hipGetLastError());
    launch_confidence(A, P, (int)cnt, V.stream);
    ALIGN_TRY(hipGetLastError());
    // log_z and the pairs' doubles land behind the packed results
    R.more_dst = V.as->post_pin.p; R.more_src = P.log_z; R.more_bytes = res_n * 8;
    return WFST_OK;
  }
  int unpack(const WordRound &R, size_t j, size_t o, int32_t) override {
    const size_t ns = (size_t)R.n_seqs;
    const double *landed = R.V->as->post_pin.p;
    if (log_z) log_z[o] = landed[j];
    for (size_t q = 0; q < ns; ++q) {
      const int32_t *r = R.landed + (j * ns + q) * pair_ints;
      if (!r[0]) continue;
      const double *x = landed + R.cnt + (j * ns + q) * dper;
      const size_t p = o * ns + q;
      const size_t len = (size_t)std::max(R.seq_len[p], 0);
      out.take(r, p, len, cap);
      if (path_logpost) path_logpost[p] = x[0];
      if (word_post) memcpy(word_post + p * cap, x + 1, len * 8);
    }
    return WFST_OK;
  }
};
}  // namespace

int wfst_decoder_word_confidence(wfst_decoder *d, const int32_t *channels, int32_t n, int32_t use_final_probs, double graph_scale,
                                 double acoustic_scale, int32_t n_seqs, int32_t cap_words, const int32_t *seq_words, const int32_t *seq_len,
                                 int64_t max_cells, int32_t *status, double *log_z, int32_t *found, int32_t *n_arcs, int32_t *begin_frame,
                                 int32_t *end_frame, double *word_post, double *path_logpost, float *tot_score, float *lm_score) {
  // (n, np, cap are used only behind the driver's checks of n, n_seqs and cap_words)
  ConfidenceQuery q((size_t)n, (size_t)n * (size_t)n_seqs, (size_t)cap_words, AlignOutputs{found, n_arcs, begin_frame, end_frame, tot_score, lm_score});
  if (!std::isfinite(graph_scale) || !std::isfinite(acoustic_scale) || graph_scale < 0.0 || acoustic_scale < 0.0)
    q.arg_error = "graph_scale / acoustic_scale must be finite and >= 0";
  q.graph_scale = graph_scale; q.acoustic_scale = acoustic_scale;
  q.log_z = log_z; q.word_post = word_post; q.path_logpost = path_logpost;
  return word_query_run(q, d, channels, n, use_final_probs, n_seqs, cap_words, seq_words, seq_len, max_cells, status);
}
