// wfst_decoder_word_alternatives: a confusion network pinned to a hypothesis.  For every word of a sequence
// wfst_decoder_align_words places in time, the words the lattice says in that word's cell of the time axis with their posterior mass,
// the first n_alts of them, and the mass of the paths that say nothing there -- for a channel list (live and finalized channels mixed)
// and several sequences per channel, one launch per stage (lattice_emit_kernel for the live channels, align_index_kernel,
// align_kernel, posterior_kernel, confidence_kernel: wfst_align.hip, wfst_posterior.hip; slot_mass_kernel, slot_none_kernel:
// wfst_altern.hip).  A translation unit of its own -- see wfst_capi_altern.h.
#include "wfst_capi_altern.h"

#include <cmath>

using namespace wfst;

namespace {
struct AlternQuery : WordQuery {
  size_t n, np, cap, K, dper;
  double graph_scale, acoustic_scale;
  AlignOutputs out;
  double *log_z, *word_post, *none_post, *alt_post, *path_logpost;
  int32_t *n_distinct, *alt_word;
  // where a round's results land, in doubles from the landing place's start (set by launch())
  size_t at_conf, at_none, at_post, at_ints;
  AlternQuery(size_t n_, size_t np_, size_t cap_, size_t n_alts_, const AlignOutputs &out_)
      : n(n_), np(np_), cap(cap_), K(n_alts_), dper(1 + cap_), out(out_) {
    name = "word alternatives"; item = "sequence"; abbr = "seq";
    default_cells = kPosteriorDefaultCells; round_cells = kPosteriorRoundCells;
    pair_ints = (size_t)kAlignHead + 2 * cap;
    chan_ints = 1;   // posterior_kernel's error word
    invariant = "a reached cell without its arrival";
  }
  std::string workspace_note(const WordRound &R) const override {
    const size_t stay = altern_stay_doubles(R.pairs, (size_t)R.A.ns_cap, cap, (size_t)altern_tab_slots(R.A.na_cap));
    return ", " + std::to_string(R.cnt * post_slot_bytes(R.A.ns_cap, R.A.na_cap)) + " bytes of posteriors, " + std::to_string(8 * stay) +
           " bytes of slot workspace";
  }
  void clear() override {
    align_zero(log_z, n); out.clear(np, cap); align_zero(word_post, np * cap); align_zero(path_logpost, np);
    align_zero(none_post, np * cap); align_zero(n_distinct, np * cap); align_zero(alt_word, np * cap * K); align_zero(alt_post, np * cap * K);
  }
  int launch(WordRound &R) override {
    const AlignView &V = *R.V;
    AlignState &S = *V.as;
    const AlignDev A = R.align_dev();
    const size_t cnt = R.cnt, pairs = R.pairs;
    // what comes back: log_z [cnt], confidence_kernel's results, none_post [pairs][cap], alt_post [pairs][cap][K], then as int32
    // n_distinct [pairs][cap] and alt_word [pairs][cap][K]
    at_conf = cnt;
    at_none = at_conf + pairs * dper;
    at_post = at_none + pairs * cap;
    at_ints = at_post + pairs * cap * K;
    const size_t n_ints = pairs * cap * (1 + K), res_n = at_ints + (n_ints + 1) / 2;
    PostDev P;
    const int rc = post_workspace(*this, R, res_n - cnt, graph_scale, acoustic_scale, &P);
    if (rc != WFST_OK) return rc;
    // what stays on the device
    const size_t tab = (size_t)altern_tab_slots(A.na_cap), stay = altern_stay_doubles(pairs, (size_t)A.ns_cap, cap, tab);
    if (S.alt.n < stay) {
      ALIGN_TRY(hipStreamSynchronize(V.stream));
      if (align_grow(S.alt, stay) != hipSuccess) {
        (void)hipGetLastError();
        return word_query_no_memory(*this, R);
      }
    }
    AltDev Q = {};
    Q.lat_toks = V.D->lat_toks;
    Q.lat_tok_cap = V.D->lat_tok_cap;
    Q.n_alts = (int32_t)K;
    Q.none = P.log_z + at_none;
    Q.alt_post = P.log_z + at_post;
    Q.n_distinct = reinterpret_cast<int32_t *>(P.log_z + at_ints);
    Q.alt_word = Q.n_distinct + pairs * cap;
    Q.acost = S.alt.p;
    Q.early = Q.acost + pairs * (size_t)A.ns_cap;
    Q.tab_key = reinterpret_cast<unsigned long long *>(Q.early + pairs * cap);
    Q.tab_mass = Q.early + pairs * cap + pairs * tab;
    Q.tab_slots = (int64_t)tab;
    launch_align_index(*V.D, A, R.chan, (int)cnt, V.stream);
    ALIGN_TRY(hipGetLastError());
    launch_align(*V.D, A, R.chan, (int)cnt, V.stream);
    ALIGN_TRY(hipGetLastError());
    launch_posterior(*V.D, A, P, R.chan, (int)cnt, V.stream);
    ALIGN_TRY(hipGetLastError());
    launch_confidence(A, P, (int)cnt, V.stream);
    ALIGN_TRY(hipGetLastError());
    launch_slot_mass(A, P, Q, (int)cnt, V.stream);
    ALIGN_TRY(hipGetLastError());
    launch_slot_none(A, P, Q, R.chan, (int)cnt, V.stream);   // (behind confidence_kernel: it takes over AlignDev::path)
    ALIGN_TRY(hipGetLastError());
    R.more_dst = S.post_pin.p; R.more_src = P.log_z; R.more_bytes = res_n * 8;
    return WFST_OK;
  }
  int unpack(const WordRound &R, size_t j, size_t o, int32_t) override {
    const size_t ns = (size_t)R.n_seqs;
    const double *landed = R.V->as->post_pin.p;
    const int32_t *ints = reinterpret_cast<const int32_t *>(landed + at_ints), *words = ints + R.pairs * cap;
    if (log_z) log_z[o] = landed[j];
    for (size_t q = 0; q < ns; ++q) {
      const size_t at = j * ns + q;
      const int32_t *r = R.landed + at * pair_ints;
      if (!r[0]) continue;
      const double *x = landed + at_conf + at * dper;
      const size_t p = o * ns + q;
      const size_t len = (size_t)std::max(R.seq_len[p], 0);
      out.take(r, p, len, cap);
      if (path_logpost) path_logpost[p] = x[0];
      if (word_post) memcpy(word_post + p * cap, x + 1, len * 8);
      if (none_post) memcpy(none_post + p * cap, landed + at_none + at * cap, len * 8);
      if (n_distinct) memcpy(n_distinct + p * cap, ints + at * cap, len * 4);
      if (alt_post) memcpy(alt_post + p * cap * K, landed + at_post + at * cap * K, len * K * 8);
      if (alt_word) memcpy(alt_word + p * cap * K, words + at * cap * K, len * K * 4);
    }
    return WFST_OK;
  }
};
}  // namespace

int wfst_decoder_word_alternatives(wfst_decoder *d, const int32_t *channels, int32_t n, int32_t use_final_probs, double graph_scale,
                                   double acoustic_scale, int32_t n_alts, int32_t n_seqs, int32_t cap_words, const int32_t *seq_words,
                                   const int32_t *seq_len, int64_t max_cells, int32_t *status, double *log_z, int32_t *found, int32_t *n_arcs,
                                   int32_t *begin_frame, int32_t *end_frame, double *word_post, double *none_post, int32_t *n_distinct,
                                   int32_t *alt_word, double *alt_post, double *path_logpost, float *tot_score, float *lm_score) {
  // (n, np, cap, n_alts are used only behind the checks of n, n_seqs, cap_words and n_alts)
  AlternQuery q((size_t)n, (size_t)n * (size_t)n_seqs, (size_t)cap_words, (size_t)n_alts,
                AlignOutputs{found, n_arcs, begin_frame, end_frame, tot_score, lm_score});
  if (!std::isfinite(graph_scale) || !std::isfinite(acoustic_scale) || graph_scale < 0.0 || acoustic_scale < 0.0)
    q.arg_error = "graph_scale / acoustic_scale must be finite and >= 0";
  else if (n_alts < 1 || n_alts > WFST_ALTERN_MAX_ALTS) q.arg_error = "1 <= n_alts <= 16 alternatives per slot";
  q.graph_scale = graph_scale; q.acoustic_scale = acoustic_scale;
  q.log_z = log_z; q.word_post = word_post; q.none_post = none_post; q.alt_post = alt_post; q.path_logpost = path_logpost;
  q.n_distinct = n_distinct; q.alt_word = alt_word;
  return word_query_run(q, d, channels, n, use_final_probs, n_seqs, cap_words, seq_words, seq_len, max_cells, status);
}
