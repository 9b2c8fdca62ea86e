// wfst_decoder_sequence_posterior: the posterior of a whole word sequence (mode 0: the share of the lattice's weight on ALL paths
// that spell it) or of a phrase (mode 1: the expected number of times a path says it, and at which frame) on a channel's raw lattice,
// for a channel list (live and finalized channels mixed) and several sequences per channel, one launch per stage
// (lattice_emit_kernel for the live channels, align_index_kernel, posterior_kernel, seqpost_kernel: wfst_align.hip,
// wfst_posterior.hip, wfst_seqpost.hip).  A translation unit of its own -- see wfst_capi_seqpost.h.
#include "wfst_capi_seqpost.h"

#include <cmath>

using namespace wfst;

namespace {
struct SeqPostQuery : WordQuery {
  size_t n, np, capf;
  int32_t mode, cap_frames;
  double graph_scale, acoustic_scale;
  int32_t *found, *n_frames;
  double *log_z, *seq_logpost, *hit_mass;
  SeqPostQuery(size_t n_, size_t np_, int32_t mode_, int32_t cap_frames_)
      : n(n_), np(np_), capf((size_t)std::max(cap_frames_, 0)), mode(mode_), cap_frames(cap_frames_) {
    name = "sequence posterior"; item = "sequence"; abbr = "seq";
    min_len = mode == 1 ? 1 : 0;
    default_cells = kSeqPostDefaultCells; round_cells = kSeqPostRoundCells;
    cell_words = 2;
    pair_ints = (size_t)kSeqPostHead;
    chan_ints = 1;   // posterior_kernel's error word
    invariant = "an unknown error word";
  }
  bool rows() const { return hit_mass && mode == 1; }
  std::string workspace_note(const WordRound &R) const override {
    return " of 8 bytes, " + std::to_string(R.cnt * post_slot_bytes(R.A.ns_cap, R.A.na_cap)) + " bytes of posteriors";
  }
  void clear() override {
    align_zero(log_z, n); align_zero(n_frames, n); align_zero(found, np); align_zero(seq_logpost, np); align_zero(hit_mass, np * capf);
  }
  int launch(WordRound &R) override {
    const AlignView &V = *R.V;
    const AlignDev A = R.align_dev();
    const size_t cnt = R.cnt, more = R.pairs + (rows() ? R.pairs * capf : 0);
    // what comes back: log_z [cnt], seq_logpost [pairs], the hit_mass rows [pairs][cap_frames]
    PostDev P;
    const int rc = post_workspace(*this, R, more, graph_scale, acoustic_scale, &P);
    if (rc != WFST_OK) return rc;
    SeqPostDev Q = {};
    Q.lat_toks = V.D->lat_toks;
    Q.lat_tok_cap = V.D->lat_tok_cap;
    Q.mode = mode;
    Q.cap_frames = cap_frames;
    Q.out = P.out;
    Q.hit = rows() ? P.out + R.pairs : nullptr;
    launch_align_index(*V.D, A, R.chan, (int)cnt, V.stream);
    ALIGN_TRY(hipGetLastError());
    launch_posterior(*V.D, A, P, R.chan, (int)cnt, V.stream);
    ALIGN_TRY(hipGetLastError());
    launch_seqpost(A, P, Q, R.chan, (int)cnt, V.stream);
    ALIGN_TRY(hipGetLastError());
    R.more_dst = V.as->post_pin.p; R.more_src = P.log_z; R.more_bytes = (cnt + more) * 8;
    return WFST_OK;
  }
  int unpack(const WordRound &R, size_t j, size_t o, int32_t channel) override {
    const size_t ns = (size_t)R.n_seqs;
    const double *landed = R.V->as->post_pin.p, *lp = landed + R.cnt, *rows_at = lp + R.pairs;
    const int32_t nf = R.landed[j * ns * pair_ints + 1];   // (every pair of the slot carries it)
    if (log_z) log_z[o] = landed[j];
    if (n_frames) n_frames[o] = nf;
    const bool fits = nf <= cap_frames;
    for (size_t q = 0; q < ns; ++q) {
      const size_t p = o * ns + q, at = j * ns + q;
      if (!R.landed[at * pair_ints]) continue;
      if (found) found[p] = 1;
      if (seq_logpost) seq_logpost[p] = lp[at];
      if (rows() && fits) memcpy(hit_mass + p * capf, rows_at + at * capf, (size_t)nf * 8);
    }
    // the lattice has more frames than the rows hold: everything else of the answer stands, n_frames is the room they take
    if (rows() && !fits)
      return capi_fail(WFST_E_CAPACITY, "channel " + std::to_string(channel) + ": sequence posterior: a lattice of " + std::to_string(nf) +
                                            " frames, cap_frames is " + std::to_string(cap_frames));
    return WFST_OK;
  }
};
}  // namespace

int wfst_decoder_sequence_posterior(wfst_decoder *d, const int32_t *channels, int32_t n, int32_t use_final_probs, double graph_scale,
                                    double acoustic_scale, int32_t mode, int32_t n_seqs, int32_t cap_words, const int32_t *seq_words,
                                    const int32_t *seq_len, int64_t max_cells, int32_t cap_frames, int32_t *status, double *log_z,
                                    int32_t *n_frames, int32_t *found, double *seq_logpost, double *hit_mass) {
  // (n and np are used only behind the driver's checks of n and n_seqs)
  SeqPostQuery q((size_t)n, (size_t)n * (size_t)n_seqs, mode, cap_frames);
  if (!std::isfinite(graph_scale) || !std::isfinite(acoustic_scale) || graph_scale < 0.0 || acoustic_scale < 0.0)
    q.arg_error = "graph_scale / acoustic_scale must be finite and >= 0";
  else if (mode < 0 || mode > 1) q.arg_error = "mode must be 0 (sentence) or 1 (phrase)";
  else if (cap_frames < 0) q.arg_error = "cap_frames < 0";
  else if (hit_mass && cap_frames == 0) q.arg_error = "hit_mass without room: cap_frames == 0";
  q.graph_scale = graph_scale; q.acoustic_scale = acoustic_scale;
  q.found = found; q.n_frames = n_frames; q.log_z = log_z; q.seq_logpost = seq_logpost; q.hit_mass = hit_mass;
  return word_query_run(q, d, channels, n, use_final_probs, n_seqs, cap_words, seq_words, seq_len, max_cells, status);
}
