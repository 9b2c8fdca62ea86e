// wfst_decoder_rescaled_words: the best path of a channel's raw lattice under other scales and a word penalty -- its words, their
// times, the alignment and the scores -- for a channel list (live and finalized channels mixed) and up to 64 settings shared by the
// listed channels, one launch per stage (lattice_emit_kernel for the live channels, align_index_kernel, rescale_kernel:
// wfst_rescale.hip).  A translation unit of its own -- see wfst_capi_rescale.h.
#include "wfst_capi_rescale.h"

#include <cmath>

using namespace wfst;

namespace {
struct RescaleQuery : WordQuery {
  size_t np, cap, tcap;   // pairs of the whole call; the caller's rows of words and of transition-ids (0: none asked for)
  RescaleSet set;
  int32_t *found, *n_arcs, *n_hyp, *n_tids, *hyp_words, *begin_frame, *end_frame, *tids;
  double *scaled_cost;
  float *tot_score, *lm_score;
  RescaleQuery(size_t np_, int32_t cap_words, size_t tcap_) : np(np_), cap((size_t)cap_words), tcap(tcap_) {
    name = "rescale"; item = "setting"; abbr = "set";
    default_cells = kRescaleDefaultCells; round_cells = kRescaleRoundCells;
    cell_words = 2;
    pair_ints = (size_t)rescale_out_ints((int64_t)cap, (int64_t)tcap);
    invariant = "a traced path that does not reproduce its cell";
  }
  std::string workspace_note(const WordRound &) const override { return " of 8 bytes"; }
  void clear() override {
    align_zero(found, np); align_zero(n_arcs, np); align_zero(n_hyp, np); align_zero(n_tids, np); align_zero(hyp_words, np * cap);
    align_zero(begin_frame, np * cap); align_zero(end_frame, np * cap); align_zero(tids, np * tcap); align_zero(scaled_cost, np);
    align_zero(tot_score, np); align_zero(lm_score, np);
  }
  int launch(WordRound &R) override {
    const AlignView &V = *R.V;
    RescaleDev Q = {};
    Q.lat_toks = V.D->lat_toks;
    Q.lat_tok_cap = V.D->lat_tok_cap;
    Q.cell_off = R.cell_off;
    Q.cells = reinterpret_cast<double *>(V.as->cells.p);
    Q.path = V.as->path.p;
    Q.path_cap = R.A.ns_cap;
    Q.n_set = R.n_seqs;
    Q.cap_words = (int32_t)cap;
    Q.cap_tids = (int32_t)tcap;
    Q.sil_bits = V.sil_bits;
    Q.n_tid = V.sil_ntid;
    Q.out = V.as->out.p;
    launch_align_index(*V.D, R.A, R.chan, (int)R.cnt, V.stream);
    ALIGN_TRY(hipGetLastError());
    launch_rescale(R.A, Q, set, R.chan, (int)R.cnt, V.stream);
    ALIGN_TRY(hipGetLastError());
    return WFST_OK;
  }
  int unpack(const WordRound &R, size_t j, size_t o, int32_t channel) override {
    const size_t ns = (size_t)R.n_seqs;
    int code = WFST_OK;
    for (size_t q = 0; q < ns; ++q) {
      const int32_t *r = R.landed + (j * ns + q) * pair_ints;
      if (!r[0]) continue;
      const size_t p = o * ns + q;
      const size_t nh = std::min((size_t)r[5], cap), nt = std::min((size_t)r[6], tcap);
      if (found) found[p] = 1;
      if (n_arcs) n_arcs[p] = r[1];
      if (tot_score) memcpy(&tot_score[p], &r[2], 4);
      if (lm_score) memcpy(&lm_score[p], &r[3], 4);
      if (n_hyp) n_hyp[p] = r[5];
      if (n_tids) n_tids[p] = r[6];
      if (scaled_cost) memcpy(&scaled_cost[p], &r[8], 8);
      if (hyp_words) memcpy(hyp_words + p * cap, r + kRescaleHead, nh * 4);
      if (begin_frame) memcpy(begin_frame + p * cap, r + kRescaleHead + cap, nh * 4);
      if (end_frame) memcpy(end_frame + p * cap, r + kRescaleHead + 2 * cap, nh * 4);
      if (tids) memcpy(tids + p * tcap, r + kRescaleHead + 3 * cap, nt * 4);
      // the path has more words or transition-ids than the caller made room for: everything else of the answer stands, the counts
      // are the room it takes
      if (((size_t)r[5] > cap || (tids && (size_t)r[6] > tcap)) && code == WFST_OK)
        code = capi_fail(WFST_E_CAPACITY, "channel " + std::to_string(channel) + ": rescale: a path of " + std::to_string(r[5]) + " words and " +
                                              std::to_string(r[6]) + " transition-ids, cap_words is " + std::to_string(cap) +
                                              (tids ? " and cap_tids " + std::to_string(tcap) : std::string()));
    }
    return code;
  }
};
}  // namespace

int wfst_decoder_rescaled_words(wfst_decoder *d, const int32_t *channels, int32_t n, int32_t use_final_probs, int32_t n_set,
                                const double *settings, int32_t cap_words, int32_t cap_tids, int64_t max_cells, int32_t *status,
                                int32_t *found, int32_t *n_arcs, int32_t *n_hyp, int32_t *n_tids, int32_t *hyp_words, int32_t *begin_frame,
                                int32_t *end_frame, int32_t *tids, double *scaled_cost, float *tot_score, float *lm_score) {
  if (!d || !channels) return capi_fail(WFST_E_ARG, "NULL decoder / channel list");
  if (n_set < 1 || n_set > kRescaleMaxSettings) return capi_fail(WFST_E_ARG, "1 <= n_set <= 64 settings");
  if (!settings) return capi_fail(WFST_E_ARG, "NULL settings");
  for (int32_t q = 0; q < n_set; ++q) {
    const double gs = settings[3 * q], as = settings[3 * q + 1], wip = settings[3 * q + 2];
    if (!std::isfinite(gs) || !std::isfinite(as) || gs < 0.0 || as < 0.0)
      return capi_fail(WFST_E_ARG, "graph_scale / acoustic_scale must be finite and >= 0");
    if (!std::isfinite(wip)) return capi_fail(WFST_E_ARG, "word_penalty must be finite");
  }
  if (cap_words <= 0) return capi_fail(WFST_E_ARG, "cap_words <= 0");
  if (cap_tids < 0) return capi_fail(WFST_E_ARG, "cap_tids < 0");
  if (max_cells < 0) return capi_fail(WFST_E_ARG, "max_cells < 0");
  // (np is used only behind the driver's checks of n)
  RescaleQuery q((size_t)n * (size_t)n_set, cap_words, tids ? (size_t)cap_tids : 0);
  q.set = RescaleSet{};
  std::copy(settings, settings + 3 * (size_t)n_set, q.set.v);
  q.found = found; q.n_arcs = n_arcs; q.n_hyp = n_hyp; q.n_tids = n_tids; q.hyp_words = hyp_words; q.begin_frame = begin_frame;
  q.end_frame = end_frame; q.tids = tids; q.scaled_cost = scaled_cost; q.tot_score = tot_score; q.lm_score = lm_score;
  // one empty sequence per (channel, setting): a table of states x 1 cells
  const std::vector<int32_t> none(std::max<size_t>((size_t)std::max(n, 0) * (size_t)n_set, 1), 0);
  return word_query_run(q, d, channels, n, use_final_probs, n_set, 1, none.data(), none.data(), max_cells, status);
}
