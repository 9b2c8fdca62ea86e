// wfst_decoder_nearest_words: the path of a channel's raw lattice nearest a reference word sequence -- least word edit distance, then
// least cost -- with the edit counts, the path's words, their times and scores, for a channel list (live and finalized channels mixed)
// and several references per channel, one launch per stage (lattice_emit_kernel for the live channels, align_index_kernel,
// nearest_kernel: wfst_nearest.hip).  A translation unit of its own -- see wfst_capi_nearest.h.
#include "wfst_capi_nearest.h"

using namespace wfst;

namespace {
struct NearestQuery : WordQuery {
  size_t np, cap, hcap;
  int32_t cap_hyp;
  int32_t *found, *n_err, *n_cor, *n_sub, *n_ins, *n_del, *n_arcs, *n_hyp, *hyp_words, *begin_frame, *end_frame, *ref_hyp;
  float *tot_score, *lm_score;
  NearestQuery(size_t np_, int32_t cap_words, int32_t cap_hyp_) : np(np_), cap((size_t)cap_words), hcap((size_t)cap_hyp_), cap_hyp(cap_hyp_) {
    name = "nearest"; item = "reference"; abbr = "ref";
    caps = "cap_words / cap_hyp"; cap_extra = cap_hyp;
    default_cells = kNearestDefaultCells; round_cells = kNearestRoundCells;
    cell_words = 2;
    path_extra = cap_words;   // a path has fewer arcs than the lattice has states, and at most one deletion per reference word
    pair_ints = (size_t)nearest_out_ints(cap_words, cap_hyp);
    arc_limit = 1 << 30;      // (a traceback step names its in-arc record in 30 bits)
    invariant = "a traced path that does not reproduce its cell";
  }
  std::string workspace_note(const WordRound &) const override { return " of 8 bytes"; }
  void clear() override {
    align_zero(found, np); align_zero(n_err, np); align_zero(n_cor, np); align_zero(n_sub, np); align_zero(n_ins, np); align_zero(n_del, np);
    align_zero(n_arcs, np); align_zero(n_hyp, np); align_zero(hyp_words, np * hcap); align_zero(begin_frame, np * hcap);
    align_zero(end_frame, np * hcap); align_zero(ref_hyp, np * cap); align_zero(tot_score, np); align_zero(lm_score, np);
  }
  int launch(WordRound &R) override {
    const AlignView &V = *R.V;
    NearestDev N = {};
    N.lat_toks = V.D->lat_toks;
    N.lat_tok_cap = V.D->lat_tok_cap;
    N.n_refs = R.n_seqs;
    N.cap_words = R.cap_words;
    N.cap_hyp = cap_hyp;
    N.path_cap = R.A.ns_cap + path_extra;
    N.sil_bits = V.sil_bits;
    N.n_tid = V.sil_ntid;
    N.cell_off = R.cell_off;
    N.ref_len = R.len;
    N.ref_words = R.words;
    N.cells = reinterpret_cast<unsigned long long *>(V.as->cells.p);
    N.path = V.as->path.p;
    N.out = V.as->out.p;
    launch_align_index(*V.D, R.A, R.chan, (int)R.cnt, V.stream);
    ALIGN_TRY(hipGetLastError());
    launch_nearest(R.A, N, R.chan, (int)R.cnt, V.stream);
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
      const size_t len = (size_t)std::max(R.seq_len[p], 0), nh = std::min((size_t)r[10], hcap);
      if (found) found[p] = 1;
      if (n_arcs) n_arcs[p] = r[1];
      if (tot_score) memcpy(&tot_score[p], &r[2], 4);
      if (lm_score) memcpy(&lm_score[p], &r[3], 4);
      if (n_err) n_err[p] = r[5];
      if (n_cor) n_cor[p] = r[6];
      if (n_sub) n_sub[p] = r[7];
      if (n_ins) n_ins[p] = r[8];
      if (n_del) n_del[p] = r[9];
      if (n_hyp) n_hyp[p] = r[10];
      if (hyp_words) memcpy(hyp_words + p * hcap, r + kNearestHead, nh * 4);
      if (begin_frame) memcpy(begin_frame + p * hcap, r + kNearestHead + hcap, nh * 4);
      if (end_frame) memcpy(end_frame + p * hcap, r + kNearestHead + 2 * hcap, nh * 4);
      if (ref_hyp) memcpy(ref_hyp + p * cap, r + kNearestHead + 3 * hcap, len * 4);
      // the path has more words than the caller made room for: everything else of the answer stands, n_hyp is the room it takes
      if ((size_t)r[10] > hcap && code == WFST_OK)
        code = capi_fail(WFST_E_CAPACITY, "channel " + std::to_string(channel) + ": nearest: a path of " + std::to_string(r[10]) +
                                              " words, cap_hyp is " + std::to_string(cap_hyp));
    }
    return code;
  }
};
}  // namespace

int wfst_decoder_nearest_words(wfst_decoder *d, const int32_t *channels, int32_t n, int32_t use_final_probs, int32_t n_refs, int32_t cap_words,
                               const int32_t *ref_words, const int32_t *ref_len, int32_t cap_hyp, int64_t max_cells, int32_t *status,
                               int32_t *found, int32_t *n_err, int32_t *n_cor, int32_t *n_sub, int32_t *n_ins, int32_t *n_del, int32_t *n_arcs,
                               int32_t *n_hyp, int32_t *hyp_words, int32_t *begin_frame, int32_t *end_frame, int32_t *ref_hyp, float *tot_score,
                               float *lm_score) {
  // (np and the capacities are used only behind the driver's checks of n, n_refs, cap_words and cap_hyp)
  NearestQuery q((size_t)n * (size_t)n_refs, cap_words, cap_hyp);
  q.found = found; q.n_err = n_err; q.n_cor = n_cor; q.n_sub = n_sub; q.n_ins = n_ins; q.n_del = n_del; q.n_arcs = n_arcs; q.n_hyp = n_hyp;
  q.hyp_words = hyp_words; q.begin_frame = begin_frame; q.end_frame = end_frame; q.ref_hyp = ref_hyp;
  q.tot_score = tot_score; q.lm_score = lm_score;
  return word_query_run(q, d, channels, n, use_final_probs, n_refs, cap_words, ref_words, ref_len, max_cells, status);
}
