// The seam between the library and wfst_capi_posterior.cc (wfst_decoder_word_confidence): the entry point that launches
// posterior_kernel and confidence_kernel (wfst_posterior.hip) behind the alignment's own launches is a translation unit of its own, as
// wfst_capi_align.cc and wfst_capi_nearest.cc are.  It sees a decoder through wfst_capi_align.h's view; its workspace sits in the
// decoder's AlignState.  Host only.
#ifndef WFST_CAPI_POSTERIOR_H_
#define WFST_CAPI_POSTERIOR_H_

#include "wfst_capi_align.h"

namespace wfst {

// max_cells = 0: wfst_decoder_align_words' default bound, 65 536 states x 65 cells
constexpr int64_t kPosteriorDefaultCells = 65536ll * 65;
// cells of one round's alignment tables (256 MiB), as wfst_decoder_align_words takes its rounds
constexpr int64_t kPosteriorRoundCells = 64ll << 20;

// The posterior workspace of a round, grown in a query's launch() hook, and the PostDev over it: alpha, beta [cnt][ns_cap],
// gamma [cnt][na_cap], then what comes back -- log_z [cnt] and res_more doubles of the query's own at P->out; sarc [cnt][na_cap], then
// done and soff [cnt][ns_cap] as int2 halves.  chan_err is the slots' error words behind the pairs' packed results (chan_ints = 1);
// the landing place holds cnt + res_more doubles.
inline int post_workspace(const WordQuery &q, const WordRound &R, size_t res_more, double graph_scale, double acoustic_scale, PostDev *P) {
  const AlignView &V = *R.V;
  AlignState &S = *V.as;
  const size_t cnt = R.cnt, nsc = (size_t)R.A.ns_cap, nac = (size_t)R.A.na_cap;
  const size_t res_at = cnt * (2 * nsc + nac), res_n = cnt + res_more, post_n = res_at + res_n;
  const size_t pidx_n = cnt * nac + cnt * nsc;
  if (S.post.n < post_n || S.post_idx.n < pidx_n) {
    ALIGN_TRY(hipStreamSynchronize(V.stream));
    if (align_grow(S.post, post_n) != hipSuccess || align_grow(S.post_idx, pidx_n) != hipSuccess) {
      (void)hipGetLastError();
      return word_query_no_memory(q, R);
    }
  }
  ALIGN_TRY(S.post_pin.reserve(res_n));
  *P = PostDev{};
  P->alpha = S.post.p;
  P->beta = P->alpha + cnt * nsc;
  P->gamma = P->beta + cnt * nsc;
  P->log_z = S.post.p + res_at;
  P->out = P->log_z + cnt;
  P->sarc = S.post_idx.p;
  P->done = reinterpret_cast<int32_t *>(S.post_idx.p + cnt * nac);
  P->soff = P->done + cnt * nsc;
  P->chan_err = S.out.p + R.pairs * q.pair_ints;
  P->graph_scale = graph_scale;
  P->acoustic_scale = acoustic_scale;
  return WFST_OK;
}

}  // namespace wfst
#endif
