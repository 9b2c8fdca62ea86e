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

}  // namespace wfst
#endif
