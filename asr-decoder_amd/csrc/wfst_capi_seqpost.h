// The seam between the library and wfst_capi_seqpost.cc (wfst_decoder_sequence_posterior): the entry point that launches
// posterior_kernel (wfst_posterior.hip) and seqpost_kernel (wfst_seqpost.hip) behind align_index_kernel is a translation unit of its
// own, as wfst_capi_posterior.cc is.  It sees a decoder through wfst_capi_align.h's view; its tables sit in AlignState::cells, 8 bytes
// per cell, and the posteriors in the workspace wfst_capi_posterior.h lays out.  Host only.
#ifndef WFST_CAPI_SEQPOST_H_
#define WFST_CAPI_SEQPOST_H_

#include "wfst_capi_posterior.h"

namespace wfst {

// max_cells = 0 and the cells of a round: wfst_decoder_align_words' bound, and 256 MiB of 8-byte cells
constexpr int64_t kSeqPostDefaultCells = kPosteriorDefaultCells;
constexpr int64_t kSeqPostRoundCells = 32ll << 20;

}  // namespace wfst
#endif
