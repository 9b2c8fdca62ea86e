// The seam between the library and wfst_capi_rescale.cc (wfst_decoder_rescaled_words): the entry point that launches rescale_kernel
// (wfst_rescale.hip) behind align_index_kernel is a translation unit of its own, as wfst_capi_nearest.cc is.  It sees a decoder
// through wfst_capi_align.h's view and runs word_query_run with one empty sequence per (channel, setting): a table of states x 1
// cells of 8 bytes each, so that max_cells bounds a lattice's states and the rounds, the channels' own failures and the error words
// are the siblings'.  Its cells, path scratch and packed results are the decoder's AlignState's.  Host only.
#ifndef WFST_CAPI_RESCALE_H_
#define WFST_CAPI_RESCALE_H_

#include "wfst_capi_align.h"

namespace wfst {

// max_cells = 0: wfst_decoder_align_words' default bound, 65 536 states x 65 cells, here of lattice states
constexpr int64_t kRescaleDefaultCells = 65536ll * 65;
// cells of one round (256 MiB at 8 bytes a cell); a channel whose own settings need more runs in a round of its own
constexpr int64_t kRescaleRoundCells = 32ll << 20;

}  // namespace wfst
#endif
