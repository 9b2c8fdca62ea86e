// The seam between the library and wfst_capi_framepost.cc (wfst_decoder_frame_posteriors): the entry point that launches
// frame_post_kernel and frame_pack_kernel (wfst_framepost.hip) behind align_index_kernel and posterior_kernel is a translation unit of
// its own, as wfst_capi_seqpost.cc is.  It sees a decoder through wfst_capi_align.h's view and runs word_query_run with one empty
// sequence per channel: a table of states x 1 cells, so that max_cells bounds a lattice's states and the rounds, the channels' own
// failures and the error words are the siblings'.  Its staging area and workspace hang off the decoder's AlignState.  Host only.
#ifndef WFST_CAPI_FRAMEPOST_H_
#define WFST_CAPI_FRAMEPOST_H_

#include "wfst_capi_posterior.h"

namespace wfst {

// max_cells = 0 and the cells of a round: wfst_decoder_word_confidence's
constexpr int64_t kFramePostDefaultCells = kPosteriorDefaultCells;
constexpr int64_t kFramePostRoundCells = kPosteriorRoundCells;

// per slot of a round: doubles (the staged posts, the sort's workspace, the frames' masses) and ints (the staged classes, the sort's
// keys, the frames' counts and n_distinct)
inline size_t frame_post_slot_doubles(size_t na_cap, size_t fr_cap) { return 2 * na_cap + fr_cap; }
inline size_t frame_post_slot_ints(size_t na_cap, size_t fr_cap) { return 2 * na_cap + 2 * fr_cap; }

}  // namespace wfst
#endif
