// The seam between wfst_capi.cc and wfst_capi_nearest.cc (wfst_decoder_nearest_words): the entry point that launches nearest_kernel
// (wfst_nearest.hip) is a translation unit of its own, as wfst_capi_align.cc is, so that wfst_capi.cc links against exactly the
// launches it always did.  It sees a decoder through wfst_capi_align.h's view and nothing else: the same channel-list checks, the
// same emit of the live channels, the same in-arc index -- and the same workspace, the decoder's AlignState (the two calls are
// synchronous and never in flight together; AlignState::cells counts 32-bit words, a cell here takes two).  Host only.
#ifndef WFST_CAPI_NEAREST_H_
#define WFST_CAPI_NEAREST_H_

#include "wfst_capi_align.h"

namespace wfst {

// max_cells = 0: a lattice of 65 536 states (the determinizer's own default bound, wfst_limits.det_raw_states) against 64 words, as
// wfst_decoder_align_words has it.  A cell is 8 bytes: 32.5 MiB of table per reference at this bound.
constexpr int64_t kNearestDefaultCells = 65536ll * 65;
// cells of one round's tables (256 MiB); a channel whose own references need more runs in a round of its own
constexpr int64_t kNearestRoundCells = 32ll << 20;

}  // namespace wfst
#endif
