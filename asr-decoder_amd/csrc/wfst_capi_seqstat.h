// The seam between the library and wfst_capi_seqstat.cc (wfst_decoder_sequence_stats): the entry point that launches acc_kernel,
// seqstat_frame_kernel, seqstat_pack_kernel and seqstat_dense_kernel (wfst_seqstat.hip) behind align_index_kernel and posterior_kernel
// is a translation unit of its own, as wfst_capi_framepost.cc is.  It sees a decoder through wfst_capi_align.h's view and runs
// word_query_run with one empty sequence per channel, so that max_cells bounds a lattice's states and the rounds, the channels' own
// failures and the error words are the siblings'.  Its staging area and workspace hang off the decoder's AlignState.  Host only.
#ifndef WFST_CAPI_SEQSTAT_H_
#define WFST_CAPI_SEQSTAT_H_

#include "wfst_capi_posterior.h"

namespace wfst {

// max_cells = 0 and the cells of a round: wfst_decoder_word_confidence's
constexpr int64_t kSeqStatDefaultCells = kPosteriorDefaultCells;
constexpr int64_t kSeqStatRoundCells = kPosteriorRoundCells;

// per slot of a round: doubles (fa, fb; w and the sort's two workspaces; the staged posts and values; tot) and ints (the sort's keys,
// the staged classes, the frames' counts and flags, the reference row)
inline size_t seq_stat_slot_doubles(size_t ns_cap, size_t na_cap, size_t fr_cap) { return 2 * ns_cap + 3 * na_cap + 2 * (na_cap + fr_cap) + 1; }
inline size_t seq_stat_slot_ints(size_t na_cap, size_t fr_cap) { return na_cap + (na_cap + fr_cap) + 3 * fr_cap; }

}  // namespace wfst
#endif
