// The seam between the library and wfst_capi_bias_sparse.cc (wfst_bias_book_compile, wfst_bias_books_*,
// wfst_decoder_biased_words_sparse): phrase boosting for lists of up to 65 536 nodes, bias_reach_kernel and bias_sparse_kernel
// (wfst_bias_sparse.hip) behind align_index_kernel.  The call has a driver of its own built from the word queries' pieces
// (align_begin, align_emit, cut_round, launch_align_index, the AlignState workspace): its cells are known only after a device pass,
// so word_query_run's "table = states x columns" does not describe it.  Host only.
//
// One index launch for all listed channels that have a lattice, then the reach stage, then the sweep in rounds of round_cells cells.
// The reach stage's regions per channel: the first holds max(1024, 4 x states) cells (never more than max_cells) and
// max(4096, 8 x arcs) edges.  A channel whose region overflowed gets that region four times as large (cells: up to max_cells; edges:
// up to 16 x max_cells, at most 2^30) and the stage is launched again -- for all the call's channels, whose regions are laid out
// anew -- until every channel fits or has failed: at most log4(max_cells / first) + 1 launches for the cells and as many for the
// edges.  Every launch terminates whatever the sizes: an overflow ends that channel's pass.  This is growth, not a retry.
#ifndef WFST_CAPI_BIAS_SPARSE_H_
#define WFST_CAPI_BIAS_SPARSE_H_

#include "wfst_capi_bias.h"

namespace wfst {

// max_cells = 0: 4 Mi cells of one channel (32 MiB per setting)
constexpr int64_t kBookDefaultCells = 4ll << 20;
constexpr int64_t kBookMaxCells = 1ll << 30;   // cell ids and edge offsets are 32-bit
constexpr int64_t kBookFirstCells = 1024, kBookFirstEdges = 4096;

}  // namespace wfst

// A set of books resident on one device; every HIP resource is an owner and goes with the set.
struct wfst_bias_books {
  int device = 0;
  int32_t n_books = 0;
  int64_t total_phrases = 0, total_nodes = 0;
  std::vector<int32_t> hdr;   // [n_books][kBookHdr], as on the device
  wfst::DevBuf<int32_t> d_hdr, d_ints;
  wfst::DevBuf<double> d_beta;
  int64_t device_bytes() const { return (int64_t)(d_hdr.bytes() + d_ints.bytes() + d_beta.bytes()); }
  wfst::BiasBooksDev view() const { return wfst::BiasBooksDev{d_hdr.p, d_ints.p, d_beta.p}; }
};
#endif
