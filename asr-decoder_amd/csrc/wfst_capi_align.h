// The seam between wfst_capi.cc and wfst_capi_align.cc (wfst_decoder_align_words): the entry point that launches align_index_kernel
// and align_kernel (wfst_align.hip) is a translation unit of its own, as wfst_capi_words.cc and wfst_capi_nbwords.cc are, so that
// wfst_capi.cc links against exactly the launches it always did.  Host only.
#ifndef WFST_CAPI_ALIGN_H_
#define WFST_CAPI_ALIGN_H_

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/wfst_decoder.h"
#include "wfst_capi_words.h"   // capi_fail, capi_fail_ctl
#include "wfst_device.h"
#include "wfst_hip_own.h"

namespace wfst {

// a decoder's alignment workspace, allocated by the first call and grown on demand: the in-arc indices of a round's channels, the
// tables and path scratch of its (channel, sequence) pairs, the staged inputs, the packed results and their page-locked landing place
struct AlignState {
  DevBuf<int32_t> idx, path, in, out;
  DevBuf<uint32_t> cells;
  PinBuf<int32_t> pin;
  // wfst_decoder_word_confidence and wfst_decoder_sequence_posterior (wfst_capi_posterior.h: post_workspace): the posterior workspace of
  // a round's channels and its results' landing place
  DevBuf<double> post;
  DevBuf<int2> post_idx;
  PinBuf<double> post_pin;
  // wfst_decoder_word_alternatives (wfst_capi_altern.h): what stays on the device -- A per state and sequence, the cells' "ended early"
  // mass, the (cell, word) tables of the sequences whose keys outgrow LDS
  DevBuf<double> alt;
  // wfst_decoder_frame_posteriors (wfst_capi_framepost.h): the frames' staged lists and sums and the workspace of the frames whose
  // records outgrow LDS; the caller's label map
  DevBuf<double> fpost;
  DevBuf<int32_t> fpost_idx, fpost_map;
  // wfst_decoder_sequence_stats (wfst_capi_seqstat.h): fa, fb, w, the staged lists and the sort's workspace; the reference rows beside
  // the frames' counts; the caller's label map; the dense rows' pointers, pitches and row counts
  DevBuf<double> sstat;
  DevBuf<int32_t> sstat_idx, sstat_map;
  DevBuf<int64_t> sstat_in;
  // wfst_decoder_biased_words (wfst_capi_bias.h): the bias list of every slot of a round
  DevBuf<int32_t> bias_list;
  // wfst_decoder_biased_words_sparse (wfst_capi_bias_sparse.h): the slots' reach regions (sets, edges, stage), their places and
  // sizes, their result words
  DevBuf<int32_t> reach, reach_head;
  DevBuf<int64_t> reach_reg;
};

// what the entry point sees of a decoder (sil_bits: the silence bitmap over transition-ids 1..sil_ntid, nullptr: none)
struct AlignView {
  int device;
  const DecoderDev *D;
  AlignState *as;
  const uint32_t *sil_bits;
  int32_t sil_ntid;
  hipStream_t stream;
};
// The checks of the channel list (WFST_E_ARG: count, range, duplicates; WFST_E_STATE: no lattice_links, a channel never
// initialised); no device work.
int align_begin(wfst_decoder *d, const int32_t *channels, int32_t n, AlignView *v);
// 0 never initialised, 1 decoding, 2 finalized
int align_channel_state(const wfst_decoder *d, int32_t channel);
// the largest ilabel of the decoder's graph, from the graph's host copy (what wfst_graph_set_tid2phone checks its map against)
int32_t align_max_ilabel(const wfst_decoder *d);
// A prefetch in flight harvested, the live channels of `list` emitted in one launch (launch_lattice_emit: the live-prune mode and
// use_final_probs as GetRawLattice takes them), the control blocks read: sizes[4 i ..] = {states, arcs, frames decoded, error word}
// of list[i]'s raw lattice as it sits on the device.  Synchronises the decoder's stream.
int align_emit(wfst_decoder *d, const std::vector<int32_t> &list, int32_t use_final_probs, std::vector<int32_t> *sizes);

// ---- the round driver of the word queries (wfst_capi_wordquery.cc) ----------------------------------------------------------
// wfst_decoder_align_words, wfst_decoder_nearest_words, wfst_decoder_word_confidence, wfst_decoder_sequence_posterior and
// wfst_decoder_word_alternatives ask the listed channels' raw lattices about n_seqs word sequences each: one table of
// states x (words + 1) cells per (channel, sequence) pair over the in-arc index align_index_kernel builds.
// wfst_decoder_frame_posteriors and wfst_decoder_sequence_stats ask about one empty sequence each (wfst_capi_framepost.h,
// wfst_capi_seqstat.h), wfst_decoder_rescaled_words about one empty sequence per setting (wfst_capi_rescale.h),
// wfst_decoder_biased_words about one sequence of (nodes - 1) per setting, so that a table is states x nodes (wfst_capi_bias.h).
// word_query_run is the sequence they share; a WordQuery is what differs.

#define ALIGN_TRY(expr)                                                                               \
  do {                                                                                                \
    hipError_t e_ = (expr);                                                                           \
    if (e_ != hipSuccess) return capi_fail(WFST_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

template <class B>
hipError_t align_grow(B &buf, size_t need) { return buf.n >= need ? hipSuccess : buf.alloc(need); }
template <class T>
void align_zero(T *p, size_t n) { if (p) std::fill(p, p + n, (T)0); }

// A round: from `first` on, the entries that run (run[i] != 0) and whose need[] fits `budget` together, in order -- at least one,
// however large, and none that would take a round that has a member over the budget; next: where the following round starts
// (need.size(): there is none).  members is empty only when nothing from `first` on runs.  No HIP in it (tests/hip_double/rounds_main.cc).
struct RoundCut {
  std::vector<size_t> members;
  int64_t cells;
  size_t next;
};
inline RoundCut cut_round(const std::vector<int64_t> &need, const std::vector<char> &run, size_t first, int64_t budget) {
  RoundCut r{{}, 0, first};
  for (; r.next < need.size(); ++r.next) {
    if (!run[r.next]) continue;
    if (!r.members.empty() && r.cells + need[r.next] > budget) break;
    r.members.push_back(r.next);
    r.cells += need[r.next];
  }
  return r;
}

// a round as a query's hooks see it: slot j of cnt is one channel, pair j * n_seqs + q one of its sequences
struct WordRound {
  const AlignView *V;
  size_t cnt, pairs;
  int64_t cells;               // of the round's tables
  int32_t n_seqs, cap_words;
  const int32_t *seq_len;      // the caller's [n][n_seqs]
  std::vector<int32_t> caller_pos;   // slot j's position in the caller's channel list
  AlignDev A;                  // the index fields: idx, idx_ints, ns_cap, na_cap, fr_cap
  // the staged inputs on the device: the pairs' table offsets (in cells, < 0: not run), the round's channels, the lengths, the words
  const int64_t *cell_off;
  const int32_t *chan, *len, *words;
  // launch() may ask for a second download behind the packed results'
  void *more_dst;
  const void *more_src;
  size_t more_bytes;
  // the packed results, landed: pair_ints per pair (its error word: [4]), then chan_ints per slot
  const int32_t *landed;
  // the AlignDev align_kernel takes: the index over the decoder's AlignState (cells, path, out) and the staged inputs
  AlignDev align_dev() const {
    AlignDev a = A;
    a.n_seqs = n_seqs; a.cap_words = cap_words;
    a.sil_bits = V->sil_bits; a.n_tid = V->sil_ntid;
    a.cell_off = cell_off; a.seq_len = len; a.seq_words = words;
    a.cells = V->as->cells.p; a.path = V->as->path.p; a.out = V->as->out.p;
    return a;
  }
};

struct WordQuery {
  const char *name;                // in messages: "align"
  const char *item, *abbr;         // what a sequence is called: "sequence" / "seq" (n_seqs, seq_len)
  const char *caps = "cap_words";  // the capacities that must be positive, and the least of those beyond cap_words
  int32_t cap_extra = 1;
  int32_t min_len = 0;             // the fewest words of a sequence that is asked for (a phrase has one at least)
  const char *arg_error = nullptr; // the entry point's check of arguments of its own, reported behind "NULL decoder / channel list"
  int64_t default_cells, round_cells;   // max_cells = 0; the cells of one round's tables
  int32_t cell_words = 1;          // 32-bit words of a cell (AlignState::cells counts words)
  int32_t path_extra = 0;          // ints of a pair's path scratch beyond ns_cap
  size_t pair_ints, chan_ints = 0; // of the packed results, per pair and per slot
  int64_t arc_limit = 0;           // > 0: a lattice of this many arcs or more is refused as a table beyond max_cells is
  const char *invariant;           // what a pair's unknown error word means
  const char *table_cols = "(words + 1)";   // what a table's second dimension is called in the "beyond max_cells" message
  virtual ~WordQuery() = default;
  // the caller's result arrays zeroed (the arguments are valid)
  virtual void clear() = 0;
  // further workspace grown, launch_align_index and the query's kernels enqueued on R.V->stream
  virtual int launch(WordRound &R) = 0;
  // slot j's results copied to position o of the caller's arrays; returns the channel's code
  virtual int unpack(const WordRound &R, size_t j, size_t o, int32_t channel) = 0;
  // what the "no device memory" message says of the cells beyond their count
  virtual std::string workspace_note(const WordRound &) const { return ""; }
};
// Everything but the hooks: the argument checks, align_begin, the word and length checks, status[] and clear(), the channels with a
// lattice, align_emit, the channels' own failures and max_cells, then round by round the index capacities, the workspace, the staged
// inputs, launch(), the download(s), the pairs' error words and unpack().
int word_query_run(WordQuery &q, wfst_decoder *d, const int32_t *channels, int32_t n, int32_t use_final_probs, int32_t n_seqs,
                   int32_t cap_words, const int32_t *seq_words, const int32_t *seq_len, int64_t max_cells, int32_t *status);
int word_query_no_memory(const WordQuery &q, const WordRound &R);   // WFST_E_CAPACITY, the workspace message

// align_kernel's results of a pair, as align_words and word_confidence hand them out
struct AlignOutputs {
  int32_t *found, *n_arcs, *begin_frame, *end_frame;
  float *tot_score, *lm_score;
  void clear(size_t np, size_t cap) const {
    align_zero(found, np); align_zero(n_arcs, np); align_zero(begin_frame, np * cap); align_zero(end_frame, np * cap); align_zero(tot_score, np); align_zero(lm_score, np);
  }
  void take(const int32_t *r, size_t p, size_t len, size_t cap) const {
    if (found) found[p] = 1;
    if (n_arcs) n_arcs[p] = r[1];
    if (tot_score) memcpy(&tot_score[p], &r[2], 4);
    if (lm_score) memcpy(&lm_score[p], &r[3], 4);
    if (begin_frame) memcpy(begin_frame + p * cap, r + kAlignHead, len * 4);
    if (end_frame) memcpy(end_frame + p * cap, r + kAlignHead + cap, len * 4);
  }
};

}  // namespace wfst
#endif
