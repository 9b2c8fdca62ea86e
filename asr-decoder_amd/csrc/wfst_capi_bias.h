// The seam between the library and wfst_capi_bias.cc (wfst_bias_compile, wfst_bias_lists_*, wfst_decoder_biased_words): the entry
// points that launch bias_kernel (wfst_bias.hip) behind align_index_kernel are a translation unit of their own, as
// wfst_capi_rescale.cc is.  The call sees a decoder through wfst_capi_align.h's view and runs word_query_run with one sequence of
// (nodes - 1) words per (channel, setting): a table of states x nodes cells of 8 bytes each, so that max_cells, the rounds, the
// channels' own failures and the error words are the siblings'.  Its cells, path scratch and packed results are the decoder's
// AlignState's.  Host only.
#ifndef WFST_CAPI_BIAS_H_
#define WFST_CAPI_BIAS_H_

#include <string>
#include <vector>

#include "wfst_capi_align.h"

namespace wfst {

// max_cells = 0: 65 536 lattice states under the largest list
constexpr int64_t kBiasDefaultCells = 65536ll * kBiasMaxNodes;
// cells of one round (256 MiB at 8 bytes a cell); a channel whose own settings need more runs in a round of its own
constexpr int64_t kBiasRoundCells = 32ll << 20;
constexpr int32_t kBiasMaxWords = 16;   // = WFST_BIAS_MAX_WORDS

// one list's automaton, nodes in breadth-first order (root 0; by depth, parent's number, word id)
struct BiasAutomaton {
  std::vector<int32_t> parent, word, fail, phrase;   // per node; phrase: its index in the list, -1: none
  std::vector<double> beta;                          // per node
  std::vector<int32_t> words;                        // the distinct word ids, ascending
  std::vector<uint8_t> table;                        // [nodes][words]: delta(i, words[k])
  std::vector<int32_t> pred_off, pred;               // per node j != 0 the nodes i with delta(i, word[j]) = j, ascending
  int32_t nodes() const { return (int32_t)word.size(); }
};
// Validation and construction, host only: WFST_E_ARG (a phrase's length, a word id, a bonus, a duplicate; `who` names the list) or
// WFST_E_CAPACITY (more than kBiasMaxNodes nodes; *n_nodes is what the list takes) through capi_fail.
int bias_compile(const std::string &who, int32_t n_phrases, const int32_t *phrase_len, const int32_t *phrase_words, const double *phrase_bonus,
                 BiasAutomaton *out, int32_t *n_nodes);

}  // namespace wfst

// A set of bias lists resident on one device.  Every HIP resource is an owner (wfst_hip_own.h) and goes with the set;
// wfst_bias_lists_free makes the set's device current first.
struct wfst_bias_lists {
  int device = 0;
  int32_t n_lists = 0;
  int64_t total_phrases = 0, total_nodes = 0;
  std::vector<int32_t> hdr;   // [n_lists][kBiasHdr], as on the device
  wfst::DevBuf<int32_t> d_hdr, d_ints;
  wfst::DevBuf<double> d_beta;
  wfst::DevBuf<uint8_t> d_table;
  int64_t device_bytes() const { return (int64_t)(d_hdr.bytes() + d_ints.bytes() + d_beta.bytes() + d_table.bytes()); }
  wfst::BiasListsDev view() const { return wfst::BiasListsDev{d_hdr.p, d_ints.p, d_beta.p, d_table.p}; }
};
#endif
