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
  std::vector<int32_t> first_child, n_child;         // per node: its children are the nodes first_child .. first_child + n_child
  std::vector<int32_t> words;                        // the distinct word ids, ascending
  std::vector<uint8_t> table;                        // [nodes][words]: delta(i, words[k])
  std::vector<int32_t> pred_off, pred;               // per node j != 0 the nodes i with delta(i, word[j]) = j, ascending
  int32_t nodes() const { return (int32_t)word.size(); }
};
// Validation and construction, host only: WFST_E_ARG (a phrase's length, a word id, a bonus, a duplicate; `who` names the list) or
// WFST_E_CAPACITY (more than max_nodes nodes; *n_nodes is what the list takes; `holder` is what the message calls it) through
// capi_fail.  bias_trie fills everything but table, pred_off and pred (wfst_capi_bias_sparse.cc needs no more); bias_compile is
// bias_trie under kBiasMaxNodes, then those.
int bias_trie(const std::string &who, int32_t n_phrases, const int32_t *phrase_len, const int32_t *phrase_words, const double *phrase_bonus,
              int32_t max_nodes, const char *holder, BiasAutomaton *out, int32_t *n_nodes);
int bias_compile(const std::string &who, int32_t n_phrases, const int32_t *phrase_len, const int32_t *phrase_words, const double *phrase_bonus,
                 BiasAutomaton *out, int32_t *n_nodes);

// the caller's result arrays of wfst_decoder_biased_words and wfst_decoder_biased_words_sparse ([pairs] or [pairs][cap] each, any of
// them NULL), and a pair's packed results (bias_kernel's out[p], wfst_device.h) handed out into them
struct BiasOutputs {
  size_t np = 0, cap = 0, hcap = 0;   // pairs of the whole call; the caller's rows of words and of hits
  int32_t *found = nullptr, *n_arcs = nullptr, *n_hyp = nullptr, *n_hits = nullptr, *hyp_words = nullptr, *begin_frame = nullptr,
          *end_frame = nullptr, *hit_phrase = nullptr, *hit_word = nullptr;
  double *biased_cost = nullptr, *bonus = nullptr;
  float *tot_score = nullptr, *lm_score = nullptr;
  void clear() const {
    align_zero(found, np); align_zero(n_arcs, np); align_zero(n_hyp, np); align_zero(n_hits, np); align_zero(hyp_words, np * cap);
    align_zero(begin_frame, np * cap); align_zero(end_frame, np * cap); align_zero(hit_phrase, np * hcap); align_zero(hit_word, np * hcap);
    align_zero(biased_cost, np); align_zero(bonus, np); align_zero(tot_score, np); align_zero(lm_score, np);
  }
  // pair p's results r (found); `code` is the channel's code so far and the return value the code after this pair
  int take(const int32_t *r, size_t p, int32_t channel, int code) const {
    const bool want_hits = hit_phrase || hit_word;
    const size_t nh = std::min((size_t)r[5], cap), nk = std::min((size_t)r[6], hcap);
    if (found) found[p] = 1;
    if (n_arcs) n_arcs[p] = r[1];
    if (tot_score) memcpy(&tot_score[p], &r[2], 4);
    if (lm_score) memcpy(&lm_score[p], &r[3], 4);
    if (n_hyp) n_hyp[p] = r[5];
    if (n_hits) n_hits[p] = r[6];
    if (biased_cost) memcpy(&biased_cost[p], &r[8], 8);
    if (bonus) memcpy(&bonus[p], &r[10], 8);
    if (hyp_words) memcpy(hyp_words + p * cap, r + kBiasHead, nh * 4);
    if (begin_frame) memcpy(begin_frame + p * cap, r + kBiasHead + cap, nh * 4);
    if (end_frame) memcpy(end_frame + p * cap, r + kBiasHead + 2 * cap, nh * 4);
    if (hit_phrase) memcpy(hit_phrase + p * hcap, r + kBiasHead + 3 * cap, nk * 4);
    if (hit_word) memcpy(hit_word + p * hcap, r + kBiasHead + 3 * cap + hcap, nk * 4);
    // the path has more words or hits than the caller made room for: everything else of the answer stands, the counts are the
    // room it takes
    if (((size_t)r[5] > cap || (want_hits && (size_t)r[6] > hcap)) && code == WFST_OK)
      code = capi_fail(WFST_E_CAPACITY, "channel " + std::to_string(channel) + ": bias: a path of " + std::to_string(r[5]) + " words and " +
                                            std::to_string(r[6]) + " hits, cap_words is " + std::to_string(cap) + " and cap_hits " +
                                            std::to_string(hcap));
    return code;
  }
};
// the checks of the settings both calls make: WFST_E_ARG through capi_fail
int bias_check_settings(int32_t n_set, const double *settings);

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
