// wfst_bias_compile, wfst_bias_lists_create / _info / _free and wfst_decoder_biased_words: per-channel phrase boosting -- the best
// path of a channel's raw lattice under new scales, a word penalty and a list of boosted phrases, for a channel list (live and
// finalized channels mixed) and up to 16 settings shared by the listed channels, one launch per stage (lattice_emit_kernel for the
// live channels, align_index_kernel, bias_kernel: wfst_bias.hip).  A translation unit of its own -- see wfst_capi_bias.h.
#include "wfst_capi_bias.h"

#include <cmath>
#include <map>
#include <memory>
#include <set>

using namespace wfst;

namespace wfst {

int bias_trie(const std::string &who, int32_t n_phrases, const int32_t *phrase_len, const int32_t *phrase_words, const double *phrase_bonus,
              int32_t max_nodes, const char *holder, BiasAutomaton *out, int32_t *n_nodes) {
  if (n_nodes) *n_nodes = 0;
  if (n_phrases < 0 || (n_phrases > 0 && (!phrase_len || !phrase_words || !phrase_bonus))) return capi_fail(WFST_E_ARG, who + "n_phrases < 0 or NULL arrays");
  // ---- the phrases, and their trie in the order they came ------------------------------------------------------------------------
  struct Tmp { int32_t parent, word, depth, phrase; };
  std::vector<Tmp> tmp(1, Tmp{-1, 0, 0, -1});
  std::map<std::pair<int32_t, int32_t>, int32_t> kid;   // (node, word) -> child, in tmp's numbering
  std::vector<double> own_tmp(1, 0.0);
  size_t at = 0;
  for (int32_t p = 0; p < n_phrases; ++p) {
    const std::string ph = who + "phrase " + std::to_string(p) + ": ";
    const int32_t len = phrase_len[p];
    if (len < 1 || len > kBiasMaxWords) return capi_fail(WFST_E_ARG, ph + "a length outside 1..16");
    if (!std::isfinite(phrase_bonus[p]) || phrase_bonus[p] < 0.0) return capi_fail(WFST_E_ARG, ph + "the bonus must be finite and >= 0");
    int32_t x = 0;
    for (int32_t k = 0; k < len; ++k) {
      const int32_t w = phrase_words[at + (size_t)k];
      if (w <= 0) return capi_fail(WFST_E_ARG, ph + "a word id <= 0");
      auto it = kid.find({x, w});
      if (it == kid.end()) {
        it = kid.emplace(std::make_pair(x, w), (int32_t)tmp.size()).first;
        tmp.push_back(Tmp{x, w, k + 1, -1});
        own_tmp.push_back(0.0);
      }
      x = it->second;
    }
    if (tmp[(size_t)x].phrase >= 0) return capi_fail(WFST_E_ARG, ph + "a duplicate of phrase " + std::to_string(tmp[(size_t)x].phrase));
    tmp[(size_t)x].phrase = p;
    own_tmp[(size_t)x] = phrase_bonus[p];
    at += (size_t)len;
  }
  const int32_t J = (int32_t)tmp.size();
  if (n_nodes) *n_nodes = J;
  if (J > max_nodes)
    return capi_fail(WFST_E_CAPACITY, who + "its phrases take " + std::to_string(J) + " nodes, a " + holder + " holds " + std::to_string(max_nodes));
  // ---- breadth first: by depth, then the parent's number, then the word ---------------------------------------------------------------
  std::vector<int32_t> num((size_t)J, 0), order(1, 0);
  for (int32_t depth = 1; depth <= kBiasMaxWords; ++depth) {
    std::vector<int32_t> level;
    for (int32_t x = 1; x < J; ++x)
      if (tmp[(size_t)x].depth == depth) level.push_back(x);
    std::sort(level.begin(), level.end(), [&](int32_t a, int32_t b) {
      const Tmp &A = tmp[(size_t)a], &B = tmp[(size_t)b];
      return std::make_pair(num[(size_t)A.parent], A.word) < std::make_pair(num[(size_t)B.parent], B.word);
    });
    for (int32_t x : level) { num[(size_t)x] = (int32_t)order.size(); order.push_back(x); }
  }
  BiasAutomaton &M = *out;
  M = BiasAutomaton();
  M.parent.resize((size_t)J); M.word.resize((size_t)J); M.fail.assign((size_t)J, 0); M.phrase.resize((size_t)J); M.beta.assign((size_t)J, 0.0);
  std::vector<double> own((size_t)J, 0.0);
  std::map<std::pair<int32_t, int32_t>, int32_t> child;
  for (int32_t j = 0; j < J; ++j) {
    const Tmp &T = tmp[(size_t)order[(size_t)j]];
    M.parent[(size_t)j] = j ? num[(size_t)T.parent] : -1;
    M.word[(size_t)j] = T.word;
    M.phrase[(size_t)j] = T.phrase;
    own[(size_t)j] = own_tmp[(size_t)order[(size_t)j]];
    if (j) child[{M.parent[(size_t)j], T.word}] = j;
  }
  // (breadth first by (depth, parent's number, word): a node's children are consecutive numbers, their words ascending)
  M.first_child.assign((size_t)J, 0); M.n_child.assign((size_t)J, 0);
  for (int32_t j = J - 1; j >= 1; --j) { M.first_child[(size_t)M.parent[(size_t)j]] = j; ++M.n_child[(size_t)M.parent[(size_t)j]]; }
  // ---- fail, delta, beta: a node's failure link is shallower than the node, so it is numbered, and finished, before it -------------------
  auto delta = [&](int32_t i, int32_t w) {
    for (;;) {
      const auto it = child.find({i, w});
      if (it != child.end()) return it->second;
      if (i == 0) return (int32_t)0;
      i = M.fail[(size_t)i];
    }
  };
  for (int32_t j = 1; j < J; ++j) {
    const int32_t p = M.parent[(size_t)j];
    M.fail[(size_t)j] = p == 0 ? 0 : delta(M.fail[(size_t)p], M.word[(size_t)j]);
    M.beta[(size_t)j] = own[(size_t)j] + M.beta[(size_t)M.fail[(size_t)j]];
    if (!std::isfinite(M.beta[(size_t)j])) return capi_fail(WFST_E_ARG, who + "the bonuses of nested phrases add up to infinity");
  }
  std::set<int32_t> ws(M.word.begin() + 1, M.word.end());
  M.words.assign(ws.begin(), ws.end());
  return WFST_OK;
}

int bias_compile(const std::string &who, int32_t n_phrases, const int32_t *phrase_len, const int32_t *phrase_words, const double *phrase_bonus,
                 BiasAutomaton *out, int32_t *n_nodes) {
  const int rc = bias_trie(who, n_phrases, phrase_len, phrase_words, phrase_bonus, kBiasMaxNodes, "list", out, n_nodes);
  if (rc != WFST_OK) return rc;
  BiasAutomaton &M = *out;
  const int32_t J = M.nodes();
  // ---- delta as a byte table, and per node the nodes it is reached from over its own word ------------------------------------------------
  auto delta = [&](int32_t i, int32_t w) {
    for (;;) {
      for (int32_t c = M.first_child[(size_t)i]; c < M.first_child[(size_t)i] + M.n_child[(size_t)i]; ++c)
        if (M.word[(size_t)c] == w) return c;
      if (i == 0) return (int32_t)0;
      i = M.fail[(size_t)i];
    }
  };
  const size_t W = M.words.size();
  M.table.assign((size_t)J * W, 0);
  for (int32_t i = 0; i < J; ++i)
    for (size_t k = 0; k < W; ++k) M.table[(size_t)i * W + k] = (uint8_t)delta(i, M.words[k]);
  M.pred_off.assign((size_t)J + 1, 0);
  for (int32_t j = 1; j < J; ++j) {
    const size_t k = (size_t)(std::lower_bound(M.words.begin(), M.words.end(), M.word[(size_t)j]) - M.words.begin());
    for (int32_t i = 0; i < J; ++i)
      if (M.table[(size_t)i * W + k] == j) M.pred.push_back(i);
    M.pred_off[(size_t)j + 1] = (int32_t)M.pred.size();
  }
  return WFST_OK;
}

int bias_check_settings(int32_t n_set, const double *settings) {
  if (n_set < 1 || n_set > kBiasMaxSettings) return capi_fail(WFST_E_ARG, "1 <= n_set <= 16 settings");
  if (!settings) return capi_fail(WFST_E_ARG, "NULL settings");
  for (int32_t q = 0; q < n_set; ++q) {
    const double gs = settings[4 * q], as = settings[4 * q + 1], wip = settings[4 * q + 2], bs = settings[4 * q + 3];
    if (!std::isfinite(gs) || !std::isfinite(as) || gs < 0.0 || as < 0.0)
      return capi_fail(WFST_E_ARG, "graph_scale / acoustic_scale must be finite and >= 0");
    if (!std::isfinite(wip)) return capi_fail(WFST_E_ARG, "word_penalty must be finite");
    if (!std::isfinite(bs) || bs < 0.0) return capi_fail(WFST_E_ARG, "boost_scale must be finite and >= 0");
  }
  return WFST_OK;
}

}  // namespace wfst

namespace {
template <class T>
int upload(DevBuf<T> &buf, const std::vector<T> &v) {
  ALIGN_TRY(buf.alloc(v.size()));
  if (!v.empty()) ALIGN_TRY(hipMemcpy(buf.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return WFST_OK;
}

struct BiasQuery : WordQuery {
  BiasOutputs O;
  BiasSet set;
  const wfst_bias_lists *lists;
  const int32_t *list_of;   // the caller's [n]
  std::vector<int32_t> h_list;   // a round's upload, alive until the driver has synchronised
  BiasQuery(size_t np, int32_t cap_words, int32_t cap_hits) {
    O.np = np; O.cap = (size_t)cap_words; O.hcap = (size_t)cap_hits;
    name = "bias"; item = "setting"; abbr = "set";
    default_cells = kBiasDefaultCells; round_cells = kBiasRoundCells;
    cell_words = 2;
    pair_ints = (size_t)bias_out_ints((int64_t)O.cap, (int64_t)O.hcap);
    invariant = "a traced path that does not reproduce its cell";
    table_cols = "nodes";
  }
  std::string workspace_note(const WordRound &) const override { return " of 8 bytes"; }
  void clear() override { O.clear(); }
  int launch(WordRound &R) override {
    const AlignView &V = *R.V;
    AlignState &S = *V.as;
    if (S.bias_list.n < R.cnt) {
      ALIGN_TRY(hipStreamSynchronize(V.stream));
      if (S.bias_list.alloc(R.cnt) != hipSuccess) {
        (void)hipGetLastError();
        return word_query_no_memory(*this, R);
      }
    }
    h_list.resize(R.cnt);
    for (size_t j = 0; j < R.cnt; ++j) h_list[j] = list_of ? list_of[(size_t)R.caller_pos[j]] : -1;
    ALIGN_TRY(hipMemcpyAsync(S.bias_list.p, h_list.data(), R.cnt * 4, hipMemcpyHostToDevice, V.stream));
    BiasDev Q = {};
    if (lists) Q.L = lists->view();
    Q.list_of = S.bias_list.p;
    Q.lat_toks = V.D->lat_toks;
    Q.lat_tok_cap = V.D->lat_tok_cap;
    Q.cell_off = R.cell_off;
    Q.cells = reinterpret_cast<double *>(S.cells.p);
    Q.path = S.path.p;
    Q.path_cap = R.A.ns_cap;
    Q.n_set = R.n_seqs;
    Q.cap_words = (int32_t)O.cap;
    Q.cap_hits = (int32_t)O.hcap;
    Q.sil_bits = V.sil_bits;
    Q.n_tid = V.sil_ntid;
    Q.out = S.out.p;
    launch_align_index(*V.D, R.A, R.chan, (int)R.cnt, V.stream);
    ALIGN_TRY(hipGetLastError());
    launch_bias(R.A, Q, set, R.chan, (int)R.cnt, V.stream);
    ALIGN_TRY(hipGetLastError());
    return WFST_OK;
  }
  int unpack(const WordRound &R, size_t j, size_t o, int32_t channel) override {
    const size_t ns = (size_t)R.n_seqs;
    int code = WFST_OK;
    for (size_t q = 0; q < ns; ++q) {
      const int32_t *r = R.landed + (j * ns + q) * pair_ints;
      if (r[0]) code = O.take(r, o * ns + q, channel, code);
    }
    return code;
  }
};
}  // namespace

extern "C" {

int wfst_bias_compile(int32_t n_phrases, const int32_t *phrase_len, const int32_t *phrase_words, const double *phrase_bonus, int32_t cap_nodes,
                      int32_t *n_nodes, int32_t *parent, int32_t *word, int32_t *fail, int32_t *phrase, double *beta) {
  if (cap_nodes < 0) return capi_fail(WFST_E_ARG, "cap_nodes < 0");
  BiasAutomaton M;
  const int rc = bias_compile("bias list: ", n_phrases, phrase_len, phrase_words, phrase_bonus, &M, n_nodes);
  if (rc != WFST_OK) return rc;
  const int32_t J = M.nodes();
  if (J > cap_nodes) return capi_fail(WFST_E_CAPACITY, "bias list: " + std::to_string(J) + " nodes, cap_nodes is " + std::to_string(cap_nodes));
  if (parent) std::copy(M.parent.begin(), M.parent.end(), parent);
  if (word) std::copy(M.word.begin(), M.word.end(), word);
  if (fail) std::copy(M.fail.begin(), M.fail.end(), fail);
  if (phrase) std::copy(M.phrase.begin(), M.phrase.end(), phrase);
  if (beta) std::copy(M.beta.begin(), M.beta.end(), beta);
  return WFST_OK;
}

int wfst_bias_lists_create(int32_t n_lists, const int32_t *n_phrases, const int32_t *phrase_len, const int32_t *phrase_words,
                           const double *phrase_bonus, int device, wfst_bias_lists **out) {
  if (!out) return capi_fail(WFST_E_ARG, "out is NULL");
  *out = nullptr;
  if (n_lists <= 0 || !n_phrases) return capi_fail(WFST_E_ARG, "empty set of bias lists or NULL arrays");
  // ---- validation and the kernel's tables, on the host: no device is touched before every list stands ----------------------------
  std::unique_ptr<wfst_bias_lists> bl(new wfst_bias_lists);
  bl->n_lists = n_lists;
  bl->hdr.assign((size_t)n_lists * kBiasHdr, 0);
  std::vector<int32_t> ints;
  std::vector<double> beta;
  std::vector<uint8_t> table;
  size_t p0 = 0, w0 = 0;
  for (int32_t l = 0; l < n_lists; ++l) {
    const int32_t P = n_phrases[l];
    if (P < 0) return capi_fail(WFST_E_ARG, "bias list " + std::to_string(l) + ": n_phrases < 0");
    if (P > 0 && (!phrase_len || !phrase_words || !phrase_bonus)) return capi_fail(WFST_E_ARG, "NULL phrase arrays");
    BiasAutomaton M;
    const int rc = bias_compile("bias list " + std::to_string(l) + " ", P, P ? phrase_len + p0 : nullptr, P ? phrase_words + w0 : nullptr,
                                P ? phrase_bonus + p0 : nullptr, &M, nullptr);
    if (rc != WFST_OK) return rc;
    for (int32_t p = 0; p < P; ++p) w0 += (size_t)phrase_len[p0 + (size_t)p];
    p0 += (size_t)P;
    const int32_t J = M.nodes();
    if (ints.size() + 4 * (size_t)J + 1 + M.words.size() + M.pred.size() > (size_t)INT32_MAX || table.size() + M.table.size() > (size_t)INT32_MAX)
      return capi_fail(WFST_E_CAPACITY, "bias lists: 2^31 entries in one set");
    int32_t *H = bl->hdr.data() + (size_t)l * kBiasHdr;
    H[0] = J; H[1] = (int32_t)M.words.size(); H[2] = (int32_t)ints.size(); H[3] = (int32_t)beta.size(); H[4] = (int32_t)table.size(); H[5] = P;
    ints.insert(ints.end(), M.word.begin(), M.word.end());
    ints.insert(ints.end(), M.fail.begin(), M.fail.end());
    ints.insert(ints.end(), M.phrase.begin(), M.phrase.end());
    ints.insert(ints.end(), M.pred_off.begin(), M.pred_off.end());
    ints.insert(ints.end(), M.words.begin(), M.words.end());
    ints.insert(ints.end(), M.pred.begin(), M.pred.end());
    beta.insert(beta.end(), M.beta.begin(), M.beta.end());
    table.insert(table.end(), M.table.begin(), M.table.end());
    bl->total_phrases += P;
    bl->total_nodes += J;
  }
  // ---- the device ---------------------------------------------------------------------------------------------------------------
  const int ndev = wfst_device_count();
  if (ndev <= 0) return capi_fail(WFST_E_DEVICE, "no HIP device available (this library has no CPU path)");
  if (device < 0 || device >= ndev) return capi_fail(WFST_E_ARG, "device index out of range");
  ALIGN_TRY(hipSetDevice(device));
  bl->device = device;
  int rc = upload(bl->d_hdr, bl->hdr);
  if (rc == WFST_OK) rc = upload(bl->d_ints, ints);
  if (rc == WFST_OK) rc = upload(bl->d_beta, beta);
  if (rc == WFST_OK) rc = upload(bl->d_table, table);
  if (rc != WFST_OK) return rc;
  *out = bl.release();
  return WFST_OK;
}

int wfst_bias_lists_info(const wfst_bias_lists *b, int32_t *n_lists, int64_t *total_phrases, int64_t *total_nodes, int32_t *n_phrases,
                         int32_t *n_nodes, int32_t *n_words, int64_t *device_bytes) {
  if (!b) return capi_fail(WFST_E_ARG, "NULL bias lists");
  if (n_lists) *n_lists = b->n_lists;
  if (total_phrases) *total_phrases = b->total_phrases;
  if (total_nodes) *total_nodes = b->total_nodes;
  for (int32_t l = 0; l < b->n_lists; ++l) {
    const int32_t *H = b->hdr.data() + (size_t)l * kBiasHdr;
    if (n_phrases) n_phrases[l] = H[5];
    if (n_nodes) n_nodes[l] = H[0];
    if (n_words) n_words[l] = H[1];
  }
  if (device_bytes) *device_bytes = b->device_bytes();
  return WFST_OK;
}

void wfst_bias_lists_free(wfst_bias_lists *b) {
  if (!b) return;
  (void)hipSetDevice(b->device);
  delete b;
}

int wfst_decoder_biased_words(wfst_decoder *d, const int32_t *channels, int32_t n, int32_t use_final_probs, const wfst_bias_lists *lists,
                              const int32_t *list_of, int32_t n_set, const double *settings, int32_t cap_words, int32_t cap_hits,
                              int64_t max_cells, int32_t *status, int32_t *found, int32_t *n_arcs, int32_t *n_hyp, int32_t *n_hits,
                              int32_t *hyp_words, int32_t *begin_frame, int32_t *end_frame, int32_t *hit_phrase, int32_t *hit_word,
                              double *biased_cost, double *bonus, float *tot_score, float *lm_score) {
  if (!d || !channels) return capi_fail(WFST_E_ARG, "NULL decoder / channel list");
  const int bad = bias_check_settings(n_set, settings);
  if (bad != WFST_OK) return bad;
  if (cap_words <= 0) return capi_fail(WFST_E_ARG, "cap_words <= 0");
  if (cap_hits < 0) return capi_fail(WFST_E_ARG, "cap_hits < 0");
  if (max_cells < 0) return capi_fail(WFST_E_ARG, "max_cells < 0");
  // the channel list, then what goes by it: the lists of the listed channels
  AlignView V;
  const int rc = align_begin(d, channels, n, &V);
  if (rc != WFST_OK) return rc;
  if (lists && lists->device != V.device) return capi_fail(WFST_E_ARG, "the bias lists live on another device than the decoder");
  const size_t N = (size_t)n, ns = (size_t)n_set;
  int32_t most = 1;
  std::vector<int32_t> len(N * ns, 0);
  for (size_t i = 0; i < N; ++i) {
    const int32_t l = list_of ? list_of[i] : -1;
    if (l < -1 || (l >= 0 && (!lists || l >= lists->n_lists))) return capi_fail(WFST_E_ARG, "list_of out of range (or a list without a set of lists)");
    const int32_t J = l < 0 ? 1 : lists->hdr[(size_t)l * kBiasHdr];
    most = std::max(most, J - 1);
    std::fill(len.begin() + (ptrdiff_t)(i * ns), len.begin() + (ptrdiff_t)((i + 1) * ns), J - 1);
  }
  BiasQuery q(N * ns, cap_words, cap_hits);
  q.set = BiasSet{};
  std::copy(settings, settings + 4 * ns, q.set.v);
  q.lists = lists; q.list_of = list_of;
  q.O.found = found; q.O.n_arcs = n_arcs; q.O.n_hyp = n_hyp; q.O.n_hits = n_hits; q.O.hyp_words = hyp_words; q.O.begin_frame = begin_frame;
  q.O.end_frame = end_frame; q.O.hit_phrase = hit_phrase; q.O.hit_word = hit_word; q.O.biased_cost = biased_cost; q.O.bonus = bonus;
  q.O.tot_score = tot_score; q.O.lm_score = lm_score;
  // per (channel, setting) one sequence as long as the channel's list has nodes beyond the root: a table of states x nodes cells
  const std::vector<int32_t> ones(N * ns * (size_t)most, 1);
  return word_query_run(q, d, channels, n, use_final_probs, n_set, most, ones.data(), len.data(), max_cells, status);
}

}  // extern "C"
