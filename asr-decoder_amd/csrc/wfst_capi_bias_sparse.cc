// wfst_bias_book_compile, wfst_bias_books_create / _info / _free and wfst_decoder_biased_words_sparse: phrase boosting for lists of
// up to 65 536 nodes -- wfst_decoder_biased_words' answers from the cells a path can reach.  A translation unit of its own -- see
// wfst_capi_bias_sparse.h for the driver's stages and the growth rule of the reach regions.
#include "wfst_capi_bias_sparse.h"

#include <memory>

using namespace wfst;

namespace {
template <class T>
int upload(DevBuf<T> &buf, const std::vector<T> &v) {
  ALIGN_TRY(buf.alloc(v.size()));
  if (!v.empty()) ALIGN_TRY(hipMemcpy(buf.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return WFST_OK;
}
}  // namespace

extern "C" {

int wfst_bias_book_compile(int32_t n_phrases, const int32_t *phrase_len, const int32_t *phrase_words, const double *phrase_bonus, int32_t cap_nodes,
                           int32_t *n_nodes, int32_t *parent, int32_t *word, int32_t *fail, int32_t *phrase, double *beta) {
  if (cap_nodes < 0) return capi_fail(WFST_E_ARG, "cap_nodes < 0");
  BiasAutomaton M;
  const int rc = bias_trie("bias book: ", n_phrases, phrase_len, phrase_words, phrase_bonus, kBiasBookMaxNodes, "book", &M, n_nodes);
  if (rc != WFST_OK) return rc;
  const int32_t J = M.nodes();
  if (J > cap_nodes) return capi_fail(WFST_E_CAPACITY, "bias book: " + std::to_string(J) + " nodes, cap_nodes is " + std::to_string(cap_nodes));
  if (parent) std::copy(M.parent.begin(), M.parent.end(), parent);
  if (word) std::copy(M.word.begin(), M.word.end(), word);
  if (fail) std::copy(M.fail.begin(), M.fail.end(), fail);
  if (phrase) std::copy(M.phrase.begin(), M.phrase.end(), phrase);
  if (beta) std::copy(M.beta.begin(), M.beta.end(), beta);
  return WFST_OK;
}

int wfst_bias_books_create(int32_t n_books, const int32_t *n_phrases, const int32_t *phrase_len, const int32_t *phrase_words,
                           const double *phrase_bonus, int device, wfst_bias_books **out) {
  if (!out) return capi_fail(WFST_E_ARG, "out is NULL");
  *out = nullptr;
  if (n_books <= 0 || !n_phrases) return capi_fail(WFST_E_ARG, "empty set of bias books or NULL arrays");
  // ---- validation and the kernels' arrays, on the host: no device is touched before every book stands ----------------------------
  std::unique_ptr<wfst_bias_books> bk(new wfst_bias_books);
  bk->n_books = n_books;
  bk->hdr.assign((size_t)n_books * kBookHdr, 0);
  std::vector<int32_t> ints;
  std::vector<double> beta;
  size_t p0 = 0, w0 = 0;
  for (int32_t l = 0; l < n_books; ++l) {
    const int32_t P = n_phrases[l];
    if (P < 0) return capi_fail(WFST_E_ARG, "bias book " + std::to_string(l) + ": n_phrases < 0");
    if (P > 0 && (!phrase_len || !phrase_words || !phrase_bonus)) return capi_fail(WFST_E_ARG, "NULL phrase arrays");
    BiasAutomaton M;
    const int rc = bias_trie("bias book " + std::to_string(l) + " ", P, P ? phrase_len + p0 : nullptr, P ? phrase_words + w0 : nullptr,
                             P ? phrase_bonus + p0 : nullptr, kBiasBookMaxNodes, "book", &M, nullptr);
    if (rc != WFST_OK) return rc;
    for (int32_t p = 0; p < P; ++p) w0 += (size_t)phrase_len[p0 + (size_t)p];
    p0 += (size_t)P;
    const int32_t J = M.nodes();
    if (ints.size() + 5 * (size_t)J + M.words.size() > (size_t)INT32_MAX) return capi_fail(WFST_E_CAPACITY, "bias books: 2^31 entries in one set");
    int32_t *H = bk->hdr.data() + (size_t)l * kBookHdr;
    H[0] = J; H[1] = (int32_t)M.words.size(); H[2] = (int32_t)ints.size(); H[3] = (int32_t)beta.size(); H[4] = P;
    ints.insert(ints.end(), M.word.begin(), M.word.end());
    ints.insert(ints.end(), M.fail.begin(), M.fail.end());
    ints.insert(ints.end(), M.phrase.begin(), M.phrase.end());
    ints.insert(ints.end(), M.first_child.begin(), M.first_child.end());
    ints.insert(ints.end(), M.n_child.begin(), M.n_child.end());
    ints.insert(ints.end(), M.words.begin(), M.words.end());
    beta.insert(beta.end(), M.beta.begin(), M.beta.end());
    bk->total_phrases += P;
    bk->total_nodes += J;
  }
  // ---- the device ---------------------------------------------------------------------------------------------------------------
  const int ndev = wfst_device_count();
  if (ndev <= 0) return capi_fail(WFST_E_DEVICE, "no HIP device available (this library has no CPU path)");
  if (device < 0 || device >= ndev) return capi_fail(WFST_E_ARG, "device index out of range");
  ALIGN_TRY(hipSetDevice(device));
  bk->device = device;
  int rc = upload(bk->d_hdr, bk->hdr);
  if (rc == WFST_OK) rc = upload(bk->d_ints, ints);
  if (rc == WFST_OK) rc = upload(bk->d_beta, beta);
  if (rc != WFST_OK) return rc;
  *out = bk.release();
  return WFST_OK;
}

int wfst_bias_books_info(const wfst_bias_books *b, int32_t *n_books, int64_t *total_phrases, int64_t *total_nodes, int32_t *n_phrases,
                         int32_t *n_nodes, int32_t *n_words, int64_t *device_bytes) {
  if (!b) return capi_fail(WFST_E_ARG, "NULL bias books");
  if (n_books) *n_books = b->n_books;
  if (total_phrases) *total_phrases = b->total_phrases;
  if (total_nodes) *total_nodes = b->total_nodes;
  for (int32_t l = 0; l < b->n_books; ++l) {
    const int32_t *H = b->hdr.data() + (size_t)l * kBookHdr;
    if (n_phrases) n_phrases[l] = H[4];
    if (n_nodes) n_nodes[l] = H[0];
    if (n_words) n_words[l] = H[1];
  }
  if (device_bytes) *device_bytes = b->device_bytes();
  return WFST_OK;
}

void wfst_bias_books_free(wfst_bias_books *b) {
  if (!b) return;
  (void)hipSetDevice(b->device);
  delete b;
}

int wfst_decoder_biased_words_sparse(wfst_decoder *d, const int32_t *channels, int32_t n, int32_t use_final_probs, const wfst_bias_books *books,
                                     const int32_t *book_of, int32_t n_set, const double *settings, int32_t cap_words, int32_t cap_hits,
                                     int64_t max_cells, int64_t round_cells, int32_t *status, int64_t *n_cells, int32_t *found, int32_t *n_arcs,
                                     int32_t *n_hyp, int32_t *n_hits, int32_t *hyp_words, int32_t *begin_frame, int32_t *end_frame,
                                     int32_t *hit_phrase, int32_t *hit_word, double *biased_cost, double *bonus, float *tot_score,
                                     float *lm_score) {
  if (!d || !channels) return capi_fail(WFST_E_ARG, "NULL decoder / channel list");
  const int bad = bias_check_settings(n_set, settings);
  if (bad != WFST_OK) return bad;
  if (cap_words <= 0) return capi_fail(WFST_E_ARG, "cap_words <= 0");
  if (cap_hits < 0) return capi_fail(WFST_E_ARG, "cap_hits < 0");
  if (max_cells < 0) return capi_fail(WFST_E_ARG, "max_cells < 0");
  if (max_cells > kBookMaxCells) return capi_fail(WFST_E_ARG, "max_cells above 2^30");
  if (round_cells < 0) return capi_fail(WFST_E_ARG, "round_cells < 0");
  AlignView V;
  int rc = align_begin(d, channels, n, &V);
  if (rc != WFST_OK) return rc;
  if (books && books->device != V.device) return capi_fail(WFST_E_ARG, "the bias books live on another device than the decoder");
  const size_t N = (size_t)n, ns = (size_t)n_set;
  for (size_t i = 0; i < N; ++i) {
    const int32_t l = book_of ? book_of[i] : -1;
    if (l < -1 || (l >= 0 && (!books || l >= books->n_books))) return capi_fail(WFST_E_ARG, "book_of out of range (or a book without a set of books)");
  }
  BiasOutputs O;
  O.np = N * ns; O.cap = (size_t)cap_words; O.hcap = (size_t)cap_hits;
  O.found = found; O.n_arcs = n_arcs; O.n_hyp = n_hyp; O.n_hits = n_hits; O.hyp_words = hyp_words; O.begin_frame = begin_frame;
  O.end_frame = end_frame; O.hit_phrase = hit_phrase; O.hit_word = hit_word; O.biased_cost = biased_cost; O.bonus = bonus;
  O.tot_score = tot_score; O.lm_score = lm_score;
  if (status) std::fill(status, status + n, (int32_t)WFST_OK);
  align_zero(n_cells, N);
  O.clear();
  // the channels with a lattice to look at, by their position in the caller's list; those without a device error of their own
  // are the slots of the index and of the reach regions
  std::vector<int32_t> pos, list;
  for (int i = 0; i < n; ++i)
    if (align_channel_state(d, channels[i]) == 1 || use_final_probs) { pos.push_back(i); list.push_back(channels[i]); }
  if (pos.empty()) return WFST_OK;
  std::vector<int32_t> sizes;
  rc = align_emit(d, list, use_final_probs, &sizes);
  if (rc != WFST_OK) return rc;
  hipStream_t st = V.stream;
  AlignState &S = *V.as;
  const int64_t limit = max_cells > 0 ? max_cells : kBookDefaultCells;
  const int64_t edge_limit = std::min<int64_t>(16 * limit, kBookMaxCells);
  std::vector<size_t> slot_i;   // slot -> index into pos / list / sizes
  for (size_t i = 0; i < pos.size(); ++i) {
    if (sizes[4 * i + 3]) {   // a device error of THIS channel's utterance
      const int code = capi_fail_ctl(list[i], sizes[4 * i + 3]);
      if (status) status[(size_t)pos[i]] = code;
      continue;
    }
    slot_i.push_back(i);
  }
  const size_t cnt = slot_i.size();
  if (!cnt) return WFST_OK;
  // ---- the index of every slot, one launch -----------------------------------------------------------------------------------------
  AlignDev A = {};
  A.ns_cap = 1; A.na_cap = 1; A.fr_cap = 2;
  std::vector<int32_t> h_chan(cnt), h_book(cnt);
  for (size_t j = 0; j < cnt; ++j) {
    const size_t i = slot_i[j];
    A.ns_cap = std::max(A.ns_cap, sizes[4 * i]);
    A.na_cap = std::max(A.na_cap, sizes[4 * i + 1]);
    A.fr_cap = std::max(A.fr_cap, sizes[4 * i + 2] + 2);
    h_chan[j] = list[i];
    h_book[j] = book_of ? book_of[(size_t)pos[i]] : -1;
  }
  A.idx_ints = align_idx_ints(A.ns_cap, A.na_cap, A.fr_cap);
  auto no_memory = [&](const std::string &what) {
    (void)hipGetLastError();
    return capi_fail(WFST_E_CAPACITY, "bias: no device memory for " + what + " of " + std::to_string(cnt) +
                                          " lattice(s): lower max_cells or ask for fewer channels at a time");
  };
  ALIGN_TRY(hipStreamSynchronize(st));
  if (align_grow(S.idx, (size_t)A.idx_ints * cnt) != hipSuccess || align_grow(S.bias_list, cnt) != hipSuccess ||
      align_grow(S.reach_head, cnt * kReachHead) != hipSuccess || align_grow(S.reach_reg, 4 * cnt) != hipSuccess)
    return no_memory("the index");
  // staged inputs of the call: the slots' channels, then per round the pairs' cell offsets (64-bit, behind an even count) and slots
  const size_t chan_ints = (cnt + 1) & ~(size_t)1, in_ints = chan_ints + 2 * cnt * ns + cnt;
  if (align_grow(S.in, in_ints) != hipSuccess) return no_memory("the staged inputs");
  ALIGN_TRY(hipMemcpy(S.in.p, h_chan.data(), cnt * 4, hipMemcpyHostToDevice));
  ALIGN_TRY(hipMemcpy(S.bias_list.p, h_book.data(), cnt * 4, hipMemcpyHostToDevice));
  A.idx = S.idx.p;
  const int32_t *d_chan = S.in.p;
  launch_align_index(*V.D, A, d_chan, (int)cnt, st);
  ALIGN_TRY(hipGetLastError());
  // ---- the reach stage: the sets and edges of every slot, its regions grown until they hold them ---------------------------------------
  BiasReachDev Q = {};
  if (books) Q.B = books->view();
  Q.book_of = S.bias_list.p;
  std::vector<int64_t> ccap(cnt), ecap(cnt), reg(4 * cnt, 0);
  std::vector<char> failed(cnt, 0);   // 1: the cells are over max_cells, 2: the edges over their bound
  for (size_t j = 0; j < cnt; ++j) {
    const size_t i = slot_i[j];
    ccap[j] = std::min(limit, std::max<int64_t>(kBookFirstCells, 4 * (int64_t)std::max(sizes[4 * i], 0)));
    ecap[j] = std::min(edge_limit, std::max<int64_t>(kBookFirstEdges, 8 * (int64_t)std::max(sizes[4 * i + 1], 0)));
  }
  std::vector<int32_t> head(cnt * kReachHead, 0);
  for (;;) {
    int64_t at = 0;
    for (size_t j = 0; j < cnt; ++j) {
      reg[4 * j] = at; reg[4 * j + 1] = failed[j] ? 0 : ccap[j]; reg[4 * j + 2] = failed[j] ? 0 : ecap[j];
      at += bias_reach_ints(A.ns_cap, A.na_cap, reg[4 * j + 1], reg[4 * j + 2]);
    }
    ALIGN_TRY(hipStreamSynchronize(st));
    if (align_grow(S.reach, (size_t)at) != hipSuccess) return no_memory("the reachable sets (" + std::to_string(at) + " ints)");
    ALIGN_TRY(hipMemcpy(S.reach_reg.p, reg.data(), reg.size() * 8, hipMemcpyHostToDevice));
    Q.ints = S.reach.p; Q.reg = S.reach_reg.p; Q.head = S.reach_head.p;
    launch_bias_reach(A, Q, (int)cnt, st);
    ALIGN_TRY(hipGetLastError());
    ALIGN_TRY(hipMemcpyAsync(head.data(), S.reach_head.p, head.size() * 4, hipMemcpyDeviceToHost, st));
    ALIGN_TRY(hipStreamSynchronize(st));
    bool again = false;
    for (size_t j = 0; j < cnt; ++j) {
      if (failed[j]) continue;
      const int32_t e = head[j * kReachHead];
      int64_t &capacity = e == kReachOverCells ? ccap[j] : ecap[j];
      const int64_t most = e == kReachOverCells ? limit : edge_limit;
      if (e != kReachOverCells && e != kReachOverEdges) continue;
      if (capacity >= most) failed[j] = e == kReachOverCells ? 1 : 2;
      else { capacity = std::min(most, 4 * capacity); again = true; }
    }
    if (!again) break;
  }
  // ---- per slot: its failure, or the cells its settings take ----------------------------------------------------------------------------
  std::vector<int64_t> need(cnt, 0);
  std::vector<char> run(cnt, 0);
  for (size_t j = 0; j < cnt; ++j) {
    const size_t i = slot_i[j], o = (size_t)pos[i];
    const int32_t *h = &head[j * kReachHead];
    if (failed[j]) {
      const bool cells = failed[j] == 1;
      const int code = capi_fail(WFST_E_CAPACITY, "channel " + std::to_string(list[i]) + ": bias: the reachable " + (cells ? "cells" : "edges") + " of " +
                                                      std::to_string(sizes[4 * i]) + " lattice states are beyond " +
                                                      (cells ? "max_cells (" + std::to_string(limit) + ")" : "16 x max_cells"));
      if (status) status[o] = code;
      if (n_cells) n_cells[o] = -1;
      continue;
    }
    if (n_cells && h[0] == 0) n_cells[o] = h[1];
    need[j] = (int64_t)ns * (h[0] == 0 ? h[1] : 0);
    run[j] = 1;   // (a slot whose index or reach pass reports an error runs: the sweep hands the error word on)
  }
  // ---- the sweep, in rounds of round_cells cells ------------------------------------------------------------------------------------------
  const int64_t budget = round_cells > 0 ? round_cells : kBiasRoundCells;
  const size_t pair_ints = (size_t)bias_out_ints((int64_t)O.cap, (int64_t)O.hcap);
  std::vector<int64_t> h_off;
  std::vector<int32_t> h_slot;
  for (size_t first = 0; first < cnt;) {
    const RoundCut cut = cut_round(need, run, first, budget);
    first = cut.next;
    if (cut.members.empty()) break;
    const std::vector<size_t> &rnd = cut.members;
    const size_t rc_cnt = rnd.size(), pairs = rc_cnt * ns, out_ints = pairs * pair_ints;
    const size_t path_need = pairs * 2 * (size_t)A.ns_cap, cell_words = 2 * (size_t)std::max<int64_t>(cut.cells, 1);
    ALIGN_TRY(hipStreamSynchronize(st));
    if (align_grow(S.path, path_need) != hipSuccess || align_grow(S.out, out_ints) != hipSuccess || align_grow(S.cells, cell_words) != hipSuccess)
      return no_memory("the cells of a round (" + std::to_string(cut.cells) + " of 8 bytes)");
    ALIGN_TRY(S.pin.reserve(out_ints));
    h_off.assign(pairs, 0);
    h_slot.assign(rc_cnt, 0);
    int64_t at = 0;
    for (size_t k = 0; k < rc_cnt; ++k) {
      h_slot[k] = (int32_t)rnd[k];
      for (size_t s = 0; s < ns; ++s) { h_off[k * ns + s] = at; at += need[rnd[k]] / (int64_t)ns; }
    }
    int64_t *d_off = reinterpret_cast<int64_t *>(S.in.p + chan_ints);
    int32_t *d_slot = S.in.p + chan_ints + 2 * cnt * ns;
    ALIGN_TRY(hipMemcpy(d_off, h_off.data(), pairs * 8, hipMemcpyHostToDevice));
    ALIGN_TRY(hipMemcpy(d_slot, h_slot.data(), rc_cnt * 4, hipMemcpyHostToDevice));
    BiasSparseDev P = {};
    P.R = Q;
    P.slot_of = d_slot;
    P.lat_toks = V.D->lat_toks;
    P.lat_tok_cap = V.D->lat_tok_cap;
    P.cell_off = d_off;
    P.cells = reinterpret_cast<double *>(S.cells.p);
    P.path = S.path.p;
    P.path_cap = A.ns_cap;
    P.n_set = n_set;
    P.cap_words = cap_words;
    P.cap_hits = cap_hits;
    P.sil_bits = V.sil_bits;
    P.n_tid = V.sil_ntid;
    P.out = S.out.p;
    BiasSet set = {};
    std::copy(settings, settings + 4 * ns, set.v);
    launch_bias_sparse(A, P, set, d_chan, (int)rc_cnt, st);
    ALIGN_TRY(hipGetLastError());
    ALIGN_TRY(hipMemcpyAsync(S.pin.p, S.out.p, out_ints * 4, hipMemcpyDeviceToHost, st));
    ALIGN_TRY(hipStreamSynchronize(st));
    for (size_t k = 0; k < rc_cnt; ++k) {
      const size_t i = slot_i[rnd[k]], o = (size_t)pos[i];
      const std::string who = "channel " + std::to_string(list[i]) + ": bias";
      int code = WFST_OK;
      for (size_t s = 0; s < ns && code == WFST_OK; ++s) {
        const int32_t e = S.pin.p[(k * ns + s) * pair_ints + 4];
        if (e == kAlnCycle) code = capi_fail(WFST_E_DEVICE, who + ": the lattice has an epsilon cycle");
        else if (e == kAlnTooLarge) code = capi_fail(WFST_E_CAPACITY, who + ": the lattice outgrew the round's index");
        else if (e) code = capi_fail(WFST_E_DEVICE, who + ": internal invariant violated on the device (a traced path that does not follow the automaton or reproduce its cell)");
      }
      for (size_t s = 0; s < ns && (code == WFST_OK || code == WFST_E_CAPACITY); ++s) {   // (a row too short: the other answers stand)
        const int32_t *r = S.pin.p + (k * ns + s) * pair_ints;
        if (r[0]) code = O.take(r, o * ns + s, list[i], code);
      }
      if (status) status[o] = code;
    }
  }
  return WFST_OK;
}

}  // extern "C"
