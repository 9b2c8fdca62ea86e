// wfst_decoder_words_enqueue / _ready / _fetch / wfst_decoder_get_words: an utterance's words, word times and scores in one launch
// (words_kernel, wfst_kernels.hip).  A translation unit of its own -- see wfst_capi_words.h.
#include "wfst_capi_words.h"

#include <algorithm>
#include <cstring>
#include <utility>

using namespace wfst;

#define W_TRY(expr)                                                                                   \
  do {                                                                                                \
    hipError_t e_ = (expr);                                                                           \
    if (e_ != hipSuccess) return capi_fail(WFST_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

// the words block of `count` list entries at cap_words: kWordsHead + 3 cap_words ints each
static size_t words_block_ints(int32_t count, int32_t cap_words) { return (size_t)count * ((size_t)kWordsHead + 3 * (size_t)cap_words); }

// launch + copy of the request (its list, capacity and use_final_probs in W) on W.st, the event behind them
static int words_launch(const WordsView &V) {
  WordsState &W = *V.ws;
  const hipStream_t st = W.st;
  const int32_t n = (int32_t)W.list.size();
  launch_words(*V.D, W.chan.p, n, W.ufp, V.sil_bits, V.sil_ntid, W.cap, W.chain_cap, W.chain.p, W.out.p, st);
  W_TRY(hipGetLastError());
  W_TRY(hipMemcpyAsync(W.pin.p + V.n_channels, W.out.p, words_block_ints(n, W.cap) * 4, hipMemcpyDeviceToHost, st));
  W_TRY(hipEventRecord(W.ev, st));
  return WFST_OK;
}

int wfst_decoder_words_enqueue(wfst_decoder *d, const int32_t *channels, int32_t n, int32_t use_final_probs, int32_t cap_words) {
  if (!d || !channels || cap_words <= 0) return capi_fail(WFST_E_ARG, "NULL decoder / channel list, or cap_words <= 0");
  const WordsView V = words_view(d);
  WordsState &W = *V.ws;
  if (W.n > 0) return capi_fail(WFST_E_STATE, kWordsOutstanding);
  if (n <= 0 || n > V.n_channels) return capi_fail(WFST_E_ARG, "bad channel count");
  hipStream_t st;
  int rc = words_begin(d, channels, n, use_final_probs, &st);
  if (rc != WFST_OK) return rc;
  if (!W.chan.p) {   // the first request: a decoder that never asks pays nothing
    DevBuf<int32_t> chan;
    Event ev;
    W_TRY(chan.alloc((size_t)V.n_channels));
    W_TRY(ev.create());
    W.chan = std::move(chan);
    W.ev = std::move(ev);
  }
  const size_t all = words_block_ints(V.n_channels, cap_words);
  if (W.out.n < words_block_ints(n, cap_words)) W_TRY(W.out.alloc(all));   // (room for every channel at this capacity, once; nothing of ours is outstanding)
  W_TRY(W.pin.reserve((size_t)V.n_channels + all));
  memcpy(W.pin.p, channels, (size_t)n * 4);   // (the last words request has been waited for: its copies are done)
  W_TRY(hipMemcpyAsync(W.chan.p, W.pin.p, (size_t)n * 4, hipMemcpyHostToDevice, st));
  W.list.assign(channels, channels + n);
  W.cap = cap_words;
  W.ufp = use_final_probs ? 1 : 0;
  W.st = st;
  rc = words_launch(V);
  if (rc != WFST_OK) return rc;
  W.n = n;
  return WFST_OK;
}

int wfst_decoder_words_ready(wfst_decoder *d) {
  if (!d) return capi_fail(WFST_E_ARG, "NULL decoder");
  const WordsView V = words_view(d);
  WordsState &W = *V.ws;
  if (W.n <= 0) return capi_fail(WFST_E_STATE, "no words request is outstanding");
  return capi_poll_event(d, W.ev);
}

int wfst_decoder_words_fetch(wfst_decoder *d, int32_t *words, int32_t *begin_frame, int32_t *end_frame, int32_t *n_words, int32_t *n_hops,
                             float *tot_score, float *lm_score) {
  if (!d) return capi_fail(WFST_E_ARG, "NULL decoder");
  const WordsView V = words_view(d);
  WordsState &W = *V.ws;
  if (W.n <= 0) return capi_fail(WFST_E_STATE, "no words request is outstanding");
  W_TRY(hipSetDevice(V.device));
  const int32_t cnt = W.n, cap = W.cap;
  W.n = 0;   // (taken, whatever it turns out to hold)
  W_TRY(hipEventSynchronize(W.ev));
  const int32_t *pin_out = W.pin.p + V.n_channels;
  const size_t per = (size_t)kWordsHead + 3 * (size_t)cap;
  // A path with more hops than the walk's LDS list and the scratch behind it hold: the scratch grows to the longest path (and
  // at least to what max_frames emitting hops take) and the list runs again -- the listed channels have not moved since.
  for (int round = 0; round < 2; ++round) {
    int32_t longest = 0;
    for (int i = 0; i < cnt; ++i)
      if (pin_out[(size_t)i * per + 4]) longest = std::max(longest, pin_out[(size_t)i * per]);
    if (!longest) break;
    if (round == 1) return capi_fail(WFST_E_DEVICE, "best path changed between two runs of one words request (were its channels advanced?)");
    const int64_t need = std::max<int64_t>(longest, (int64_t)V.D->max_frames + 2) - words_chain_lds();
    const int32_t grown = (int32_t)std::min<int64_t>((need + 1023) & ~1023ll, 1 << 24);
    W_TRY(hipStreamSynchronize(W.st));   // (nothing reads the old scratch any more)
    W_TRY(W.chain.alloc((size_t)V.n_channels * (size_t)grown));
    W.chain_cap = grown;
    const int rc = words_launch(V);
    if (rc != WFST_OK) return rc;
    W_TRY(hipEventSynchronize(W.ev));
  }
  // a device error of ANOTHER channel's utterance is that channel's, not this request's
  for (int i = 0; i < cnt; ++i)
    if (pin_out[(size_t)i * per + 5]) return capi_fail_ctl(W.list[(size_t)i], pin_out[(size_t)i * per + 5]);
  bool too_long = false;
  for (int i = 0; i < cnt; ++i) {
    const int32_t *o = pin_out + (size_t)i * per;
    const size_t k = (size_t)std::min(std::max(o[1], 0), cap) * 4;
    if (n_hops) n_hops[i] = o[0];
    if (n_words) n_words[i] = o[1];
    if (tot_score) memcpy(&tot_score[i], &o[2], 4);
    if (lm_score) memcpy(&lm_score[i], &o[3], 4);
    if (words) memcpy(words + (size_t)i * (size_t)cap, o + kWordsHead, k);
    if (begin_frame) memcpy(begin_frame + (size_t)i * (size_t)cap, o + kWordsHead + cap, k);
    if (end_frame) memcpy(end_frame + (size_t)i * (size_t)cap, o + kWordsHead + 2 * (size_t)cap, k);
    if (o[1] > cap) too_long = true;
  }
  if (too_long) return capi_fail(WFST_E_CAPACITY, "more words than cap_words; n_words holds the needed size");
  return WFST_OK;
}

int wfst_decoder_get_words(wfst_decoder *d, const int32_t *channels, int32_t n, int32_t use_final_probs, int32_t cap_words, int32_t *words,
                           int32_t *begin_frame, int32_t *end_frame, int32_t *n_words, int32_t *n_hops, float *tot_score, float *lm_score) {
  const int rc = wfst_decoder_words_enqueue(d, channels, n, use_final_probs, cap_words);
  if (rc != WFST_OK) return rc;
  return wfst_decoder_words_fetch(d, words, begin_frame, end_frame, n_words, n_hops, tot_score, lm_score);
}
