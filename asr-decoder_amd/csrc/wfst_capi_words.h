// The seam between wfst_capi.cc and wfst_capi_words.cc (wfst_decoder_words_enqueue / _ready / _fetch / wfst_decoder_get_words):
// the entry points that launch words_kernel are a translation unit of their own, so that wfst_capi.cc links against exactly the
// launches it always did (tests build it alone against a double of the HIP runtime and of those launches).  Host only.
#ifndef WFST_CAPI_WORDS_H_
#define WFST_CAPI_WORDS_H_

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/wfst_decoder.h"
#include "wfst_device.h"
#include "wfst_hip_own.h"

namespace wfst {

// a decoder's words request: the outstanding request's list, its device and page-locked blocks ([n_channels] list entries, then per
// entry kWordsHead ints + 3 cap_words) and the event behind its copies; chain: chain_cap ints per list entry for the hops of a walk
// that LDS does not hold (none until a path needs them)
struct WordsState {
  DevBuf<int32_t> chan, out, chain;
  PinBuf<int32_t> pin;
  Event ev;
  std::vector<int32_t> list;
  hipStream_t st = nullptr;   // the results stream the request went on
  int32_t n = 0, cap = 0, ufp = 0, chain_cap = 0;   // (n == 0: nothing outstanding)
};

static const char *const kWordsOutstanding = "a words request is outstanding (wfst_decoder_words_fetch takes it)";

// what the words entry points see of a decoder (sil_bits: the silence bitmap over transition-ids 1..sil_ntid, nullptr: none)
struct WordsView {
  int device;
  int32_t n_channels;
  const DecoderDev *D;
  WordsState *ws;
  const uint32_t *sil_bits;
  int32_t sil_ntid;
};
WordsView words_view(wfst_decoder *d);
// GetBestPath's checks of a channel list (range, duplicates, InitDecoding, the use_final_probs rule after FinalizeDecoding), then the
// results stream behind the listed channels' own enqueued work
int words_begin(wfst_decoder *d, const int32_t *channels, int32_t n, int32_t use_final_probs, hipStream_t *st);
int capi_fail(int code, const std::string &msg);          // sets wfst_last_error, returns code
int capi_fail_ctl(int channel, int error_word);           // a channel's device error word, as every call reports it
int capi_poll_event(wfst_decoder *d, hipEvent_t ev);      // 1 passed, 0 not yet, < 0 error

}  // namespace wfst
#endif
