// The seam between wfst_capi.cc and wfst_capi_nbwords.cc (wfst_decoder_get_nbest_words): the entry point that launches
// nbest_words_kernel is a translation unit of its own, as wfst_capi_words.cc is, so that wfst_capi.cc links against exactly the
// launches it always did.  Host only.
#ifndef WFST_CAPI_NBWORDS_H_
#define WFST_CAPI_NBWORDS_H_

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/wfst_decoder.h"
#include "wfst_device.h"
#include "wfst_hip_own.h"

namespace wfst {

// a decoder's n-best text block: packed on the device, its page-locked landing place (both grown on demand)
struct NbWordsState {
  DevBuf<int32_t> out;
  PinBuf<int32_t> pin;
};

// The whole-call checks of wfst_decoder_get_nbest_words (WFST_E_ARG / WFST_E_STATE, no device work), then the determinizer's
// workspace and a prefetch in flight harvested; *slots = lattices one round takes, *ws = the decoder's text block, *stream its stream.
int nbw_begin(wfst_decoder *d, const int32_t *channels, int32_t n, int32_t n_paths, const wfst_lm *old_lm, const wfst_lm *new_lm,
              int32_t cap_words, int32_t *slots, NbWordsState **ws, hipStream_t *stream);
// 0 never initialised, 1 decoding, 2 finalized
int nbw_channel_state(const wfst_decoder *d, int32_t channel);
// wfst_decoder_get_determinizer_slots: the workspace (allocated by the first use), its slots and what one of them takes
int nbw_det_slots(wfst_decoder *d, int32_t *slots, int64_t *bytes_per_slot);
// One round over `list` (at most *slots channels, none of them a finalized one asked without final-probs): the live channels'
// lattices emitted, all determinized (slot i = list[i]) unless the slots hold them, composed with the LMs if given, NShortestPath
// launched -- one launch per stage.  status[i]: WFST_OK or the channel's own error (its slot's paths are not to be used); *P: where
// the paths and their lattices sit on the device, for launch_nbest_words on the same stream.
int nbw_round(wfst_decoder *d, const std::vector<int32_t> &list, int32_t use_final_probs, const wfst_lm *old_lm, const wfst_lm *new_lm,
              int32_t n_paths, std::vector<int32_t> *status, NbPathsDev *P);

}  // namespace wfst
#endif
