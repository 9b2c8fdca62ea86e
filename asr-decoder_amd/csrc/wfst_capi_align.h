// The seam between wfst_capi.cc and wfst_capi_align.cc (wfst_decoder_align_words): the entry point that launches align_index_kernel
// and align_kernel (wfst_align.hip) is a translation unit of its own, as wfst_capi_words.cc and wfst_capi_nbwords.cc are, so that
// wfst_capi.cc links against exactly the launches it always did.  Host only.
#ifndef WFST_CAPI_ALIGN_H_
#define WFST_CAPI_ALIGN_H_

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/wfst_decoder.h"
#include "wfst_device.h"
#include "wfst_hip_own.h"

namespace wfst {

// a decoder's alignment workspace, allocated by the first call and grown on demand: the in-arc indices of a round's channels, the
// tables and path scratch of its (channel, sequence) pairs, the staged inputs, the packed results and their page-locked landing place
struct AlignState {
  DevBuf<int32_t> idx, path, in, out;
  DevBuf<uint32_t> cells;
  PinBuf<int32_t> pin;
  // wfst_decoder_word_confidence (wfst_capi_posterior.cc): the posterior workspace of a round's channels and its results' landing place
  DevBuf<double> post;
  DevBuf<int2> post_idx;
  PinBuf<double> post_pin;
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
// A prefetch in flight harvested, the live channels of `list` emitted in one launch (launch_lattice_emit: the live-prune mode and
// use_final_probs as GetRawLattice takes them), the control blocks read: sizes[4 i ..] = {states, arcs, frames decoded, error word}
// of list[i]'s raw lattice as it sits on the device.  Synchronises the decoder's stream.
int align_emit(wfst_decoder *d, const std::vector<int32_t> &list, int32_t use_final_probs, std::vector<int32_t> *sizes);

}  // namespace wfst
#endif
