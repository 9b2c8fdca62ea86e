// The seam between wfst_capi.cc and wfst_capi_forced.cc (wfst_align_graphs_*, wfst_decoder_force_align): the entry points that
// launch forced_align_kernel (wfst_forced.hip) are a translation unit of their own, as the other getters' are, so that wfst_capi.cc
// links against exactly the launches it always did.  Host only.
#ifndef WFST_CAPI_FORCED_H_
#define WFST_CAPI_FORCED_H_

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/wfst_decoder.h"
#include "wfst_device.h"
#include "wfst_hip_own.h"

namespace wfst {

constexpr int64_t kFalignDefaultCells = 65536ll * 65;   // max_cells = 0: wfst_decoder_align_words' default bound
constexpr int64_t kFalignRoundCells = 64ll << 20;       // backpointer cells of one round: 256 MiB

// a decoder's forced-alignment workspace, allocated by the first call and grown on demand: the backpointers, the cost rows of the
// graphs beyond kFalignLdsStates, the traced paths, the list entries, the column and class maps, the packed results
struct ForcedState {
  DevBuf<int32_t> bp, path, maps, out;
  DevBuf<float> rows;
  DevBuf<ForcedChan> chan;
  int64_t bytes() const { return (int64_t)(bp.bytes() + path.bytes() + maps.bytes() + out.bytes() + rows.bytes() + chan.bytes()); }
};

// what the entry point sees of a decoder: the host mirrors are the decoder's own arrays, [channel]
struct ForcedView {
  int device;
  int32_t n_channels;
  ForcedState *fs;
  const int32_t *state;          // 0 = never inited, 1 = decoding, 2 = finalized
  const int32_t *decoded;
  const int32_t *hist_rows;      // frames the channel's library-held history holds
  float *const *hist_dev;        // row 0 of that history
  const float *const *ll_base;   // the rows the channel's search reads (the caller's matrix where it is not the history)
  int32_t hist_stride, ll_stride;
  const std::vector<int32_t> *tid2pdf;   // of the decoder's graph (empty: the column is the transition-id)
};
ForcedView forced_view(wfst_decoder *d);
// the stream the histories are written on (made if there is none yet): work enqueued on it runs behind the channels' ingests
int forced_stream(wfst_decoder *d, hipStream_t *s);

}  // namespace wfst
#endif
