// The seam between wfst_capi.cc and wfst_capi_liveprune.cc (wfst_decoder_set_live_lattice_prune / _get_live_lattice_prune): the
// entry points are a translation unit of their own, as wfst_capi_words.cc and wfst_capi_nbwords.cc are; the snapshot's launch itself
// sits inside launch_lattice_emit, so wfst_capi.cc links against exactly the launches it always did.  Host only.
#ifndef WFST_CAPI_LIVEPRUNE_H_
#define WFST_CAPI_LIVEPRUNE_H_

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/wfst_decoder.h"
#include "wfst_device.h"
#include "wfst_hip_own.h"

namespace wfst {

// a decoder's snapshot scratch: {orderable extra, cost bits} per arena entry of every channel (DecoderDev::snap_extra), allocated when
// the mode is first set and kept until the decoder goes
struct LivePruneState {
  DevBuf<uint2> extra;
};

// what the entry points see of a decoder: mode / scratch are the two fields of its DecoderDev that launch_lattice_emit keys on
struct LivePruneView {
  int device;
  int32_t lattice, n_channels;
  int64_t arena_cap;
  LivePruneState *st;
  int32_t *mode;
  uint2 **scratch;
};
LivePruneView live_prune_view(wfst_decoder *d);
// forgets what the decoder keeps of LIVE channels' lattices (the determinized lattice of a live channel, the live entries of the
// second-pass and n-best caches): they belong to the other mode.  What is kept for finalized channels stays.
void live_prune_drop_live(wfst_decoder *d);

}  // namespace wfst
#endif
