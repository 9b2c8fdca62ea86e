// wfst_decoder_set_live_lattice_prune / _get_live_lattice_prune: live getters serve the SNAPSHOT lattice of a live channel (what it
// would hold if the utterance ended at this frame; lattice_snapshot_kernel, wfst_kernels.hip) instead of everything alive.  A
// translation unit of its own -- see wfst_capi_liveprune.h.
#include "wfst_capi_liveprune.h"

#include <string>

#include "wfst_capi_words.h"   // capi_fail

using namespace wfst;

int wfst_decoder_set_live_lattice_prune(wfst_decoder *d, int32_t mode) {
  if (!d) return capi_fail(WFST_E_ARG, "NULL decoder");
  if (mode != 0 && mode != 1) return capi_fail(WFST_E_ARG, "live lattice prune: the mode is 0 or 1");
  const LivePruneView v = live_prune_view(d);
  if (!v.lattice) return capi_fail(WFST_E_STATE, "live lattice prune needs a decoder created with wfst_limits.lattice_links > 0");
  if (mode == *v.mode) return WFST_OK;
  if (mode == 1 && !v.st->extra.p) {   // first use: the scratch extras, one pair per arena entry (nothing reads them before the snapshot kernel has written them)
    hipError_t e = hipSetDevice(v.device);
    if (e == hipSuccess) e = v.st->extra.alloc((size_t)v.n_channels * (size_t)v.arena_cap);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return capi_fail(e == hipErrorOutOfMemory ? WFST_E_CAPACITY : WFST_E_DEVICE,
                       "live lattice prune: no device memory for the snapshot scratch (" +
                           std::to_string((size_t)v.n_channels * (size_t)v.arena_cap * sizeof(uint2)) + " bytes): " + hipGetErrorString(e));
    }
    *v.scratch = v.st->extra.p;
  }
  *v.mode = mode;   // (the launches read it from the DecoderDev they are handed: the next live getter sees it)
  live_prune_drop_live(d);
  return WFST_OK;
}

int wfst_decoder_get_live_lattice_prune(wfst_decoder *d, int32_t *mode, int64_t *scratch_bytes) {
  if (!d) return capi_fail(WFST_E_ARG, "NULL decoder");
  const LivePruneView v = live_prune_view(d);
  if (!v.lattice) return capi_fail(WFST_E_STATE, "live lattice prune needs a decoder created with wfst_limits.lattice_links > 0");
  if (mode) *mode = *v.mode;
  if (scratch_bytes) *scratch_bytes = (int64_t)v.st->extra.bytes();
  return WFST_OK;
}
