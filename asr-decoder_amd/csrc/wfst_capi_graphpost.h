// The seam between wfst_capi.cc and wfst_capi_graphpost.cc (wfst_decoder_graph_posteriors): the entry point that launches
// graphpost_kernel, graphpost_pack_kernel and graphpost_dense_kernel (wfst_graphpost.hip) is a translation unit of its own, as the
// other getters' are, so that wfst_capi.cc links against exactly the launches it always did.  Host only.
#ifndef WFST_CAPI_GRAPHPOST_H_
#define WFST_CAPI_GRAPHPOST_H_

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/wfst_decoder.h"
#include "wfst_device.h"
#include "wfst_hip_own.h"

namespace wfst {

// a decoder's graph-posterior workspace, allocated by the first call and grown on demand: the alpha tables, the rolling rows of the
// graphs beyond kGpostLdsStates, gamma and the occupancies, the class sums, the list lengths, the list entries, the column map and
// the class CSRs, the packed results; the events that order the dense rows against the consumer's stream
struct GraphPostState {
  DevBuf<double> tab, rows, gam, post, dout;
  DevBuf<int32_t> cnt, maps, out;
  DevBuf<GpostChan> chan;
  Event free_ev, rows_ev;
  int64_t bytes() const {
    return (int64_t)(tab.bytes() + rows.bytes() + gam.bytes() + post.bytes() + dout.bytes() + cnt.bytes() + maps.bytes() + out.bytes() + chan.bytes());
  }
};
GraphPostState *graphpost_state(wfst_decoder *d);

}  // namespace wfst
#endif
