// The seam between wfst_capi.cc and wfst_capi_forced.cc (wfst_align_graphs_*, wfst_decoder_force_align): the entry points that
// launch forced_align_kernel (wfst_forced.hip) are a translation unit of their own, as the other getters' are, so that wfst_capi.cc
// links against exactly the launches it always did.  Host only.
#ifndef WFST_CAPI_FORCED_H_
#define WFST_CAPI_FORCED_H_

#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>
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

// the by-source tables wfst_decoder_graph_posteriors adds to a set on its first call (wfst_capi_graphpost.cc)
struct GpostTables;
void gpost_tables_free(GpostTables *t);
// the stream the histories are written on (made if there is none yet): work enqueued on it runs behind the channels' ingests
int forced_stream(wfst_decoder *d, hipStream_t *s);

}  // namespace wfst

// A set of small graphs resident on one device.  Every HIP resource is an owner (wfst_hip_own.h) and goes with the set;
// wfst_align_graphs_free makes the set's device current first.
struct wfst_align_graphs {
  int device = 0;
  int32_t n_graphs = 0;
  int64_t total_states = 0, total_arcs = 0;
  std::vector<int32_t> hdr;                    // [n_graphs][kFalignHdr], as on the device
  std::vector<int32_t> labels;                 // the graphs' distinct ilabels, concatenated (hdr[10]: where a graph's begin)
  // host copies for the by-source tables: per state {first arc, first emitting arc} at hdr[6] (S + 1 entries a graph), and the
  // caller's arcs {ilabel, olabel, bits of the weight, nextstate} at hdr[11]
  std::vector<int2> h_out_off;
  std::vector<int4> h_arcs;
  wfst::DevBuf<int32_t> d_hdr, d_lvl_state, d_lvl_off, d_labels;
  wfst::DevBuf<int2> d_in_off;
  wfst::DevBuf<int4> d_rec, d_arcs;
  // built by the set's first wfst_decoder_graph_posteriors, under the lock: a set is shared between decoders and threads
  mutable std::mutex gpost_mu;
  mutable wfst::GpostTables *gpost = nullptr;
  int64_t device_bytes() const {
    return (int64_t)(d_hdr.bytes() + d_lvl_state.bytes() + d_lvl_off.bytes() + d_labels.bytes() + d_in_off.bytes() + d_rec.bytes() + d_arcs.bytes());
  }
  wfst::ForcedGraphsDev view() const { return wfst::ForcedGraphsDev{d_hdr.p, d_in_off.p, d_rec.p, d_lvl_state.p, d_lvl_off.p, d_labels.p, d_arcs.p}; }
};
#endif
