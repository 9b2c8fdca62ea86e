// The seam between wfst_capi.cc and wfst_capi_ingest.cc (wfst_decoder_set_score_transform / wfst_decoder_advance_chunk /
// wfst_decoder_get_scores): the entry points that launch ingest_kernel are a translation unit of their own, like the words entry
// points (wfst_capi_words.h), so that wfst_capi.cc links against exactly the launches it always did.  Host only.
#ifndef WFST_CAPI_INGEST_H_
#define WFST_CAPI_INGEST_H_

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/wfst_decoder.h"
#include "wfst_hip_own.h"
#include "wfst_ingest.h"

namespace wfst {

// a decoder's score transform and the staging of its chunk calls: the per-entry tables go up through page-locked sets used in
// rotation (a call waits for the ingest that used ITS set kSets calls ago, not for the one in flight)
struct IngestState {
  static constexpr int kSets = 4;
  float scale = 1.0f;
  int32_t prior_cols = 0;        // 0: no priors
  DevBuf<float> priors;          // (rounded up to a multiple of 8 floats, the pad 0: the kernel reads whole vectors)
  DevBuf<IngestEntry> table;     // [kSets][n_channels]
  PinBuf<IngestEntry> pin;       // [kSets][n_channels]
  Event set_ev[kSets];           // the ingest that read set k is over
  int next = 0;
  Event prod_ev, done_ev;        // the producer's rows are written; the ingest is over
  int32_t n_cols = 0;            // of the rows the histories hold (0: none ingested yet)
};

// what the ingest entry points see of a decoder: the host mirrors are the decoder's own arrays, [channel]
struct IngestView {
  int device;
  int32_t n_channels, max_frames, max_col;   // max_col: the graph's largest log-likelihood column
  IngestState *is;
  hipStream_t stream;            // the decode stream
  hipStream_t copy_stream;       // the upload stream (nullptr until ingest_reserve or wfst_decoder_advance_host made it)
  const int32_t *state;          // 0 = never inited, 1 = decoding, 2 = finalized
  const int32_t *decoded;
  int32_t *hist_rows;            // frames the channel's history holds
  float *const *hist_dev;        // row 0 of the channel's history (nullptr: no history yet)
  const float *const *ll_base;   // the rows the channel's search reads
  int32_t hist_stride;           // of the frames the histories hold (0: none yet)
};
IngestView ingest_view(wfst_decoder *d);
// the history of wfst_decoder_advance_host at `stride`, with room for need_rows rows per channel (same allocation, same regrowth),
// and the upload stream
int ingest_reserve(wfst_decoder *d, const int32_t *channels, int32_t cnt, size_t need_rows, int32_t stride);
// the upload stream, made to wait for the listed channels' last enqueued work (their InitDecoding: the rows of a history are the
// previous utterance's until then)
int ingest_behind_channels(wfst_decoder *d, const int32_t *channels, int32_t cnt);
// AdvanceDecoding(max_num_frames) of the listed channels over their histories' frames
int ingest_advance(wfst_decoder *d, const int32_t *channels, int32_t n, int32_t stride, int32_t max_num_frames);
int capi_fail(int code, const std::string &msg);          // sets wfst_last_error, returns code

}  // namespace wfst
#endif
