// wfst_decoder_set_score_transform / wfst_decoder_advance_chunk / wfst_decoder_get_scores: chunks of acoustic-model output ingested on
// the device (ingest_kernel, wfst_ingest.hip).  A translation unit of its own -- see wfst_capi_ingest.h.
#include "wfst_capi_ingest.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>
#include <vector>

using namespace wfst;

#define I_TRY(expr)                                                                                   \
  do {                                                                                                \
    hipError_t e_ = (expr);                                                                           \
    if (e_ != hipSuccess) return capi_fail(WFST_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

static int32_t round_up4(int32_t n) { return (n + 3) & ~3; }

int wfst_decoder_set_score_transform(wfst_decoder *d, float acoustic_scale, const float *log_priors, int32_t n_cols) {
  if (!d) return capi_fail(WFST_E_ARG, "NULL decoder");
  if (n_cols < 0 || (log_priors && n_cols == 0) || (!log_priors && n_cols != 0))
    return capi_fail(WFST_E_ARG, "score transform: log_priors and n_cols > 0 go together (NULL and 0 clear the priors)");
  if (!std::isfinite(acoustic_scale)) return capi_fail(WFST_E_ARG, "score transform: acoustic_scale is not finite");
  const IngestView V = ingest_view(d);
  for (int c = 0; c < V.n_channels; ++c)
    if (V.state[c] == 1 && V.hist_rows[c] > 0)
      return capi_fail(WFST_E_STATE, "score transform changed mid-utterance: channel " + std::to_string(c) + " holds ingested frames");
  I_TRY(hipSetDevice(V.device));
  IngestState &S = *V.is;
  if (V.copy_stream) I_TRY(hipStreamSynchronize(V.copy_stream));   // (the ingest of a finished utterance may still read the old priors)
  if (log_priors) {
    std::vector<float> padded(((size_t)n_cols + 7) & ~(size_t)7, 0.0f);
    memcpy(padded.data(), log_priors, (size_t)n_cols * 4);
    DevBuf<float> pri;
    I_TRY(pri.alloc(padded.size()));
    I_TRY(hipMemcpy(pri.p, padded.data(), padded.size() * 4, hipMemcpyHostToDevice));
    S.priors = std::move(pri);
  } else {
    S.priors.release();
  }
  S.prior_cols = n_cols;
  S.scale = acoustic_scale;
  return WFST_OK;
}

int wfst_decoder_advance_chunk(wfst_decoder *d, const int32_t *channels, int32_t n, const void *const *rows, const int32_t *n_new_frames,
                               const int64_t *row_pitch, int32_t dtype, int32_t n_cols, void *producer_stream, int32_t max_num_frames) {
  if (!d) return capi_fail(WFST_E_ARG, "NULL decoder");
  if (!rows || !n_new_frames) return capi_fail(WFST_E_ARG, "NULL rows / n_new_frames");
  if (dtype != WFST_DTYPE_F32 && dtype != WFST_DTYPE_F16 && dtype != WFST_DTYPE_BF16) return capi_fail(WFST_E_ARG, "unknown dtype (WFST_DTYPE_F32 / _F16 / _BF16)");
  if (n_cols <= 0) return capi_fail(WFST_E_ARG, "n_cols <= 0");
  IngestView V = ingest_view(d);
  IngestState &S = *V.is;
  if (S.prior_cols != 0 && S.prior_cols != n_cols)
    return capi_fail(WFST_E_ARG, "n_cols " + std::to_string(n_cols) + " differs from the log priors' " + std::to_string(S.prior_cols));
  if (n_cols <= V.max_col) return capi_fail(WFST_E_ARG, "n_cols too small: the graph reads log-likelihood column " + std::to_string(V.max_col));
  const int32_t cnt = channels ? n : V.n_channels;
  if (cnt <= 0 || cnt > V.n_channels) return capi_fail(WFST_E_ARG, "bad channel count");
  const uintptr_t elem = dtype == WFST_DTYPE_F32 ? 4 : 2;
  {
    std::vector<char> seen((size_t)V.n_channels, 0);
    for (int i = 0; i < cnt; ++i) {
      const int c = channels ? channels[i] : i;
      if (c < 0 || c >= V.n_channels) return capi_fail(WFST_E_ARG, "channel index out of range");
      if (seen[(size_t)c]) return capi_fail(WFST_E_ARG, "duplicate channel in list");
      seen[(size_t)c] = 1;
      if (n_new_frames[i] < 0) return capi_fail(WFST_E_ARG, "negative n_new_frames");
      if (row_pitch && row_pitch[i] < n_cols) return capi_fail(WFST_E_ARG, "row pitch below n_cols");
      if (n_new_frames[i] > 0 && !rows[i]) return capi_fail(WFST_E_ARG, "NULL row pointer with frames to append");
      if (reinterpret_cast<uintptr_t>(rows[i]) % elem) return capi_fail(WFST_E_ARG, "row pointer not aligned to its element size");
    }
  }
  const int32_t stride = round_up4(n_cols);
  if (V.hist_stride != 0 && V.hist_stride != stride)
    for (int c = 0; c < V.n_channels; ++c)
      if (V.hist_rows[c] > 0) return capi_fail(WFST_E_ARG, "stride changed while channels hold frames");
  for (int i = 0; i < cnt; ++i) {
    const int c = channels ? channels[i] : i;
    if (V.state[c] == 0) return capi_fail(WFST_E_STATE, "AdvanceDecoding before InitDecoding");
    if (V.state[c] == 2) return capi_fail(WFST_E_STATE, "AdvanceDecoding after FinalizeDecoding");
    if (V.decoded[c] > V.hist_rows[c]) return capi_fail(WFST_E_STATE, "the channel's utterance is fed through wfst_decoder_advance (the caller's own matrix)");
  }
  size_t need_rows = 0;
  int32_t n_entries = 0;
  for (int i = 0; i < cnt; ++i) {
    const int c = channels ? channels[i] : i;
    const int64_t want = (int64_t)V.hist_rows[c] + n_new_frames[i];
    if (want > V.max_frames) return capi_fail(WFST_E_CAPACITY, "utterance longer than wfst_limits.max_frames");
    need_rows = std::max(need_rows, (size_t)want);
    if (n_new_frames[i] > 0) ++n_entries;
  }
  I_TRY(hipSetDevice(V.device));
  if (n_entries > 0) {
    int rc = ingest_reserve(d, channels, cnt, need_rows, stride);
    if (rc != WFST_OK) return rc;
    V = ingest_view(d);   // (the upload stream may be new)
    if (!S.table.p) {   // the first chunk: a decoder that never ingests pays nothing
      DevBuf<IngestEntry> table;
      PinBuf<IngestEntry> pin;
      Event ev[IngestState::kSets], prod;
      I_TRY(table.alloc((size_t)IngestState::kSets * (size_t)V.n_channels));
      I_TRY(pin.alloc((size_t)IngestState::kSets * (size_t)V.n_channels));
      for (Event &e : ev) I_TRY(e.create());
      I_TRY(prod.create());
      S.table = std::move(table);
      S.pin = std::move(pin);
      for (int k = 0; k < IngestState::kSets; ++k) S.set_ev[k] = std::move(ev[k]);
      S.prod_ev = std::move(prod);
    }
    const int set = S.next;
    S.next = (S.next + 1) % IngestState::kSets;
    I_TRY(hipEventSynchronize(S.set_ev[set]));   // (never recorded: returns at once)
    IngestEntry *tab = S.pin.p + (size_t)set * (size_t)V.n_channels;
    std::vector<int32_t> fresh;   // channels whose utterance starts with this chunk
    int32_t k = 0, tiles = 0;
    for (int i = 0; i < cnt; ++i) {
      const int c = channels ? channels[i] : i;
      if (n_new_frames[i] == 0) continue;
      if (V.hist_rows[c] == 0) fresh.push_back(c);
      tab[k].src = rows[i];
      tab[k].pitch = row_pitch ? row_pitch[i] : (int64_t)n_cols;
      tab[k].dst = V.hist_dev[c] + (size_t)V.hist_rows[c] * (size_t)stride;
      tab[k].rows = n_new_frames[i];
      tab[k].tile0 = tiles;
      tiles += (n_new_frames[i] + kIngestRows - 1) / kIngestRows;
      ++k;
    }
    // rows 0.. of a history are the previous utterance's until the channel's InitDecoding and whatever was enqueued before it are over
    if (!fresh.empty()) { rc = ingest_behind_channels(d, fresh.data(), (int32_t)fresh.size()); if (rc != WFST_OK) return rc; }
    const bool linked = producer_stream != WFST_STREAM_NONE;
    const hipStream_t prod = linked ? static_cast<hipStream_t>(producer_stream) : nullptr;
    if (linked) {
      I_TRY(hipEventRecord(S.prod_ev, prod));
      I_TRY(hipStreamWaitEvent(V.copy_stream, S.prod_ev, 0));
    }
    IngestEntry *tab_dev = S.table.p + (size_t)set * (size_t)V.n_channels;
    I_TRY(hipMemcpyAsync(tab_dev, tab, (size_t)k * sizeof(IngestEntry), hipMemcpyHostToDevice, V.copy_stream));
    launch_ingest(tab_dev, k, tiles, dtype, n_cols, stride, S.prior_cols ? S.priors.p : nullptr, S.scale, V.copy_stream);
    I_TRY(hipGetLastError());
    I_TRY(hipEventRecord(S.set_ev[set], V.copy_stream));
    I_TRY(hipStreamWaitEvent(V.stream, S.set_ev[set], 0));   // the frames' kernels run behind the rows; the host does not wait
    if (linked) I_TRY(hipStreamWaitEvent(prod, S.set_ev[set], 0));   // ... and so does whatever the producer enqueues next
    for (int i = 0; i < cnt; ++i) V.hist_rows[channels ? channels[i] : i] += n_new_frames[i];
    S.n_cols = n_cols;
  }
  return ingest_advance(d, channels, n, stride, max_num_frames);
}

int wfst_decoder_get_scores(wfst_decoder *d, int32_t channel, int32_t first_frame, int32_t n_frames, float *out) {
  if (!d) return capi_fail(WFST_E_ARG, "NULL decoder");
  const IngestView V = ingest_view(d);
  if (channel < 0 || channel >= V.n_channels) return capi_fail(WFST_E_ARG, "channel index out of range");
  if (V.ll_base[channel] && V.ll_base[channel] != V.hist_dev[channel])
    return capi_fail(WFST_E_STATE, "the channel reads the caller's own matrix (wfst_decoder_advance): the library holds no scores of it");
  if (first_frame < 0 || n_frames < 0 || (int64_t)first_frame + n_frames > V.hist_rows[channel])
    return capi_fail(WFST_E_ARG, "frame range outside the " + std::to_string(V.hist_rows[channel]) + " frames the channel's history holds");
  if (n_frames == 0) return WFST_OK;
  if (!out) return capi_fail(WFST_E_ARG, "NULL out");
  I_TRY(hipSetDevice(V.device));
  const int32_t stride = V.hist_stride;
  const int32_t cols = (V.is->n_cols > 0 && round_up4(V.is->n_cols) == stride) ? V.is->n_cols : stride;
  // on the upload stream: behind the channel's ingests (and the copies of wfst_decoder_advance_host)
  I_TRY(hipMemcpy2DAsync(out, (size_t)cols * 4, V.hist_dev[channel] + (size_t)first_frame * (size_t)stride, (size_t)stride * 4, (size_t)cols * 4,
                         (size_t)n_frames, hipMemcpyDeviceToHost, V.copy_stream));
  I_TRY(hipStreamSynchronize(V.copy_stream));
  return WFST_OK;
}
