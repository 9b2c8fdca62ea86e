// Chunks of acoustic-model output handed to a GpuBatchDecoder where the model left them, on the device
// (wfst_decoder_set_score_transform / wfst_decoder_advance_chunk: ingest_kernel): the reference's --acoustic-scale and
// DecodableMatrixScaledMapped(trans_model, loglikes, acoustic_scale) (kaldi-nnet3bin/kaldi-hclg-my-decoder.cc:37-41,107), its own
// network's `_acoustic_scale * output[...]` (nnet/nnet-nnet.h:212-232) and the prior layer in front of it (nnet/nnet-layer.cc:30).
// A translation unit of its own: wfst-host.cc is also linked against doubles of the C ABI that end at the calls it makes.
#include "wfst-host.h"

#include <stdexcept>
#include <string>

namespace datemoon {

static void FatalIngest(const char *what) { throw std::runtime_error(std::string(what) + ": " + wfst_last_error()); }

void GpuBatchDecoder::SetScoreTransform(float acoustic_scale, const std::vector<float> &log_priors) {
  if (wfst_decoder_set_score_transform(_dec, acoustic_scale, log_priors.empty() ? nullptr : log_priors.data(), (int32_t)log_priors.size()) != WFST_OK)
    FatalIngest("SetScoreTransform");
}

void GpuBatchDecoder::AdvanceDecodingChunk(const std::vector<int> &ch, const std::vector<const void *> &device_rows,
                                           const std::vector<int> &num_new_frames, int dtype, int n_cols, void *producer_stream,
                                           const std::vector<int64_t> &row_pitch, int max_num_frames) {
  const size_t cnt = ch.empty() ? (size_t)_n : ch.size();
  if (device_rows.size() != cnt || num_new_frames.size() != cnt || (!row_pitch.empty() && row_pitch.size() != cnt))
    throw std::runtime_error("AdvanceDecodingChunk: one row pointer, frame count (and pitch) per listed channel");
  if (wfst_decoder_advance_chunk(_dec, ch.empty() ? nullptr : ch.data(), (int)ch.size(), device_rows.data(), num_new_frames.data(),
                                 row_pitch.empty() ? nullptr : row_pitch.data(), dtype, n_cols, producer_stream, max_num_frames) != WFST_OK)
    FatalIngest("AdvanceDecodingChunk");
}

}  // namespace datemoon
