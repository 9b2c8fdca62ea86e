// ingest_kernel (wfst_ingest.hip): a chunk of acoustic-model output -- float32, float16 or bfloat16 rows on the device -- becomes
// rows of the channels' float32 log-likelihood histories, scaled and with the log priors taken off.  The launch declaration and
// the per-entry table the host stages (wfst_capi_ingest.cc).
#ifndef WFST_INGEST_H_
#define WFST_INGEST_H_

#include <hip/hip_runtime.h>

#include <cstdint>

namespace wfst {

constexpr int kIngestRows = 4;       // rows of one entry per workgroup (a tile)
constexpr int kIngestThreads = 256;

// one listed channel that appends rows (channels that append none are not in the table)
struct IngestEntry {
  const void *src;   // the first new row
  int64_t pitch;     // elements between two source rows
  float *dst;        // the history row the first new row becomes
  int32_t rows;
  int32_t tile0;     // tiles of the entries in front of this one
};

// dst[r][j] = (float(src[r][j]) - priors[j]) * scale for j < n_cols, 0 for n_cols <= j < stride; priors_dev == nullptr: nothing is
// subtracted; scale == 1: nothing is multiplied.  dtype: WFST_DTYPE_*.  stride is a multiple of 4 and every dst 16-byte aligned.
void launch_ingest(const IngestEntry *table_dev, int n_entries, int n_tiles, int dtype, int n_cols, int stride, const float *priors_dev,
                   float scale, hipStream_t s);

}  // namespace wfst
#endif
