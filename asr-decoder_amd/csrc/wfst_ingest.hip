// ingest_kernel: what the reference's decodable does to a chunk of network output before the search reads it -- the prior layer's
// AddVecToRows(out, frames, cols, _log_priors, -1.0, 1.0) (nnet/nnet-layer.cc:30, nnet/nnet-nnet.cc:156-164), then
// `_acoustic_scale * output[...]` (nnet/nnet-nnet.h:212-232; DecodableMatrixScaledMapped(trans_model, loglikes, acoustic_scale),
// kaldi-nnet3bin/kaldi-hclg-my-decoder.cc:37-41,107) -- on rows that an acoustic model left on the device in float32, float16 or
// bfloat16, written into the channels' float32 histories (wfst_decoder_advance_chunk, wfst_capi_ingest.cc):
//   hist[f][j] = (float(x[r][j]) - log_priors[j]) * acoustic_scale        in float32, no FMA (the library's -ffp-contract=off);
// no priors: no subtraction; scale 1: no multiplication (float32 in, neither: a bit copy).  The widening conversions are exact.
//
// One launch per call for the whole channel list: the grid runs over the (entry, tile of kIngestRows rows) pairs of the table the
// host staged; a workgroup finds its entry by bisection over the entries' first tiles (entries without rows are not in the table).
// A source whose first row and row pitch are 16-byte aligned goes through 16-byte loads -- 8 halves or 4 floats a lane -- and one
// or two 16-byte stores; anything else, and the columns behind the last whole vector up to the history's stride (the pad columns
// are written as 0), element by element.  A pure stream: every byte is read once and written once.
#include "wfst_ingest.h"

#include <hip/hip_fp16.h>

#include "../../include/wfst_decoder.h"

namespace wfst {

template <int DT>
__device__ __forceinline__ float ingest_widen(uint32_t bits) {
  if (DT == WFST_DTYPE_F32) return __uint_as_float(bits);
  if (DT == WFST_DTYPE_F16) return __half2float(__ushort_as_half((unsigned short)bits));
  return __uint_as_float(bits << 16);   // bfloat16: the upper half of a float32
}

// flags: 1 = subtract the prior, 2 = multiply by the scale
__device__ __forceinline__ float ingest_score(float x, float prior, float scale, int flags) {
  if (flags & 1) x = x - prior;
  if (flags & 2) x = x * scale;
  return x;
}

__device__ __forceinline__ float4 ingest_score4(float4 x, const float *pri, float scale, int flags) {
  float4 p = {0.0f, 0.0f, 0.0f, 0.0f};
  if (flags & 1) p = *reinterpret_cast<const float4 *>(pri);
  return float4{ingest_score(x.x, p.x, scale, flags), ingest_score(x.y, p.y, scale, flags), ingest_score(x.z, p.z, scale, flags),
                ingest_score(x.w, p.w, scale, flags)};
}

template <int DT>
__global__ __launch_bounds__(kIngestThreads) void ingest_kernel(const IngestEntry *__restrict__ tab, int n_entries, int n_cols, int stride,
                                                                const float *__restrict__ pri, float scale, int flags) {
  constexpr int kElem = DT == WFST_DTYPE_F32 ? 4 : 2;   // bytes of a source element
  constexpr int kVec = 16 / kElem;                      // elements of a 16-byte load
  const int tile = blockIdx.x;
  int lo = 0, hi = n_entries - 1;   // the last entry whose first tile is not behind this one (uniform over the workgroup)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].tile0 <= tile) lo = mid;
    else hi = mid - 1;
  }
  const IngestEntry E = tab[lo];
  const int r0 = (tile - E.tile0) * kIngestRows;
  const int nr = min(kIngestRows, E.rows - r0);
  if (nr <= 0) return;
  const int64_t pitch_b = E.pitch * kElem;
  const char *src = reinterpret_cast<const char *>(E.src) + (int64_t)r0 * pitch_b;
  float *dst = E.dst + (size_t)r0 * (size_t)stride;
  const bool fast = ((reinterpret_cast<uintptr_t>(E.src) | (uintptr_t)pitch_b) & 15u) == 0;
  const int nvec = fast ? n_cols / kVec : 0;
  for (int idx = threadIdx.x; idx < nr * nvec; idx += kIngestThreads) {
    const int r = idx / nvec, v = idx - r * nvec;
    const uint4 q = *reinterpret_cast<const uint4 *>(src + (int64_t)r * pitch_b + (size_t)v * 16);
    float4 *o = reinterpret_cast<float4 *>(dst + (size_t)r * (size_t)stride + (size_t)v * kVec);
    const float *p = pri + (size_t)v * kVec;
    if (DT == WFST_DTYPE_F32) {
      o[0] = ingest_score4(float4{__uint_as_float(q.x), __uint_as_float(q.y), __uint_as_float(q.z), __uint_as_float(q.w)}, p, scale, flags);
    } else {
      o[0] = ingest_score4(float4{ingest_widen<DT>(q.x & 0xffffu), ingest_widen<DT>(q.x >> 16), ingest_widen<DT>(q.y & 0xffffu),
                                  ingest_widen<DT>(q.y >> 16)}, p, scale, flags);
      o[1] = ingest_score4(float4{ingest_widen<DT>(q.z & 0xffffu), ingest_widen<DT>(q.z >> 16), ingest_widen<DT>(q.w & 0xffffu),
                                  ingest_widen<DT>(q.w >> 16)}, p + 4, scale, flags);
    }
  }
  // element by element: the columns behind the last whole vector (the whole row of an unaligned source) and the pad columns
  const int c0 = nvec * kVec, nt = stride - c0;
  for (int idx = threadIdx.x; idx < nr * nt; idx += kIngestThreads) {
    const int r = idx / nt, j = c0 + (idx - r * nt);
    float y = 0.0f;
    if (j < n_cols) {
      const char *e = src + (int64_t)r * pitch_b + (size_t)j * kElem;
      const uint32_t bits = DT == WFST_DTYPE_F32 ? *reinterpret_cast<const uint32_t *>(e) : (uint32_t)*reinterpret_cast<const unsigned short *>(e);
      y = ingest_score(ingest_widen<DT>(bits), (flags & 1) ? pri[j] : 0.0f, scale, flags);
    }
    dst[(size_t)r * (size_t)stride + (size_t)j] = y;
  }
}

void launch_ingest(const IngestEntry *table_dev, int n_entries, int n_tiles, int dtype, int n_cols, int stride, const float *priors_dev,
                   float scale, hipStream_t s) {
  if (n_entries <= 0 || n_tiles <= 0) return;
  const int flags = (priors_dev ? 1 : 0) | (scale != 1.0f ? 2 : 0);
  const dim3 grid((unsigned)n_tiles), block(kIngestThreads);
  if (dtype == WFST_DTYPE_F32) hipLaunchKernelGGL(ingest_kernel<WFST_DTYPE_F32>, grid, block, 0, s, table_dev, n_entries, n_cols, stride, priors_dev, scale, flags);
  else if (dtype == WFST_DTYPE_F16) hipLaunchKernelGGL(ingest_kernel<WFST_DTYPE_F16>, grid, block, 0, s, table_dev, n_entries, n_cols, stride, priors_dev, scale, flags);
  else hipLaunchKernelGGL(ingest_kernel<WFST_DTYPE_BF16>, grid, block, 0, s, table_dev, n_entries, n_cols, stride, priors_dev, scale, flags);
}

}  // namespace wfst
