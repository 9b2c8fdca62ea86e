// The in-arc index align_index_kernel (wfst_align.hip) leaves in a slot's block of AlignDev::idx, as the kernels that read it carve it:
// align_kernel, nearest_kernel (wfst_nearest.hip), posterior_kernel / confidence_kernel (wfst_posterior.hip), seqpost_kernel
// (wfst_seqpost.hip), slot_mass_kernel / slot_none_kernel (wfst_altern.hip), frame_post_kernel / frame_pack_kernel
// (wfst_framepost.hip), rescale_kernel (wfst_rescale.hip), bias_kernel (wfst_bias.hip) and acc_kernel / seqstat_frame_kernel / seqstat_pack_kernel /
// seqstat_dense_kernel (wfst_seqstat.hip).  What the log-semiring kernels among them do alike over this index -- the levelled frame
// sweep, the log-sum, the frame-class reduction -- is in wfst_lattice_sweep.h.  Device code only: included by the .hip files.
#ifndef WFST_ALIGN_INDEX_H_
#define WFST_ALIGN_INDEX_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wfst_device.h"

namespace wfst {
namespace {

// float <-> the uint32 whose unsigned order is the floats' order
__device__ __forceinline__ uint32_t aln_f2o(float f) {
  const uint32_t u = __float_as_uint(f);
  return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float aln_o2f(uint32_t o) { return __uint_as_float(o ^ ((o >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }
__device__ __forceinline__ unsigned long long aln_wave_min_64(unsigned long long v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned long long o = __shfl_xor(v, m, 64);
    v = o < v ? o : v;
  }
  return v;
}

struct AlnIndex {   // a slot's block of AlignDev::idx, carved
  const int4 *recA, *recB;
  int32_t *head, *off, *cur, *fbeg, *fend, *feps;
};
__device__ __forceinline__ AlnIndex aln_carve(const AlignDev &A, int slot, int4 **wa, int4 **wb) {
  int32_t *base = A.idx + (size_t)slot * A.idx_ints;
  AlnIndex X;
  *wa = reinterpret_cast<int4 *>(base);
  *wb = *wa + A.na_cap;
  X.recA = *wa;
  X.recB = *wb;
  X.head = base + 8 * (size_t)A.na_cap;
  X.off = X.head + 8;
  X.cur = X.off + A.ns_cap + 1;
  X.fbeg = X.cur + A.ns_cap;
  X.fend = X.fbeg + A.fr_cap;
  X.feps = X.fend + A.fr_cap;
  return X;
}

}  // namespace
}  // namespace wfst
#endif
