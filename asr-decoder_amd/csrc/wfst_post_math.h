// The float64 arithmetic the log-semiring kernels share (posterior_kernel, confidence_kernel: wfst_posterior.hip; seqpost_kernel:
// wfst_seqpost.hip; slot_none_kernel: wfst_altern.hip): +inf, "is finite", and an in-arc record's cost c(a) with the "no arc" rule.  Device code only.
#ifndef WFST_POST_MATH_H_
#define WFST_POST_MATH_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wfst_device.h"

namespace wfst {
namespace {

__device__ __forceinline__ double post_inf() { return __longlong_as_double(0x7FF0000000000000ll); }
__device__ __forceinline__ bool post_finite(double x) { return x - x == 0.0; }
// c(a), false where the arc is no arc
__device__ __forceinline__ bool post_cost(const PostDev &P, const int4 &R, double *c) {
  const float g = __int_as_float(R.z), a = __int_as_float(R.w), v = g + a;
  *c = P.graph_scale * (double)g + P.acoustic_scale * (double)a;
  return v - v == 0.0f;
}

}  // namespace
}  // namespace wfst
#endif
