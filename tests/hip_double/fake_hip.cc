// A TEST DOUBLE of the HIP runtime for the host half of the library (asr-decoder_amd/csrc/wfst_capi.cc) under AddressSanitizer:
// no device, no kernels -- "device" and page-locked memory come from calloc, copies and memsets are memcpy / memset, streams,
// events, graphs and graph executables are small heap objects, and the launch wrappers of wfst_device.h do nothing.  What it is
// for is OWNERSHIP: it counts what is live of every kind, aborts on a double free or a handle it never handed out, and can be told
// to fail the k-th creating call (hipMalloc, hipHostMalloc, hipEventCreate*, hipStreamCreate*, hipGraphInstantiate) with
// hipErrorOutOfMemory.  It fakes no results: the control blocks the kernels would write stay zero.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>

#include "../../asr-decoder_amd/csrc/wfst_device.h"
#include "fake_hip.h"

namespace {
std::map<void *, size_t> g_mem[2];   // [kFakeDevice / kFakePinned] allocation -> bytes
std::set<void *> g_obj[kFakeKinds];  // events, streams, graphs, execs
const char *const kKindName[kFakeKinds] = {"device", "pinned", "event", "stream", "graph", "exec"};
long g_created = 0, g_fail_at = 0;
bool g_fault_hit = false;
hipError_t g_last = hipSuccess;

[[noreturn]] void die(const char *what, int kind, const void *p) {
  fprintf(stderr, "FAKE HIP: %s (%s %p)\n", what, kKindName[kind], p);
  abort();
}
// every creating call comes here first: true = this is the one to fail
bool faulted() {
  if (++g_created != g_fail_at) return false;
  g_fault_hit = true;
  g_last = hipErrorOutOfMemory;
  return true;
}
hipError_t mem_alloc(int kind, void **ptr, size_t bytes) {
  *ptr = nullptr;
  if (faulted()) return hipErrorOutOfMemory;
  void *p = calloc(bytes ? bytes : 1, 1);
  if (!p) { g_last = hipErrorOutOfMemory; return g_last; }
  g_mem[kind][p] = bytes;
  *ptr = p;
  return hipSuccess;
}
hipError_t mem_free(int kind, void *p) {
  if (!p) return hipSuccess;
  if (!g_mem[kind].erase(p)) die("free of memory that is not live", kind, p);
  free(p);
  return hipSuccess;
}
template <class H>
hipError_t obj_new(int kind, H *out) {
  *out = nullptr;
  if (faulted()) return hipErrorOutOfMemory;
  void *p = malloc(8);
  g_obj[kind].insert(p);
  *out = (H)p;
  return hipSuccess;
}
hipError_t obj_delete(int kind, void *p) {
  if (!g_obj[kind].erase(p)) die("destroy of a handle that is not live", kind, p);
  free(p);
  return hipSuccess;
}
void known(int kind, const void *p, bool null_ok = false) {
  if (!(null_ok && !p) && !g_obj[kind].count(const_cast<void *>(p))) die("use of a handle that is not live", kind, p);
}
}  // namespace

long fake_hip_live(int kind) { return kind < 2 ? (long)g_mem[kind].size() : (long)g_obj[kind].size(); }
const char *fake_hip_kind_name(int kind) { return kKindName[kind]; }
long fake_hip_created(void) { return g_created; }
void fake_hip_fail_at(long k) { g_created = 0; g_fail_at = k; g_fault_hit = false; g_last = hipSuccess; }
int fake_hip_fault_hit(void) { return g_fault_hit ? 1 : 0; }

extern "C" {

const char *hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : e == hipErrorOutOfMemory ? "out of memory" : "error"; }
hipError_t hipGetLastError(void) { const hipError_t e = g_last; g_last = hipSuccess; return e; }
hipError_t hipGetDeviceCount(int *n) { *n = 1; return hipSuccess; }
hipError_t hipSetDevice(int dev) { return dev == 0 ? hipSuccess : hipErrorInvalidDevice; }
hipError_t hipDeviceSynchronize(void) { return hipSuccess; }
hipError_t hipMemGetInfo(size_t *free_b, size_t *total_b) { *free_b = *total_b = (size_t)1 << 30; return hipSuccess; }

hipError_t hipMalloc(void **ptr, size_t bytes) { return mem_alloc(kFakeDevice, ptr, bytes); }
hipError_t hipFree(void *p) { return mem_free(kFakeDevice, p); }
hipError_t hipHostMalloc(void **ptr, size_t bytes, unsigned int) { return mem_alloc(kFakePinned, ptr, bytes); }
hipError_t hipHostFree(void *p) { return mem_free(kFakePinned, p); }
hipError_t hipPointerGetAttributes(hipPointerAttribute_t *at, const void *ptr) {
  memset(at, 0, sizeof(*at));
  for (int kind = 0; kind < 2; ++kind) {
    auto it = g_mem[kind].upper_bound(const_cast<void *>(ptr));
    if (it == g_mem[kind].begin()) continue;
    --it;
    if ((const char *)ptr < (const char *)it->first + it->second) {
      at->type = kind == kFakePinned ? hipMemoryTypeHost : hipMemoryTypeDevice;
      return hipSuccess;
    }
  }
  g_last = hipErrorInvalidValue;   // pageable memory, as the runtime answers
  return g_last;
}

hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind) { memcpy(dst, src, bytes); return hipSuccess; }
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind, hipStream_t st) {
  known(kFakeStream, st, true);
  memcpy(dst, src, bytes);
  return hipSuccess;
}
hipError_t hipMemcpy2DAsync(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height, hipMemcpyKind,
                            hipStream_t st) {
  known(kFakeStream, st, true);
  for (size_t r = 0; r < height; ++r) memcpy((char *)dst + r * dpitch, (const char *)src + r * spitch, width);
  return hipSuccess;
}
hipError_t hipMemsetAsync(void *dst, int value, size_t bytes, hipStream_t st) {
  known(kFakeStream, st, true);
  memset(dst, value, bytes);
  return hipSuccess;
}

hipError_t hipStreamCreateWithFlags(hipStream_t *st, unsigned int) { return obj_new(kFakeStream, st); }
hipError_t hipStreamDestroy(hipStream_t st) { return obj_delete(kFakeStream, st); }
hipError_t hipStreamSynchronize(hipStream_t st) { known(kFakeStream, st, true); return hipSuccess; }
hipError_t hipStreamQuery(hipStream_t st) { known(kFakeStream, st, true); return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t st, hipEvent_t ev, unsigned int) {
  known(kFakeStream, st, true);
  known(kFakeEvent, ev);
  return hipSuccess;
}

hipError_t hipEventCreate(hipEvent_t *ev) { return obj_new(kFakeEvent, ev); }
hipError_t hipEventCreateWithFlags(hipEvent_t *ev, unsigned) { return obj_new(kFakeEvent, ev); }
hipError_t hipEventDestroy(hipEvent_t ev) { return obj_delete(kFakeEvent, ev); }
hipError_t hipEventRecord(hipEvent_t ev, hipStream_t st) {
  known(kFakeEvent, ev);
  known(kFakeStream, st, true);
  return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t ev) { known(kFakeEvent, ev); return hipSuccess; }
hipError_t hipEventQuery(hipEvent_t ev) { known(kFakeEvent, ev); return hipSuccess; }
hipError_t hipEventElapsedTime(float *ms, hipEvent_t a, hipEvent_t b) {
  known(kFakeEvent, a);
  known(kFakeEvent, b);
  *ms = 0.0f;
  return hipSuccess;
}

hipError_t hipStreamBeginCapture(hipStream_t st, hipStreamCaptureMode) { known(kFakeStream, st, true); return hipSuccess; }
hipError_t hipStreamEndCapture(hipStream_t st, hipGraph_t *graph) {   // (hands a graph out, but is not one of the calls told to fail)
  known(kFakeStream, st, true);
  void *p = malloc(8);
  g_obj[kFakeGraph].insert(p);
  *graph = (hipGraph_t)p;
  return hipSuccess;
}
hipError_t hipGraphDestroy(hipGraph_t graph) { return obj_delete(kFakeGraph, graph); }
hipError_t hipGraphInstantiate(hipGraphExec_t *exec, hipGraph_t graph, hipGraphNode_t *, char *, size_t) {
  known(kFakeGraph, graph);
  return obj_new(kFakeExec, exec);
}
hipError_t hipGraphExecDestroy(hipGraphExec_t exec) { return obj_delete(kFakeExec, exec); }
hipError_t hipGraphLaunch(hipGraphExec_t exec, hipStream_t st) {
  known(kFakeExec, exec);
  known(kFakeStream, st, true);
  return hipSuccess;
}

}  // extern "C"

// the launch wrappers of wfst_device.h: nothing runs
namespace wfst {
int insert_kernel_set_lds(int) { return 0; }
void launch_nbest(const DecoderDev &, const NbestDev &, const int32_t *, int, hipStream_t) {}
void launch_determinize(const DecoderDev &, const DetDev &, const int32_t *, int, hipStream_t, int) {}
void launch_det_pack(const DetDev &, int, int4 *, float2 *, int64_t, hipStream_t) {}
void launch_nbest_paths(const NbPathsDev &, int, hipStream_t, int) {}
void launch_compose2(const DetDev &, const CmpDev &, const LmDev &, const LmDev &, int, hipStream_t) {}
void launch_init(const DecoderDev &, const int32_t *, int, hipStream_t) {}
void launch_expand(const DecoderDev &, int, int, int, hipStream_t) {}
void launch_insert(const DecoderDev &, int, int, const int32_t *, int, int, int, int, hipStream_t) {}
void launch_closure(const DecoderDev &, int, int, const int32_t *, int, int, int, hipStream_t, int) {}
void launch_lattice_prune_step(const DecoderDev &, int, int, const int32_t *, int, int, hipStream_t, int) {}
int prune_raw_resident_workgroups(int) { return 1 << 20; }
int prune_raw_grid(int chan_cnt) { return chan_cnt; }
void launch_set_finalized(const DecoderDev &, const int32_t *, int, hipStream_t) {}
void launch_delay(int, hipStream_t) {}
void launch_lattice_prune(const DecoderDev &, const int32_t *, int, hipStream_t) {}
void launch_lattice_emit(const DecoderDev &, const int32_t *, int, int, hipStream_t) {}
void launch_best_path(const DecoderDev &, const int32_t *, int, int, int, int32_t *, int32_t *, float *, float *, int32_t *, int32_t *,
                      hipStream_t) {}
void launch_endpoint(const DecoderDev &, const int32_t *, int, const uint32_t *, int, int32_t *, hipStream_t) {}
void launch_partial(const DecoderDev &, const int32_t *, int, int32_t *, int64_t, int, int32_t *, hipStream_t) {}
}  // namespace wfst
