// Owners of the HIP resources the host half of the library holds (wfst_capi.cc): device and page-locked buffers, events, streams,
// graphs and graph executables.  Host only.  Every type is move-only (the cache of executables: fixed), gives its resource back in
// the destructor and does nothing there when empty; none of them sets the device -- whoever destroys one has made its device current.
#ifndef WFST_HIP_OWN_H_
#define WFST_HIP_OWN_H_

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <map>
#include <utility>
#include <vector>

namespace wfst {

// move construction / assignment for an owner whose state is all in release() and swap()
#define WFST_MOVE_ONLY(T)                                  \
  T(const T &) = delete;                                   \
  T &operator=(const T &) = delete;                        \
  T(T &&o) noexcept { swap(o); }                           \
  T &operator=(T &&o) noexcept {                           \
    if (this != &o) { release(); swap(o); }                \
    return *this;                                          \
  }                                                        \
  ~T() { release(); }

template <class T>
struct DevBuf {   // n elements of device memory
  T *p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  WFST_MOVE_ONLY(DevBuf)
  hipError_t alloc(size_t count) {
    release();
    const hipError_t e = hipMalloc((void **)&p, std::max<size_t>(count, 1) * sizeof(T));
    if (e != hipSuccess) { p = nullptr; return e; }   // (n stays 0: a failed buffer is never taken for a large enough one)
    n = count;
    return e;
  }
  void release() {
    if (p) (void)hipFree((void *)p);
    p = nullptr;
    n = 0;
  }
  void swap(DevBuf &o) { std::swap(p, o.p); std::swap(n, o.n); }
  size_t bytes() const { return n * sizeof(T); }
};

template <class T>
struct PinBuf {   // n elements of page-locked host memory
  T *p = nullptr;
  size_t n = 0;
  PinBuf() = default;
  WFST_MOVE_ONLY(PinBuf)
  hipError_t alloc(size_t count) {
    release();
    const hipError_t e = hipHostMalloc((void **)&p, std::max<size_t>(count, 1) * sizeof(T), hipHostMallocDefault);
    if (e != hipSuccess) { p = nullptr; return e; }
    n = count;
    return e;
  }
  // room for count elements: grows only (to count + slack), and what the buffer held is not kept
  hipError_t reserve(size_t count, size_t slack = 0) { return count <= n ? hipSuccess : alloc(count + slack); }
  void release() {
    if (p) (void)hipHostFree((void *)p);
    p = nullptr;
    n = 0;
  }
  void swap(PinBuf &o) { std::swap(p, o.p); std::swap(n, o.n); }
  size_t bytes() const { return n * sizeof(T); }
};

struct Event {
  hipEvent_t h = nullptr;
  Event() = default;
  WFST_MOVE_ONLY(Event)
  hipError_t create(unsigned flags = hipEventDisableTiming) {
    release();
    const hipError_t e = hipEventCreateWithFlags(&h, flags);
    if (e != hipSuccess) h = nullptr;
    return e;
  }
  void release() {
    if (h) (void)hipEventDestroy(h);
    h = nullptr;
  }
  void swap(Event &o) { std::swap(h, o.h); }
  operator hipEvent_t() const { return h; }
};

struct Stream {   // a non-blocking stream of its own, or (borrow) someone else's, which it leaves alone
  hipStream_t h = nullptr;
  bool owned = false;
  Stream() = default;
  WFST_MOVE_ONLY(Stream)
  hipError_t create() {
    release();
    const hipError_t e = hipStreamCreateWithFlags(&h, hipStreamNonBlocking);
    if (e != hipSuccess) h = nullptr;
    owned = h != nullptr;
    return e;
  }
  void borrow(hipStream_t s) {
    release();
    h = s;
  }
  void release() {
    if (h && owned) (void)hipStreamDestroy(h);
    h = nullptr;
    owned = false;
  }
  void swap(Stream &o) { std::swap(h, o.h); std::swap(owned, o.owned); }
  operator hipStream_t() const { return h; }
};

struct Graph {   // a captured graph between hipStreamEndCapture and its instantiation
  hipGraph_t h = nullptr;
  Graph() = default;
  WFST_MOVE_ONLY(Graph)
  void release() {
    if (h) (void)hipGraphDestroy(h);
    h = nullptr;
  }
  void swap(Graph &o) { std::swap(h, o.h); }
};

struct GraphExecCache {   // graph executables by key (stays where it is: neither copied nor moved)
  std::map<std::vector<int>, hipGraphExec_t> m;
  GraphExecCache() = default;
  GraphExecCache(const GraphExecCache &) = delete;
  GraphExecCache &operator=(const GraphExecCache &) = delete;
  ~GraphExecCache() { destroy_all(); }
  void destroy_all() {   // (none of them may still be running)
    for (auto &kv : m) (void)hipGraphExecDestroy(kv.second);
    m.clear();
  }
  // instantiates `graph` under `key` (not held yet)
  hipError_t add(const std::vector<int> &key, hipGraph_t graph, hipGraphExec_t *exec) {
    const hipError_t e = hipGraphInstantiate(exec, graph, nullptr, nullptr, 0);
    if (e == hipSuccess) m.emplace(key, *exec);
    return e;
  }
};

#undef WFST_MOVE_ONLY

}  // namespace wfst
#endif
