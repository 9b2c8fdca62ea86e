// ingest_probe: the time of ingest_kernel (csrc/wfst_ingest.hip) on a service-sized chunk call -- 128 channels x 25 rows x 3000
// columns by default, float16 / bfloat16 / float32 sources, scale 0.1 and priors -- beside a hipMemcpy2DAsync device-to-device
// copy of the same destination bytes (25 x 3000 floats into each channel's history).  Prints the mean of `reps` event-timed
// runs of each; under `rocprofv3 --kernel-trace --stats -- ./ingest_probe` the kernel times come from the trace.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -o tools/ingest_probe tools/ingest_probe.hip
//   tools/ingest_probe [channels rows cols reps]
#include "../asr-decoder_amd/csrc/wfst_ingest.hip"

#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(expr)                                                                          \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #expr, hipGetErrorString(e_)); return 1; } \
  } while (0)

int main(int argc, char **argv) {
  const int B = argc > 1 ? atoi(argv[1]) : 128, R = argc > 2 ? atoi(argv[2]) : 25, N = argc > 3 ? atoi(argv[3]) : 3000, reps = argc > 4 ? atoi(argv[4]) : 20;
  if (B <= 0 || R <= 0 || N <= 0 || reps <= 0) { fprintf(stderr, "usage: ingest_probe [channels rows cols reps]\n"); return 1; }
  const int stride = (N + 3) & ~3, cap = 256 > R ? 256 : R;   // a history of `cap` rows per channel
  const size_t src_elems = (size_t)B * R * N, hist = (size_t)B * cap * stride;
  void *src = nullptr;
  float *dst = nullptr, *pri = nullptr;
  wfst::IngestEntry *tab = nullptr;
  CHECK(hipMalloc(&src, src_elems * 4));
  CHECK(hipMalloc((void **)&dst, hist * 4));
  CHECK(hipMalloc((void **)&pri, (size_t)(stride + 8) * 4));
  CHECK(hipMalloc((void **)&tab, (size_t)B * sizeof(wfst::IngestEntry)));
  CHECK(hipMemset(src, 0x3c, src_elems * 4));   // (0x3c3c: 1.06 as float16, 0.0115 as bfloat16; a small float32)
  CHECK(hipMemset(pri, 0, (size_t)(stride + 8) * 4));
  hipStream_t st;
  hipEvent_t e0, e1;
  CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  const double dst_bytes = (double)B * R * N * 4;
  const char *names[3] = {"f32", "f16", "bf16"};
  for (int dt = 0; dt < 3; ++dt) {
    const size_t elem = dt == WFST_DTYPE_F32 ? 4 : 2;
    std::vector<wfst::IngestEntry> h((size_t)B);
    int tiles = 0;
    for (int c = 0; c < B; ++c) {
      h[(size_t)c] = wfst::IngestEntry{(const char *)src + (size_t)c * R * N * elem, (int64_t)N, dst + (size_t)c * cap * stride, R, tiles};
      tiles += (R + wfst::kIngestRows - 1) / wfst::kIngestRows;
    }
    CHECK(hipMemcpy(tab, h.data(), h.size() * sizeof(wfst::IngestEntry), hipMemcpyHostToDevice));
    for (int k = 0; k < 3; ++k) wfst::launch_ingest(tab, B, tiles, dt, N, stride, pri, 0.1f, st);
    CHECK(hipEventRecord(e0, st));
    for (int k = 0; k < reps; ++k) wfst::launch_ingest(tab, B, tiles, dt, N, stride, pri, 0.1f, st);
    CHECK(hipEventRecord(e1, st));
    CHECK(hipEventSynchronize(e1));
    CHECK(hipGetLastError());
    float ms = 0.0f;
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    const double us = ms * 1e3 / reps, moved = dst_bytes + (double)src_elems * elem;
    printf("ingest %-4s %d x %d x %d: %.2f us per launch (events, back to back), %.1f MB moved, %.2f TB/s\n", names[dt], B, R, N, us, moved / 1e6, moved / us / 1e6);
  }
  // the same destination bytes as one 2-D device-to-device copy: B rows of R * N floats, cap * stride floats apart
  for (int k = 0; k < 3; ++k)
    CHECK(hipMemcpy2DAsync(dst, (size_t)cap * stride * 4, src, (size_t)R * N * 4, (size_t)R * N * 4, (size_t)B, hipMemcpyDeviceToDevice, st));
  CHECK(hipEventRecord(e0, st));
  for (int k = 0; k < reps; ++k)
    CHECK(hipMemcpy2DAsync(dst, (size_t)cap * stride * 4, src, (size_t)R * N * 4, (size_t)R * N * 4, (size_t)B, hipMemcpyDeviceToDevice, st));
  CHECK(hipEventRecord(e1, st));
  CHECK(hipEventSynchronize(e1));
  float ms = 0.0f;
  CHECK(hipEventElapsedTime(&ms, e0, e1));
  printf("hipMemcpy2DAsync D2D %d x %d floats: %.2f us per copy (events, back to back), %.1f MB moved, %.2f TB/s\n", B, R * N, ms * 1e3 / reps,
         2 * dst_bytes / 1e6, 2 * dst_bytes / (ms * 1e3 / reps) / 1e6);
  (void)hipFree(src); (void)hipFree(dst); (void)hipFree(pri); (void)hipFree(tab);
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipStreamDestroy(st);
  return 0;
}
