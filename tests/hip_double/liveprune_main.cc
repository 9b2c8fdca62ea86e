// Driver of tests/test_host_live_prune_own.py: the real wfst_capi.cc and wfst_capi_liveprune.cc linked against the HIP double
// (fake_hip.cc), under AddressSanitizer + UBSan -- who owns the snapshot scratch of wfst_decoder_set_live_lattice_prune, and what a
// failed allocation leaves behind.  Prints one line per check; returns the number of checks that failed.
#include <cstdio>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/wfst_decoder.h"
#include "fake_hip.h"

namespace {
int failed = 0;
void check(bool ok, const char *what) {
  printf("%s %s\n", ok ? "ok" : "FAILED", what);
  if (!ok) ++failed;
}

int make_graph(wfst_graph **out) {   // (own_main.cc's six-state graph)
  const wfst_state_info st[6] = {{2, 0, 0}, {2, 1, 0}, {1, 0, 0}, {2, 1, 0}, {1, 0, 0}, {0, 0, 0}};
  const wfst_arc arcs[8] = {{1, 1, 0.5f, 1}, {2, 0, 1.0f, 2}, {0, 0, 0.25f, 2}, {3, 2, 0.5f, 3}, {1, 3, 0.75f, 3},
                            {0, 0, 0.125f, 4}, {2, 0, 0.5f, 5}, {3, 1, 1.5f, 5}};
  int rc = wfst_graph_from_arrays(0, 5, 6, 8, st, arcs, 0, out);
  if (rc != WFST_OK) return rc;
  const int32_t tid2pdf[4] = {0, 1, 2, 3};
  return wfst_graph_set_tid2pdf(*out, tid2pdf, 3);
}

wfst_decoder *make_decoder(wfst_graph *g, int64_t lattice_links, int32_t channels) {
  wfst_config cfg;
  wfst_config_default(&cfg);
  wfst_limits lim;
  memset(&lim, 0, sizeof(lim));
  lim.max_frames = 64;
  lim.max_tokens_per_frame = 256;
  lim.arena_tokens = 4096;
  lim.lattice_links = lattice_links;
  wfst_decoder *d = nullptr;
  if (wfst_decoder_create_biglm(g, &cfg, channels, &lim, nullptr, nullptr, nullptr, nullptr, &d) != WFST_OK) return nullptr;
  return d;
}
}  // namespace

int main() {
  long base[kFakeKinds];
  for (int k = 0; k < kFakeKinds; ++k) base[k] = fake_hip_live(k);
  wfst_graph *g = nullptr;
  check(make_graph(&g) == WFST_OK, "graph");
  int32_t mode = 7;
  int64_t bytes = 7;

  // argument and state errors
  check(wfst_decoder_set_live_lattice_prune(nullptr, 1) == WFST_E_ARG, "NULL decoder: WFST_E_ARG");
  check(wfst_decoder_get_live_lattice_prune(nullptr, &mode, &bytes) == WFST_E_ARG && mode == 7 && bytes == 7, "NULL decoder (getter): WFST_E_ARG, outputs untouched");
  wfst_decoder *best = make_decoder(g, 0, 2);
  check(best != nullptr, "best-path decoder");
  check(wfst_decoder_set_live_lattice_prune(best, 1) == WFST_E_STATE, "no lattice_links: WFST_E_STATE");
  check(wfst_decoder_get_live_lattice_prune(best, &mode, &bytes) == WFST_E_STATE, "no lattice_links (getter): WFST_E_STATE");
  wfst_decoder_free(best);

  const int32_t B = 3;
  wfst_decoder *d = make_decoder(g, 4096, B);
  check(d != nullptr, "lattice decoder");
  std::vector<float> rows(8 * 16);
  std::vector<const float *> ll((size_t)B, rows.data());
  std::vector<int32_t> ready((size_t)B, 5);
  check(wfst_decoder_init(d, nullptr, 0) == WFST_OK && wfst_decoder_advance(d, nullptr, 0, ll.data(), ready.data(), 8, -1) == WFST_OK, "init + advance");
  check(wfst_decoder_get_live_lattice_prune(d, &mode, &bytes) == WFST_OK && mode == 0 && bytes == 0, "default: mode 0, no scratch");
  check(wfst_decoder_set_live_lattice_prune(d, 2) == WFST_E_ARG && wfst_decoder_set_live_lattice_prune(d, -1) == WFST_E_ARG, "mode outside {0, 1}: WFST_E_ARG");
  check(wfst_decoder_set_live_lattice_prune(d, 0) == WFST_OK && fake_hip_created() >= 0, "mode 0 -> 0: nothing to do");

  // the scratch cannot be allocated: the error comes back, the mode stays 0, nothing is held
  const long dev_before = fake_hip_live(kFakeDevice);
  fake_hip_fail_at(1);
  const int rc = wfst_decoder_set_live_lattice_prune(d, 1);
  check(fake_hip_fault_hit() != 0 && (rc == WFST_E_CAPACITY || rc == WFST_E_DEVICE), "failed allocation: the setter returns the error");
  fake_hip_fail_at(0);
  check(wfst_decoder_get_live_lattice_prune(d, &mode, &bytes) == WFST_OK && mode == 0 && bytes == 0, "failed allocation: mode stays 0, no scratch");
  check(fake_hip_live(kFakeDevice) == dev_before, "failed allocation: no device buffer more than before");

  // first use allocates once; the scratch stays with the decoder whatever the mode
  check(wfst_decoder_set_live_lattice_prune(d, 1) == WFST_OK, "mode 1");
  check(fake_hip_live(kFakeDevice) == dev_before + 1, "mode 1: one device buffer more");
  check(wfst_decoder_get_live_lattice_prune(d, &mode, &bytes) == WFST_OK && mode == 1 && bytes == (int64_t)8 * 4096 * B, "mode 1: 8 bytes x arena_tokens x channels");
  check(wfst_decoder_get_live_lattice_prune(d, nullptr, nullptr) == WFST_OK, "getter: both outputs may be NULL");
  check(wfst_decoder_set_live_lattice_prune(d, 0) == WFST_OK && wfst_decoder_set_live_lattice_prune(d, 1) == WFST_OK && fake_hip_live(kFakeDevice) == dev_before + 1,
        "mode 1 -> 0 -> 1: the same scratch");
  check(wfst_decoder_finalize(d, nullptr, 0) == WFST_OK, "finalize in mode 1");
  wfst_decoder_free(d);
  wfst_graph_free(g);
  bool clean = true;
  for (int k = 0; k < kFakeKinds; ++k) clean = clean && fake_hip_live(k) == base[k];
  check(clean, "everything given back");
  printf("failed %d\n", failed);
  return failed;
}
