// Driver of the ownership test (tests/test_host_ownership.py): the real wfst_capi.cc linked against the HIP double (fake_hip.cc).
//   own_main lifecycle   every decoder kind through create .. free once; prints the creating calls it made and what is still live
//   own_main sweep       the same sequence with the k-th creating call failing, k = 1, 2, .. until a run completes unfaulted
// One line per kind; exit status 1 if anything stayed live or a faulted run did not come back as a device error.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/wfst_decoder.h"
#include "fake_hip.h"

namespace {

enum Kind { kBest = 0, kLattice, kBiglm, kKinds };
const char *const kKindNames[kKinds] = {"best", "lattice", "biglm"};

struct Run {
  wfst_graph *g = nullptr;
  wfst_lm *lm_old = nullptr, *lm_new = nullptr;
  wfst_decoder *d = nullptr;
  hipStream_t user_stream = nullptr;   // the lattice decoder runs on a stream of its caller's
  float *pinned = nullptr;
  const char *step = "";
};

// six states, start 0, final 5; states 1 and 3 have an epsilon arc out (first, as the flat format wants); ilabels 1..3, olabels 0..3
int make_graph(wfst_graph **out) {
  const wfst_state_info st[6] = {{2, 0, 0}, {2, 1, 0}, {1, 0, 0}, {2, 1, 0}, {1, 0, 0}, {0, 0, 0}};
  const wfst_arc arcs[8] = {{1, 1, 0.5f, 1}, {2, 0, 1.0f, 2}, {0, 0, 0.25f, 2}, {3, 2, 0.5f, 3}, {1, 3, 0.75f, 3},
                            {0, 0, 0.125f, 4}, {2, 0, 0.5f, 5}, {3, 1, 1.5f, 5}};
  int rc = wfst_graph_from_arrays(0, 5, 6, 8, st, arcs, 0, out);
  if (rc != WFST_OK) return rc;
  const int32_t tid2pdf[4] = {0, 1, 2, 3}, tid2phone[4] = {0, 1, 2, 2};
  rc = wfst_graph_set_tid2pdf(*out, tid2pdf, 3);
  if (rc != WFST_OK) return rc;
  return wfst_graph_set_tid2phone(*out, tid2phone, 3);
}

// a bigram LM over words 0..3 (<s> = 1, </s> = 2): the empty history with an arc per word, one history state that backs off to it
int make_lm(float scale, wfst_lm **out) {
  const wfst_lm_state st[2] = {{4, 0.0f, 0}, {2, 0.5f, 0}};
  const wfst_lm_arc arcs[6] = {{0, 1.0f, 0}, {1, 1.0f, 1}, {2, 1.0f, 0}, {3, 1.0f, 1}, {2, 0.5f, 0}, {3, 0.25f, 1}};
  return wfst_lm_from_arrays(1, 2, 0, 2, st, 6, arcs, scale, 0, out);
}

constexpr int kStride = 8;

// create .. free of one decoder kind; stops at the first call that fails and returns its code
int sequence(Kind kind, Run &r) {
  int rc;
#define STEP(name, expr) do { r.step = name; rc = (expr); if (rc != WFST_OK) return rc; } while (0)
  STEP("graph", make_graph(&r.g));
  if (kind == kBiglm) {
    STEP("old lm", make_lm(1.0f, &r.lm_old));
    STEP("new lm", make_lm(0.5f, &r.lm_new));
  }
  if (kind == kLattice) STEP("caller's stream", hipStreamCreateWithFlags(&r.user_stream, hipStreamNonBlocking) == hipSuccess ? WFST_OK : WFST_E_DEVICE);
  const int32_t B = kind == kBest ? 128 : 2;   // 128 channels: three channel groups, their streams and events
  wfst_config cfg;
  wfst_config_default(&cfg);
  wfst_limits lim;
  memset(&lim, 0, sizeof(lim));
  lim.max_frames = 2048;   // (above 1024: the host-fed history is not allocated whole at first use)
  lim.max_tokens_per_frame = 256;
  lim.arena_tokens = 4096;
  lim.lattice_links = kind == kLattice ? 4096 : 0;
  lim.lm_pairs = 256;
  STEP("create", wfst_decoder_create_biglm(r.g, &cfg, B, &lim, nullptr, r.lm_old, r.lm_new, r.user_stream, &r.d));

  // first utterance: rows "on the device" (nothing reads them here)
  std::vector<float> rows((size_t)kStride * 16);
  std::vector<const float *> ll((size_t)B, rows.data());
  std::vector<int32_t> ready((size_t)B, 0);
  STEP("init", wfst_decoder_init(r.d, nullptr, 0));
  // frame counts that differ call by call: every one is a graph capture per channel group, and on the 128-channel decoder more
  // than the 64 executables its cache holds
  int frames = 0;
  for (int delta = 4; delta < (kind == kBest ? 28 : 7); ++delta) {
    frames += delta;
    std::fill(ready.begin(), ready.end(), frames);
    STEP("advance", wfst_decoder_advance(r.d, nullptr, 0, ll.data(), ready.data(), kStride, -1));
  }
  if (kind == kBest) {   // the lazily made results stream, its staging, and the endpoint buffers (what comes back is not looked at)
    const int32_t some[3] = {5, 0, 77}, sil[1] = {1};
    std::vector<int32_t> il(3 * 8), ol(3 * 8), nh(3);
    std::vector<float> gc(3 * 8), ac(3 * 8);
    STEP("best path enqueue", wfst_decoder_best_path_enqueue(r.d, some, 3, 1, 8));
    STEP("best path fetch", wfst_decoder_best_path_fetch(r.d, il.data(), ol.data(), gc.data(), ac.data(), nh.data()));
    wfst_endpoint_config ep;
    wfst_endpoint_config_default(&ep);
    ep.n_silence_phones = 1;
    ep.silence_phones = sil;
    STEP("endpoint config", wfst_decoder_set_endpoint_config(r.d, &ep));
  }
  STEP("finalize", wfst_decoder_finalize(r.d, nullptr, 0));

  // second utterance: rows handed over from the host, 300 frames and then 700 -- the history slab regrows
  const size_t per = (size_t)700 * kStride;
  std::vector<float> pageable;
  const float *host = nullptr;
  if (kind == kLattice) {   // page-locked rows: the copies go through the copy stream's event
    r.step = "host alloc";
    r.pinned = (float *)wfst_host_alloc((size_t)B * per * sizeof(float));
    if (!r.pinned) return WFST_E_DEVICE;
    host = r.pinned;
  } else {
    pageable.assign((size_t)B * per, -1.0f);
    host = pageable.data();
  }
  for (int32_t c = 0; c < B; ++c) ll[(size_t)c] = host + (size_t)c * per;
  STEP("init again", wfst_decoder_init(r.d, nullptr, 0));
  std::fill(ready.begin(), ready.end(), 300);
  STEP("advance_host 300", wfst_decoder_advance_host(r.d, nullptr, 0, ll.data(), ready.data(), kStride, -1));
  std::fill(ready.begin(), ready.end(), 700);
  STEP("advance_host 700", wfst_decoder_advance_host(r.d, nullptr, 0, ll.data(), ready.data(), kStride, -1));
  STEP("finalize again", wfst_decoder_finalize(r.d, nullptr, 0));
#undef STEP
  r.step = "done";
  return WFST_OK;
}

// gives back what was handed out, whatever the sequence got to
void release(Run &r) {
  wfst_decoder_free(r.d);
  wfst_lm_free(r.lm_old);
  wfst_lm_free(r.lm_new);
  wfst_graph_free(r.g);
  wfst_host_free(r.pinned);
  if (r.user_stream) (void)hipStreamDestroy(r.user_stream);
}

// what is live beyond `base` (and raises base to it: a leak is reported once)
std::string live_beyond(long base[kFakeKinds]) {
  std::string s;
  for (int k = 0; k < kFakeKinds; ++k) {
    const long n = fake_hip_live(k);
    if (n != base[k]) s += std::string(" ") + fake_hip_kind_name(k) + "+" + std::to_string(n - base[k]);
    base[k] = n;
  }
  return s;
}

}  // namespace

int main(int argc, char **argv) {
  const bool sweep = argc > 1 && !strcmp(argv[1], "sweep");
  if (argc != 2 || (!sweep && strcmp(argv[1], "lifecycle"))) { fprintf(stderr, "usage: own_main lifecycle|sweep\n"); return 2; }
  setvbuf(stdout, nullptr, _IOLBF, 0);   // (a run may end in the double's abort: what was found until then is on record)
  long base[kFakeKinds] = {0, 0, 0, 0, 0, 0};
  int bad = 0;
  for (int kind = 0; kind < kKinds; ++kind) {
    if (!sweep) {
      fake_hip_fail_at(0);
      Run r;
      const int rc = sequence((Kind)kind, r);
      release(r);
      const std::string live = live_beyond(base);
      printf("lifecycle %s rc %d creating %ld live%s\n", kKindNames[kind], rc, fake_hip_created(), live.empty() ? " 0" : live.c_str());
      if (rc != WFST_OK) printf("  failed at %s: %s\n", r.step, wfst_last_error());
      bad += rc != WFST_OK || !live.empty();
      continue;
    }
    long k = 1, leaks = 0, wrong_rc = 0;
    for (;; ++k) {
      fake_hip_fail_at(k);
      Run r;
      const int rc = sequence((Kind)kind, r);
      const bool hit = fake_hip_fault_hit() != 0;
      release(r);
      const std::string live = live_beyond(base);
      if (!live.empty()) { ++leaks; printf("  LEAK %s k=%ld at %s (%s):%s\n", kKindNames[kind], k, r.step, wfst_last_error(), live.c_str()); }
      if (!hit) {
        if (rc != WFST_OK) { ++wrong_rc; printf("  the unfaulted run of %s failed at %s: %s\n", kKindNames[kind], r.step, wfst_last_error()); }
        break;
      }
      if (rc != WFST_E_DEVICE) { ++wrong_rc; printf("  WRONG RC %s k=%ld at %s: %d\n", kKindNames[kind], k, r.step, rc); }
    }
    printf("sweep %s faulted %ld leaks %ld wrong_rc %ld\n", kKindNames[kind], k - 1, leaks, wrong_rc);
    bad += leaks != 0 || wrong_rc != 0;
  }
  return bad ? 1 : 0;
}
