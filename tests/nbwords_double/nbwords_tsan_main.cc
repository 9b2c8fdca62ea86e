// Driver of GpuChannelPool's kNbestWords request over the C-ABI test double (fake_wfstdec_nbwords.cc), built with -fsanitize=thread:
// N threads x one GpuLatticeDecoder(pool) each x ragged utterances in chunks; after every chunk the thread asks GetNbestWords with
// one of two (n, use_final_probs) questions.  Every answer must name the asking thread's channel, its frames and its question; the
// batcher must have grouped (fewer calls than requests, and no call mixing two questions: the double echoes the question).
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <thread>
#include <vector>

#include "../../asr-decoder_amd/host/wfst-host.h"

using namespace datemoon;
extern "C" long long fake_nbw_calls(int what);

namespace {
struct Utt { int frames, cols; std::vector<float> m; };
class Pull : public DecodableInterface {
 public:
  explicit Pull(const Utt &u) : _u(u), _ready(0) {}
  float LogLikelihood(int f, int i) override { return _u.m[(size_t)f * _u.cols + i]; }
  bool IsLastFrame(int f) const override { return f == _u.frames - 1; }
  int NumFramesReady() const override { return _ready; }
  int NumIndices() const override { return _u.cols - 1; }
  void SetReady(int n) { _ready = n < _u.frames ? n : _u.frames; }
 private:
  const Utt &_u;
  int _ready;
};
}  // namespace

int main(int argc, char **argv) {
  const int n_threads = argc > 1 ? atoi(argv[1]) : 16, n_utts = argc > 2 ? atoi(argv[2]) : 64, chunk = 5;
  std::vector<Utt> utts((size_t)n_utts);
  unsigned seed = 4321;
  auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return (seed >> 8) & 0xFFFF; };
  for (Utt &u : utts) {
    u.frames = 6 + (int)(rnd() % 30);
    u.cols = 9;
    u.m.resize((size_t)u.frames * u.cols);
    for (float &x : u.m) x = (float)(rnd() % 1000) / 37.0f;
  }
  LatticeFasterDecoderConfig cfg;
  Fst fst;   // (never read: the test double ignores the graph)
  GpuChannelPool pool(&fst, cfg, n_threads, nullptr, /*linger_us=*/20);
  std::atomic<size_t> next(0);
  std::atomic<int> bad(0);
  std::atomic<long long> asked(0);
  auto worker = [&](int k) {
    GpuLatticeDecoder dec(&pool);
    for (;;) {
      const size_t ui = next.fetch_add(1);
      if (ui >= utts.size()) return;
      const Utt &u = utts[ui];
      Pull p(u);
      dec.InitDecoding();
      for (int ready = chunk;; ready += chunk) {
        p.SetReady(ready);
        dec.AdvanceDecoding(&p);
        if (ready >= u.frames) break;
        const int n = (k % 2) ? 5 : 1;   // two questions among the threads: two groups per batcher pass at most
        std::vector<std::vector<int> > w;
        std::vector<float> t, l;
        int st = -99;
        const bool any = dec.GetNbestWords(&w, &t, &l, n, false, nullptr, nullptr, &st);
        asked++;
        if (!any || st != WFST_OK || (int)w.size() != (n < 2 ? n : 2) || t.size() != w.size() || l.size() != w.size()) { bad++; continue; }
        for (const std::vector<int> &x : w)
          if (x.size() != 4 || x[1] != dec.NumFramesDecoded() || x[2] != 2 * n || x[3] != 5) bad++;
        if (w[0][0] != w.back()[0]) bad++;   // (one channel answered both paths)
      }
      dec.FinalizeDecoding();
      std::vector<std::vector<int> > w;
      if (dec.GetNbestWords(&w, nullptr, nullptr, 3, false)) bad++;   // finalized, without final-probs: no lattice
      asked++;
      Lattice best;
      if (!dec.GetBestPath(&best)) bad++;
    }
  };
  std::vector<std::thread> th;
  for (int k = 1; k < n_threads; ++k) th.emplace_back(worker, k);
  worker(0);
  for (std::thread &t : th) t.join();
  const GpuChannelPool::Stats st = pool.GetStats();
  printf("bad %d asked %lld requests %lld calls %lld fake_calls %lld fake_channels %lld\n", bad.load(), asked.load(), st.nbest_words_requests,
         st.nbest_words_calls, fake_nbw_calls(0), fake_nbw_calls(1));
  if (bad.load() != 0 || st.nbest_words_requests != asked.load() || fake_nbw_calls(1) != asked.load() || fake_nbw_calls(0) != st.nbest_words_calls) return 1;
  // it grouped: a pass issues one call per distinct question, so sixteen threads asking two questions need fewer calls than requests
  // (how many fewer is the threads' timing; that requests shared calls at all is the property)
  if (n_threads >= 8 && st.nbest_words_calls >= st.nbest_words_requests) return 2;
  return 0;
}
