// Driver of GpuChannelPool's partial-words request kind over the C-ABI test double (fake_partial.cc), built with -fsanitize=thread:
// N threads x one GpuLatticeDecoder(pool) each x ragged utterances fed in chunks; between the chunks every thread asks for its
// partial words.  Every answer must be the asking channel's own at its own frame count (the double derives the words from both),
// the batcher must never have a second list outstanding, must issue at most one list per pass, and must have batched.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>

#include "../../asr-decoder_amd/host/wfst-host.h"

using namespace datemoon;
extern "C" long long fake_partial_count(int k);

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
  const int n_threads = argc > 1 ? atoi(argv[1]) : 16, n_utts = argc > 2 ? atoi(argv[2]) : 96, chunk = 5;
  std::vector<Utt> utts((size_t)n_utts);
  unsigned seed = 4321;
  auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return (seed >> 8) & 0xFFFF; };
  for (Utt &u : utts) {
    u.frames = 1 + (int)(rnd() % 60);
    u.cols = 9;
    u.m.resize((size_t)u.frames * u.cols);
    for (float &x : u.m) x = (float)(rnd() % 1000) / 37.0f;
  }
  LatticeFasterDecoderConfig cfg;
  Fst fst;   // (never read: the test double ignores the graph)
  GpuChannelPool pool(&fst, cfg, n_threads, nullptr, /*linger_us=*/20);
  std::atomic<size_t> next(0);
  std::atomic<int> bad(0), misuse_caught(0);
  std::atomic<long long> asked(0);
  auto worker = [&](int k) {
    GpuLatticeDecoder dec(&pool);
    std::vector<int> w;
    int ns = -1;
    if (k == 0) {   // misuse: partial words before InitDecoding -- this thread's exception, nobody else's
      try { dec.GetPartialWords(&w, &ns); bad++; } catch (const std::runtime_error &) { misuse_caught++; }
    }
    int chan = -1;
    for (;;) {
      const size_t ui = next.fetch_add(1);
      if (ui >= utts.size()) return;
      const Utt &u = utts[ui];
      Pull p(u);
      dec.InitDecoding();
      if (!dec.GetPartialWords(&w, &ns)) { if (!w.empty() || ns != 0) bad++; } else bad++;   // no frame decoded: nothing, and false
      asked++;
      for (int ready = chunk;; ready += chunk) {
        p.SetReady(ready);
        dec.AdvanceDecoding(&p);
        if (ready >= u.frames) break;
        if (!dec.GetPartialWords(&w, &ns)) bad++;
        asked++;
        const int rows = ready;
        if ((int)w.size() != 1 + rows / 3 || ns != rows / 6) { bad++; continue; }
        if (chan < 0) chan = w[0];   // (the channel this object leased, learnt from its first answer)
        if (w[0] != chan) bad++;
        for (size_t q = 1; q < w.size(); ++q)
          if (w[q] != 8 * rows + (int)q) { bad++; break; }
      }
      dec.FinalizeDecoding();
      Lattice best;
      if (!dec.GetBestPath(&best)) { bad++; continue; }
      std::vector<int> words, phones;
      float tot = 0, lm = 0;
      LatticeToVector(best, words, phones, tot, lm);
      if (chan >= 0 && (words.empty() || words[0] != chan)) bad++;   // (the double's best path carries channel + 1 too)
    }
  };
  std::vector<std::thread> th;
  for (int k = 1; k < n_threads; ++k) th.emplace_back(worker, k);
  worker(0);
  for (std::thread &t : th) t.join();
  const GpuChannelPool::Stats st = pool.GetStats();
  printf("bad %d misuse_caught %d asked %lld partial_requests %lld partial_calls %lld max_per_pass %lld fake_enqueues %lld fake_overlapping %lld batches %lld\n",
         bad.load(), misuse_caught.load(), asked.load(), st.partial_requests, st.partial_calls, st.partial_max_per_pass, fake_partial_count(0),
         fake_partial_count(1), st.batches);
  if (bad.load() != 0 || misuse_caught.load() != 1) return 1;
  if (fake_partial_count(1) != 0 || st.partial_max_per_pass > 1) return 2;
  return 0;
}
