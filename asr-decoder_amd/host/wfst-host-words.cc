// Words with times of the best path (wfst_decoder_get_words: words_kernel) for the two decoder classes of wfst-host.h: what the
// reference's services deliver per utterance -- OnebestLatticeToString's words, tot_score and lm_score
// (kaldi-nnet3/kaldi-online-nnet3-my-decoder.cc:107-121) and AlignStruct's (start, end) per word
// (gpu-asr/gpu-worker-pool-itf.h:85-97) -- in frames.  A translation unit of its own: wfst-host.cc is also linked against doubles
// of the C ABI that end at the calls it makes.
#include "wfst-host.h"

#include <algorithm>
#include <stdexcept>
#include <string>

namespace datemoon {

static void FatalWords(const char *what) { throw std::runtime_error(std::string(what) + ": " + wfst_last_error()); }

void GpuBatchDecoder::SetSilencePhones(const std::vector<int> &phones) {
  const std::vector<int32_t> p(phones.begin(), phones.end());
  if (wfst_decoder_set_silence_phones(_dec, p.empty() ? nullptr : p.data(), (int32_t)p.size()) != WFST_OK) FatalWords("SetSilencePhones");
}

void GpuBatchDecoder::GetWords(const std::vector<int> &channels, std::vector<std::vector<int> > *words,
                               std::vector<std::vector<std::pair<int, int> > > *frames, std::vector<float> *tot, std::vector<float> *lm,
                               std::vector<bool> *ok, bool use_final_probs) {
  std::vector<int32_t> ch(channels.begin(), channels.end());
  if (ch.empty())
    for (int c = 0; c < _n; ++c) ch.push_back(c);
  const int32_t cnt = (int32_t)ch.size();
  int32_t cap = 64;
  for (int32_t c : ch) cap = std::max(cap, NumFramesDecoded(c) / 4 + 64);
  std::vector<int32_t> nw((size_t)cnt), nh((size_t)cnt);
  std::vector<float> t((size_t)cnt), l((size_t)cnt);
  for (int attempt = 0; attempt < 2; ++attempt) {
    std::vector<int32_t> w((size_t)cnt * cap), b((size_t)cnt * cap), e((size_t)cnt * cap);
    const int rc = wfst_decoder_get_words(_dec, ch.data(), cnt, use_final_probs ? 1 : 0, cap, w.data(), b.data(), e.data(), nw.data(), nh.data(),
                                          t.data(), l.data());
    if (rc == WFST_E_CAPACITY && attempt == 0 && *std::max_element(nw.begin(), nw.end()) > cap) {
      cap = *std::max_element(nw.begin(), nw.end());
      continue;
    }
    if (rc == WFST_E_STATE) throw std::runtime_error(wfst_last_error());  // reference: LOG_ERR
    if (rc != WFST_OK) FatalWords("GetWords");
    if (words) words->assign((size_t)cnt, std::vector<int>());
    if (frames) frames->assign((size_t)cnt, std::vector<std::pair<int, int> >());
    for (int32_t i = 0; i < cnt; ++i) {
      const size_t o = (size_t)i * cap;
      if (words) (*words)[(size_t)i].assign(w.begin() + o, w.begin() + o + nw[(size_t)i]);
      if (frames)
        for (int32_t k = 0; k < nw[(size_t)i]; ++k) (*frames)[(size_t)i].push_back(std::make_pair((int)b[o + k], (int)e[o + k]));
    }
    break;
  }
  if (tot) tot->assign(t.begin(), t.end());
  if (lm) lm->assign(l.begin(), l.end());
  if (ok) {
    ok->assign((size_t)cnt, false);
    for (int32_t i = 0; i < cnt; ++i) (*ok)[(size_t)i] = nh[(size_t)i] > 0;
  }
}

void GpuLatticeDecoder::SetSilencePhones(const std::vector<int> &phones) {
  if (_pool) throw std::runtime_error("SetSilencePhones: not served over a channel pool (word ends are the next word's begin there)");
  const std::vector<int32_t> p(phones.begin(), phones.end());
  if (wfst_decoder_set_silence_phones(_dec, p.empty() ? nullptr : p.data(), (int32_t)p.size()) != WFST_OK) FatalWords("SetSilencePhones");
}

bool GpuLatticeDecoder::GetWords(std::vector<int> *words, std::vector<std::pair<int, int> > *frames, float *tot, float *lm,
                                 bool use_final_probs) {
  if (words) words->clear();
  if (frames) frames->clear();
  float t = 0.0f, l = 0.0f;
  bool ok = false;
  if (_pool) {
    // over a pool the channel's best path is one of the batcher's list (GetBestPath); the same result from its hops, on the host
    Lattice best;
    ok = GetBestPath(&best, use_final_probs);
    int frame = 0;
    for (StateId s = best.Start(); ok && s != kNoStateId;) {
      LatticeState *st = best.GetState(s);
      if (st->GetArcSize() == 0) break;
      const LatticeArc *a = st->GetArc(0);
      if (a->_output != 0) {
        if (frames && !frames->empty()) frames->back().second = frame;
        if (words) words->push_back(a->_output);
        if (frames) frames->push_back(std::make_pair(frame, frame));
      }
      l += a->_w.Value1();
      t += a->_w.Value1() + a->_w.Value2();
      if (a->_input != 0) ++frame;
      s = a->_to;
    }
    if (frames && !frames->empty()) frames->back().second = frame;
  } else {
    const int32_t c = 0;
    int32_t cap = std::max(1, NumFramesDecoded()) / 4 + 64, nw = 0, nh = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
      std::vector<int32_t> w((size_t)cap), b((size_t)cap), e((size_t)cap);
      const int rc = wfst_decoder_get_words(_dec, &c, 1, use_final_probs ? 1 : 0, cap, w.data(), b.data(), e.data(), &nw, &nh, &t, &l);
      if (rc == WFST_E_CAPACITY && nw > cap && attempt == 0) { cap = nw; continue; }
      if (rc == WFST_E_STATE) throw std::runtime_error(wfst_last_error());  // reference: LOG_ERR
      if (rc != WFST_OK) FatalWords("GetWords");
      if (words) words->assign(w.begin(), w.begin() + nw);
      if (frames)
        for (int32_t k = 0; k < nw; ++k) frames->push_back(std::make_pair((int)b[(size_t)k], (int)e[(size_t)k]));
      break;
    }
    ok = nh > 0;
  }
  if (tot) *tot = t;
  if (lm) *lm = l;
  return ok;
}

}  // namespace datemoon
