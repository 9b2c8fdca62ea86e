// Implementation of wfst-host.h: thin C++ over the C ABI.  No decoding happens on the host.
#include "wfst-host.h"

#include <atomic>
#include <thread>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <iostream>
#include <sstream>
#include <tuple>

// wfst_decoder_get_nbest_words is referenced weakly: this file is also linked against doubles of the C ABI that end at the calls
// it made before (the pool's and the partial words' sanitizer harnesses); there the n-best text reports itself missing.
#pragma weak wfst_decoder_get_nbest_words
// ... and so are the pruned live lattices' two calls: SetLiveLatticePrune reports itself missing there
#pragma weak wfst_decoder_set_live_lattice_prune
#pragma weak wfst_decoder_get_live_lattice_prune
// ... and the word alignment's: AlignWords reports itself missing there
#pragma weak wfst_decoder_align_words
// ... and the lattice edit distance's: NearestWords reports itself missing there
#pragma weak wfst_decoder_nearest_words
#pragma weak wfst_decoder_word_confidence
#pragma weak wfst_decoder_sequence_posterior
#pragma weak wfst_decoder_word_alternatives
#pragma weak wfst_decoder_frame_posteriors
#pragma weak wfst_decoder_rescaled_words
#pragma weak wfst_bias_lists_create
#pragma weak wfst_bias_lists_free
#pragma weak wfst_decoder_biased_words
#pragma weak wfst_bias_books_create
#pragma weak wfst_bias_books_free
#pragma weak wfst_decoder_biased_words_sparse
#pragma weak wfst_decoder_sequence_stats
#pragma weak wfst_decoder_force_align
#pragma weak wfst_align_graphs_load
#pragma weak wfst_align_graphs_free
#pragma weak wfst_decoder_graph_posteriors

namespace datemoon {

namespace {
[[noreturn]] void Fatal(const std::string &what) { throw std::runtime_error(what + ": " + wfst_last_error()); }
// (one stdio call per line: the worker threads of a service share stderr, and a line put together by several << would interleave)
void Warn(const std::string &msg) { const std::string line = "WARNING (wfst) " + msg + "\n"; fputs(line.c_str(), stderr); fflush(stderr); }

// hop list (start->final order) -> the linear Lattice the reference's GetBestPath builds
// (base-inl.h:1080-1091): last state = start, state 0 = final.
void HopsToLattice(const int32_t *il, const int32_t *ol, const float *g, const float *ac, int n, Lattice *ofst) {
  ofst->DeleteStates();
  StateId state = ofst->AddState();
  ofst->SetFinal(state);
  for (int k = n - 1; k >= 0; --k) {
    StateId ns = ofst->AddState();
    ofst->AddArc(ns, LatticeArc(il[k], ol[k], state, LatticeWeight(g[k], ac[k])));
    state = ns;
  }
  ofst->SetStart(state);
}
}  // namespace

// ---- config -------------------------------------------------------------------------------
void LatticeFasterDecoderConfig::ReadConfigFile(const std::string &path) {
  std::ifstream in(path.c_str());
  if (!in) throw std::runtime_error("cannot open config file " + path);
  std::string line;
  while (std::getline(in, line)) {
    size_t h = line.find('#');
    if (h != std::string::npos) line.erase(h);
    size_t b = line.find_first_not_of(" \t\r\n");
    if (b == std::string::npos) continue;
    line = line.substr(b, line.find_last_not_of(" \t\r\n") - b + 1);
    if (line.compare(0, 2, "--") != 0) throw std::runtime_error("bad config line: " + line);
    size_t eq = line.find('=');
    if (eq == std::string::npos) throw std::runtime_error("bad config line (no '='): " + line);
    std::string name = line.substr(2, eq - 2), val = line.substr(eq + 1);
    std::replace(name.begin(), name.end(), '_', '-');
    if (name == "beam") _beam = (float)atof(val.c_str());
    else if (name == "max-active") _max_active = atoi(val.c_str());
    else if (name == "min-active") _min_active = atoi(val.c_str());
    else if (name == "lattice-beam") _lattice_beam = (float)atof(val.c_str());
    else if (name == "prune-interval") _prune_interval = atoi(val.c_str());
    else if (name == "beam-delta") _beam_delta = (float)atof(val.c_str());
    else if (name == "hash-ratio") _hash_ratio = (float)atof(val.c_str());
    else if (name == "determinize-lattice") _determinize_lattice = (val == "true" || val == "1");
    else if (name.compare(0, 9, "endpoint.") == 0) continue;   // OnlineEndpointConfig's lines (a service keeps one config file)
    else throw std::runtime_error("unknown decoder option --" + name);
  }
}

void LatticeFasterDecoderConfig::Check() const {
  if (!(_beam > 0.0 && _max_active > 1 && _lattice_beam > 0.0 && _prune_interval > 0 && _beam_delta > 0.0 &&
        _hash_ratio >= 1.0 && _prune_scale > 0.0 && _prune_scale < 1.0))
    throw std::runtime_error("LatticeFasterDecoderConfig::Check failed");
}

wfst_config LatticeFasterDecoderConfig::ToC() const {
  wfst_config c;
  c.beam = _beam;
  c.max_active = _max_active;
  c.min_active = _min_active;
  c.lattice_beam = _lattice_beam;
  c.prune_interval = _prune_interval;
  c.beam_delta = _beam_delta;
  c.hash_ratio = _hash_ratio;
  c.prune_scale = _prune_scale;
  return c;
}

// ---- graph ----------------------------------------------------------------------------------
Fst::~Fst() { wfst_graph_free(_graph); }

bool Fst::ReadFst(const char *file, int device) {
  wfst_graph_free(_graph);
  _graph = nullptr;
  if (wfst_graph_load(file, device, &_graph) != WFST_OK) {
    std::cerr << "ReadFst " << file << " failed: " << wfst_last_error() << std::endl;
    return false;
  }
  wfst_graph_info(_graph, &_start, &_final, &_states, &_arcs, nullptr);
  return true;
}

void Fst::SetTid2Pdf(const std::vector<int32_t> &m) {
  if (!_graph) throw std::runtime_error("SetTid2Pdf before ReadFst");
  if (wfst_graph_set_tid2pdf(_graph, m.data(), (int32_t)m.size() - 1) != WFST_OK) Fatal("wfst_graph_set_tid2pdf");
  _tid2pdf = m;
}

void Fst::SetTid2Phone(const std::vector<int32_t> &m) {
  if (!_graph) throw std::runtime_error("SetTid2Phone before ReadFst");
  if (m.size() < 2 || wfst_graph_set_tid2phone(_graph, m.data(), (int32_t)m.size() - 1) != WFST_OK) Fatal("wfst_graph_set_tid2phone");
}

// ---- OnlineEndpointConfig ---------------------------------------------------------------------
static bool ParseBool(const std::string &v, const std::string &name) {
  if (v == "true" || v == "1") return true;
  if (v == "false" || v == "0") return false;
  throw std::runtime_error("bad boolean for --" + name + ": " + v);
}
static float ParseFloat(const std::string &v, const std::string &name) {
  if (v == "inf" || v == "+inf" || v == "infinity") return std::numeric_limits<float>::infinity();
  char *end = nullptr;
  const float f = strtof(v.c_str(), &end);
  if (v.empty() || *end) throw std::runtime_error("bad number for --" + name + ": " + v);
  return f;
}
bool OnlineEndpointConfig::ParseOption(const std::string &arg) {
  if (arg.compare(0, 11, "--endpoint.") != 0) return false;
  const size_t eq = arg.find('=');
  if (eq == std::string::npos) throw std::runtime_error("option without '=': " + arg);
  std::string name = arg.substr(2, eq - 2);
  const std::string val = arg.substr(eq + 1);
  std::replace(name.begin(), name.end(), '_', '-');
  if (name == "endpoint.silence-phones") { silence_phones = val; return true; }
  if (name == "endpoint.frame-shift") { frame_shift = ParseFloat(val, name); return true; }
  OnlineEndpointRule *rules[5] = {&rule1, &rule2, &rule3, &rule4, &rule5};
  if (name.compare(0, 13, "endpoint.rule") == 0 && name.size() > 15 && name[13] >= '1' && name[13] <= '5' && name[14] == '.') {
    OnlineEndpointRule &r = *rules[name[13] - '1'];
    const std::string f = name.substr(15);
    if (f == "must-contain-nonsilence") r.must_contain_nonsilence = ParseBool(val, name);
    else if (f == "min-trailing-silence") r.min_trailing_silence = ParseFloat(val, name);
    else if (f == "max-relative-cost") r.max_relative_cost = ParseFloat(val, name);
    else if (f == "min-utterance-length") r.min_utterance_length = ParseFloat(val, name);
    else throw std::runtime_error("unknown endpoint option --" + name);
    return true;
  }
  throw std::runtime_error("unknown endpoint option --" + name);
}
void OnlineEndpointConfig::ReadConfigFile(const std::string &path) {
  std::ifstream in(path.c_str());
  if (!in) throw std::runtime_error("cannot open config file " + path);
  std::string line;
  while (std::getline(in, line)) {
    size_t h = line.find('#');
    if (h != std::string::npos) line.erase(h);
    size_t b = line.find_first_not_of(" \t\r\n");
    if (b == std::string::npos) continue;
    line = line.substr(b, line.find_last_not_of(" \t\r\n") - b + 1);
    if (line.compare(0, 2, "--") != 0) throw std::runtime_error("bad config line: " + line);
    (void)ParseOption(line);
  }
}
std::vector<int32_t> OnlineEndpointConfig::SilencePhones() const {
  std::vector<int32_t> v;
  size_t p = 0;
  while (p <= silence_phones.size() && !silence_phones.empty()) {
    size_t q = silence_phones.find(':', p);
    if (q == std::string::npos) q = silence_phones.size();
    const std::string tok = silence_phones.substr(p, q - p);
    char *end = nullptr;
    const long x = strtol(tok.c_str(), &end, 10);
    if (tok.empty() || *end) throw std::runtime_error("bad --endpoint.silence-phones: " + silence_phones);
    v.push_back((int32_t)x);
    p = q + 1;
  }
  wfst_endpoint_config c = ToCRaw(v);
  int32_t rule = 0;
  if (wfst_endpoint_rules(&c, 0, 0, 0.0f, &rule) != WFST_OK) Fatal("OnlineEndpointConfig");   // (the library's checks)
  return v;
}
wfst_endpoint_config OnlineEndpointConfig::ToCRaw(const std::vector<int32_t> &phones) const {
  wfst_endpoint_config c;
  const OnlineEndpointRule *rules[5] = {&rule1, &rule2, &rule3, &rule4, &rule5};
  for (int k = 0; k < 5; ++k)
    c.rule[k] = {rules[k]->must_contain_nonsilence ? 1 : 0, rules[k]->min_trailing_silence, rules[k]->max_relative_cost,
                 rules[k]->min_utterance_length};
  c.frame_shift = frame_shift;
  c.n_silence_phones = (int32_t)phones.size();
  c.silence_phones = phones.empty() ? nullptr : phones.data();
  return c;
}
wfst_endpoint_config OnlineEndpointConfig::ToC(std::vector<int32_t> *phones) const {
  *phones = SilencePhones();
  return ToCRaw(*phones);
}
// the bytes that tell two configs apart (what a decoder has set on the device is set again only when it changes)
static std::string EndpointKey(const wfst_endpoint_config &c) {
  std::string k((const char *)c.rule, sizeof(c.rule));
  k.append((const char *)&c.frame_shift, sizeof(c.frame_shift));
  k.append((const char *)c.silence_phones, (size_t)c.n_silence_phones * sizeof(int32_t));
  return k;
}

// ---- LatticeToVector --------------------------------------------------------------------------
bool LatticeToVector(Lattice &best_path, std::vector<int> &words, std::vector<int> &phones, float &tot, float &lm) {
  if (best_path.Start() == kNoStateId) return false;
  tot = 0;
  lm = 0;
  LatticeState *cur = best_path.GetState(best_path.Start());
  while (!cur->IsFinal()) {
    LatticeArc *arc = cur->GetArc(0);
    if (arc->_input != 0) phones.push_back(arc->_input);
    if (arc->_output != 0) words.push_back(arc->_output);
    lm += arc->_w.Value1();
    tot += arc->_w.Value1() + arc->_w.Value2();
    cur = best_path.GetState(arc->_to);
  }
  return true;
}

// ---- on-disk lattice (reference format, see wfst-host.h) ----------------------------------------
bool Lattice::Write(FILE *fp) {
  if (!fp) return false;
  const uint64_t n = _states.size();
  const int32_t start = _start;
  if (fwrite(&n, 8, 1, fp) != 1 || fwrite(&start, 4, 1, fp) != 1) {
    std::cerr << "Write lattice state number error." << std::endl;
    return false;
  }
  for (LatticeState &st : _states) {
    const int32_t fin = st.IsFinal() ? 1 : 0;
    const uint64_t na = st.GetArcSize();
    if (fwrite(&fin, 4, 1, fp) != 1 || fwrite(&na, 8, 1, fp) != 1) {
      std::cerr << "Write state error." << std::endl;
      return false;
    }
    for (unsigned i = 0; i < na; ++i) {
      const LatticeArc *a = st.GetArc(i);
      const int32_t lab[2] = {a->_input, a->_output};
      const float w[2] = {a->_w.Value1(), a->_w.Value2()};
      const int32_t to = a->_to;
      if (fwrite(lab, 4, 2, fp) != 2 || fwrite(w, 4, 2, fp) != 2 || fwrite(&to, 4, 1, fp) != 1) {
        std::cerr << "Write state arc error." << std::endl;
        return false;
      }
    }
  }
  return true;
}
bool Lattice::Write(const std::string &file) {
  FILE *fp = fopen(file.c_str(), "ab");
  if (!fp) {
    std::cerr << "Write " << file << " failed." << std::endl;
    return false;
  }
  const bool ok = Write(fp);
  fclose(fp);
  if (!ok) std::cerr << "Write " << file << " failed." << std::endl;
  return ok;
}
bool Lattice::Read(FILE *fp) {
  DeleteStates();
  if (!fp) return false;
  uint64_t n = 0;
  int32_t start = 0;
  if (fread(&n, 8, 1, fp) != 1 || fread(&start, 4, 1, fp) != 1) return false;  // also: clean end of file
  for (uint64_t s = 0; s < n; ++s) {
    int32_t fin = 0;
    uint64_t na = 0;
    if (fread(&fin, 4, 1, fp) != 1 || fread(&na, 8, 1, fp) != 1) {
      std::cerr << "Read state error." << std::endl;
      DeleteStates();
      return false;
    }
    const StateId id = AddState();
    if (fin) SetFinal(id);
    for (uint64_t i = 0; i < na; ++i) {
      int32_t lab[2], to;
      float w[2];
      if (fread(lab, 4, 2, fp) != 2 || fread(w, 4, 2, fp) != 2 || fread(&to, 4, 1, fp) != 1) {
        std::cerr << "Read state arc " << i << " error." << std::endl;
        DeleteStates();
        return false;
      }
      AddArc(id, LatticeArc(lab[0], lab[1], to, LatticeWeight(w[0], w[1])));
    }
  }
  _start = start;
  return true;
}
bool Lattice::Read(const std::string &file) {
  FILE *fp = fopen(file.c_str(), "rb");
  if (!fp) {
    std::cerr << "Open " << file << " failed." << std::endl;
    return false;
  }
  const bool ok = Read(fp);
  fclose(fp);
  if (!ok) std::cerr << "Read " << file << " failed." << std::endl;
  return ok;
}

// ---- language model (biglm) -------------------------------------------------------------------
ArpaLm::~ArpaLm() { wfst_lm_free(_lm); }
bool ArpaLm::Read(const char *file, int device) {
  wfst_lm_free(_lm);
  _lm = nullptr;
  _file = file;
  _device = device;
  if (wfst_lm_load(file, _scale, device, &_lm) != WFST_OK) {  // checks the file now; re-uploaded if Rescale follows
    std::cerr << "Read " << file << " failed: " << wfst_last_error() << std::endl;
    return false;
  }
  int32_t ns, na, nw;
  int64_t bytes;
  wfst_lm_info(_lm, &_bos, &_eos, &ns, &na, &nw, &bytes);
  return true;
}
void ArpaLm::Rescale(float scale) {  // arpa2fsa.cc:264-275: weights *= scale (applied when the automaton is uploaded)
  if (scale == 1.0f) return;
  _scale *= scale;
  wfst_lm_free(_lm);
  _lm = nullptr;
}
const wfst_lm *ArpaLm::Handle() {
  // several worker threads construct their decoders over the same two LMs at once (wfst-decode --inflight): the upload
  // happens once, under the lock, into a local that is published only when complete
  std::lock_guard<std::mutex> lock(_mu);
  if (!_lm) {
    if (_file.empty()) throw std::runtime_error("ArpaLm used before Read()");
    wfst_lm *lm = nullptr;
    if (wfst_lm_load(_file.c_str(), _scale, _device, &lm) != WFST_OK) Fatal("ArpaLm upload");
    _lm = lm;
  }
  return _lm;
}

// ---- channel pool: many decoder objects, one batched device decoder ------------------------------
GpuChannelPool::GpuChannelPool(Fst *graph, const LatticeFasterDecoderConfig &config, int n_channels, const wfst_limits *limits, int linger_us)
    : _dec(nullptr), _graph(graph), _n(n_channels), _linger_us(linger_us), _n_leased(0), _stop(false), _stats() {
  config.Check();
  wfst_config c = config.ToC();
  if (n_channels < 1) throw std::runtime_error("GpuChannelPool needs at least one channel");
  if (wfst_decoder_create(graph->Handle(), &c, n_channels, limits, nullptr, &_dec) != WFST_OK) Fatal("wfst_decoder_create");
  Start(linger_us);
}
GpuChannelPool::GpuChannelPool(Fst *graph, const LatticeFasterDecoderConfig &config, ArpaLm *oldlm, ArpaLm *newlm, int n_channels,
                               const wfst_limits *limits, int linger_us)
    : _dec(nullptr), _graph(graph), _n(n_channels), _linger_us(linger_us), _n_leased(0), _stop(false), _stats() {
  config.Check();
  wfst_config c = config.ToC();
  if (n_channels < 1) throw std::runtime_error("GpuChannelPool needs at least one channel");
  if (!oldlm || !newlm) throw std::runtime_error("biglm decoder needs both LMs");
  if (wfst_decoder_create_biglm(graph->Handle(), &c, n_channels, limits, nullptr, oldlm->Handle(), newlm->Handle(), nullptr, &_dec) != WFST_OK)
    Fatal("wfst_decoder_create_biglm");
  Start(linger_us);
}
void GpuChannelPool::Start(int linger_us) {
  _linger_us = std::max(0, linger_us);
  _leased.assign((size_t)_n, 0);
  if (const char *tf = getenv("WFST_POOL_TRACE")) _trace_file = tf;
  _t_origin = _t_first = std::chrono::steady_clock::now();
  _thread = std::thread([this] { Run(); });
}
GpuChannelPool::~GpuChannelPool() {
  {
    std::lock_guard<std::mutex> lk(_mu);
    _stop = true;
  }
  _cv_work.notify_all();
  if (_thread.joinable()) _thread.join();
  wfst_decoder_free(_dec);   // (waits for the device: no row of the slab is on its way any more)
  if (_slab) wfst_host_free(_slab);
  if (!_trace_file.empty()) {
    if (FILE *f = fopen(_trace_file.c_str(), "w")) {
      fprintf(f, "# ms since the pool started: first request, batch closed, pass done | requests init advance finalize best-path calls endpoint partial | ms of each | device busy at close\n");
      for (const TracePass &t : _trace)
        fprintf(f, "%.3f %.3f %.3f | %d %d %d %d %d %d %d | %.3f %.3f %.3f %.3f %.3f %.3f %.3f | %d\n", t.t_first, t.t_closed, t.t_end, t.n[0], t.n[1], t.n[2], t.n[3],
                t.n[4], t.n[5], t.n[6], t.ms[0], t.ms[1], t.ms[2], t.ms[3], t.ms[4], t.ms[5], t.ms[6], t.busy);
      fclose(f);
    }
  }
}
float *GpuChannelPool::RowSlot(int channel, size_t floats, size_t *slot_floats) {
  std::lock_guard<std::mutex> lk(_slab_mu);
  if (!_slab) {
    if (_slab_pitch != 0) return nullptr;   // (tried before: no page-locked memory of that size)
    _slab_pitch = (std::max<size_t>(floats, (size_t)1 << 16) + 1023) & ~(size_t)1023;
    _slab = (float *)wfst_host_alloc((size_t)_n * _slab_pitch * sizeof(float));
    if (!_slab) return nullptr;
  }
  if (floats > _slab_pitch || channel < 0 || channel >= _n) return nullptr;
  *slot_floats = _slab_pitch;
  return _slab + (size_t)channel * _slab_pitch;
}
GpuChannelPool::Stats GpuChannelPool::GetStats() {
  std::lock_guard<std::mutex> lk(_mu);
  return _stats;
}
int GpuChannelPool::Lease() {
  std::unique_lock<std::mutex> lk(_mu);
  for (;;) {
    for (int c = 0; c < _n; ++c)
      if (!_leased[(size_t)c]) { _leased[(size_t)c] = 1; ++_n_leased; return c; }
    _cv_free.wait(lk);   // (more decoder objects than channels: this one waits for a destructor)
  }
}
int GpuChannelPool::TryLease() {
  std::lock_guard<std::mutex> lk(_mu);
  for (int c = 0; c < _n; ++c)
    if (!_leased[(size_t)c]) { _leased[(size_t)c] = 1; ++_n_leased; return c; }
  return -1;
}
void GpuChannelPool::Release(int c) {
  {
    std::lock_guard<std::mutex> lk(_mu);
    if (c >= 0 && c < _n && _leased[(size_t)c]) { _leased[(size_t)c] = 0; --_n_leased; }
  }
  _cv_free.notify_one();
}
void GpuChannelPool::Submit(Request *r) {
  {
    std::lock_guard<std::mutex> lk(_mu);
    if (_stop) throw std::runtime_error("GpuChannelPool is shutting down");
    r->done = false;
    r->error = nullptr;
    if (_queue.empty() && !_trace_file.empty()) _t_first = std::chrono::steady_clock::now();
    _queue.push_back(r);
    // (the batcher sleeps without a time-out only on an empty queue; while a batch forms it looks again every few tens of
    // microseconds -- it is woken for the first request and for the one that completes the batch, not sixty-four times)
    if (_queue.size() == 1 || (int)_queue.size() + _n_bp_outstanding >= _n_leased) _cv_work.notify_one();
  }
  {
    std::unique_lock<std::mutex> lk(r->m);
    r->cv.wait(lk, [&] { return r->done; });
  }
  if (r->error) std::rethrow_exception(r->error);
}
void GpuChannelPool::Done(Request *r) {
  std::lock_guard<std::mutex> lk(r->m);
  r->done = true;
  r->cv.notify_one();   // (under the request's mutex: its thread cannot leave Submit -- and destroy the request -- before this returns)
}
void GpuChannelPool::Finish(std::vector<Request *> &rs) {
  for (Request *r : rs) r->decoded = wfst_decoder_num_frames_decoded(_dec, r->channel);
  for (Request *r : rs) Done(r);
}
void GpuChannelPool::Run() {
  std::unique_lock<std::mutex> lk(_mu);
  for (;;) {
    const auto t_wait = std::chrono::steady_clock::now();
    // wait for requests; a best-path list on the device is looked after meanwhile (its results are taken as soon as they have landed)
    while (!_stop && _queue.empty()) {
      if (_bp_flight.empty() && _bp_wait.empty() && _pt_flight.empty() && _pt_wait.empty()) { _cv_work.wait(lk); continue; }
      lk.unlock();
      const bool bp_taken = PollBestPaths(false), pt_taken = PollPartials(false), progressed = bp_taken || pt_taken;
      if (!bp_taken && _bp_flight.empty()) StartBestPaths();
      if (!pt_taken && _pt_flight.empty()) StartPartials();
      lk.lock();
      if (!progressed && _queue.empty() && !_stop) _cv_work.wait_until(lk, std::chrono::system_clock::now() + std::chrono::microseconds(30));
    }
    if (_queue.empty()) {   // (_stop: what is on the device is taken, what waits is served, then out)
      lk.unlock();
      while (!_bp_flight.empty() || !_bp_wait.empty()) { PollBestPaths(true); StartBestPaths(); }
      while (!_pt_flight.empty() || !_pt_wait.empty()) { PollPartials(true); StartPartials(); }
      return;
    }
    // the other leased channels' requests are on their way more often than not (their threads were released together): a short
    // wait makes one batch of them instead of two.  Threads that wait for a best path (on the device, or in line for it) are not
    // coming: they count as arrived.
    // ... and while the device has a backlog, requests go on joining (two cohorts of threads that alternate merge into one; a
    // frame of 40 channels takes the device as long as a frame of 64): wfst_decoder_calls_in_flight counts the advance calls not
    // yet finished -- with three or more outstanding the batch may grow for nothing, below that it goes (the device is a call or
    // two from running dry, and this batch's rows have to get there first)
    // ... and with three advance calls outstanding the batch waits in any case: a fourth would stand in wfst_decoder_advance_host
    // until the device has caught up (its staging sets are used in rotation), and the batcher with it -- finished utterances' best
    // paths would lie on the device untaken, their threads idle
    auto arrived = [&] { return (int)(_queue.size() + _bp_wait.size() + _bp_flight.size() + _pt_wait.size() + _pt_flight.size()); };
    {
      const auto t_first = std::chrono::steady_clock::now();
      for (;;) {
        if (_stop) break;
        // (a batch that is at least half full waits ten times as long for the rest: threads released together come back spread over
        // a few hundred microseconds, and cut in two they stay two cohorts -- a device call of half the channels takes as long as one
        // of all)
        const auto waited = std::chrono::steady_clock::now() - t_first;
        const bool lingered = waited >= std::chrono::microseconds(_linger_us) &&
                              (2 * arrived() < _n_leased || waited >= std::chrono::microseconds(10 * (long long)_linger_us));
        if (lingered || arrived() >= _n_leased) {
          lk.unlock();
          const int depth = wfst_decoder_calls_in_flight(_dec);
          if (!_bp_flight.empty()) PollBestPaths(false);
          if (!_pt_flight.empty()) PollPartials(false);
          lk.lock();
          if (depth < 3) break;   // (2: the same, measured)
        }
        // (wait_until on the SYSTEM clock = pthread_cond_timedwait: what ThreadSanitizer's runtime intercepts -- a steady-clock wait is
        // pthread_cond_clockwait, which gcc 11's does not, and the tool then loses the mutex's hand-over; a jump of the wall clock
        // costs one short wait at most, the loop looks at its conditions again either way)
        _cv_work.wait_until(lk, std::chrono::system_clock::now() + std::chrono::microseconds(lingered ? 20 : std::max(1, _linger_us)));
      }
    }
    std::vector<Request *> batch;
    batch.swap(_queue);
    _stats.ms_waiting += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_wait).count();
    const auto t_first = _t_first;
    lk.unlock();
    if (!_trace_file.empty()) {
      auto ms = [&](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(t - _t_origin).count(); };
      TracePass tp;
      memset(&tp, 0, sizeof(tp));
      tp.t_first = ms(t_first);
      tp.t_closed = ms(std::chrono::steady_clock::now());
      tp.busy = wfst_decoder_busy(_dec);
      for (Request *r : batch) tp.n[r->kind] += 1;
      _trace.push_back(tp);
    }
    Execute(batch);   // (releases every kind's requesters as soon as that kind is served: Finish)
    if (!_trace_file.empty()) _trace.back().t_end = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - _t_origin).count();
    lk.lock();
    _stats.batches += 1;
    _stats.requests += (long long)batch.size();
  }
}
// One pass over what has arrived.  A channel has at most one request in a batch (its thread waits for it), so the kinds can be
// served in any order: init, advance, finalize, best path, then the one-off calls.  A batched C-ABI call validates every listed
// channel before it enqueues anything: when it refuses the batch, the requests are retried one by one and each gets its own verdict.
void GpuChannelPool::Execute(std::vector<Request *> &batch) {
  std::vector<Request *> by_kind[kKinds];
  for (Request *r : batch) by_kind[r->kind].push_back(r);
  auto listed = [&](std::vector<Request *> &rs, const char *what, auto &&call) {
    if (rs.empty()) return;
    std::vector<int32_t> ch;
    for (Request *r : rs) ch.push_back(r->channel);
    if (call(ch.data(), (int32_t)ch.size()) == WFST_OK) return;
    if (rs.size() == 1) { rs[0]->error = std::make_exception_ptr(std::runtime_error(std::string(what) + ": " + wfst_last_error())); return; }
    for (Request *r : rs) {
      const int32_t c = r->channel;
      if (call(&c, 1) != WFST_OK) r->error = std::make_exception_ptr(std::runtime_error(std::string(what) + ": " + wfst_last_error()));
    }
  };
  double ms[kKinds] = {0, 0, 0, 0, 0, 0, 0, 0};
  // a kind's requesters go on as soon as that kind is served: the threads whose chunks have just been enqueued pull their next
  // chunks while the batcher fetches other channels' best paths (which waits for the device)
  auto clocked = [&](int kind, auto &&f) {
    if (by_kind[kind].empty()) return;
    const auto t0 = std::chrono::steady_clock::now();
    f();
    ms[kind] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    for (Request *r : by_kind[kind]) r->decoded = wfst_decoder_num_frames_decoded(_dec, r->channel);
    for (Request *r : by_kind[kind]) Done(r);
  };
  clocked(kInit, [&] { listed(by_kind[kInit], "InitDecoding", [&](const int32_t *ch, int32_t n) { return wfst_decoder_init(_dec, ch, n); }); });
  clocked(kAdvance, [&] { ExecuteAdvance(by_kind[kAdvance]); });
  clocked(kFinalize, [&] { listed(by_kind[kFinalize], "FinalizeDecoding", [&](const int32_t *ch, int32_t n) { return wfst_decoder_finalize(_dec, ch, n); }); });
  // best paths: the requests join the waiting list; what is on the device is looked at, the next list is started -- the requesters
  // are released when THEIR list's results have landed (PollBestPaths), not at the end of this pass
  {
    const auto t0 = std::chrono::steady_clock::now();
    for (Request *r : by_kind[kBestPath]) _bp_wait.push_back(r);
    CountBestPaths();
    PollBestPaths(false);
    StartBestPaths();
    ms[kBestPath] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  // partial words: the same shape -- the pass's requests join the waiting list and go to the device as ONE list
  {
    const auto t0 = std::chrono::steady_clock::now();
    for (Request *r : by_kind[kPartial]) _pt_wait.push_back(r);
    CountBestPaths();
    PollPartials(false);
    const long long before = _stats.partial_calls;   // (written by this thread alone)
    StartPartials();
    if (_stats.partial_calls - before > _stats.partial_max_per_pass) {
      std::lock_guard<std::mutex> lk(_mu);
      _stats.partial_max_per_pass = _stats.partial_calls - before;
    }
    ms[kPartial] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  clocked(kEndpoint, [&] { ExecuteEndpoint(by_kind[kEndpoint]); });
  clocked(kNbestWords, [&] { ExecuteNbestWords(by_kind[kNbestWords]); });
  clocked(kCall, [&] {
    for (Request *r : by_kind[kCall]) {
      try {
        r->call(_dec);
      } catch (...) {
        r->error = std::current_exception();
      }
    }
  });
  {
    std::lock_guard<std::mutex> lk(_mu);
    for (int k = 0; k <= kCall; ++k) _stats.ms_by_kind[k] += ms[k];
    _stats.ms_endpoint += ms[kEndpoint];
    _stats.ms_partial += ms[kPartial];
    _stats.ms_nbest_words += ms[kNbestWords];
  }
  if (!_trace_file.empty() && !_trace.empty())
    for (int k = 0; k < kKinds; ++k) _trace.back().ms[k] = ms[k];
}
// EndpointDetected of every waiting channel: one wfst_decoder_endpoint_detected per distinct config (a service has one); a list the
// library refuses is retried request by request, each with its own verdict
void GpuChannelPool::ExecuteEndpoint(std::vector<Request *> &requests) {
  // each distinct config object is checked and converted once per pass (a service's threads share one); requests whose configs
  // convert to the same bytes form one group
  struct Conf { std::vector<int32_t> phones; wfst_endpoint_config c; std::string key; std::exception_ptr error; };
  std::map<const OnlineEndpointConfig *, Conf> confs;
  std::map<std::string, std::vector<Request *> > groups;
  std::map<std::string, const Conf *> group_conf;
  for (Request *r : requests) {
    auto it = confs.find(r->endpoint_config);
    if (it == confs.end()) {
      Conf &cf = confs[r->endpoint_config];
      try {
        cf.c = r->endpoint_config->ToC(&cf.phones);
        cf.key = EndpointKey(cf.c);
      } catch (...) {
        cf.error = std::current_exception();
      }
      it = confs.find(r->endpoint_config);
    }
    if (it->second.error) { r->error = it->second.error; continue; }
    groups[it->second.key].push_back(r);
    group_conf[it->second.key] = &it->second;
  }
  for (auto &gr : groups) {
    std::vector<Request *> &group = gr.second;
    if (gr.first != _ep_key) {
      if (wfst_decoder_set_endpoint_config(_dec, &group_conf[gr.first]->c) != WFST_OK) {
        const std::string m = std::string("EndpointDetected: ") + wfst_last_error();
        for (Request *r : group) r->error = std::make_exception_ptr(std::runtime_error(m));
        continue;
      }
      _ep_key = gr.first;
    }
    auto call = [&](const std::vector<Request *> &rs) {
      std::vector<int32_t> ch, rule(rs.size());
      for (Request *r : rs) ch.push_back(r->channel);
      const int rc = wfst_decoder_endpoint_detected(_dec, ch.data(), (int32_t)ch.size(), nullptr, rule.data(), nullptr, nullptr);
      if (rc == WFST_OK)
        for (size_t i = 0; i < rs.size(); ++i) rs[i]->endpoint_rule = rule[i];
      std::lock_guard<std::mutex> lk(_mu);
      _stats.endpoint_calls += 1;
      _stats.endpoint_requests += (long long)rs.size();
      return rc;
    };
    if (call(group) == WFST_OK) continue;
    for (Request *r : group)
      if (call(std::vector<Request *>(1, r)) != WFST_OK)
        r->error = std::make_exception_ptr(std::runtime_error(std::string("EndpointDetected: ") + wfst_last_error()));
  }
}
void GpuChannelPool::ExecuteAdvance(std::vector<Request *> &requests) {
  // one call per (stride, max_num_frames): in a service every stream has the same model, i.e. one call
  std::vector<Request *> all(requests);   // (consumed below; the caller's list is what it marks done)
  while (!all.empty()) {
    std::vector<Request *> rs, rest;
    for (Request *r : all) (r->stride == all[0]->stride && r->max_num_frames == all[0]->max_num_frames ? rs : rest).push_back(r);
    all.swap(rest);
    // (in channel order: the rows of consecutive channels are equally spaced slots of the pool's slab -- the library uploads such
    // runs as one 2-D copy each)
    std::sort(rs.begin(), rs.end(), [](const Request *x, const Request *y) { return x->channel < y->channel; });
    auto call = [&](std::vector<Request *> &q) {
      std::vector<int32_t> ch, ready;
      std::vector<const float *> rows;
      for (Request *r : q) { ch.push_back(r->channel); ready.push_back(r->ready); rows.push_back(r->rows); }
      return wfst_decoder_advance_host(_dec, ch.data(), (int32_t)ch.size(), rows.data(), ready.data(), q[0]->stride, q[0]->max_num_frames);
    };
    long long frames = 0;
    for (Request *r : rs) frames += std::max(0, r->ready - wfst_decoder_num_frames_decoded(_dec, r->channel));
    {
      std::lock_guard<std::mutex> lk(_mu);
      _stats.advance_calls += 1;
      _stats.advance_requests += (long long)rs.size();
      _stats.frames += frames;
    }
    if (call(rs) == WFST_OK) continue;
    if (rs.size() == 1) { rs[0]->error = std::make_exception_ptr(std::runtime_error(std::string("AdvanceDecoding: ") + wfst_last_error())); continue; }
    for (Request *r : rs) {
      std::vector<Request *> one(1, r);
      if (call(one) != WFST_OK) r->error = std::make_exception_ptr(std::runtime_error(std::string("AdvanceDecoding: ") + wfst_last_error()));
    }
  }
}
void GpuChannelPool::StartBestPaths() {
  if (!_bp_flight.empty() || _bp_wait.empty()) return;
  _bp_ufp = _bp_wait[0]->use_final_probs ? 1 : 0;
  std::vector<Request *> rest;
  for (Request *r : _bp_wait) ((r->use_final_probs ? 1 : 0) == _bp_ufp ? _bp_flight : rest).push_back(r);
  _bp_wait.swap(rest);
  std::vector<int32_t> ch;
  int maxf = 1;
  for (Request *r : _bp_flight) { ch.push_back(r->channel); maxf = std::max(maxf, wfst_decoder_num_frames_decoded(_dec, r->channel)); }
  _bp_cap = 4 * maxf + 64;
  if (wfst_decoder_best_path_enqueue(_dec, ch.data(), (int32_t)ch.size(), _bp_ufp, _bp_cap) != WFST_OK) {
    // refused (one of the channels: GetBestPath before InitDecoding ...): request by request, each its own verdict
    std::vector<Request *> rs;
    rs.swap(_bp_flight);
    CountBestPaths();
    ExecuteBestPath(rs);
    Finish(rs);
  }
}
// true: a list's results were taken (its requesters are released)
bool GpuChannelPool::PollBestPaths(bool block) {
  if (_bp_flight.empty()) return false;
  if (!block && wfst_decoder_best_path_ready(_dec) != 1) return false;
  const int cnt = (int)_bp_flight.size(), cap = _bp_cap;
  std::vector<int32_t> il((size_t)cnt * cap), ol((size_t)cnt * cap), n((size_t)cnt, 0);
  std::vector<float> g((size_t)cnt * cap), ac((size_t)cnt * cap);
  const int rc = wfst_decoder_best_path_fetch(_dec, il.data(), ol.data(), g.data(), ac.data(), n.data());
  std::vector<Request *> rs;
  rs.swap(_bp_flight);
  CountBestPaths();
  if (rc != WFST_OK) {
    // a path longer than the capacity, or one channel's device error: the synchronous path sorts it out request by request
    ExecuteBestPath(rs);
    Finish(rs);
    return true;
  }
  for (int i = 0; i < cnt; ++i) {
    Request *r = rs[(size_t)i];
    r->n_hops = n[(size_t)i];
    const size_t o = (size_t)i * cap;
    r->il.assign(il.begin() + (long)o, il.begin() + (long)o + r->n_hops);
    r->ol.assign(ol.begin() + (long)o, ol.begin() + (long)o + r->n_hops);
    r->g.assign(g.begin() + (long)o, g.begin() + (long)o + r->n_hops);
    r->ac.assign(ac.begin() + (long)o, ac.begin() + (long)o + r->n_hops);
    // (the final result says whether the per-frame token limit bound on the way; partial results do not stop for it)
    int32_t dg = 0;
    if (_bp_ufp && wfst_decoder_get_degraded_frames(_dec, r->channel, &dg) == WFST_OK) r->degraded = dg;
  }
  Finish(rs);
  return true;
}
void GpuChannelPool::StartPartials() {
  if (!_pt_flight.empty() || _pt_wait.empty()) return;
  _pt_flight.swap(_pt_wait);
  std::vector<int32_t> ch;
  int maxf = 1;
  for (Request *r : _pt_flight) { ch.push_back(r->channel); maxf = std::max(maxf, wfst_decoder_num_frames_decoded(_dec, r->channel)); }
  _pt_cap = maxf + 64;
  {
    std::lock_guard<std::mutex> lk(_mu);
    _stats.partial_calls += 1;
    _stats.partial_requests += (long long)ch.size();
  }
  if (wfst_decoder_partial_enqueue(_dec, ch.data(), (int32_t)ch.size(), _pt_cap) != WFST_OK) {
    // refused (one of the channels: before InitDecoding, after FinalizeDecoding ...): request by request, each its own verdict
    std::vector<Request *> rs;
    rs.swap(_pt_flight);
    CountBestPaths();
    ExecutePartial(rs);
    Finish(rs);
  }
}
// true: a list's results were taken (its requesters are released)
bool GpuChannelPool::PollPartials(bool block) {
  if (_pt_flight.empty()) return false;
  if (!block && wfst_decoder_partial_ready(_dec) != 1) return false;
  const int cnt = (int)_pt_flight.size(), cap = _pt_cap;
  std::vector<int32_t> w((size_t)cnt * cap), nw((size_t)cnt, 0), ns((size_t)cnt, 0);
  const int rc = wfst_decoder_partial_fetch(_dec, w.data(), nw.data(), ns.data(), nullptr);
  std::vector<Request *> rs;
  rs.swap(_pt_flight);
  CountBestPaths();
  if (rc != WFST_OK) {
    ExecutePartial(rs);   // (more words than the capacity: request by request, with the size it needs)
    Finish(rs);
    return true;
  }
  for (int i = 0; i < cnt; ++i) {
    Request *r = rs[(size_t)i];
    r->words.assign(w.begin() + (long)((size_t)i * cap), w.begin() + (long)((size_t)i * cap) + nw[(size_t)i]);
    r->n_stable = ns[(size_t)i];
  }
  Finish(rs);
  return true;
}
void GpuChannelPool::ExecutePartial(std::vector<Request *> &rs) {
  for (Request *r : rs) {
    const int32_t c = r->channel;
    int32_t cap = std::max(1, wfst_decoder_num_frames_decoded(_dec, c)) + 64, nw = 0, ns = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
      std::vector<int32_t> w((size_t)cap);
      const int rc = wfst_decoder_get_partial(_dec, &c, 1, cap, w.data(), &nw, &ns, nullptr);
      if (rc == WFST_E_CAPACITY && nw > cap && attempt == 0) { cap = nw; continue; }
      if (rc != WFST_OK) { r->error = std::make_exception_ptr(std::runtime_error(std::string("GetPartialWords: ") + wfst_last_error())); break; }
      r->words.assign(w.begin(), w.begin() + nw);
      r->n_stable = ns;
      break;
    }
  }
}
void GpuChannelPool::ExecuteBestPath(std::vector<Request *> &all) {
  for (int ufp = 0; ufp < 2; ++ufp) {
    std::vector<Request *> rs;
    for (Request *r : all)
      if ((r->use_final_probs ? 1 : 0) == ufp) rs.push_back(r);
    if (rs.empty()) continue;
    const int cnt = (int)rs.size();
    std::vector<int32_t> ch((size_t)cnt);
    int maxf = 1;
    for (int i = 0; i < cnt; ++i) { ch[(size_t)i] = rs[(size_t)i]->channel; maxf = std::max(maxf, wfst_decoder_num_frames_decoded(_dec, ch[(size_t)i])); }
    int cap = 4 * maxf + 64;
    for (int attempt = 0; attempt < 2; ++attempt) {
      std::vector<int32_t> il((size_t)cnt * cap), ol((size_t)cnt * cap), n((size_t)cnt, 0);
      std::vector<float> g((size_t)cnt * cap), ac((size_t)cnt * cap);
      const int rc = wfst_decoder_get_best_path(_dec, ch.data(), cnt, ufp, cap, il.data(), ol.data(), g.data(), ac.data(), n.data());
      if (rc == WFST_E_CAPACITY && *std::max_element(n.begin(), n.end()) > cap && attempt == 0) { cap = *std::max_element(n.begin(), n.end()); continue; }
      if (rc != WFST_OK && cnt > 1 && attempt == 0) {
        // the batch was refused for one of its channels (GetBestPath before InitDecoding, a channel's device error ...): one by one
        for (Request *r : rs) { std::vector<Request *> one(1, r); ExecuteBestPath(one); }
        break;
      }
      for (int i = 0; i < cnt; ++i) {
        Request *r = rs[(size_t)i];
        if (rc != WFST_OK) { r->error = std::make_exception_ptr(std::runtime_error(std::string("GetBestPath: ") + wfst_last_error())); continue; }
        r->n_hops = n[(size_t)i];
        const size_t o = (size_t)i * cap;
        r->il.assign(il.begin() + (long)o, il.begin() + (long)o + r->n_hops);
        r->ol.assign(ol.begin() + (long)o, ol.begin() + (long)o + r->n_hops);
        r->g.assign(g.begin() + (long)o, g.begin() + (long)o + r->n_hops);
        r->ac.assign(ac.begin() + (long)o, ac.begin() + (long)o + r->n_hops);
        // (the final result says whether the per-frame token limit bound on the way; partial results do not stop for it)
        int32_t dg = 0;
        if (ufp && wfst_decoder_get_degraded_frames(_dec, r->channel, &dg) == WFST_OK) r->degraded = dg;
      }
      break;
    }
  }
}

// ---- single-stream decoder --------------------------------------------------------------------
GpuLatticeDecoder::GpuLatticeDecoder(Fst *graph, const LatticeFasterDecoderConfig &config, const wfst_limits *limits)
    : _dec(nullptr), _pool(nullptr), _chan(0), _decoded(0), _rows(nullptr), _rows_cap(0), _rows_pinned(false), _stride(0), _rows_ready(0), _inited(false) {
  config.Check();
  Share(graph, config, nullptr, nullptr, limits);
  if (_pool) return;
  wfst_config c = config.ToC();
  if (wfst_decoder_create(graph->Handle(), &c, 1, limits, nullptr, &_dec) != WFST_OK) Fatal("wfst_decoder_create");
  SetColumns(graph);
}
GpuLatticeDecoder::GpuLatticeDecoder(Fst *graph, const LatticeFasterDecoderConfig &config, ArpaLm *oldlm, ArpaLm *newlm,
                                     const wfst_limits *limits)
    : _dec(nullptr), _pool(nullptr), _chan(0), _decoded(0), _rows(nullptr), _rows_cap(0), _rows_pinned(false), _stride(0), _rows_ready(0), _inited(false) {
  config.Check();
  if (!oldlm || !newlm) throw std::runtime_error("biglm decoder needs both LMs");
  Share(graph, config, oldlm, newlm, limits);
  if (_pool) return;
  wfst_config c = config.ToC();
  if (wfst_decoder_create_biglm(graph->Handle(), &c, 1, limits, nullptr, oldlm->Handle(), newlm->Handle(), nullptr, &_dec) != WFST_OK)
    Fatal("wfst_decoder_create_biglm");
  SetColumns(graph);
}

// ---- ShareDevice: the reference's constructor shape over shared device decoders ------------------------------------------------
namespace {
struct SharedEntry {
  const wfst_graph *graph;
  wfst_config cfg;
  bool has_lim;
  wfst_limits lim;
  ArpaLm *oldlm, *newlm;
  std::shared_ptr<GpuChannelPool> pool;
};
struct SharedRegistry {
  std::mutex mu;
  int n_channels = 0, linger_us = 50;
  std::vector<SharedEntry> entries;
};
// (never destroyed: worker threads may still hold decoder objects when the process leaves main, and the device runtime's own
// teardown order is not ours to rely on)
SharedRegistry &Registry() { static SharedRegistry *r = new SharedRegistry(); return *r; }
}  // namespace

void GpuLatticeDecoder::ShareDevice(int n_channels, int linger_us) {
  SharedRegistry &R = Registry();
  std::lock_guard<std::mutex> lk(R.mu);
  R.n_channels = std::max(0, n_channels);
  R.linger_us = linger_us;
  if (R.n_channels == 0) R.entries.clear();   // (a shared decoder goes when its last object does)
}
void GpuLatticeDecoder::Share(Fst *graph, const LatticeFasterDecoderConfig &config, ArpaLm *oldlm, ArpaLm *newlm, const wfst_limits *limits) {
  SharedRegistry &R = Registry();
  std::lock_guard<std::mutex> lk(R.mu);
  if (R.n_channels <= 0) return;
  const wfst_config c = config.ToC();
  for (SharedEntry &e : R.entries) {
    if (e.graph != graph->Handle() || memcmp(&e.cfg, &c, sizeof(c)) != 0 || e.oldlm != oldlm || e.newlm != newlm) continue;
    if (e.has_lim != (limits != nullptr) || (limits && memcmp(&e.lim, limits, sizeof(*limits)) != 0)) continue;
    const int ch = e.pool->TryLease();
    if (ch < 0) continue;   // (full: the next one, or a new one)
    _shared = e.pool;
    _pool = _shared.get();
    _dec = _pool->_dec;
    _chan = ch;
    SetColumns(graph);
    return;
  }
  SharedEntry e;
  e.graph = graph->Handle();
  e.cfg = c;
  e.has_lim = limits != nullptr;
  memset(&e.lim, 0, sizeof(e.lim));
  if (limits) e.lim = *limits;
  e.oldlm = oldlm; e.newlm = newlm;
  e.pool.reset(oldlm ? new GpuChannelPool(graph, config, oldlm, newlm, R.n_channels, limits, R.linger_us)
                     : new GpuChannelPool(graph, config, R.n_channels, limits, R.linger_us));
  const int ch = e.pool->TryLease();
  _shared = e.pool;
  _pool = _shared.get();
  _dec = _pool->_dec;
  _chan = ch;
  SetColumns(graph);
  R.entries.push_back(e);
}
GpuLatticeDecoder::GpuLatticeDecoder(GpuChannelPool *pool)
    : _dec(nullptr), _pool(pool), _chan(0), _decoded(0), _rows(nullptr), _rows_cap(0), _rows_pinned(false), _stride(0), _rows_ready(0), _inited(false) {
  if (!pool) throw std::runtime_error("GpuLatticeDecoder: NULL pool");
  _dec = pool->_dec;
  SetColumns(pool->_graph);
  _chan = pool->Lease();
}
// the graph reads column tid2pdf[ilabel]: one representative transition-id per pdf is all the decodable is asked for (wfst-host.h,
// Fst::SetTid2Pdf)
void GpuLatticeDecoder::SetColumns(const Fst *graph) {
  _rep.clear();
  if (!graph) return;
  const std::vector<int32_t> &m = graph->Tid2Pdf();
  int32_t n_pdf = 0;
  for (size_t t = 1; t < m.size(); ++t) n_pdf = std::max(n_pdf, m[t] + 1);
  if (n_pdf <= 0) return;
  _rep.assign((size_t)n_pdf, 0);
  for (size_t t = m.size() - 1; t >= 1; --t)
    if (m[t] >= 0) _rep[(size_t)m[t]] = (int32_t)t;   // (the lowest transition-id of the pdf)
}
GpuLatticeDecoder::~GpuLatticeDecoder() {
  // (rows of an utterance abandoned right behind an AdvanceDecoding may still be on their way to the device from the page-locked
  // buffer freed below: the device is waited for first; an object that fetched its result, or never decoded, has nothing in flight)
  if (_rows_pinned && _rows_ready > 0 && _inited) {
    try {
      OnDevice([&] { (void)wfst_decoder_sync(_dec); });
    } catch (...) {
    }
  }
  if (_pool) _pool->Release(_chan);
  else wfst_decoder_free(_dec);
  if (_rows_in_pool) _rows = nullptr;   // (the pool's)
  else if (_rows_pinned) wfst_host_free(_rows);
  else free(_rows);
  _shared.reset();   // (ShareDevice: the shared decoder goes with its last object once the registry has let go of it)
}
// the rows pulled from the decodable live in page-locked memory (they are uploaded chunk by chunk, beside the search over the chunk
// before): grown by doubling, the history kept
void GpuLatticeDecoder::GrowRows(size_t floats) {
  if (floats <= _rows_cap) return;
  if (_pool && !_rows) {
    // the channel's slot of the pool's slab, if the rows fit there (they do when the service has reserved its longest utterance)
    size_t cap = 0;
    if (float *slot = _pool->RowSlot(_chan, floats, &cap)) {
      _rows = slot;
      _rows_cap = cap;
      _rows_pinned = true;
      _rows_in_pool = true;
      return;
    }
  }
  const size_t ncap = std::max<size_t>(floats, std::max<size_t>(2 * _rows_cap, (size_t)1 << 16));
  bool pinned = true;
  float *np = (float *)wfst_host_alloc(ncap * sizeof(float));
  if (!np) {
    pinned = false;
    np = (float *)malloc(ncap * sizeof(float));
    if (!np) throw std::bad_alloc();
  }
  if (_rows && _rows_ready > 0) memcpy(np, _rows, (size_t)_rows_ready * _stride * sizeof(float));
  // (rows of the old page-locked buffer may still be on their way to the device -- wfst_decoder_advance_host returns when they are
  // enqueued: the device is waited for before the buffer goes; a slot of the pool's slab stays where it is)
  if (_rows_in_pool) {
    _rows_in_pool = false;
  } else {
    if (_rows_pinned && _rows_ready > 0 && _inited) OnDevice([&] { (void)wfst_decoder_sync(_dec); });
    if (_rows_pinned) wfst_host_free(_rows);
    else free(_rows);
  }
  _rows = np;
  _rows_cap = ncap;
  _rows_pinned = pinned;
}

// the C-ABI calls of one decoder are not re-entrant: with a pool they run in its batcher thread, one request after the other
template <class F>
void GpuLatticeDecoder::OnDevice(F &&f) {
  if (!_pool) { f(); return; }
  GpuChannelPool::Request r;
  r.kind = GpuChannelPool::kCall;
  r.channel = _chan;
  r.call = [&](wfst_decoder *) { f(); };
  _pool->Submit(&r);
  _decoded = r.decoded;
}

void GpuLatticeDecoder::ReserveRows(int frames, int num_indices) {
  const size_t stride = _rep.empty() ? (size_t)(num_indices + 1) : (((size_t)_rep.size() + 3) & ~(size_t)3);   // (per-pdf rows where the graph maps)
  if (frames > 0 && num_indices > 0) GrowRows((size_t)frames * stride);
}

void GpuLatticeDecoder::InitDecoding() {
  if (_pool) {
    GpuChannelPool::Request r;
    r.kind = GpuChannelPool::kInit;
    r.channel = _chan;
    _pool->Submit(&r);
    _decoded = r.decoded;
  } else if (wfst_decoder_init(_dec, nullptr, 0) != WFST_OK) Fatal("InitDecoding");
  _rows_ready = 0;   // (the buffer stays: the next utterance's rows go over this one's)
  _stride = 0;
  _inited = true;
}

void GpuLatticeDecoder::Pull(AmInterface *d) {
  const int ready = d->NumFramesReady();
  MatrixDecodable *md = dynamic_cast<MatrixDecodable *>(d);
  if (!_rep.empty() && !md) {
    // rows of one column per pdf (padded to a multiple of four columns: the expansion stages such a row in LDS by 16-byte DMAs)
    const int n_pdf = (int)_rep.size(), stride = (n_pdf + 3) & ~3;
    if (_stride == 0) _stride = stride;
    if (stride != _stride) throw std::runtime_error("decodable changed its shape within an utterance");
    if (d->NumIndices() < *std::max_element(_rep.begin(), _rep.end())) throw std::runtime_error("the decodable has fewer indices than the graph's tid2pdf maps");
    if (ready <= _rows_ready) return;
    GrowRows((size_t)ready * _stride);
    for (int f = _rows_ready; f < ready; ++f) {
      float *row = &_rows[(size_t)f * _stride];
      for (int p = 0; p < n_pdf; ++p) row[p] = _rep[(size_t)p] > 0 ? d->LogLikelihood(f, _rep[(size_t)p]) : 0.0f;
      for (int p = n_pdf; p < _stride; ++p) row[p] = 0.0f;
    }
    _rows_ready = ready;
    return;
  }
  const int stride = d->NumIndices() + 1;
  if (_stride == 0) _stride = stride;
  if (stride != _stride) throw std::runtime_error("decodable changed NumIndices() within an utterance");
  if (ready <= _rows_ready) return;
  GrowRows((size_t)ready * _stride);
  if (MatrixDecodable *m = md) {
    if (m->Stride() != _stride) throw std::runtime_error("MatrixDecodable::Stride() != NumIndices()+1");
    memcpy(&_rows[(size_t)_rows_ready * _stride], m->HostRows() + (size_t)_rows_ready * _stride,
           (size_t)(ready - _rows_ready) * _stride * sizeof(float));
  } else {
    for (int f = _rows_ready; f < ready; ++f) {
      float *row = &_rows[(size_t)f * _stride];
      row[0] = 0.0f;
      for (int i = 1; i < _stride; ++i) row[i] = d->LogLikelihood(f, i);
    }
  }
  _rows_ready = ready;
}

void GpuLatticeDecoder::AdvanceDecoding(AmInterface *decodable, int32 max_num_frames) {
  if (!_inited) throw std::runtime_error("You must call InitDecoding() before AdvanceDecoding");
  Pull(decodable);   // (in the caller's thread: with a pool, while the device decodes the batch before)
  const float *rows = _rows;
  int32_t ready = _rows_ready;
  if (ready == 0) return;
  if (_pool) {
    GpuChannelPool::Request r;
    r.kind = GpuChannelPool::kAdvance;
    r.channel = _chan;
    r.rows = rows; r.ready = ready; r.stride = _stride; r.max_num_frames = max_num_frames;
    _pool->Submit(&r);
    _decoded = r.decoded;
    return;
  }
  if (wfst_decoder_advance_host(_dec, nullptr, 0, &rows, &ready, _stride, max_num_frames) != WFST_OK)
    Fatal("AdvanceDecoding");
}

BaseFloat GpuLatticeDecoder::ProcessEmitting(AmInterface *decodable) {
  AdvanceDecoding(decodable, 1);
  return 0.0f;
}

void GpuLatticeDecoder::FinalizeDecoding() {
  if (_pool) {
    GpuChannelPool::Request r;
    r.kind = GpuChannelPool::kFinalize;
    r.channel = _chan;
    _pool->Submit(&r);
    _decoded = r.decoded;
    return;
  }
  if (wfst_decoder_finalize(_dec, nullptr, 0) != WFST_OK) Fatal("FinalizeDecoding");
}

void GpuLatticeDecoder::SetEndpointConfig(wfst_decoder *dec, const OnlineEndpointConfig &config, std::string *key) {
  std::vector<int32_t> phones;
  const wfst_endpoint_config c = config.ToC(&phones);
  const std::string k = EndpointKey(c);
  if (k == *key) return;
  if (wfst_decoder_set_endpoint_config(dec, &c) != WFST_OK) Fatal("EndpointDetected");
  *key = k;
}

bool GpuLatticeDecoder::EndpointDetected(const OnlineEndpointConfig &config, int *rule) {
  int r = 0;
  if (_pool) {
    GpuChannelPool::Request q;
    q.kind = GpuChannelPool::kEndpoint;
    q.channel = _chan;
    q.endpoint_config = &config;
    _pool->Submit(&q);
    _decoded = q.decoded;
    r = q.endpoint_rule;
  } else {
    SetEndpointConfig(_dec, config, &_ep_key);
    const int32_t c = 0;
    if (wfst_decoder_endpoint_detected(_dec, &c, 1, nullptr, &r, nullptr, nullptr) != WFST_OK) Fatal("EndpointDetected");
  }
  if (rule) *rule = r;
  return r != 0;
}

bool GpuLatticeDecoder::GetPartialWords(std::vector<int> *words, int *n_stable) {
  words->clear();
  int ns = 0;
  if (_pool) {
    GpuChannelPool::Request q;
    q.kind = GpuChannelPool::kPartial;
    q.channel = _chan;
    _pool->Submit(&q);
    _decoded = q.decoded;
    words->assign(q.words.begin(), q.words.end());
    ns = q.n_stable;
  } else {
    const int32_t c = 0;
    int32_t cap = std::max(1, NumFramesDecoded()) + 64, nw = 0, s32 = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
      std::vector<int32_t> w((size_t)cap);
      const int rc = wfst_decoder_get_partial(_dec, &c, 1, cap, w.data(), &nw, &s32, nullptr);
      if (rc == WFST_E_CAPACITY && nw > cap && attempt == 0) { cap = nw; continue; }
      if (rc != WFST_OK) Fatal("GetPartialWords");
      words->assign(w.begin(), w.begin() + nw);
      break;
    }
    ns = s32;
  }
  if (n_stable) *n_stable = ns;
  return NumFramesDecoded() > 0;
}

int32 GpuLatticeDecoder::NumFramesDecoded() const { return _pool ? _decoded : wfst_decoder_num_frames_decoded(_dec, 0); }

bool GpuLatticeDecoder::Decode(AmInterface *decodable) {
  InitDecoding();
  AdvanceDecoding(decodable);
  FinalizeDecoding();
  Lattice tmp;
  return GetBestPath(&tmp, true);
}

static void WarnIfDegraded(wfst_decoder *dec, int channel);
static void WarnDegraded(int channel, int n);

bool GpuLatticeDecoder::GetBestPath(Lattice *ofst, bool use_final_probs) {
  ofst->DeleteStates();
  if (_pool) {
    // batched with the other channels' requests (one wfst_decoder_get_best_path for all of them); the lattice is built here, in
    // the caller's thread
    GpuChannelPool::Request r;
    r.kind = GpuChannelPool::kBestPath;
    r.channel = _chan;
    r.use_final_probs = use_final_probs;
    _pool->Submit(&r);
    _decoded = r.decoded;
    if (r.degraded > 0) WarnDegraded(_chan, r.degraded);
    if (r.n_hops == 0) { Warn("No final token found."); return false; }
    HopsToLattice(r.il.data(), r.ol.data(), r.g.data(), r.ac.data(), r.n_hops, ofst);
    return true;
  }
  int cap = 4 * std::max(1, NumFramesDecoded()) + 64;
  for (int attempt = 0; attempt < 2; ++attempt) {
    std::vector<int32_t> il(cap), ol(cap);
    std::vector<float> g(cap), ac(cap);
    int32_t n = 0;
    int rc = wfst_decoder_get_best_path(_dec, nullptr, 0, use_final_probs ? 1 : 0, cap, il.data(), ol.data(), g.data(),
                                        ac.data(), &n);
    if (rc == WFST_E_CAPACITY && n > cap) { cap = n; continue; }
    if (rc == WFST_E_STATE) throw std::runtime_error(wfst_last_error());  // reference: LOG_ERR
    if (rc != WFST_OK) Fatal("GetBestPath");
    WarnIfDegraded(_dec, 0);
    if (n == 0) { Warn("No final token found."); return false; }
    HopsToLattice(il.data(), ol.data(), g.data(), ac.data(), n, ofst);
    return true;
  }
  return false;
}

// GetRawLattice (base-inl.h:869-975) of one channel through the C ABI.  Served after
// FinalizeDecoding by a decoder created in lattice mode (wfst_limits.lattice_links > 0).
static bool RawLatticeOfChannel(wfst_decoder *dec, int channel, Lattice *ofst, bool use_final_probs) {
  ofst->DeleteStates();
  int32_t ns = 0, na = 0;
  int rc = wfst_decoder_get_raw_lattice(dec, channel, use_final_probs ? 1 : 0, 0, 0, &ns, &na, nullptr, nullptr, nullptr,
                                        nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  if (rc == WFST_E_STATE) { Warn(wfst_last_error()); return false; }
  if (rc != WFST_OK && !(rc == WFST_E_CAPACITY && ns > 0)) Fatal("GetRawLattice");
  if (ns == 0) {
    if (!use_final_probs)  // base-inl.h:879-884
      Warn("You cannot call FinalizeDecoding() and then call GetRawLattice() with use_final_probs == false");
    return false;
  }
  std::vector<int32_t> fin(ns), src(na), dst(na), il(na), ol(na);
  std::vector<float> g(na), ac(na);
  if (wfst_decoder_get_raw_lattice(dec, channel, 1, ns, na, &ns, &na, fin.data(), nullptr, nullptr, nullptr, src.data(),
                                   dst.data(), il.data(), ol.data(), g.data(), ac.data()) != WFST_OK)
    Fatal("GetRawLattice");
  for (int s = 0; s < ns; ++s) {
    StateId id = ofst->AddState();
    if (fin[s]) ofst->SetFinal(id);
  }
  ofst->SetStart(0);
  for (int k = 0; k < na; ++k) ofst->AddArc(src[k], LatticeArc(il[k], ol[k], dst[k], LatticeWeight(g[k], ac[k])));
  return ofst->NumStates() > 0;
}

// GetLattice (base-inl.h:850-866) of one channel: the determinized lattice, built on the device.
static bool DetLatticeOfChannel(wfst_decoder *dec, int channel, Lattice *ofst, bool use_final_probs) {
  ofst->DeleteStates();
  int32_t ns = 0, na = 0;
  int rc = wfst_decoder_get_determinized_lattice(dec, channel, use_final_probs ? 1 : 0, 0, 0, &ns, &na, nullptr, nullptr, nullptr,
                                                 nullptr, nullptr, nullptr, nullptr);
  if (rc == WFST_E_STATE) { Warn(wfst_last_error()); return false; }
  if (rc != WFST_OK && !(rc == WFST_E_CAPACITY && ns > 0)) Fatal("GetLattice");
  if (ns == 0) return false;
  std::vector<int32_t> fin(ns), src(na), dst(na), il(na), ol(na);
  std::vector<float> g(na), ac(na);
  if (wfst_decoder_get_determinized_lattice(dec, channel, use_final_probs ? 1 : 0, ns, na, &ns, &na, fin.data(), src.data(), dst.data(),
                                            il.data(), ol.data(), g.data(), ac.data()) != WFST_OK)
    Fatal("GetLattice");
  for (int s = 0; s < ns; ++s) {
    StateId id = ofst->AddState();
    if (fin[s]) ofst->SetFinal(id);
  }
  ofst->SetStart(0);
  for (int k = 0; k < na; ++k) ofst->AddArc(src[k], LatticeArc(il[k], ol[k], dst[k], LatticeWeight(g[k], ac[k])));
  return true;
}

// GetLattice under --use-second (kaldi-nnet3/kaldi-online-nnet3-my-decoder.cc:53-78): determinized lattice o old LM (scale -1) o new LM,
// ComposeLattice twice on the device.
static bool RescoredLatticeOfChannel(wfst_decoder *dec, int channel, Lattice *ofst, ArpaLm *oldlm, ArpaLm *newlm, bool use_final_probs) {
  ofst->DeleteStates();
  if (!oldlm || !newlm) throw std::runtime_error("second-pass GetLattice needs both LMs");
  int32_t ns = 0, na = 0;
  int rc = wfst_decoder_get_rescored_lattice(dec, channel, use_final_probs ? 1 : 0, oldlm->Handle(), newlm->Handle(), 0, 0, &ns, &na, nullptr,
                                             nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  if (rc == WFST_E_STATE) { Warn(wfst_last_error()); return false; }
  if (rc != WFST_OK && !(rc == WFST_E_CAPACITY && ns > 0)) Fatal("GetLattice (second pass)");
  if (ns == 0) return false;
  std::vector<int32_t> fin(ns), src(na), dst(na), il(na), ol(na);
  std::vector<float> g(na), ac(na);
  if (wfst_decoder_get_rescored_lattice(dec, channel, use_final_probs ? 1 : 0, oldlm->Handle(), newlm->Handle(), ns, na, &ns, &na, fin.data(),
                                        src.data(), dst.data(), il.data(), ol.data(), g.data(), ac.data()) != WFST_OK)
    Fatal("GetLattice (second pass)");
  for (int s = 0; s < ns; ++s) {
    StateId id = ofst->AddState();
    if (fin[s]) ofst->SetFinal(id);
  }
  ofst->SetStart(0);
  for (int k = 0; k < na; ++k) ofst->AddArc(src[k], LatticeArc(il[k], ol[k], dst[k], LatticeWeight(g[k], ac[k])));
  return true;
}

static bool ShortlistOfChannel(wfst_decoder *dec, int channel, std::vector<Lattice> &out, int n) {
  out.clear();
  if (n <= 0) return false;
  const int max_words = 1024;
  int32_t np = 0;
  std::vector<int32_t> nw((size_t)n), words((size_t)n * max_words);
  std::vector<float> tot((size_t)n), lm((size_t)n);
  const int32_t ch = channel;
  int rc = wfst_decoder_get_nbest(dec, &ch, 1, n, max_words, &np, nw.data(), words.data(), tot.data(), lm.data());
  if (rc == WFST_E_STATE) { Warn(wfst_last_error()); return false; }
  if (rc != WFST_OK) Fatal("GetNbest");
  for (int k = 0; k < np; ++k) {
    Lattice lat;
    StateId cur = lat.AddState();
    lat.SetStart(cur);
    const int L = std::min(nw[k], max_words);
    // the path weight rides on the first arc (an <eps> arc when the path has no word)
    for (int j = 0; j < std::max(L, 1); ++j) {
      StateId next = lat.AddState();
      const LatticeWeight w = j == 0 ? LatticeWeight(lm[k], tot[k] - lm[k]) : LatticeWeight(0.0f, 0.0f);
      lat.AddArc(cur, LatticeArc(0, L ? words[(size_t)k * max_words + j] : 0, next, w));
      cur = next;
    }
    lat.SetFinal(cur);
    out.push_back(lat);
  }
  return !out.empty();
}

// GetNbest as the service defines it: NShortestPath over GetLattice's result, every path a linear lattice shaped as
// ConvertNbestToVector leaves it (newfst/lattice-to-nbest.cc:149-199): an <eps> arc of weight One in front (the start state the
// second Reverse adds), the lattice's arcs, the final weight's arc, the super-final state's arc and the first Reverse's <eps>.
static bool NbestOfChannel(wfst_decoder *dec, int channel, std::vector<Lattice> &out, int n, ArpaLm *oldlm, ArpaLm *newlm) {
  out.clear();
  if (n <= 0) return false;
  if ((oldlm == nullptr) != (newlm == nullptr)) throw std::runtime_error("second-pass GetNbest needs both LMs");
  const wfst_lm *l1 = oldlm ? oldlm->Handle() : nullptr, *l2 = newlm ? newlm->Handle() : nullptr;
  int32_t np = 0, na = 0;
  std::vector<int32_t> off((size_t)n + 1), ol((size_t)n * 128);
  std::vector<float> tot((size_t)n), g(ol.size()), ac(ol.size());
  int rc = wfst_decoder_get_nbest_paths(dec, channel, n, 1, l1, l2, n, (int32_t)ol.size(), &np, &na, off.data(), tot.data(), ol.data(), g.data(), ac.data());
  if (rc == WFST_E_CAPACITY && na > (int32_t)ol.size()) {
    ol.resize((size_t)na); g.resize((size_t)na); ac.resize((size_t)na);
    rc = wfst_decoder_get_nbest_paths(dec, channel, n, 1, l1, l2, n, na, &np, &na, off.data(), tot.data(), ol.data(), g.data(), ac.data());
  }
  if (rc == WFST_E_STATE) { Warn(wfst_last_error()); return false; }
  if (rc != WFST_OK) Fatal("GetNbest");
  for (int k = 0; k < np; ++k) {
    Lattice lat;
    StateId cur = lat.AddState();
    lat.SetStart(cur);
    auto add = [&](int word, float w1, float w2) {
      StateId next = lat.AddState();
      lat.AddArc(cur, LatticeArc(0, word, next, LatticeWeight(w1, w2)));
      cur = next;
    };
    add(0, 0.0f, 0.0f);
    for (int j = off[k]; j < off[k + 1]; ++j) add(ol[j], g[j], ac[j]);
    add(0, 0.0f, 0.0f);
    add(0, 0.0f, 0.0f);
    lat.SetFinal(cur);
    out.push_back(lat);
  }
  return !out.empty();
}

bool GpuLatticeDecoder::GetNbest(std::vector<Lattice> &nbest_paths, int n) {
  bool ok = false;
  OnDevice([&] { ok = NbestOfChannel(_dec, _chan, nbest_paths, n, nullptr, nullptr); });
  return ok;
}
bool GpuLatticeDecoder::GetNbest(std::vector<Lattice> &nbest_paths, int n, ArpaLm *oldlm, ArpaLm *newlm) {
  bool ok = false;
  OnDevice([&] { ok = NbestOfChannel(_dec, _chan, nbest_paths, n, oldlm, newlm); });
  return ok;
}
bool GpuLatticeDecoder::GetNbestShortlist(std::vector<Lattice> &nbest_paths, int n) {
  bool ok = false;
  OnDevice([&] { ok = ShortlistOfChannel(_dec, _chan, nbest_paths, n); });
  return ok;
}

bool GpuLatticeDecoder::GetLattice(Lattice *ofst, bool use_final_probs) {
  bool ok = false;
  OnDevice([&] { ok = DetLatticeOfChannel(_dec, _chan, ofst, use_final_probs); });
  return ok;
}
bool GpuLatticeDecoder::GetLattice(Lattice *ofst, ArpaLm *oldlm, ArpaLm *newlm, bool use_final_probs) {
  bool ok = false;
  OnDevice([&] { ok = RescoredLatticeOfChannel(_dec, _chan, ofst, oldlm, newlm, use_final_probs); });
  return ok;
}

bool GpuLatticeDecoder::GetRawLattice(Lattice *ofst, bool use_final_probs) {
  bool ok = false;
  OnDevice([&] { ok = RawLatticeOfChannel(_dec, _chan, ofst, use_final_probs); });
  return ok;
}

// ---- batch decoder ------------------------------------------------------------------------------
void GpuBatchDecoder::GetRawLattices(const std::vector<int> &channels, std::vector<Lattice> *ofsts, std::vector<bool> *ok,
                                     bool use_final_probs, int threads) {
  std::vector<int> ch(channels);
  if (ch.empty())
    for (int c = 0; c < _n; ++c) ch.push_back(c);
  const size_t n = ch.size();
  ofsts->assign(n, Lattice());
  std::vector<char> good(n, 0);
  if (n == 0) { ok->clear(); return; }
  good[0] = RawLatticeOfChannel(_dec, ch[0], &(*ofsts)[0], use_final_probs);  // fetches every finalized channel's lists
  int nt = threads > 0 ? threads : (int)std::min<size_t>(16, std::max(1u, std::thread::hardware_concurrency()));
  nt = (int)std::min<size_t>((size_t)nt, n);
  std::atomic<size_t> next(1);
  std::vector<std::string> errors((size_t)nt);
  auto work = [&](int k) {
    try {
      for (size_t i = next.fetch_add(1); i < n; i = next.fetch_add(1))
        good[i] = RawLatticeOfChannel(_dec, ch[i], &(*ofsts)[i], use_final_probs);
    } catch (const std::exception &e) {
      errors[(size_t)k] = e.what();
    }
  };
  std::vector<std::thread> pool;
  for (int k = 1; k < nt; ++k) pool.emplace_back(work, k);
  work(0);
  for (std::thread &t : pool) t.join();
  for (const std::string &e : errors)
    if (!e.empty()) throw std::runtime_error(e);
  ok->assign(good.begin(), good.end());
}
bool GpuBatchDecoder::GetNbest(int channel, std::vector<Lattice> &nbest_paths, int n) {
  return NbestOfChannel(_dec, channel, nbest_paths, n, nullptr, nullptr);
}
bool GpuBatchDecoder::GetNbest(int channel, std::vector<Lattice> &nbest_paths, int n, ArpaLm *oldlm, ArpaLm *newlm) {
  return NbestOfChannel(_dec, channel, nbest_paths, n, oldlm, newlm);
}
bool GpuBatchDecoder::GetNbestShortlist(int channel, std::vector<Lattice> &nbest_paths, int n) {
  return ShortlistOfChannel(_dec, channel, nbest_paths, n);
}
bool GpuBatchDecoder::GetLattice(int channel, Lattice *ofst, bool use_final_probs) {
  return DetLatticeOfChannel(_dec, channel, ofst, use_final_probs);
}
bool GpuBatchDecoder::GetLattice(int channel, Lattice *ofst, ArpaLm *oldlm, ArpaLm *newlm, bool use_final_probs) {
  return RescoredLatticeOfChannel(_dec, channel, ofst, oldlm, newlm, use_final_probs);
}
bool GpuBatchDecoder::GetRawLattice(int channel, Lattice *ofst, bool use_final_probs) {
  return RawLatticeOfChannel(_dec, channel, ofst, use_final_probs);
}
void GpuBatchDecoder::PrefetchLattices() {
  if (wfst_decoder_prefetch_determinized(_dec) != WFST_OK) Fatal("wfst_decoder_prefetch_determinized");
}
void GpuBatchDecoder::PrefetchLatticesDetached() {
  if (wfst_decoder_prefetch_determinized_detached(_dec) != WFST_OK) Fatal("wfst_decoder_prefetch_determinized_detached");
}
void GpuBatchDecoder::HarvestPrefetchedLattices() {
  if (wfst_decoder_harvest_prefetched(_dec) != WFST_OK) Fatal("wfst_decoder_harvest_prefetched");
}
bool GpuBatchDecoder::GetPrefetchedLattice(int channel, Lattice *ofst) {
  ofst->DeleteStates();
  int32_t ns = 0, na = 0;
  int rc = wfst_decoder_get_prefetched_lattice(_dec, channel, 0, 0, &ns, &na, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  if (rc == WFST_E_STATE) { Warn(wfst_last_error()); return false; }
  if (rc != WFST_OK && !(rc == WFST_E_CAPACITY && ns > 0)) Fatal("GetPrefetchedLattice");
  if (ns == 0) return false;
  std::vector<int32_t> fin(ns), src(na), dst(na), il(na), ol(na);
  std::vector<float> g(na), ac(na);
  if (wfst_decoder_get_prefetched_lattice(_dec, channel, ns, na, &ns, &na, fin.data(), src.data(), dst.data(), il.data(), ol.data(), g.data(),
                                          ac.data()) != WFST_OK)
    Fatal("GetPrefetchedLattice");
  for (int s = 0; s < ns; ++s) {
    StateId id = ofst->AddState();
    if (fin[s]) ofst->SetFinal(id);
  }
  ofst->SetStart(0);
  for (int k = 0; k < na; ++k) ofst->AddArc(src[k], LatticeArc(il[k], ol[k], dst[k], LatticeWeight(g[k], ac[k])));
  return true;
}
void GpuBatchDecoder::GetLattices(const std::vector<int> &channels, std::vector<Lattice> *ofsts, std::vector<bool> *ok, ArpaLm *oldlm,
                                  ArpaLm *newlm, bool use_final_probs) {
  if (!oldlm || !newlm) throw std::runtime_error("second-pass GetLattice needs both LMs");
  std::vector<int32_t> ch(channels.begin(), channels.end());
  const int rc = wfst_decoder_rescore_lattices(_dec, ch.empty() ? nullptr : ch.data(), (int32_t)ch.size(), use_final_probs ? 1 : 0,
                                               oldlm->Handle(), newlm->Handle());
  if (rc == WFST_E_STATE) Warn(wfst_last_error());   // (a channel that is not finalized: the per-channel calls below serve it)
  else if (rc != WFST_OK) Fatal("GetLattices");
  ofsts->assign(channels.size(), Lattice());
  ok->assign(channels.size(), false);
  for (size_t i = 0; i < channels.size(); ++i) (*ok)[i] = RescoredLatticeOfChannel(_dec, channels[i], &(*ofsts)[i], oldlm, newlm, use_final_probs);
}
void GpuBatchDecoder::GetNbests(const std::vector<int> &channels, std::vector<std::vector<Lattice> > *nbests, std::vector<bool> *ok, int n,
                                ArpaLm *oldlm, ArpaLm *newlm) {
  if ((oldlm == nullptr) != (newlm == nullptr)) throw std::runtime_error("second-pass GetNbest needs both LMs");
  nbests->assign(channels.size(), std::vector<Lattice>());
  ok->assign(channels.size(), false);
  if (n <= 0) return;
  std::vector<int32_t> ch(channels.begin(), channels.end());
  if (n <= 4096) {
    const int rc = wfst_decoder_nbest_paths_batch(_dec, ch.empty() ? nullptr : ch.data(), (int32_t)ch.size(), n, 1,
                                                  oldlm ? oldlm->Handle() : nullptr, newlm ? newlm->Handle() : nullptr);
    if (rc == WFST_E_STATE || rc == WFST_E_CAPACITY) Warn(wfst_last_error());   // (the per-channel calls below serve what the batch could not)
    else if (rc != WFST_OK) Fatal("GetNbests");
  }
  for (size_t i = 0; i < channels.size(); ++i) (*ok)[i] = NbestOfChannel(_dec, channels[i], (*nbests)[i], n, oldlm, newlm);
}
GpuBatchDecoder::GpuBatchDecoder(Fst *graph, const LatticeFasterDecoderConfig &config, int n_channels,
                                 const wfst_limits *limits, void *hip_stream)
    : _dec(nullptr), _n(n_channels) {
  config.Check();
  wfst_config c = config.ToC();
  if (wfst_decoder_create(graph->Handle(), &c, n_channels, limits, hip_stream, &_dec) != WFST_OK)
    Fatal("wfst_decoder_create");
}
GpuBatchDecoder::GpuBatchDecoder(Fst *graph, const LatticeFasterDecoderConfig &config, ArpaLm *oldlm, ArpaLm *newlm,
                                 int n_channels, const wfst_limits *limits, void *hip_stream)
    : _dec(nullptr), _n(n_channels) {
  config.Check();
  wfst_config c = config.ToC();
  if (!oldlm || !newlm) throw std::runtime_error("biglm decoder needs both LMs");
  if (wfst_decoder_create_biglm(graph->Handle(), &c, n_channels, limits, nullptr, oldlm->Handle(), newlm->Handle(), hip_stream,
                                &_dec) != WFST_OK)
    Fatal("wfst_decoder_create_biglm");
}
GpuBatchDecoder::~GpuBatchDecoder() { wfst_decoder_free(_dec); }

void GpuBatchDecoder::InitDecoding(const std::vector<int> &ch) {
  if (wfst_decoder_init(_dec, ch.empty() ? nullptr : ch.data(), (int)ch.size()) != WFST_OK) Fatal("InitDecoding");
}
void GpuBatchDecoder::AdvanceDecoding(const std::vector<int> &ch, const std::vector<const float *> &ll,
                                      const std::vector<int> &ready, int stride, int max_num_frames) {
  if (wfst_decoder_advance(_dec, ch.empty() ? nullptr : ch.data(), (int)ch.size(), ll.data(), ready.data(), stride,
                           max_num_frames) != WFST_OK)
    Fatal("AdvanceDecoding");
}
void GpuBatchDecoder::AdvanceDecodingHost(const std::vector<int> &ch, const std::vector<const float *> &ll,
                                          const std::vector<int> &ready, int stride, int max_num_frames) {
  if (wfst_decoder_advance_host(_dec, ch.empty() ? nullptr : ch.data(), (int)ch.size(), ll.data(), ready.data(),
                                stride, max_num_frames) != WFST_OK)
    Fatal("AdvanceDecoding");
}
void GpuBatchDecoder::FinalizeDecoding(const std::vector<int> &ch) {
  if (wfst_decoder_finalize(_dec, ch.empty() ? nullptr : ch.data(), (int)ch.size()) != WFST_OK)
    Fatal("FinalizeDecoding");
}
int GpuBatchDecoder::NumFramesDecoded(int channel) const { return wfst_decoder_num_frames_decoded(_dec, channel); }

// A best-path decoder does not fail at wfst_limits.max_tokens_per_frame, it goes on from the limit-th cheapest token (the limit
// acts as a max_active): the result may then differ from the reference's at the configured beam.  Said once per utterance and
// channel, where the reference would have said nothing because it has no such limit.
static void WarnDegraded(int channel, int n) {
  Warn("channel " + std::to_string(channel) + ": " + std::to_string(n) + " frame(s) held more tokens than max_tokens_per_frame; the search "
       "went on from the cheapest of them (a max_active): raise wfst_limits.max_tokens_per_frame for the result at the configured beam");
}
static void WarnIfDegraded(wfst_decoder *dec, int channel) {
  int32_t n = 0;
  if (wfst_decoder_get_degraded_frames(dec, channel, &n) == WFST_OK && n > 0) WarnDegraded(channel, n);
}

void GpuBatchDecoder::GetBestPaths(const std::vector<int> &channels, std::vector<Lattice> *ofsts,
                                   std::vector<bool> *ok, bool use_final_probs) {
  const int cnt = channels.empty() ? _n : (int)channels.size();
  int maxf = 1;
  for (int i = 0; i < cnt; ++i) maxf = std::max(maxf, NumFramesDecoded(channels.empty() ? i : channels[i]));
  int cap = 4 * maxf + 64;
  ofsts->assign(cnt, Lattice());
  ok->assign(cnt, false);
  for (int attempt = 0; attempt < 2; ++attempt) {
    std::vector<int32_t> il((size_t)cnt * cap), ol((size_t)cnt * cap), n(cnt);
    std::vector<float> g((size_t)cnt * cap), ac((size_t)cnt * cap);
    int rc = wfst_decoder_get_best_path(_dec, channels.empty() ? nullptr : channels.data(), (int)channels.size(),
                                        use_final_probs ? 1 : 0, cap, il.data(), ol.data(), g.data(), ac.data(), n.data());
    if (rc == WFST_E_CAPACITY && *std::max_element(n.begin(), n.end()) > cap) {
      cap = *std::max_element(n.begin(), n.end());
      continue;
    }
    if (rc == WFST_E_STATE) throw std::runtime_error(wfst_last_error());
    if (rc != WFST_OK) Fatal("GetBestPath");
    for (int i = 0; i < cnt; ++i) {
      WarnIfDegraded(_dec, channels.empty() ? i : channels[i]);
      if (n[i] == 0) continue;
      HopsToLattice(&il[(size_t)i * cap], &ol[(size_t)i * cap], &g[(size_t)i * cap], &ac[(size_t)i * cap], n[i],
                    &(*ofsts)[i]);
      (*ok)[i] = true;
    }
    return;
  }
}

void GpuBatchDecoder::EndpointDetected(const std::vector<int> &channels, const OnlineEndpointConfig &config, std::vector<bool> *detected,
                                       std::vector<int> *rule) {
  std::vector<int32_t> phones;
  const wfst_endpoint_config c = config.ToC(&phones);
  const std::string k = EndpointKey(c);
  if (k != _ep_key) {
    if (wfst_decoder_set_endpoint_config(_dec, &c) != WFST_OK) Fatal("EndpointDetected");
    _ep_key = k;
  }
  std::vector<int32_t> ch(channels.begin(), channels.end()), r(channels.size());
  if (!ch.empty() && wfst_decoder_endpoint_detected(_dec, ch.data(), (int32_t)ch.size(), nullptr, r.data(), nullptr, nullptr) != WFST_OK)
    Fatal("EndpointDetected");
  detected->assign(channels.size(), false);
  for (size_t i = 0; i < r.size(); ++i) (*detected)[i] = r[i] != 0;
  if (rule) rule->assign(r.begin(), r.end());
}

void GpuBatchDecoder::GetPartialWords(const std::vector<int> &channels, std::vector<std::vector<int> > *words, std::vector<int> *n_stable,
                                      std::vector<int> *stable_frame) {
  const int cnt = (int)channels.size();
  words->assign((size_t)cnt, std::vector<int>());
  if (n_stable) n_stable->assign((size_t)cnt, 0);
  if (stable_frame) stable_frame->assign((size_t)cnt, 0);
  if (cnt == 0) return;
  std::vector<int32_t> ch(channels.begin(), channels.end()), nw((size_t)cnt, 0), ns((size_t)cnt, 0), sf((size_t)cnt, 0);
  int32_t cap = 65;
  for (int c : channels) cap = std::max(cap, (c >= 0 && c < _n ? wfst_decoder_num_frames_decoded(_dec, c) : 0) + 64);
  for (int attempt = 0; attempt < 2; ++attempt) {
    std::vector<int32_t> w((size_t)cnt * (size_t)cap);
    const int rc = wfst_decoder_get_partial(_dec, ch.data(), cnt, cap, w.data(), nw.data(), ns.data(), sf.data());
    if (rc == WFST_E_CAPACITY && *std::max_element(nw.begin(), nw.end()) > cap && attempt == 0) { cap = *std::max_element(nw.begin(), nw.end()); continue; }
    if (rc != WFST_OK) Fatal("GetPartialWords");
    for (int i = 0; i < cnt; ++i) {
      (*words)[(size_t)i].assign(w.begin() + (long)((size_t)i * cap), w.begin() + (long)((size_t)i * cap) + nw[(size_t)i]);
      if (n_stable) (*n_stable)[(size_t)i] = ns[(size_t)i];
      if (stable_frame) (*stable_frame)[(size_t)i] = sf[(size_t)i];
    }
    return;
  }
}
bool GpuBatchDecoder::GetPartialWords(int channel, std::vector<int> *words, int *n_stable) {
  std::vector<std::vector<int> > w;
  std::vector<int> ns;
  GetPartialWords(std::vector<int>(1, channel), &w, &ns);
  *words = w[0];
  if (n_stable) *n_stable = ns[0];
  return NumFramesDecoded(channel) > 0;
}
bool GpuBatchDecoder::EndpointDetected(int channel, const OnlineEndpointConfig &config, int *rule) {
  std::vector<bool> d;
  std::vector<int> r;
  EndpointDetected(std::vector<int>(1, channel), config, &d, &r);
  if (rule) *rule = r[0];
  return d[0];
}

bool GpuBatchDecoder::GetBestPath(int channel, Lattice *ofst, bool use_final_probs) {
  std::vector<Lattice> l;
  std::vector<bool> ok;
  GetBestPaths(std::vector<int>(1, channel), &l, &ok, use_final_probs);
  *ofst = l[0];
  return ok[0];
}

// ---- the n-best text of channel lists (wfst_decoder_get_nbest_words) ------------------------------------------------------------
// One C-ABI call for `ch`; words / tot / lm [i][k] of listed channel i's path k, status[i] its own code.  A path with more words
// than the first capacity: once more with the size the call reports.  Returns the call's own code.
static int NbestWordsCall(wfst_decoder *dec, const std::vector<int32_t> &ch, int n, bool use_final_probs, const wfst_lm *l1, const wfst_lm *l2,
                          std::vector<std::vector<std::vector<int> > > *words, std::vector<std::vector<float> > *tot,
                          std::vector<std::vector<float> > *lm, std::vector<int> *status) {
  if (!wfst_decoder_get_nbest_words) throw std::runtime_error("GetNbestWords: this build's device library has no wfst_decoder_get_nbest_words");
  const size_t cnt = ch.size(), np = (size_t)std::max(n, 1);
  int32_t cap = 64;
  for (int32_t c : ch) cap = std::max(cap, wfst_decoder_num_frames_decoded(dec, c) / 4 + 64);
  std::vector<int32_t> st(cnt), got(cnt), nw(cnt * np);
  std::vector<float> t(cnt * np), l(cnt * np);
  for (int attempt = 0; attempt < 2; ++attempt) {
    std::vector<int32_t> w(cnt * np * (size_t)cap);
    const int rc = wfst_decoder_get_nbest_words(dec, ch.data(), (int32_t)cnt, n, use_final_probs ? 1 : 0, l1, l2, cap, st.data(), got.data(), nw.data(),
                                                w.data(), t.data(), l.data(), nullptr);
    if (rc != WFST_OK) return rc;
    const int32_t longest = nw.empty() ? 0 : *std::max_element(nw.begin(), nw.end());
    if (longest > cap && attempt == 0) { cap = longest; continue; }
    words->assign(cnt, std::vector<std::vector<int> >());
    tot->assign(cnt, std::vector<float>());
    lm->assign(cnt, std::vector<float>());
    for (size_t i = 0; i < cnt; ++i)
      for (int32_t k = 0; k < got[i]; ++k) {
        const int32_t *p = w.data() + (i * np + (size_t)k) * (size_t)cap;
        (*words)[i].push_back(std::vector<int>(p, p + std::min(nw[i * np + (size_t)k], cap)));
        (*tot)[i].push_back(t[i * np + (size_t)k]);
        (*lm)[i].push_back(l[i * np + (size_t)k]);
      }
    break;
  }
  status->assign(st.begin(), st.end());
  return WFST_OK;
}

// GetNbestWords of every waiting channel: the requests grouped by what they ask -- (n, use_final_probs, LM pair): a service has
// one -- and one wfst_decoder_get_nbest_words per group; a list the library refuses is retried request by request
void GpuChannelPool::ExecuteNbestWords(std::vector<Request *> &requests) {
  typedef std::tuple<int, bool, const wfst_lm *, const wfst_lm *> Key;
  std::map<Key, std::vector<Request *> > groups;
  for (Request *r : requests) groups[Key(r->nb_n, r->use_final_probs, r->nb_old, r->nb_new)].push_back(r);
  for (auto &gr : groups) {
    auto call = [&](const std::vector<Request *> &rs) {
      std::vector<int32_t> ch;
      for (Request *r : rs) ch.push_back(r->channel);
      std::vector<std::vector<std::vector<int> > > w;
      std::vector<std::vector<float> > t, l;
      std::vector<int> st;
      const int rc = NbestWordsCall(_dec, ch, std::get<0>(gr.first), std::get<1>(gr.first), std::get<2>(gr.first), std::get<3>(gr.first), &w, &t, &l, &st);
      if (rc == WFST_OK)
        for (size_t i = 0; i < rs.size(); ++i) { rs[i]->nb_words.swap(w[i]); rs[i]->nb_tot.swap(t[i]); rs[i]->nb_lm.swap(l[i]); rs[i]->nb_status = st[i]; }
      std::lock_guard<std::mutex> lk(_mu);
      _stats.nbest_words_calls += 1;
      _stats.nbest_words_requests += (long long)rs.size();
      return rc;
    };
    try {
      if (call(gr.second) == WFST_OK) continue;
      for (Request *r : gr.second)
        if (gr.second.size() == 1 || call(std::vector<Request *>(1, r)) != WFST_OK)
          r->error = std::make_exception_ptr(std::runtime_error(std::string("GetNbestWords: ") + wfst_last_error()));
    } catch (...) {
      for (Request *r : gr.second) r->error = std::current_exception();
    }
  }
}

bool GpuLatticeDecoder::GetNbestWords(std::vector<std::vector<int> > *words, std::vector<float> *tot, std::vector<float> *lm, int n,
                                      bool use_final_probs, ArpaLm *oldlm, ArpaLm *newlm, int *status) {
  const wfst_lm *l1 = oldlm ? oldlm->Handle() : nullptr, *l2 = newlm ? newlm->Handle() : nullptr;
  std::vector<std::vector<int> > w;
  std::vector<float> t, l;
  int st = WFST_OK;
  if (_pool) {
    GpuChannelPool::Request q;
    q.kind = GpuChannelPool::kNbestWords;
    q.channel = _chan;
    q.nb_n = n;
    q.use_final_probs = use_final_probs;
    q.nb_old = l1;
    q.nb_new = l2;
    _pool->Submit(&q);
    _decoded = q.decoded;
    w.swap(q.nb_words); t.swap(q.nb_tot); l.swap(q.nb_lm);
    st = q.nb_status;
  } else {
    std::vector<std::vector<std::vector<int> > > ww;
    std::vector<std::vector<float> > tt, ll;
    std::vector<int> ss;
    if (NbestWordsCall(_dec, std::vector<int32_t>(1, 0), n, use_final_probs, l1, l2, &ww, &tt, &ll, &ss) != WFST_OK) Fatal("GetNbestWords");
    w.swap(ww[0]); t.swap(tt[0]); l.swap(ll[0]);
    st = ss[0];
  }
  if (status) *status = st;
  else if (st != WFST_OK && !(st == WFST_E_CAPACITY && !w.empty())) throw std::runtime_error(std::string("GetNbestWords: ") + wfst_last_error());
  if (words) words->swap(w);
  if (tot) tot->swap(t);
  if (lm) lm->swap(l);
  return words ? !words->empty() : !w.empty();
}

void GpuBatchDecoder::GetNbestWords(const std::vector<int> &channels, int n, ArpaLm *oldlm, ArpaLm *newlm, bool use_final_probs,
                                    std::vector<std::vector<std::vector<int> > > *words, std::vector<std::vector<float> > *tot,
                                    std::vector<std::vector<float> > *lm, std::vector<int> *status) {
  std::vector<int32_t> ch(channels.begin(), channels.end());
  if (ch.empty())
    for (int c = 0; c < _n; ++c) ch.push_back(c);
  std::vector<std::vector<std::vector<int> > > w;
  std::vector<std::vector<float> > t, l;
  std::vector<int> st;
  if (NbestWordsCall(_dec, ch, n, use_final_probs, oldlm ? oldlm->Handle() : nullptr, newlm ? newlm->Handle() : nullptr, &w, &t, &l, &st) != WFST_OK)
    Fatal("GetNbestWords");
  if (words) words->swap(w);
  if (tot) tot->swap(t);
  if (lm) lm->swap(l);
  if (status) *status = st;
}

// ---- the word queries of a raw lattice: what AlignWords, WordConfidences and NearestWords do alike ------------------------------------
namespace {
typedef std::vector<std::vector<std::vector<int> > > SeqLists;   // [listed channel][sequence][word]

// seqs[i][q] as the C ABI takes them: words[cnt][ns][cap] (padded with 0) and len[cnt][ns] (-1: the channel has no such sequence)
struct PackedSeqs {
  size_t cnt, ns = 1, cap = 1, np;
  std::vector<int32_t> words, len;
  explicit PackedSeqs(const SeqLists &seqs) : cnt(seqs.size()) {
    for (const auto &s : seqs) {
      ns = std::max(ns, s.size());
      for (const auto &w : s) cap = std::max(cap, w.size());
    }
    np = cnt * ns;
    words.assign(np * cap, 0);
    len.assign(np, -1);
    for (size_t i = 0; i < cnt; ++i)
      for (size_t q = 0; q < seqs[i].size(); ++q) {
        len[i * ns + q] = (int32_t)seqs[i][q].size();
        std::copy(seqs[i][q].begin(), seqs[i][q].end(), words.begin() + (i * ns + q) * cap);
      }
  }
};

// GpuBatchDecoder's wrapper: call(ch, &out, &status) is one C-ABI call for the listed channels (none listed: all n_channels)
template <class T, class Call>
void BatchWordQuery(const char *what, const std::vector<int> &channels, int n_channels, std::vector<std::vector<T> > *out,
                    std::vector<int> *status, Call call) {
  std::vector<int32_t> ch(channels.begin(), channels.end());
  if (ch.empty())
    for (int c = 0; c < n_channels; ++c) ch.push_back(c);
  std::vector<std::vector<T> > o;
  std::vector<int> st;
  if (call(ch, &o, &st) != WFST_OK) Fatal(what);
  if (!status)
    for (int s : st)
      if (s != WFST_OK) Fatal(what);
  if (out) out->swap(o);
  if (status) *status = st;
}

// GpuLatticeDecoder's wrapper: call(ch, seqs, &out, &status) for the one channel, inside on_device (OnDevice: the C-ABI calls of one
// decoder are not re-entrant, over a pool this runs in the batcher thread, like GetNbest)
template <class T, class Run, class Call>
void StreamWordQuery(const char *what, int chan, const std::vector<std::vector<int> > &seqs, std::vector<T> *out, Run on_device, Call call) {
  std::vector<std::vector<T> > o;
  if (!seqs.empty()) {
    std::vector<int> st;
    int rc = WFST_OK;
    std::string msg;
    on_device([&] {
      rc = call(std::vector<int32_t>(1, chan), SeqLists(1, seqs), &o, &st);
      if (rc != WFST_OK || st[0] != WFST_OK) msg = wfst_last_error();
    });
    if (rc != WFST_OK || st[0] != WFST_OK) throw std::runtime_error(std::string(what) + ": " + msg);
  }
  if (out) {
    out->clear();
    if (!o.empty()) out->swap(o[0]);
  }
}
}  // namespace

// ---- word times for any word sequence of the lattice (wfst_decoder_align_words) -----------------------------------------------------
// One C-ABI call for `ch`: (*out)[i][q] for seqs[i][q], (*status)[i] the channel's own code.  Returns the call's own code.
static int AlignWordsCall(wfst_decoder *dec, const std::vector<int32_t> &ch, const SeqLists &seqs, bool use_final_probs, long long max_cells,
                          std::vector<std::vector<WordAlignment> > *out, std::vector<int> *status) {
  if (!wfst_decoder_align_words) throw std::runtime_error("AlignWords: this build's device library has no wfst_decoder_align_words");
  if (seqs.size() != ch.size()) throw std::runtime_error("AlignWords: one list of sequences per listed channel");
  const PackedSeqs in(seqs);
  const size_t cnt = in.cnt, ns = in.ns, cap = in.cap, np = in.np;
  std::vector<int32_t> st(cnt), found(np), na(np), b(np * cap), e(np * cap);
  std::vector<float> t(np), l(np);
  const int rc = wfst_decoder_align_words(dec, ch.data(), (int32_t)cnt, use_final_probs ? 1 : 0, (int32_t)ns, (int32_t)cap, in.words.data(),
                                          in.len.data(), max_cells, st.data(), found.data(), na.data(), b.data(), e.data(), t.data(), l.data());
  if (rc != WFST_OK) return rc;
  out->assign(cnt, std::vector<WordAlignment>());
  for (size_t i = 0; i < cnt; ++i) {
    (*out)[i].resize(seqs[i].size());
    for (size_t q = 0; q < seqs[i].size(); ++q) {
      WordAlignment &a = (*out)[i][q];
      const size_t p = i * ns + q;
      a.found = found[p] != 0;
      if (!a.found) continue;
      a.n_arcs = na[p]; a.tot = t[p]; a.lm = l[p];
      for (size_t k = 0; k < seqs[i][q].size(); ++k) a.frames.push_back(std::make_pair(b[p * cap + k], e[p * cap + k]));
    }
  }
  status->assign(st.begin(), st.end());
  return WFST_OK;
}

void GpuBatchDecoder::AlignWords(const std::vector<int> &channels, const std::vector<std::vector<std::vector<int> > > &seqs, bool use_final_probs,
                                 std::vector<std::vector<WordAlignment> > *out, std::vector<int> *status, long long max_cells) {
  BatchWordQuery("AlignWords", channels, _n, out, status, [&](const auto &ch, auto *o, auto *st) {
    return AlignWordsCall(_dec, ch, seqs, use_final_probs, max_cells, o, st);
  });
}

void GpuLatticeDecoder::GetNbestWordTimes(const std::vector<std::vector<int> > &nbest, std::vector<WordAlignment> *out, bool use_final_probs) {
  StreamWordQuery("AlignWords", _chan, nbest, out, [&](auto &&f) { OnDevice(f); },
                  [&](const auto &ch, const SeqLists &seqs, auto *o, auto *st) {
                    return AlignWordsCall(_dec, ch, seqs, use_final_probs, 0, o, st);
                  });
}

bool GpuLatticeDecoder::AlignWords(const std::vector<int> &words, std::vector<std::pair<int, int> > *frames, float *tot, float *lm, bool use_final_probs) {
  std::vector<WordAlignment> a;
  GetNbestWordTimes(std::vector<std::vector<int> >(1, words), &a, use_final_probs);
  if (frames) frames->swap(a[0].frames);
  if (tot) *tot = a[0].tot;
  if (lm) *lm = a[0].lm;
  return a[0].found;
}

// ---- word confidences from the lattice's posteriors (wfst_decoder_word_confidence) -----------------------------------------------------
// One C-ABI call for `ch`: (*out)[i][q] for seqs[i][q], (*status)[i] the channel's own code.  Returns the call's own code.
static int WordConfidencesCall(wfst_decoder *dec, const std::vector<int32_t> &ch, const SeqLists &seqs, bool use_final_probs, double graph_scale,
                               double acoustic_scale, long long max_cells, std::vector<std::vector<WordConfidence> > *out, std::vector<int> *status) {
  if (!wfst_decoder_word_confidence) throw std::runtime_error("WordConfidences: this build's device library has no wfst_decoder_word_confidence");
  if (seqs.size() != ch.size()) throw std::runtime_error("WordConfidences: one list of sequences per listed channel");
  const PackedSeqs in(seqs);
  const size_t cnt = in.cnt, ns = in.ns, cap = in.cap, np = in.np;
  std::vector<int32_t> st(cnt), found(np), na(np), b(np * cap), e(np * cap);
  std::vector<float> t(np), l(np);
  std::vector<double> lz(cnt), wp(np * cap), plp(np);
  const int rc = wfst_decoder_word_confidence(dec, ch.data(), (int32_t)cnt, use_final_probs ? 1 : 0, graph_scale, acoustic_scale, (int32_t)ns,
                                              (int32_t)cap, in.words.data(), in.len.data(), max_cells, st.data(), lz.data(), found.data(), na.data(),
                                              b.data(), e.data(), wp.data(), plp.data(), t.data(), l.data());
  if (rc != WFST_OK) return rc;
  out->assign(cnt, std::vector<WordConfidence>());
  for (size_t i = 0; i < cnt; ++i) {
    (*out)[i].resize(seqs[i].size());
    for (size_t q = 0; q < seqs[i].size(); ++q) {
      WordConfidence &a = (*out)[i][q];
      const size_t p = i * ns + q;
      a.log_z = lz[i];
      a.found = found[p] != 0;
      if (!a.found) continue;
      a.n_arcs = na[p]; a.tot = t[p]; a.lm = l[p]; a.path_logpost = plp[p];
      for (size_t k = 0; k < seqs[i][q].size(); ++k) {
        a.frames.push_back(std::make_pair(b[p * cap + k], e[p * cap + k]));
        a.word_post.push_back(wp[p * cap + k]);
        a.conf.push_back(std::min(1.0, wp[p * cap + k]));
      }
    }
  }
  status->assign(st.begin(), st.end());
  return WFST_OK;
}

void GpuBatchDecoder::WordConfidences(const std::vector<int> &channels, const std::vector<std::vector<std::vector<int> > > &seqs, bool use_final_probs,
                                      double graph_scale, double acoustic_scale, std::vector<std::vector<WordConfidence> > *out,
                                      std::vector<int> *status, long long max_cells) {
  BatchWordQuery("WordConfidences", channels, _n, out, status, [&](const auto &ch, auto *o, auto *st) {
    return WordConfidencesCall(_dec, ch, seqs, use_final_probs, graph_scale, acoustic_scale, max_cells, o, st);
  });
}

void GpuLatticeDecoder::WordConfidences(const std::vector<std::vector<int> > &seqs, std::vector<WordConfidence> *out, bool use_final_probs,
                                        double graph_scale, double acoustic_scale) {
  StreamWordQuery("WordConfidences", _chan, seqs, out, [&](auto &&f) { OnDevice(f); },
                  [&](const auto &ch, const SeqLists &s, auto *o, auto *st) {
                    return WordConfidencesCall(_dec, ch, s, use_final_probs, graph_scale, acoustic_scale, 0, o, st);
                  });
}

// ---- word alternatives per slot (wfst_decoder_word_alternatives) -----------------------------------------------------------------------
// One C-ABI call for `ch`: (*out)[i][q] for seqs[i][q], (*status)[i] the channel's own code.  Returns the call's own code.
static int WordAlternativesCall(wfst_decoder *dec, const std::vector<int32_t> &ch, const SeqLists &seqs, int n_alts, bool use_final_probs,
                                double graph_scale, double acoustic_scale, long long max_cells,
                                std::vector<std::vector<struct WordAlternatives> > *out, std::vector<int> *status) {
  if (!wfst_decoder_word_alternatives)
    throw std::runtime_error("WordAlternatives: this build's device library has no wfst_decoder_word_alternatives");
  if (seqs.size() != ch.size()) throw std::runtime_error("WordAlternatives: one list of sequences per listed channel");
  const PackedSeqs in(seqs);
  const size_t cnt = in.cnt, ns = in.ns, cap = in.cap, np = in.np, K = (size_t)std::max(n_alts, 1);
  std::vector<int32_t> st(cnt), found(np), na(np), b(np * cap), e(np * cap), nd(np * cap), aw(np * cap * K);
  std::vector<float> t(np), l(np);
  std::vector<double> lz(cnt), wp(np * cap), nop(np * cap), ap(np * cap * K), plp(np);
  const int rc = wfst_decoder_word_alternatives(dec, ch.data(), (int32_t)cnt, use_final_probs ? 1 : 0, graph_scale, acoustic_scale, n_alts,
                                                (int32_t)ns, (int32_t)cap, in.words.data(), in.len.data(), max_cells, st.data(), lz.data(),
                                                found.data(), na.data(), b.data(), e.data(), wp.data(), nop.data(), nd.data(), aw.data(),
                                                ap.data(), plp.data(), t.data(), l.data());
  if (rc != WFST_OK) return rc;
  out->assign(cnt, std::vector<struct WordAlternatives>());
  for (size_t i = 0; i < cnt; ++i) {
    (*out)[i].resize(seqs[i].size());
    for (size_t q = 0; q < seqs[i].size(); ++q) {
      struct WordAlternatives &a = (*out)[i][q];
      const size_t p = i * ns + q;
      a.log_z = lz[i];
      a.found = found[p] != 0;
      if (!a.found) continue;
      a.n_arcs = na[p]; a.tot = t[p]; a.lm = l[p]; a.path_logpost = plp[p];
      for (size_t k = 0; k < seqs[i][q].size(); ++k) {
        const size_t at = p * cap + k;
        a.frames.push_back(std::make_pair(b[at], e[at]));
        a.word_post.push_back(wp[at]);
        a.conf.push_back(std::min(1.0, wp[at]));
        a.none_post.push_back(nop[at]);
        a.n_distinct.push_back(nd[at]);
        a.alts.push_back(std::vector<std::pair<int, double> >());
        for (size_t j = 0; j < std::min(K, (size_t)nd[at]); ++j) a.alts.back().push_back(std::make_pair((int)aw[at * K + j], ap[at * K + j]));
      }
    }
  }
  status->assign(st.begin(), st.end());
  return WFST_OK;
}

void GpuBatchDecoder::WordAlternatives(const std::vector<int> &channels, const std::vector<std::vector<std::vector<int> > > &seqs, int n_alts,
                                       bool use_final_probs, double graph_scale, double acoustic_scale,
                                       std::vector<std::vector<struct WordAlternatives> > *out, std::vector<int> *status, long long max_cells) {
  BatchWordQuery("WordAlternatives", channels, _n, out, status, [&](const auto &ch, auto *o, auto *st) {
    return WordAlternativesCall(_dec, ch, seqs, n_alts, use_final_probs, graph_scale, acoustic_scale, max_cells, o, st);
  });
}

void GpuLatticeDecoder::WordAlternatives(const std::vector<std::vector<int> > &seqs, std::vector<struct WordAlternatives> *out, int n_alts,
                                         bool use_final_probs, double graph_scale, double acoustic_scale) {
  StreamWordQuery("WordAlternatives", _chan, seqs, out, [&](auto &&f) { OnDevice(f); },
                  [&](const auto &ch, const SeqLists &s, auto *o, auto *st) {
                    return WordAlternativesCall(_dec, ch, s, n_alts, use_final_probs, graph_scale, acoustic_scale, 0, o, st);
                  });
}

// ---- sentence and phrase posteriors (wfst_decoder_sequence_posterior) -------------------------------------------------------------------
// One C-ABI call for `ch`: (*out)[i][q] for seqs[i][q], (*status)[i] the channel's own code.  Returns the call's own code.  A lattice
// with more frames than the first call's rows hold is asked for again with n_frames' room.
static int SequencePosteriorsCall(wfst_decoder *dec, const std::vector<int32_t> &ch, const SeqLists &seqs, bool phrase, bool use_final_probs,
                                  double graph_scale, double acoustic_scale, long long max_cells, bool hit_mass,
                                  std::vector<std::vector<SequencePosterior> > *out, std::vector<int> *status) {
  if (!wfst_decoder_sequence_posterior)
    throw std::runtime_error("SequencePosteriors: this build's device library has no wfst_decoder_sequence_posterior");
  if (seqs.size() != ch.size()) throw std::runtime_error("SequencePosteriors: one list of sequences per listed channel");
  const PackedSeqs in(seqs);
  const size_t cnt = in.cnt, ns = in.ns, np = in.np;
  const bool rows = phrase && hit_mass;
  std::vector<int32_t> st(cnt), nf(cnt), found(np);
  std::vector<double> lz(cnt), lp(np), hit;
  size_t capf = rows ? 256 : 0;
  for (int pass = 0;; ++pass) {
    hit.assign(np * capf, 0.0);
    const int rc = wfst_decoder_sequence_posterior(dec, ch.data(), (int32_t)cnt, use_final_probs ? 1 : 0, graph_scale, acoustic_scale, phrase ? 1 : 0,
                                                   (int32_t)ns, (int32_t)in.cap, in.words.data(), in.len.data(), max_cells, (int32_t)capf, st.data(),
                                                   lz.data(), nf.data(), found.data(), lp.data(), rows ? hit.data() : nullptr);
    if (rc != WFST_OK) return rc;
    const size_t most = (size_t)*std::max_element(nf.begin(), nf.end());
    if (!rows || most <= capf || pass) break;
    capf = most;
  }
  out->assign(cnt, std::vector<SequencePosterior>());
  for (size_t i = 0; i < cnt; ++i) {
    (*out)[i].resize(seqs[i].size());
    for (size_t q = 0; q < seqs[i].size(); ++q) {
      SequencePosterior &a = (*out)[i][q];
      const size_t p = i * ns + q;
      a.log_z = lz[i];
      if (rows && (size_t)nf[i] <= capf) a.hit_mass.assign(hit.begin() + p * capf, hit.begin() + p * capf + nf[i]);
      a.found = found[p] != 0;
      if (!a.found) continue;
      a.logpost = lp[p]; a.count = std::exp(lp[p]); a.conf = std::min(1.0, a.count);
      if (!a.hit_mass.empty()) a.peak = (int)(std::max_element(a.hit_mass.begin(), a.hit_mass.end()) - a.hit_mass.begin());
    }
  }
  status->assign(st.begin(), st.end());
  return WFST_OK;
}

void GpuBatchDecoder::SequencePosteriors(const std::vector<int> &channels, const std::vector<std::vector<std::vector<int> > > &seqs, bool phrase,
                                         bool use_final_probs, double graph_scale, double acoustic_scale,
                                         std::vector<std::vector<SequencePosterior> > *out, std::vector<int> *status, long long max_cells,
                                         bool hit_mass) {
  BatchWordQuery("SequencePosteriors", channels, _n, out, status, [&](const auto &ch, auto *o, auto *st) {
    return SequencePosteriorsCall(_dec, ch, seqs, phrase, use_final_probs, graph_scale, acoustic_scale, max_cells, hit_mass, o, st);
  });
}

void GpuLatticeDecoder::SequencePosteriors(const std::vector<std::vector<int> > &seqs, std::vector<SequencePosterior> *out, bool phrase,
                                           bool use_final_probs, double graph_scale, double acoustic_scale, bool hit_mass) {
  StreamWordQuery("SequencePosteriors", _chan, seqs, out, [&](auto &&f) { OnDevice(f); },
                  [&](const auto &ch, const SeqLists &s, auto *o, auto *st) {
                    return SequencePosteriorsCall(_dec, ch, s, phrase, use_final_probs, graph_scale, acoustic_scale, 0, hit_mass, o, st);
                  });
}

// ---- frame posteriors (wfst_decoder_frame_posteriors) ----------------------------------------------------------------------------------
// One C-ABI call for `ch`: (*out)[i] for listed channel i, its own code in status.  Returns the call's own code.  The rows take their
// room from the frames decoded; a lattice that needs more is asked for again, once, with n_frames' and n_entries' room.
static int FramePosteriorsCall(wfst_decoder *dec, const std::vector<int32_t> &ch, bool use_final_probs, double graph_scale, double acoustic_scale,
                               const std::vector<int> &label_map, double min_post, long long max_cells,
                               std::vector<struct FramePosteriors> *out) {
  if (!wfst_decoder_frame_posteriors)
    throw std::runtime_error("FramePosteriors: this build's device library has no wfst_decoder_frame_posteriors");
  const size_t cnt = ch.size();
  const std::vector<int32_t> map(label_map.begin(), label_map.end());
  size_t capf = 1;
  for (int32_t c : ch) capf = std::max(capf, (size_t)std::max(wfst_decoder_num_frames_decoded(dec, c), 0));
  size_t cape = 64 * capf;
  std::vector<int32_t> st(cnt), nf(cnt), ne(cnt), off, nd, cls;
  std::vector<double> lz(cnt), mass, post;
  for (int pass = 0;; ++pass) {
    off.assign(cnt * (capf + 1), 0); nd.assign(cnt * capf, 0); mass.assign(cnt * capf, 0.0);
    cls.assign(cnt * cape, 0); post.assign(cnt * cape, 0.0);
    const int rc = wfst_decoder_frame_posteriors(dec, ch.data(), (int32_t)cnt, use_final_probs ? 1 : 0, graph_scale, acoustic_scale,
                                                 map.empty() ? nullptr : map.data(), map.empty() ? 0 : (int32_t)map.size() - 1, min_post, max_cells,
                                                 (int32_t)capf, (int32_t)cape, st.data(), lz.data(), nf.data(), ne.data(), off.data(), nd.data(),
                                                 mass.data(), cls.data(), post.data());
    if (rc != WFST_OK) return rc;
    size_t need_f = capf, need_e = cape;
    for (size_t i = 0; i < cnt; ++i)
      if (st[i] == WFST_E_CAPACITY) { need_f = std::max(need_f, (size_t)nf[i]); need_e = std::max(need_e, (size_t)ne[i]); }
    if (pass || (need_f == capf && need_e == cape)) break;
    capf = need_f; cape = need_e;
  }
  out->assign(cnt, FramePosteriors());
  for (size_t i = 0; i < cnt; ++i) {
    struct FramePosteriors &a = (*out)[i];
    a.status = st[i];
    a.log_z = lz[i];
    a.n_frames = nf[i];
    if (st[i] != WFST_OK) continue;
    const size_t f = (size_t)nf[i], e = (size_t)ne[i];
    a.frame_off.assign(off.begin() + i * (capf + 1), off.begin() + i * (capf + 1) + f + 1);
    a.n_distinct.assign(nd.begin() + i * capf, nd.begin() + i * capf + f);
    a.frame_mass.assign(mass.begin() + i * capf, mass.begin() + i * capf + f);
    a.classes.assign(cls.begin() + i * cape, cls.begin() + i * cape + e);
    a.posts.assign(post.begin() + i * cape, post.begin() + i * cape + e);
  }
  return WFST_OK;
}

void GpuBatchDecoder::FramePosteriors(const std::vector<int> &channels, bool use_final_probs, double graph_scale, double acoustic_scale,
                                      const std::vector<int> &label_map, double min_post, std::vector<struct FramePosteriors> *out,
                                      std::vector<int> *status, long long max_cells) {
  std::vector<int32_t> ch(channels.begin(), channels.end());
  if (ch.empty())
    for (int c = 0; c < _n; ++c) ch.push_back(c);
  std::vector<struct FramePosteriors> o;
  if (FramePosteriorsCall(_dec, ch, use_final_probs, graph_scale, acoustic_scale, label_map, min_post, max_cells, &o) != WFST_OK)
    Fatal("FramePosteriors");
  if (status) status->clear();
  for (const struct FramePosteriors &a : o) {
    if (status) status->push_back(a.status);
    else if (a.status != WFST_OK) Fatal("FramePosteriors");
  }
  if (out) out->swap(o);
}

void GpuLatticeDecoder::FramePosteriors(struct FramePosteriors *out, const std::vector<int> &label_map, double min_post, bool use_final_probs,
                                        double graph_scale, double acoustic_scale) {
  std::vector<struct FramePosteriors> o;
  int rc = WFST_OK;
  std::string msg;
  OnDevice([&] {
    rc = FramePosteriorsCall(_dec, std::vector<int32_t>(1, _chan), use_final_probs, graph_scale, acoustic_scale, label_map, min_post, 0, &o);
    if (rc != WFST_OK || o[0].status != WFST_OK) msg = wfst_last_error();
  });
  if (rc != WFST_OK || o[0].status != WFST_OK) throw std::runtime_error("FramePosteriors: " + msg);
  if (out) *out = o[0];
}

// ---- sequence-training statistics (wfst_decoder_sequence_stats) -------------------------------------------------------------------------
// One C-ABI call for `ch`: (*out)[i] for listed channel i, its own code in status.  Returns the call's own code.  The rows take their
// room from the frames decoded; a lattice that needs more is asked for again, once, with n_frames' and n_entries' room.
static int SequenceStatsCall(wfst_decoder *dec, const std::vector<int32_t> &ch, const std::vector<std::vector<int> > &refs,
                             const SequenceStatsOptions &opt, std::vector<struct SequenceStats> *out) {
  if (!wfst_decoder_sequence_stats) throw std::runtime_error("SequenceStats: this build's device library has no wfst_decoder_sequence_stats");
  const size_t cnt = ch.size();
  if (refs.size() != cnt) throw std::runtime_error("SequenceStats: one reference per listed channel");
  if (!opt.grad.empty() && (opt.grad.size() != cnt || opt.grad_frames.size() != cnt || (!opt.grad_pitch.empty() && opt.grad_pitch.size() != cnt)))
    throw std::runtime_error("SequenceStats: grad, grad_frames and grad_pitch hold one entry per listed channel");
  const std::vector<int32_t> map(opt.label_map.begin(), opt.label_map.end()), sil(opt.sil_classes.begin(), opt.sil_classes.end());
  size_t cap_ref = 1;
  for (const std::vector<int> &r : refs) cap_ref = std::max(cap_ref, r.size());
  std::vector<int32_t> ref(cnt * cap_ref, -1), n_ref(cnt), rows(opt.grad_frames.begin(), opt.grad_frames.end());
  for (size_t i = 0; i < cnt; ++i) {
    std::copy(refs[i].begin(), refs[i].end(), ref.begin() + i * cap_ref);
    n_ref[i] = (int32_t)refs[i].size();
  }
  const std::vector<int64_t> pitch(opt.grad_pitch.begin(), opt.grad_pitch.end());
  size_t capf = 1;
  for (int32_t c : ch) capf = std::max(capf, (size_t)std::max(wfst_decoder_num_frames_decoded(dec, c), 0));
  size_t cape = 64 * capf;
  std::vector<int32_t> st(cnt), nf(cnt), nr(cnt), nd(cnt), ne(cnt), off, cls;
  std::vector<double> lz(cnt), tot(cnt), post, val;
  for (int pass = 0;; ++pass) {
    off.assign(cnt * (capf + 1), 0); cls.assign(cnt * cape, 0); post.assign(cnt * cape, 0.0); val.assign(cnt * cape, 0.0);
    const int rc = wfst_decoder_sequence_stats(dec, ch.data(), (int32_t)cnt, opt.mmi ? WFST_SEQ_MMI : WFST_SEQ_SMBR, opt.use_final_probs ? 1 : 0,
                                               opt.graph_scale, opt.acoustic_scale, map.empty() ? nullptr : map.data(),
                                               map.empty() ? 0 : (int32_t)map.size() - 1, ref.data(), n_ref.data(), (int32_t)cap_ref,
                                               sil.empty() ? nullptr : sil.data(), (int32_t)sil.size(), opt.drop_frames ? 1 : 0, opt.max_cells,
                                               (int32_t)capf, (int32_t)cape, opt.grad.empty() ? nullptr : opt.grad.data(),
                                               pitch.empty() ? nullptr : pitch.data(), rows.empty() ? nullptr : rows.data(), opt.n_cols,
                                               opt.grad_scale, opt.consumer_stream, st.data(), lz.data(), tot.data(), nf.data(), nr.data(),
                                               nd.data(), ne.data(), off.data(), cls.data(), post.data(), val.data());
    if (rc != WFST_OK) return rc;
    size_t need_f = capf, need_e = cape;
    for (size_t i = 0; i < cnt; ++i)
      if (st[i] == WFST_E_CAPACITY) { need_f = std::max(need_f, (size_t)nf[i]); need_e = std::max(need_e, (size_t)ne[i]); }
    if (pass || (need_f == capf && need_e == cape)) break;
    capf = need_f; cape = need_e;
  }
  out->assign(cnt, SequenceStats());
  for (size_t i = 0; i < cnt; ++i) {
    struct SequenceStats &a = (*out)[i];
    a.status = st[i];
    a.log_z = lz[i];
    a.n_frames = nf[i];
    if (st[i] != WFST_OK) continue;
    a.tot_acc = tot[i];
    a.n_ref_frames = nr[i];
    a.n_dropped = nd[i];
    const size_t f = (size_t)nf[i], e = (size_t)ne[i];
    a.frame_off.assign(off.begin() + i * (capf + 1), off.begin() + i * (capf + 1) + f + 1);
    a.classes.assign(cls.begin() + i * cape, cls.begin() + i * cape + e);
    a.posts.assign(post.begin() + i * cape, post.begin() + i * cape + e);
    a.values.assign(val.begin() + i * cape, val.begin() + i * cape + e);
  }
  return WFST_OK;
}

void GpuBatchDecoder::SequenceStats(const std::vector<int> &channels, const std::vector<std::vector<int> > &refs, const SequenceStatsOptions &opt,
                                    std::vector<struct SequenceStats> *out, std::vector<int> *status) {
  std::vector<int32_t> ch(channels.begin(), channels.end());
  if (ch.empty())
    for (int c = 0; c < _n; ++c) ch.push_back(c);
  std::vector<struct SequenceStats> o;
  if (SequenceStatsCall(_dec, ch, refs, opt, &o) != WFST_OK) Fatal("SequenceStats");
  if (status) status->clear();
  for (const struct SequenceStats &a : o) {
    if (status) status->push_back(a.status);
    else if (a.status != WFST_OK) Fatal("SequenceStats");
  }
  if (out) out->swap(o);
}

void GpuLatticeDecoder::SequenceStats(const std::vector<int> &ref, struct SequenceStats *out, const SequenceStatsOptions &opt) {
  std::vector<struct SequenceStats> o;
  int rc = WFST_OK;
  std::string msg;
  OnDevice([&] {
    rc = SequenceStatsCall(_dec, std::vector<int32_t>(1, _chan), std::vector<std::vector<int> >(1, ref), opt, &o);
    if (rc != WFST_OK || o[0].status != WFST_OK) msg = wfst_last_error();
  });
  if (rc != WFST_OK || o[0].status != WFST_OK) throw std::runtime_error("SequenceStats: " + msg);
  if (out) *out = o[0];
}

// ---- forced alignment against per-utterance graphs (wfst_decoder_force_align) -----------------------------------------------------------
AlignGraphs::~AlignGraphs() {
  if (_g && wfst_align_graphs_free) wfst_align_graphs_free(_g);
}

bool AlignGraphs::Read(const std::vector<std::string> &files, int device) {
  if (!wfst_align_graphs_load) throw std::runtime_error("AlignGraphs: this build's device library has no wfst_align_graphs_load");
  if (_g) { wfst_align_graphs_free(_g); _g = nullptr; _n = 0; }
  std::vector<const char *> paths;
  for (const std::string &f : files) paths.push_back(f.c_str());
  if (wfst_align_graphs_load((int32_t)paths.size(), paths.data(), device, &_g) != WFST_OK) {
    Warn(std::string("AlignGraphs: ") + wfst_last_error());
    _g = nullptr;
    return false;
  }
  _n = (int)files.size();
  return true;
}

// One C-ABI call for `ch`: (*out)[i] for listed channel i, its own code in status.  Returns the call's own code.  The rows take their
// room from the frames decoded; a path that needs more is asked for again, once, with the room it reports.
static int ForceAlignCall(wfst_decoder *dec, const std::vector<int32_t> &ch, const AlignGraphs &graphs, const std::vector<int> &graph_of,
                          const std::vector<int> &label_map, long long max_cells, std::vector<ForcedAlignment> *out) {
  if (!wfst_decoder_force_align) throw std::runtime_error("ForceAlign: this build's device library has no wfst_decoder_force_align");
  const size_t cnt = ch.size();
  if (!graph_of.empty() && graph_of.size() != cnt) throw std::runtime_error("ForceAlign: one graph per listed channel");
  std::vector<int32_t> gof(graph_of.begin(), graph_of.end());
  if (gof.empty())
    for (size_t i = 0; i < cnt; ++i) gof.push_back((int32_t)i);
  const std::vector<int32_t> map(label_map.begin(), label_map.end());
  size_t capf = 1;
  for (int32_t c : ch) capf = std::max(capf, (size_t)std::max(wfst_decoder_num_frames_decoded(dec, c), 0));
  size_t caph = 2 * capf + 8, capw = capf + 8;
  std::vector<int32_t> st(cnt), fnd(cnt), nf(cnt), nh(cnt), nw(cnt), hops, ali, words, wf;
  std::vector<float> cost(cnt), tot(cnt), lm(cnt);
  for (int pass = 0;; ++pass) {
    hops.assign(cnt * caph, 0); ali.assign(cnt * capf, 0); words.assign(cnt * capw, 0); wf.assign(cnt * capw, 0);
    const int rc = wfst_decoder_force_align(dec, ch.data(), (int32_t)cnt, graphs.Handle(), gof.data(), nullptr, map.empty() ? nullptr : map.data(),
                                            map.empty() ? 0 : (int32_t)map.size() - 1, max_cells, (int32_t)capf, (int32_t)caph, (int32_t)capw,
                                            st.data(), fnd.data(), nf.data(), cost.data(), tot.data(), lm.data(), nh.data(), hops.data(),
                                            ali.data(), nw.data(), words.data(), wf.data());
    if (rc != WFST_OK) return rc;
    size_t need_f = capf, need_h = caph, need_w = capw;
    for (size_t i = 0; i < cnt; ++i)
      if (st[i] == WFST_E_CAPACITY) {
        need_f = std::max(need_f, (size_t)nf[i]); need_h = std::max(need_h, (size_t)nh[i]); need_w = std::max(need_w, (size_t)nw[i]);
      }
    if (pass || (need_f == capf && need_h == caph && need_w == capw)) break;
    capf = need_f; caph = need_h; capw = need_w;
  }
  out->assign(cnt, ForcedAlignment());
  for (size_t i = 0; i < cnt; ++i) {
    ForcedAlignment &a = (*out)[i];
    a.status = st[i];
    if (st[i] != WFST_OK || !fnd[i]) continue;
    a.found = true;
    a.n_frames = nf[i];
    a.path_cost = cost[i]; a.tot = tot[i]; a.lm = lm[i];
    a.hop_arc.assign(hops.begin() + i * caph, hops.begin() + i * caph + nh[i]);
    a.alignment.assign(ali.begin() + i * capf, ali.begin() + i * capf + nf[i]);
    a.words.assign(words.begin() + i * capw, words.begin() + i * capw + nw[i]);
    a.word_frame.assign(wf.begin() + i * capw, wf.begin() + i * capw + nw[i]);
  }
  return WFST_OK;
}

void GpuBatchDecoder::ForceAlign(const std::vector<int> &channels, const AlignGraphs &graphs, const std::vector<int> &graph_of,
                                 const std::vector<int> &label_map, std::vector<ForcedAlignment> *out, std::vector<int> *status,
                                 long long max_cells) {
  std::vector<int32_t> ch(channels.begin(), channels.end());
  if (ch.empty())
    for (int c = 0; c < _n; ++c) ch.push_back(c);
  std::vector<ForcedAlignment> o;
  if (ForceAlignCall(_dec, ch, graphs, graph_of, label_map, max_cells, &o) != WFST_OK) Fatal("ForceAlign");
  if (status) status->clear();
  for (const ForcedAlignment &a : o) {
    if (status) status->push_back(a.status);
    else if (a.status != WFST_OK) Fatal("ForceAlign");
  }
  if (out) out->swap(o);
}

void GpuLatticeDecoder::ForceAlign(const AlignGraphs &graphs, int graph, ForcedAlignment *out, const std::vector<int> &label_map) {
  std::vector<ForcedAlignment> o;
  int rc = WFST_OK;
  std::string msg;
  OnDevice([&] {
    rc = ForceAlignCall(_dec, std::vector<int32_t>(1, _chan), graphs, std::vector<int>(1, graph), label_map, 0, &o);
    if (rc != WFST_OK || o[0].status != WFST_OK) msg = wfst_last_error();
  });
  if (rc != WFST_OK || o[0].status != WFST_OK) throw std::runtime_error("ForceAlign: " + msg);
  if (out) *out = o[0];
}

// ---- graph posteriors over per-utterance graphs (wfst_decoder_graph_posteriors) ---------------------------------------------------------
// One C-ABI call for `ch`: (*out)[i] for listed channel i, its own code in status.  Returns the call's own code.  The rows take their
// room from the frames decoded and the graphs' arcs; a channel that needs more is asked for again, once, with the room it reports.
static int GraphPosteriorsCall(wfst_decoder *dec, const std::vector<int32_t> &ch, const AlignGraphs &graphs, const std::vector<int> &graph_of,
                               const GraphPosteriorsOptions &opt, std::vector<struct GraphPosteriors> *out) {
  if (!wfst_decoder_graph_posteriors) throw std::runtime_error("GraphPosteriors: this build's device library has no wfst_decoder_graph_posteriors");
  const size_t cnt = ch.size();
  if (!graph_of.empty() && graph_of.size() != cnt) throw std::runtime_error("GraphPosteriors: one graph per listed channel");
  if (!opt.grad.empty() && (opt.grad.size() != cnt || opt.grad_frames.size() != cnt || (!opt.grad_pitch.empty() && opt.grad_pitch.size() != cnt)))
    throw std::runtime_error("GraphPosteriors: one grad pointer, frame count and pitch per listed channel");
  std::vector<int32_t> gof(graph_of.begin(), graph_of.end());
  if (gof.empty())
    for (size_t i = 0; i < cnt; ++i) gof.push_back((int32_t)i);
  const std::vector<int32_t> map(opt.label_map.begin(), opt.label_map.end());
  const std::vector<int64_t> pitch(opt.grad_pitch.begin(), opt.grad_pitch.end());
  const std::vector<int32_t> rows(opt.grad_frames.begin(), opt.grad_frames.end());
  size_t capf = 1, capa = 0;
  for (int32_t c : ch) capf = std::max(capf, (size_t)std::max(wfst_decoder_num_frames_decoded(dec, c), 0));
  size_t cape = capf * 64;
  if (opt.arc_occupancy) capa = 1;
  std::vector<int32_t> st(cnt), fnd(cnt), nf(cnt), ne(cnt), na(cnt), off, nd, cls;
  std::vector<double> ll(cnt), mass, post, occ;
  for (int pass = 0;; ++pass) {
    off.assign(cnt * (capf + 1), 0); nd.assign(cnt * capf, 0); cls.assign(cnt * cape, 0);
    mass.assign(cnt * capf, 0.0); post.assign(cnt * cape, 0.0); occ.assign(cnt * capa, 0.0);
    const int rc = wfst_decoder_graph_posteriors(
        dec, ch.data(), (int32_t)cnt, graphs.Handle(), gof.data(), nullptr, map.empty() ? nullptr : map.data(), map.empty() ? 0 : (int32_t)map.size() - 1,
        opt.graph_scale, opt.acoustic_scale, opt.min_post, opt.max_cells, (int32_t)capf, (int32_t)cape, (int32_t)capa,
        opt.grad.empty() ? nullptr : opt.grad.data(), pitch.empty() ? nullptr : pitch.data(), rows.empty() ? nullptr : rows.data(), opt.n_cols,
        opt.grad_scale, opt.consumer_stream, st.data(), fnd.data(), nf.data(), ll.data(), ne.data(), na.data(), off.data(), nd.data(), mass.data(),
        cls.data(), post.data(), opt.arc_occupancy ? occ.data() : nullptr);
    if (rc != WFST_OK) return rc;
    size_t need_f = capf, need_e = cape, need_a = capa;
    for (size_t i = 0; i < cnt; ++i)
      if (st[i] == WFST_E_CAPACITY) {
        need_f = std::max(need_f, (size_t)nf[i]); need_e = std::max(need_e, (size_t)ne[i]);
        if (opt.arc_occupancy) need_a = std::max(need_a, (size_t)na[i]);
      }
    if (pass || (need_f == capf && need_e == cape && need_a == capa)) break;
    capf = need_f; cape = need_e; capa = need_a;
  }
  out->assign(cnt, GraphPosteriors());
  for (size_t i = 0; i < cnt; ++i) {
    struct GraphPosteriors &a = (*out)[i];
    a.status = st[i];
    if (st[i] != WFST_OK || !fnd[i]) continue;
    a.found = true;
    a.n_frames = nf[i];
    a.log_like = ll[i];
    a.frame_off.assign(off.begin() + i * (capf + 1), off.begin() + i * (capf + 1) + nf[i] + 1);
    a.n_distinct.assign(nd.begin() + i * capf, nd.begin() + i * capf + nf[i]);
    a.frame_mass.assign(mass.begin() + i * capf, mass.begin() + i * capf + nf[i]);
    a.classes.assign(cls.begin() + i * cape, cls.begin() + i * cape + ne[i]);
    a.posts.assign(post.begin() + i * cape, post.begin() + i * cape + ne[i]);
    if (opt.arc_occupancy) a.arc_occ.assign(occ.begin() + i * capa, occ.begin() + i * capa + na[i]);
  }
  return WFST_OK;
}

void GpuBatchDecoder::GraphPosteriors(const std::vector<int> &channels, const AlignGraphs &graphs, const std::vector<int> &graph_of,
                                      const GraphPosteriorsOptions &opt, std::vector<struct GraphPosteriors> *out, std::vector<int> *status) {
  std::vector<int32_t> ch(channels.begin(), channels.end());
  if (ch.empty())
    for (int c = 0; c < _n; ++c) ch.push_back(c);
  std::vector<struct GraphPosteriors> o;
  if (GraphPosteriorsCall(_dec, ch, graphs, graph_of, opt, &o) != WFST_OK) Fatal("GraphPosteriors");
  if (status) status->clear();
  for (const struct GraphPosteriors &a : o) {
    if (status) status->push_back(a.status);
    else if (a.status != WFST_OK) Fatal("GraphPosteriors");
  }
  if (out) out->swap(o);
}

void GpuLatticeDecoder::GraphPosteriors(const AlignGraphs &graphs, int graph, struct GraphPosteriors *out, const GraphPosteriorsOptions &opt) {
  std::vector<struct GraphPosteriors> o;
  int rc = WFST_OK;
  std::string msg;
  OnDevice([&] {
    rc = GraphPosteriorsCall(_dec, std::vector<int32_t>(1, _chan), graphs, std::vector<int>(1, graph), opt, &o);
    if (rc != WFST_OK || o[0].status != WFST_OK) msg = wfst_last_error();
  });
  if (rc != WFST_OK || o[0].status != WFST_OK) throw std::runtime_error("GraphPosteriors: " + msg);
  if (out) *out = o[0];
}

// ---- the lattice path nearest a transcript (wfst_decoder_nearest_words) ---------------------------------------------------------------
// One C-ABI call for `ch`: (*out)[i][q] for refs[i][q], (*status)[i] the channel's own code.  Returns the call's own code.  A path with
// more words than the first call made room for is asked for again with n_hyp's room.
static int NearestWordsCall(wfst_decoder *dec, const std::vector<int32_t> &ch, const SeqLists &refs, bool use_final_probs, long long max_cells,
                            std::vector<std::vector<NearestPath> > *out, std::vector<int> *status) {
  if (!wfst_decoder_nearest_words) throw std::runtime_error("NearestWords: this build's device library has no wfst_decoder_nearest_words");
  if (refs.size() != ch.size()) throw std::runtime_error("NearestWords: one list of references per listed channel");
  const PackedSeqs in(refs);
  const size_t cnt = in.cnt, ns = in.ns, cap = in.cap, np = in.np;
  std::vector<int32_t> st(cnt), found(np), ne(np), nc(np), nsub(np), ni(np), ndel(np), na(np), nh(np), rh(np * cap);
  std::vector<int32_t> hyp, b, e;
  std::vector<float> t(np), l(np);
  size_t hcap = cap + 16;
  for (int pass = 0;; ++pass) {
    hyp.assign(np * hcap, 0); b.assign(np * hcap, 0); e.assign(np * hcap, 0);
    const int rc = wfst_decoder_nearest_words(dec, ch.data(), (int32_t)cnt, use_final_probs ? 1 : 0, (int32_t)ns, (int32_t)cap, in.words.data(), in.len.data(),
                                              (int32_t)hcap, max_cells, st.data(), found.data(), ne.data(), nc.data(), nsub.data(), ni.data(),
                                              ndel.data(), na.data(), nh.data(), hyp.data(), b.data(), e.data(), rh.data(), t.data(), l.data());
    if (rc != WFST_OK) return rc;
    const size_t most = (size_t)*std::max_element(nh.begin(), nh.end());
    if (most <= hcap || pass) break;
    hcap = most;
  }
  out->assign(cnt, std::vector<NearestPath>());
  for (size_t i = 0; i < cnt; ++i) {
    (*out)[i].resize(refs[i].size());
    for (size_t q = 0; q < refs[i].size(); ++q) {
      NearestPath &a = (*out)[i][q];
      const size_t p = i * ns + q;
      a.found = found[p] != 0;
      if (!a.found) continue;
      a.errors = ne[p]; a.cor = nc[p]; a.sub = nsub[p]; a.ins = ni[p]; a.del = ndel[p]; a.n_arcs = na[p]; a.tot = t[p]; a.lm = l[p];
      for (size_t j = 0; j < std::min((size_t)nh[p], hcap); ++j) {
        a.words.push_back(hyp[p * hcap + j]);
        a.frames.push_back(std::make_pair(b[p * hcap + j], e[p * hcap + j]));
      }
      a.ref_hyp.assign(rh.begin() + p * cap, rh.begin() + p * cap + refs[i][q].size());
    }
  }
  status->assign(st.begin(), st.end());
  return WFST_OK;
}

void GpuBatchDecoder::NearestWords(const std::vector<int> &channels, const std::vector<std::vector<std::vector<int> > > &refs, bool use_final_probs,
                                   std::vector<std::vector<NearestPath> > *out, std::vector<int> *status, long long max_cells) {
  BatchWordQuery("NearestWords", channels, _n, out, status, [&](const auto &ch, auto *o, auto *st) {
    return NearestWordsCall(_dec, ch, refs, use_final_probs, max_cells, o, st);
  });
}

void GpuLatticeDecoder::NearestWords(const std::vector<std::vector<int> > &refs, std::vector<NearestPath> *out, bool use_final_probs) {
  StreamWordQuery("NearestWords", _chan, refs, out, [&](auto &&f) { OnDevice(f); },
                  [&](const auto &ch, const SeqLists &r, auto *o, auto *st) {
                    return NearestWordsCall(_dec, ch, r, use_final_probs, 0, o, st);
                  });
}

// ---- best paths under new scales (wfst_decoder_rescaled_words) -------------------------------------------------------------------------
// One C-ABI call for `ch`: (*out)[i][q] for settings[q], (*status)[i] the channel's own code.  Returns the call's own code.  A path
// with more words or transition-ids than the first call made room for is asked for again, once, with the room needed.
static int RescaledWordsCall(wfst_decoder *dec, const std::vector<int32_t> &ch, const std::vector<RescaleSetting> &settings, bool use_final_probs,
                             bool alignment, long long max_cells, std::vector<std::vector<struct RescaledWords> > *out, std::vector<int> *status) {
  if (!wfst_decoder_rescaled_words) throw std::runtime_error("RescaledWords: this build's device library has no wfst_decoder_rescaled_words");
  const size_t cnt = ch.size(), ns = settings.size(), np = cnt * ns;
  std::vector<double> set;
  for (const RescaleSetting &s : settings) { set.push_back(s.graph_scale); set.push_back(s.acoustic_scale); set.push_back(s.word_penalty); }
  size_t cap = 256, tcap = 1;
  if (alignment)
    for (int32_t c : ch) tcap = std::max(tcap, (size_t)std::max(wfst_decoder_num_frames_decoded(dec, c), 0));
  std::vector<int32_t> st(cnt), found(np), na(np), nh(np), nt(np), hyp, b, e, tids;
  std::vector<double> cost(np);
  std::vector<float> t(np), l(np);
  for (int pass = 0;; ++pass) {
    hyp.assign(np * cap, 0); b.assign(np * cap, 0); e.assign(np * cap, 0);
    if (alignment) tids.assign(np * tcap, 0);
    const int rc = wfst_decoder_rescaled_words(dec, ch.data(), (int32_t)cnt, use_final_probs ? 1 : 0, (int32_t)ns, set.data(), (int32_t)cap,
                                               (int32_t)tcap, max_cells, st.data(), found.data(), na.data(), nh.data(), nt.data(), hyp.data(),
                                               b.data(), e.data(), alignment ? tids.data() : nullptr, cost.data(), t.data(), l.data());
    if (rc != WFST_OK) return rc;
    const size_t most = np ? (size_t)*std::max_element(nh.begin(), nh.end()) : 0;
    const size_t most_t = np && alignment ? (size_t)*std::max_element(nt.begin(), nt.end()) : 0;
    if ((most <= cap && most_t <= tcap) || pass) break;
    cap = std::max(cap, most);
    tcap = std::max(tcap, most_t);
  }
  out->assign(cnt, std::vector<struct RescaledWords>(ns));
  for (size_t i = 0; i < cnt; ++i)
    for (size_t q = 0; q < ns; ++q) {
      struct RescaledWords &a = (*out)[i][q];
      const size_t p = i * ns + q;
      a.found = found[p] != 0;
      if (!a.found) continue;
      a.n_arcs = na[p]; a.scaled_cost = cost[p]; a.tot = t[p]; a.lm = l[p];
      for (size_t j = 0; j < std::min((size_t)nh[p], cap); ++j) {
        a.words.push_back(hyp[p * cap + j]);
        a.frames.push_back(std::make_pair(b[p * cap + j], e[p * cap + j]));
      }
      if (alignment) a.tids.assign(tids.begin() + p * tcap, tids.begin() + p * tcap + std::min((size_t)nt[p], tcap));
    }
  status->assign(st.begin(), st.end());
  return WFST_OK;
}

void GpuBatchDecoder::RescaledWords(const std::vector<int> &channels, const std::vector<RescaleSetting> &settings, bool use_final_probs,
                                    std::vector<std::vector<struct RescaledWords> > *out, std::vector<int> *status, bool alignment,
                                    long long max_cells) {
  BatchWordQuery("RescaledWords", channels, _n, out, status, [&](const auto &ch, auto *o, auto *st) {
    return RescaledWordsCall(_dec, ch, settings, use_final_probs, alignment, max_cells, o, st);
  });
}

void GpuLatticeDecoder::RescaledWords(const std::vector<RescaleSetting> &settings, std::vector<struct RescaledWords> *out, bool use_final_probs,
                                      bool alignment) {
  std::vector<std::vector<struct RescaledWords> > o;
  std::vector<int> st;
  int rc = WFST_OK;
  std::string msg;
  OnDevice([&] {
    rc = RescaledWordsCall(_dec, std::vector<int32_t>(1, _chan), settings, use_final_probs, alignment, 0, &o, &st);
    if (rc != WFST_OK || st[0] != WFST_OK) msg = wfst_last_error();
  });
  if (rc != WFST_OK || st[0] != WFST_OK) throw std::runtime_error("RescaledWords: " + msg);
  if (out) out->swap(o[0]);
}

// ---- phrase boosting (wfst_bias_lists_*, wfst_decoder_biased_words) ---------------------------------------------------------------------
BiasLists::~BiasLists() {
  if (_b && wfst_bias_lists_free) wfst_bias_lists_free(_b);
}

bool BiasLists::Set(const std::vector<std::vector<BiasPhrase> > &lists, int device) {
  if (!wfst_bias_lists_create) throw std::runtime_error("BiasLists: this build's device library has no wfst_bias_lists_create");
  if (_b) { wfst_bias_lists_free(_b); _b = nullptr; _n = 0; }
  std::vector<int32_t> n_phrases, len, words;
  std::vector<double> bonus;
  for (const std::vector<BiasPhrase> &list : lists) {
    n_phrases.push_back((int32_t)list.size());
    for (const BiasPhrase &p : list) {
      len.push_back((int32_t)p.words.size());
      words.insert(words.end(), p.words.begin(), p.words.end());
      bonus.push_back(p.bonus);
    }
  }
  if (wfst_bias_lists_create((int32_t)lists.size(), n_phrases.data(), len.data(), words.data(), bonus.data(), device, &_b) != WFST_OK) {
    Warn(std::string("BiasLists: ") + wfst_last_error());
    _b = nullptr;
    return false;
  }
  _n = (int)lists.size();
  return true;
}

BiasBooks::~BiasBooks() {
  if (_b && wfst_bias_books_free) wfst_bias_books_free(_b);
}

bool BiasBooks::Set(const std::vector<std::vector<BiasPhrase> > &books, int device) {
  if (!wfst_bias_books_create) throw std::runtime_error("BiasBooks: this build's device library has no wfst_bias_books_create");
  if (_b) { wfst_bias_books_free(_b); _b = nullptr; _n = 0; }
  std::vector<int32_t> n_phrases, len, words;
  std::vector<double> bonus;
  for (const std::vector<BiasPhrase> &book : books) {
    n_phrases.push_back((int32_t)book.size());
    for (const BiasPhrase &p : book) {
      len.push_back((int32_t)p.words.size());
      words.insert(words.end(), p.words.begin(), p.words.end());
      bonus.push_back(p.bonus);
    }
  }
  if (wfst_bias_books_create((int32_t)books.size(), n_phrases.data(), len.data(), words.data(), bonus.data(), device, &_b) != WFST_OK) {
    Warn(std::string("BiasBooks: ") + wfst_last_error());
    _b = nullptr;
    return false;
  }
  _n = (int)books.size();
  return true;
}

// One C-ABI call for `ch` -- wfst_decoder_biased_words with `lists`, or wfst_decoder_biased_words_sparse with `books` where that is
// given: (*out)[i][q] for settings[q], (*status)[i] the channel's own code.  Returns the call's own code.  A path with more words or
// hits than the first call made room for is asked for again, once, with the room needed.
static int BiasedWordsCore(wfst_decoder *dec, const std::vector<int32_t> &ch, const wfst_bias_lists *lists, const wfst_bias_books *books, bool sparse,
                           const std::vector<int> &list_of, const std::vector<BiasSetting> &settings, bool use_final_probs, long long max_cells,
                           long long round_cells, std::vector<std::vector<struct BiasedWords> > *out, std::vector<int> *status) {
  if (!sparse && !wfst_decoder_biased_words) throw std::runtime_error("BiasedWords: this build's device library has no wfst_decoder_biased_words");
  if (sparse && !wfst_decoder_biased_words_sparse)
    throw std::runtime_error("BiasedWordsSparse: this build's device library has no wfst_decoder_biased_words_sparse");
  const size_t cnt = ch.size(), ns = settings.size(), np = cnt * ns;
  if (!list_of.empty() && list_of.size() != cnt) throw std::runtime_error("BiasedWords: one list per listed channel");
  std::vector<int64_t> cells(cnt, 0);
  std::vector<int32_t> lo(list_of.begin(), list_of.end());
  std::vector<double> set;
  for (const BiasSetting &s : settings) { set.push_back(s.graph_scale); set.push_back(s.acoustic_scale); set.push_back(s.word_penalty); set.push_back(s.boost_scale); }
  size_t cap = 256, hcap = 64;
  std::vector<int32_t> st(cnt), found(np), na(np), nh(np), nk(np), hyp, b, e, hp, hw;
  std::vector<double> cost(np), bonus(np);
  std::vector<float> t(np), l(np);
  for (int pass = 0;; ++pass) {
    hyp.assign(np * cap, 0); b.assign(np * cap, 0); e.assign(np * cap, 0); hp.assign(np * hcap, 0); hw.assign(np * hcap, 0);
    const int rc = sparse
        ? wfst_decoder_biased_words_sparse(dec, ch.data(), (int32_t)cnt, use_final_probs ? 1 : 0, books, lo.empty() ? nullptr : lo.data(), (int32_t)ns,
                                           set.data(), (int32_t)cap, (int32_t)hcap, max_cells, round_cells, st.data(), cells.data(), found.data(),
                                           na.data(), nh.data(), nk.data(), hyp.data(), b.data(), e.data(), hp.data(), hw.data(), cost.data(),
                                           bonus.data(), t.data(), l.data())
        : wfst_decoder_biased_words(dec, ch.data(), (int32_t)cnt, use_final_probs ? 1 : 0, lists, lo.empty() ? nullptr : lo.data(),
                                    (int32_t)ns, set.data(), (int32_t)cap, (int32_t)hcap, max_cells, st.data(), found.data(), na.data(),
                                    nh.data(), nk.data(), hyp.data(), b.data(), e.data(), hp.data(), hw.data(), cost.data(), bonus.data(),
                                    t.data(), l.data());
    if (rc != WFST_OK) return rc;
    const size_t most = np ? (size_t)*std::max_element(nh.begin(), nh.end()) : 0;
    const size_t most_k = np ? (size_t)*std::max_element(nk.begin(), nk.end()) : 0;
    if ((most <= cap && most_k <= hcap) || pass) break;
    cap = std::max(cap, most);
    hcap = std::max(hcap, most_k);
  }
  out->assign(cnt, std::vector<struct BiasedWords>(ns));
  for (size_t i = 0; i < cnt; ++i)
    for (size_t q = 0; q < ns; ++q) {
      struct BiasedWords &a = (*out)[i][q];
      const size_t p = i * ns + q;
      a.found = found[p] != 0;
      a.n_cells = (long long)cells[i];
      if (!a.found) continue;
      a.n_arcs = na[p]; a.biased_cost = cost[p]; a.bonus = bonus[p]; a.tot = t[p]; a.lm = l[p];
      for (size_t j = 0; j < std::min((size_t)nh[p], cap); ++j) {
        a.words.push_back(hyp[p * cap + j]);
        a.frames.push_back(std::make_pair(b[p * cap + j], e[p * cap + j]));
      }
      for (size_t j = 0; j < std::min((size_t)nk[p], hcap); ++j) a.hits.push_back(std::make_pair(hp[p * hcap + j], hw[p * hcap + j]));
    }
  status->assign(st.begin(), st.end());
  return WFST_OK;
}

static int BiasedWordsCall(wfst_decoder *dec, const std::vector<int32_t> &ch, const BiasLists &lists, const std::vector<int> &list_of,
                           const std::vector<BiasSetting> &settings, bool use_final_probs, long long max_cells,
                           std::vector<std::vector<struct BiasedWords> > *out, std::vector<int> *status) {
  return BiasedWordsCore(dec, ch, lists.Handle(), nullptr, false, list_of, settings, use_final_probs, max_cells, 0, out, status);
}
static int BiasedWordsSparseCall(wfst_decoder *dec, const std::vector<int32_t> &ch, const BiasBooks &books, const std::vector<int> &book_of,
                                 const std::vector<BiasSetting> &settings, bool use_final_probs, long long max_cells, long long round_cells,
                                 std::vector<std::vector<struct BiasedWords> > *out, std::vector<int> *status) {
  return BiasedWordsCore(dec, ch, nullptr, books.Handle(), true, book_of, settings, use_final_probs, max_cells, round_cells, out, status);
}

void GpuBatchDecoder::BiasedWords(const std::vector<int> &channels, const BiasLists &lists, const std::vector<int> &list_of,
                                  const std::vector<BiasSetting> &settings, bool use_final_probs,
                                  std::vector<std::vector<struct BiasedWords> > *out, std::vector<int> *status, long long max_cells) {
  BatchWordQuery("BiasedWords", channels, _n, out, status, [&](const auto &ch, auto *o, auto *st) {
    return BiasedWordsCall(_dec, ch, lists, list_of, settings, use_final_probs, max_cells, o, st);
  });
}

void GpuLatticeDecoder::BiasedWords(const BiasLists &lists, int list, const std::vector<BiasSetting> &settings, std::vector<struct BiasedWords> *out,
                                    bool use_final_probs) {
  std::vector<std::vector<struct BiasedWords> > o;
  std::vector<int> st;
  int rc = WFST_OK;
  std::string msg;
  OnDevice([&] {
    rc = BiasedWordsCall(_dec, std::vector<int32_t>(1, _chan), lists, std::vector<int>(1, list), settings, use_final_probs, 0, &o, &st);
    if (rc != WFST_OK || st[0] != WFST_OK) msg = wfst_last_error();
  });
  if (rc != WFST_OK || st[0] != WFST_OK) throw std::runtime_error("BiasedWords: " + msg);
  if (out) out->swap(o[0]);
}

void GpuBatchDecoder::BiasedWordsSparse(const std::vector<int> &channels, const BiasBooks &books, const std::vector<int> &book_of,
                                        const std::vector<BiasSetting> &settings, bool use_final_probs,
                                        std::vector<std::vector<struct BiasedWords> > *out, std::vector<int> *status, long long max_cells,
                                        long long round_cells) {
  BatchWordQuery("BiasedWordsSparse", channels, _n, out, status, [&](const auto &ch, auto *o, auto *st) {
    return BiasedWordsSparseCall(_dec, ch, books, book_of, settings, use_final_probs, max_cells, round_cells, o, st);
  });
}

void GpuLatticeDecoder::BiasedWordsSparse(const BiasBooks &books, int book, const std::vector<BiasSetting> &settings,
                                          std::vector<struct BiasedWords> *out, bool use_final_probs) {
  std::vector<std::vector<struct BiasedWords> > o;
  std::vector<int> st;
  int rc = WFST_OK;
  std::string msg;
  OnDevice([&] {
    rc = BiasedWordsSparseCall(_dec, std::vector<int32_t>(1, _chan), books, std::vector<int>(1, book), settings, use_final_probs, 0, 0, &o, &st);
    if (rc != WFST_OK || st[0] != WFST_OK) msg = wfst_last_error();
  });
  if (rc != WFST_OK || st[0] != WFST_OK) throw std::runtime_error("BiasedWordsSparse: " + msg);
  if (out) out->swap(o[0]);
}

// ---- pruned live lattices (wfst_decoder_set_live_lattice_prune) ------------------------------------------------------------------
static void LiveLatticePruneCall(wfst_decoder *dec, bool on) {
  if (!wfst_decoder_set_live_lattice_prune) throw std::runtime_error("SetLiveLatticePrune: this build's device library has no wfst_decoder_set_live_lattice_prune");
  if (wfst_decoder_set_live_lattice_prune(dec, on ? 1 : 0) != WFST_OK) Fatal("SetLiveLatticePrune");
}
void GpuChannelPool::SetLiveLatticePrune(bool on) { LiveLatticePruneCall(_dec, on); }
void GpuLatticeDecoder::SetLiveLatticePrune(bool on) {
  OnDevice([&] { LiveLatticePruneCall(_dec, on); });
}
void GpuBatchDecoder::SetLiveLatticePrune(bool on) { LiveLatticePruneCall(_dec, on); }

}  // namespace datemoon
