// C++ host mirror of the reference's interface for the token-passing path, over the C ABI of
// include/wfst_decoder.h.  Same names, argument meaning and error behaviour as the reference so
// that a caller written against datemoon/ASR-decoder compiles against this header instead:
//
//   DecodableInterface / AmInterface     src/itf/decodable-itf.h:65-104
//   DecoderItf                            src/my-decoder/decoder-itf.h:10-25
//   LatticeFasterDecoderConfig            src/my-decoder/lattice-faster-decoder-conf.h:8-68
//   Fst (ReadFst/Start/IsFinal/TotState)  src/newfst/optimize-fst.h:53-307
//   Lattice / LatticeArc / LatticeWeight  src/newfst/lattice-fst.h:15-346, src/newfst/weigth.h:192-262
//   LatticeToVector                       src/newfst/lattice-functions.cc:179-217
//   ArpaLm (Read / Rescale)               src/newlm/arpa2fsa.h:249-441          (biglm)
//   OnlineLatticeDecoderMempoolBiglm      src/my-decoder/online-decoder-mempool-base-biglm.h:21-30,570
//
// GpuLatticeDecoder is the drop-in for OnlineLatticeDecoderMempool (one utterance stream,
// decodable pulled through LogLikelihood()); GpuBatchDecoder is the batch shape the MI355X wants
// (many channels per call, matrices already in HBM).  Nothing here decodes on the CPU.
#ifndef WFST_HOST_H_
#define WFST_HOST_H_

#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <exception>
#include <functional>
#include <limits>
#include <memory>
#include <stdexcept>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/wfst_decoder.h"

namespace datemoon {

typedef float BaseFloat;
typedef int int32;
typedef int StateId;
typedef int Label;
const int kNoStateId = -1;

// ---- boundary A: what the decoder calls ---------------------------------------------------
// Under -DKALDI the reference's AmInterface IS kaldi::DecodableInterface (src/itf/decodable-itf.h:
// 55-62), so that any Kaldi decodable (nnet3 looped, DecodableMatrixScaledMapped, ...) plugs in.
// Same switch here: -DWFST_KALDI_DECODABLE (or the reference's own -DKALDI) with Kaldi's src/ on
// the include path.
#if defined(WFST_KALDI_DECODABLE) || defined(KALDI)
}  // namespace datemoon
#include "itf/decodable-itf.h"
namespace datemoon {
typedef kaldi::DecodableInterface DecodableInterface;
#else
class DecodableInterface {
 public:
  virtual float LogLikelihood(int frame, int index) = 0;  // already scaled; the decoder negates it
  virtual bool IsLastFrame(int frame) const = 0;
  virtual int NumFramesReady() const = 0;
  virtual int NumIndices() const = 0;  // indices are 1-based: 1..NumIndices()
  virtual ~DecodableInterface() {}
};
#endif
typedef DecodableInterface AmInterface;

// Optional fast path: a decodable that can hand over its rows in one piece (no per-element
// virtual calls).  Row f must hold LogLikelihood(f, i) at column i, i in [0, NumIndices()].
class MatrixDecodable : public DecodableInterface {
 public:
  virtual const float *HostRows() const = 0;  // row-major [NumFramesReady()][Stride()]
  virtual int Stride() const = 0;
};

// ---- config ---------------------------------------------------------------------------------
struct LatticeFasterDecoderConfig {
  float _beam;
  int _max_active;
  int _min_active;
  float _lattice_beam;
  int _prune_interval;
  bool _determinize_lattice;
  float _beam_delta;
  float _hash_ratio;
  float _prune_scale;
  LatticeFasterDecoderConfig()
      : _beam(16.0f), _max_active(std::numeric_limits<int>::max()), _min_active(200), _lattice_beam(10.0f),
        _prune_interval(25), _determinize_lattice(true), _beam_delta(0.5f), _hash_ratio(2.0f), _prune_scale(0.1f) {}
  // "--name=value" lines (beam, max-active, min-active, lattice-beam, prune-interval, beam-delta,
  // hash-ratio), the option names the reference registers (conf.h:46-61).  Unknown names throw.
  void ReadConfigFile(const std::string &path);
  void Check() const;  // same conditions as the reference's asserts (conf.h:62-67); throws
  wfst_config ToC() const;
};

// ---- endpointing (Kaldi's online2/online-endpoint.h) -------------------------------------------------------------------
// OnlineEndpointRule / OnlineEndpointConfig with Kaldi's option names: --endpoint.silence-phones=a:b:c and
// --endpoint.ruleN.{must-contain-nonsilence,min-trailing-silence,max-relative-cost,min-utterance-length} (N = 1..5), plus
// --endpoint.frame-shift (seconds per decoded frame; Kaldi takes it from the decodable: 0.01, 0.03 for frame-subsampled models).
struct OnlineEndpointRule {
  bool must_contain_nonsilence;
  float min_trailing_silence;
  float max_relative_cost;
  float min_utterance_length;
  OnlineEndpointRule(bool must_contain_nonsilence = true, float min_trailing_silence = 1.0f,
                     float max_relative_cost = std::numeric_limits<float>::infinity(), float min_utterance_length = 0.0f)
      : must_contain_nonsilence(must_contain_nonsilence), min_trailing_silence(min_trailing_silence),
        max_relative_cost(max_relative_cost), min_utterance_length(min_utterance_length) {}
};
struct OnlineEndpointConfig {
  std::string silence_phones;   // colon-separated phone ids; must be set
  OnlineEndpointRule rule1, rule2, rule3, rule4, rule5;
  float frame_shift;
  OnlineEndpointConfig()   // Kaldi's defaults
      : rule1(false, 5.0f, std::numeric_limits<float>::infinity(), 0.0f), rule2(true, 0.5f, 2.0f, 0.0f), rule3(true, 1.0f, 8.0f, 0.0f),
        rule4(true, 2.0f, std::numeric_limits<float>::infinity(), 0.0f), rule5(false, 0.0f, std::numeric_limits<float>::infinity(), 20.0f),
        frame_shift(0.01f) {}
  // one "--endpoint.name=value" argument: true if it is one of these options (a bad value throws), false for any other argument
  bool ParseOption(const std::string &arg);
  // "--name=value" lines as LatticeFasterDecoderConfig::ReadConfigFile reads them; the --endpoint.* lines are taken (an unknown
  // --endpoint.* name throws), the others are left to the other configs that read the same file
  void ReadConfigFile(const std::string &path);
  std::vector<int32_t> SilencePhones() const;   // parsed and checked (non-empty, no duplicates, every phone > 0); throws
  wfst_endpoint_config ToC(std::vector<int32_t> *phones) const;   // (the C struct points into *phones)
  wfst_endpoint_config ToCRaw(const std::vector<int32_t> &phones) const;   // (unchecked)
};

// ---- graph ----------------------------------------------------------------------------------
class Fst {
 public:
  Fst() : _graph(nullptr) {}
  ~Fst();
  bool ReadFst(const char *file, int device = 0);  // false (with a message on stderr) on failure
  bool Init(const char *file, const char *) { return ReadFst(file); }
  // entry 0 unused.  The graph's rows then read log-likelihood column tid2pdf[ilabel] (what DecodableMatrixScaledMapped does with the
  // transition model, kaldi-hclg-my-decoder.cc:107), and a GpuLatticeDecoder over this graph pulls ONE score per pdf from its
  // decodable -- LogLikelihood(frame, a transition-id of that pdf) -- instead of one per transition-id: half the calls, half the
  // bytes, rows narrow enough for the expansion's LDS row.  For decodables whose score depends on the transition-id's pdf only
  // (every Kaldi decodable).
  void SetTid2Pdf(const std::vector<int32_t> &tid2pdf);
  const std::vector<int32_t> &Tid2Pdf() const { return _tid2pdf; }
  // TransitionModel::TransitionIdToPhone as a table (entry 0 unused): what EndpointDetected's silence phones are looked up in
  void SetTid2Phone(const std::vector<int32_t> &tid2phone);
  StateId Start() const { return _start; }
  bool IsFinal(StateId id) const { return id == _final; }
  StateId TotState() const { return _states; }
  int TotArc() const { return _arcs; }
  const wfst_graph *Handle() const { return _graph; }

 private:
  Fst(const Fst &);
  Fst &operator=(const Fst &);
  wfst_graph *_graph;
  std::vector<int32_t> _tid2pdf;
  int32_t _start = 0, _final = 0, _states = 0, _arcs = 0;
};

// ---- language model (biglm) -----------------------------------------------------------------
// The reference's ArpaLm as the biglm caller uses it (kaldi-nnet3bin/kaldi-hclg-my-decoder-biglm.cc:
// 55-60): `lm1.Read(file); lm2.Read(file); lm1.Rescale(-1.0);`.  Read checks the file; the automaton
// goes to HBM, with the scale applied, when a decoder first asks for it.
class ArpaLm {
 public:
  ArpaLm() : _scale(1.0f), _device(0), _lm(nullptr) {}
  ~ArpaLm();
  bool Read(const char *file, int device = 0);  // false (with a message on stderr) on failure
  void Rescale(float scale);
  int BosSymbol() const { return _bos; }
  int EosSymbol() const { return _eos; }
  const wfst_lm *Handle();

 private:
  ArpaLm(const ArpaLm &);
  ArpaLm &operator=(const ArpaLm &);
  std::string _file;
  float _scale;
  int _device;
  wfst_lm *_lm;
  std::mutex _mu;   // Handle() may be called by several worker threads at once (one decoder per thread over shared LMs)
  int32_t _bos = -1, _eos = -1;
};

// ---- lattice (linear best path is all this path produces) ---------------------------------------
struct LatticeWeight {
  float _value1, _value2;  // graph cost, acoustic cost
  LatticeWeight() : _value1(0), _value2(0) {}
  LatticeWeight(float a, float b) : _value1(a), _value2(b) {}
  float Value1() const { return _value1; }
  float Value2() const { return _value2; }
  static LatticeWeight One() { return LatticeWeight(0.0f, 0.0f); }
};
struct LatticeArc {
  Label _input, _output;
  LatticeWeight _w;
  StateId _to;
  LatticeArc() : _input(0), _output(0), _to(0) {}
  LatticeArc(Label i, Label o, StateId to, LatticeWeight w) : _input(i), _output(o), _w(w), _to(to) {}
};
class LatticeState {
 public:
  LatticeState() : _final(false) {}
  bool IsFinal() const { return _final; }
  void SetFinal() { _final = true; }
  void AddArc(const LatticeArc &a) { _arcs.push_back(a); }
  LatticeArc *GetArc(unsigned i) { return i < _arcs.size() ? &_arcs[i] : nullptr; }
  unsigned GetArcSize() const { return (unsigned)_arcs.size(); }

 private:
  std::vector<LatticeArc> _arcs;
  bool _final;
};
class Lattice {
 public:
  Lattice() : _start(kNoStateId) {}
  void DeleteStates() { _states.clear(); _start = kNoStateId; }
  StateId AddState() { _states.push_back(LatticeState()); return (StateId)_states.size() - 1; }
  void SetStart(StateId s) { _start = s; }
  void SetFinal(StateId s) { _states[s].SetFinal(); }
  void AddArc(StateId s, const LatticeArc &a) { _states[s].AddArc(a); }
  StateId Start() const { return _start; }
  StateId NumStates() const { return (StateId)_states.size(); }
  LatticeState *GetState(StateId s) { return &_states[s]; }
  // The reference's on-disk lattice (newfst/lattice-fst.cc:38-101, lattice-fst.h:124-172,
  // arc.h:38-86, weigth.h:229-258), little-endian, LP64: u64 number of states, i32 start state,
  // then per state {i32 final, u64 number of arcs, arcs x {i32 ilabel, i32 olabel, f32 graph cost,
  // f32 acoustic cost, i32 nextstate}}.  Write(file) APPENDS, as the reference does ("ab"), so one
  // file holds the lattices of consecutive utterances; Read(FILE*) reads the next one.
  bool Write(FILE *fp);
  bool Write(const std::string &file);
  bool Read(FILE *fp);
  bool Read(const std::string &file);

 private:
  std::vector<LatticeState> _states;
  StateId _start;
};

bool LatticeToVector(Lattice &best_path, std::vector<int> &best_words_arr, std::vector<int> &best_phones_arr,
                     float &best_tot_score, float &best_lm_score);

// ---- boundary B: what callers use -------------------------------------------------------------
class DecoderItf {
 public:
  virtual ~DecoderItf() {}
  virtual void InitDecoding() = 0;
  virtual void AdvanceDecoding(AmInterface *decodable, int32 max_num_frames = -1) = 0;
  virtual void FinalizeDecoding() = 0;
  virtual int32 NumFramesDecoded() const = 0;
  virtual BaseFloat ProcessEmitting(AmInterface *decodable) = 0;
  virtual void ProcessNonemitting(BaseFloat cost_cutoff) = 0;
  virtual bool Decode(AmInterface *decodable) = 0;
  virtual bool GetBestPath(Lattice *ofst, bool use_final_probs = true) = 0;
  virtual bool GetRawLattice(Lattice *ofst, bool use_final_probs = true) = 0;
};

// ---- many DecoderItf objects over ONE batched device decoder ------------------------------------
// The reference's service creates one decoder object per worker thread over a shared graph (v2-asr/v2-asr-work-thread.h:66,
// v2-asrbin/v2-asr-service.cc:95-105); N private 1-channel device decoders would be N latency-bound launch chains.  The pool owns
// one n_channels-wide device decoder and a batcher thread, the way the GPU service the reference ships batches its streams
// dynamically (gpu-asr/v1-gpu-kaldi-worker-pool.h:20-204: Push(corr_id, chunk) -> dynamic batcher -> batched pipeline): every
// GpuLatticeDecoder(pool) leases a channel for its lifetime; its InitDecoding / AdvanceDecoding / FinalizeDecoding / GetBestPath
// deposit a request and wait; the batcher takes whatever has arrived (plus what arrives within `linger_us`, as long as leased
// channels are still missing) and issues ONE wfst_decoder_init / _advance_host / _finalize / _get_best_path for all of them --
// while the device decodes one batch of chunks, the threads pull the next chunks from their decodables and the next batch forms.
// Everything else a decoder object may ask for (GetRawLattice, GetLattice, GetNbest ...) runs in the batcher thread too, one
// request after the other: the C ABI's calls on one decoder are not re-entrant.
// Results are those of the private decoder, bit for bit (a channel's search does not depend on its neighbours).
// At most n_channels decoder objects can be alive at a time: a further constructor waits for a channel to be released.
// The pool outlives its decoder objects (destroy them first; the pool's destructor stops the batcher and frees the device decoder).
class GpuChannelPool {
 public:
  GpuChannelPool(Fst *graph, const LatticeFasterDecoderConfig &config, int n_channels, const wfst_limits *limits = nullptr,
                 int linger_us = 50);
  GpuChannelPool(Fst *graph, const LatticeFasterDecoderConfig &config, ArpaLm *oldlm, ArpaLm *newlm, int n_channels,
                 const wfst_limits *limits = nullptr, int linger_us = 50);   // biglm
  ~GpuChannelPool();
  int NumChannels() const { return _n; }
  struct Stats {
    long long batches;            // passes of the batcher over its queue
    long long requests;           // requests served
    long long advance_calls;      // wfst_decoder_advance_host calls issued ...
    long long advance_requests;   // ... for this many AdvanceDecoding requests (their ratio = the mean batch)
    long long frames;             // frames handed to the device
    double ms_by_kind[5];         // batcher time in the C-ABI calls: init, advance, finalize, best path, one-off calls
    double ms_waiting;            // ... and waiting for requests (idle, or letting a batch form)
    long long endpoint_calls;     // wfst_decoder_endpoint_detected calls issued ...
    long long endpoint_requests;  // ... for this many EndpointDetected requests
    double ms_endpoint;           // batcher time in them
    long long partial_calls;      // wfst_decoder_partial_enqueue calls issued ...
    long long partial_requests;   // ... for this many GetPartialWords requests
    double ms_partial;            // batcher time in them (enqueueing and fetching; the device works beside the batcher)
    long long nbest_words_calls;      // wfst_decoder_get_nbest_words calls issued ...
    long long nbest_words_requests;   // ... for this many GetNbestWords requests
    double ms_nbest_words;            // batcher time in them (synchronous)
    long long partial_max_per_pass;   // the most of those LIST calls one batcher pass issued (one).  Not counted here or in partial_calls: the
                                      // synchronous request-by-request calls after a refused list or a capacity too small, which hold the batcher
  };
  Stats GetStats();
  // Pruned live lattices (wfst_decoder_set_live_lattice_prune): the live getters of every channel of the pool's decoder -- GetRawLattice,
  // GetLattice, GetNbest, GetNbestWords, GetNbestShortlist before FinalizeDecoding -- serve the lattice the channel would hold if the
  // utterance ended at this frame (FinalizeDecoding's pruning on a snapshot; the channel decodes on untouched).  The setting is the
  // device decoder's: call it before worker threads lease channels.
  void SetLiveLatticePrune(bool on);
  wfst_decoder *Handle() { return _dec; }

 private:
  friend class GpuLatticeDecoder;
  GpuChannelPool(const GpuChannelPool &);
  GpuChannelPool &operator=(const GpuChannelPool &);
  enum Kind { kInit = 0, kAdvance, kFinalize, kBestPath, kCall, kEndpoint, kPartial, kNbestWords, kKinds };
  struct Request {
    Kind kind;
    int channel;
    // kAdvance
    const float *rows; int ready, stride, max_num_frames;
    // kBestPath
    bool use_final_probs;
    std::vector<int32_t> il, ol; std::vector<float> g, ac; int n_hops, degraded;
    // kCall
    std::function<void(wfst_decoder *)> call;
    // kEndpoint: the config asked with; the rule that fired (0: none)
    const OnlineEndpointConfig *endpoint_config = nullptr;
    int endpoint_rule = 0;
    // kPartial: the words of the partial best path, the first n_stable of them final
    std::vector<int32_t> words;
    int n_stable = 0;
    // kNbestWords: asked with (nb_n paths, use_final_probs, the LM pair or none); the channel's status and its paths' text
    int nb_n = 0, nb_status = 0;
    const wfst_lm *nb_old = nullptr, *nb_new = nullptr;
    std::vector<std::vector<int> > nb_words;
    std::vector<float> nb_tot, nb_lm;
    // outcome
    int decoded;                  // NumFramesDecoded of the channel after the request
    std::exception_ptr error;
    bool done;
    // (every request is waited for on a condition variable of its own: sixty-four threads released together through ONE variable
    // and the pool's mutex wake up one behind the other -- milliseconds at an utterance boundary)
    std::mutex m;
    std::condition_variable cv;
    Request() : kind(kCall), channel(0), rows(nullptr), ready(0), stride(0), max_num_frames(-1), use_final_probs(true), n_hops(0),
                degraded(0), decoded(0), done(false) {}
  };
  void Start(int linger_us);
  int Lease();
  int TryLease();                 // -1: every channel is leased
  void Release(int channel);
  void Submit(Request *r);        // enqueue, wait, rethrow what the batcher thread caught
  void Run();
  void Execute(std::vector<Request *> &batch);
  void ExecuteAdvance(std::vector<Request *> &rs);
  void ExecuteEndpoint(std::vector<Request *> &rs);   // one wfst_decoder_endpoint_detected per distinct config
  std::string _ep_key;                                 // the config last set on the device decoder (its C struct's bytes + phones)
  void ExecuteBestPath(std::vector<Request *> &rs);   // synchronous (the fall-back when a list is refused: request by request)
  // best paths WITHOUT the batcher standing still: the waiting requests of one kind (with / without final-probs) go to the device as
  // one list (wfst_decoder_best_path_enqueue), the batcher goes on feeding the device, and takes the results when they have landed
  void StartBestPaths();
  bool PollBestPaths(bool block);
  void Finish(std::vector<Request *> &rs);
  // partial words the same way: ONE wfst_decoder_partial_enqueue per batcher pass for every waiting request, polled with _ready
  // (the synchronous endpoint call holds the batcher until the device has answered; this one does not)
  void StartPartials();
  bool PollPartials(bool block);
  void ExecutePartial(std::vector<Request *> &rs);    // synchronous, request by request (a refused list, a capacity too small)
  std::vector<Request *> _pt_wait, _pt_flight;   // (the batcher thread's own)
  // GetNbestWords of every waiting channel: one wfst_decoder_get_nbest_words per distinct (n, use_final_probs, LM pair); synchronous
  void ExecuteNbestWords(std::vector<Request *> &rs);
  int _pt_cap = 0;
  // The decoder objects' row buffers as slots of ONE page-locked allocation, equally spaced: rows of consecutive channels that cover
  // the same frames then go to the device as one 2-D copy (wfst_decoder_advance_host).  Allocated by the first object that asks, every
  // slot as large as that request (a service reserves its longest utterance: ReserveRows); nullptr: no room for `floats` in a slot --
  // the object keeps a buffer of its own.
  float *RowSlot(int channel, size_t floats, size_t *slot_floats);
  std::mutex _slab_mu;
  float *_slab = nullptr;
  size_t _slab_pitch = 0;   // floats per slot
  std::vector<Request *> _bp_wait, _bp_flight;   // (the batcher thread's own)
  int _bp_cap = 0, _bp_ufp = 1;
  std::atomic<int> _n_bp_outstanding{0};         // their number, for the submitting threads (which one completes a batch)
  void CountBestPaths() { _n_bp_outstanding.store((int)(_bp_wait.size() + _bp_flight.size() + _pt_wait.size() + _pt_flight.size())); }   // (and partial words)
  wfst_decoder *_dec;
  Fst *_graph;
  int _n, _linger_us;
  std::mutex _mu;
  std::condition_variable _cv_work, _cv_free;
  static void Done(Request *r);   // marks it served and wakes its thread (the request may be gone when this returns)
  std::vector<Request *> _queue;
  std::vector<char> _leased;
  int _n_leased;
  bool _stop;
  Stats _stats;
  // WFST_POOL_TRACE=<file>: one line per batcher pass (when its first request arrived, when it was closed, what it held, how long each
  // kind's device calls took, whether the device was still busy when it closed), written when the pool goes
  struct TracePass { double t_first, t_closed, t_end; int n[kKinds]; double ms[kKinds]; int busy; };
  std::vector<TracePass> _trace;
  std::string _trace_file;
  std::chrono::steady_clock::time_point _t_origin, _t_first;
  std::thread _thread;
};

// One utterance stream on channel 0 of a private 1-channel device decoder -- or, constructed over a GpuChannelPool, on a channel
// leased from the pool's batched decoder (the shape for a service's worker threads).  Scores are pulled
// through LogLikelihood(f, i) for the frames that became ready since the last call (or taken in
// one piece from a MatrixDecodable) and shipped to the GPU; the search runs there.
// Fatal conditions throw std::runtime_error (the reference's LOG_ERR does, util/log-message.cc:
// 122-145); soft ones print a warning and return false, as in the reference.
// One word sequence aligned on a channel's raw lattice (wfst_decoder_align_words): the cheapest path that spells it.  frames[k] =
// (begin, end) of word k in frames, end exclusive, by GetWords' definition with the aligned path's arcs as the hops; tot / lm =
// LatticeToVector's two scores of that path; found = false (and everything else empty / zero): the sequence is not in the lattice.
struct WordAlignment {
  bool found = false;
  int n_arcs = 0;
  float tot = 0.0f, lm = 0.0f;
  std::vector<std::pair<int, int> > frames;
};

// A WordAlignment with the confidences of its words (wfst_decoder_word_confidence): word_post[k] = the posterior mass of the lattice's
// arcs that say word k in the word's cell of the time axis (cells cut at the midpoints of consecutive begin frames; above 1 where
// paths say a short word twice inside one cell), conf[k] = min(1, word_post[k]); path_logpost = the log posterior of the aligned path
// itself; log_z = the log of the lattice's total weight.  Arcs cost graph_scale * graph + acoustic_scale * acoustic, in double; the
// alignment's own fields stay unscaled.  The doubles are reproducible to rounding, not bit for bit.
struct WordConfidence : WordAlignment {
  std::vector<double> conf, word_post;
  double path_logpost = 0.0, log_z = 0.0;
};

// A WordConfidence with the alternatives of every word's slot (wfst_decoder_word_alternatives), a confusion network pinned to the
// sequence: alts[k] = the words the lattice says in word k's cell of the time axis as (word, posterior mass), by mass descending and
// word id ascending, the first n_alts of them (unclamped; the sequence's own word is among them where it ranks that high, and
// word_post[k] is its mass); n_distinct[k] = how many words the cell has in all; none_post[k] = the share of the lattice's weight on the
// paths that say nothing in the cell.  The doubles are reproducible to rounding, not bit for bit; a list is ordered on the device's sums.
struct WordAlternatives : WordConfidence {
  std::vector<std::vector<std::pair<int, double> > > alts;
  std::vector<double> none_post;
  std::vector<int> n_distinct;
};

// The posterior of a whole word sequence, or of a phrase, on a channel's raw lattice (wfst_decoder_sequence_posterior).  A sentence:
// logpost = the log of the share of the lattice's weight on ALL paths that spell the sequence, count = exp(logpost).  A phrase: count
// = the expected number of times a path says it (overlapping occurrences included: it may pass 1), logpost = log(count), and -- where
// asked for -- hit_mass[f] = the count by the frame f at which the phrase's last word begins, peak = the lowest frame of its largest
// entry (-1: no rows, or nothing found).  conf = min(1, count); log_z = the log of the lattice's total weight.  found = false
// (logpost, count and conf zero): no path spells the sequence / says the phrase, or the channel has no lattice.  Arcs cost
// graph_scale * graph + acoustic_scale * acoustic, in double.  The doubles are reproducible to rounding, not bit for bit.
struct SequencePosterior {
  bool found = false;
  double logpost = 0.0, count = 0.0, conf = 0.0, log_z = 0.0;
  std::vector<double> hit_mass;
  int peak = -1;
};

// Frame posteriors of a channel's raw lattice (wfst_decoder_frame_posteriors), Kaldi's lattice-to-post: per frame f the classes of the
// frame's emitting arcs -- the transition-id, or label_map[transition-id]: a pdf, a phone -- with their posterior mass, as
// classes / posts[frame_off[f] .. frame_off[f + 1]), by class ascending, only those with a mass > 0 and >= min_post; n_distinct[f] =
// the classes with a mass > 0 and frame_mass[f] = their sum, both before the threshold.  n_frames = 0 (log_z 0, nothing listed): the
// channel has no lattice.  status: WFST_OK or the channel's own error code.  The doubles are reproducible to rounding, not bit for bit.
struct FramePosteriors {
  int status = 0, n_frames = 0;
  double log_z = 0.0;
  std::vector<int> frame_off, classes, n_distinct;
  std::vector<double> posts, frame_mass;
};

// Sequence-training statistics of a channel's raw lattice against a reference alignment (wfst_decoder_sequence_stats), Kaldi's
// LatticeForwardBackwardMpeVariants "smbr" and LatticeForwardBackwardMmi: per frame f the classes with a posterior mass > 0 as
// classes / posts / values[frame_off[f] .. frame_off[f + 1]), by class ascending; values = the derivative of the criterion with
// respect to the class' score at that frame (under MMI with one more entry where the reference class is outside the lattice, or the
// frame dropped: n_dropped); tot_acc = the expected number of correct frames (0 under MMI).  n_frames = 0: the channel has no
// lattice.  status: WFST_OK or the channel's own error code.  The doubles are reproducible to rounding, not bit for bit.
struct SequenceStats {
  int status = 0, n_frames = 0, n_ref_frames = 0, n_dropped = 0;
  double log_z = 0.0, tot_acc = 0.0;
  std::vector<int> frame_off, classes;
  std::vector<double> posts, values;
};
// What SequenceStats is asked with.  label_map: n_tid + 1 entries >= 0, entry 0 unused (empty: the class is the transition-id);
// sil_classes: up to 64 class ids, ascending.  The dense output (see wfst_decoder_sequence_stats): grad[i] = a DEVICE pointer to
// float32 [grad_frames[i]][n_cols] rows of grad_pitch[i] floats for listed channel i, or nullptr (grad empty: none; grad_pitch empty:
// n_cols); consumer_stream: the hipStream_t that reads the rows next (nullptr: the default stream; WFST_STREAM_NONE: none).
struct SequenceStatsOptions {
  bool mmi = false, use_final_probs = true, drop_frames = false;
  double graph_scale = 1.0, acoustic_scale = 1.0;
  std::vector<int> label_map, sil_classes;
  std::vector<void *> grad;
  std::vector<long long> grad_pitch;
  std::vector<int> grad_frames;
  int n_cols = 0;
  double grad_scale = 1.0;
  void *consumer_stream = WFST_STREAM_NONE;
  long long max_cells = 0;
};

// Forced alignment of a channel's scores against the utterance's own graph (wfst_decoder_force_align; Kaldi's align-compiled-mapped):
// exact float32 Viterbi, bit for bit reproducible.  hop_arc = the path's arcs as indices into the graph's arc array; alignment = one
// class per frame (the transition-id, or label_map of it: SequenceStats' `ref` as it stands); words / word_frame = the path's words
// with the frame each begins at; path_cost = the table's cost of the path, tot / lm = LatticeToVector's two scores of it.
// found = false (everything else empty / zero): the graph does not accept the channel's frames.
struct ForcedAlignment {
  int status = 0;
  bool found = false;
  int n_frames = 0;
  float path_cost = 0.0f, tot = 0.0f, lm = 0.0f;
  std::vector<int> hop_arc, alignment, words, word_frame;
};
// A set of per-utterance graphs resident on a device (wfst_align_graphs): files[i] in any format Fst::ReadFst reads.
class AlignGraphs {
 public:
  AlignGraphs() : _g(nullptr), _n(0) {}
  ~AlignGraphs();
  bool Read(const std::vector<std::string> &files, int device = 0);  // false (with a message on stderr) on failure
  int Size() const { return _n; }
  const wfst_align_graphs *Handle() const { return _g; }

 private:
  AlignGraphs(const AlignGraphs &);
  AlignGraphs &operator=(const AlignGraphs &);
  wfst_align_graphs *_g;
  int _n;
};

// Graph posteriors of a channel's scores over the utterance's own graph (wfst_decoder_graph_posteriors): the forward-backward pass
// force_align takes the best path of.  log_like = the log of the sum over the graph's paths (MMI's numerator term); per frame f the
// classes of the graph's emitting arcs with their posterior, in FramePosteriors' list format; arc_occ[a] = the expected count of arc a
// of the graph (empty unless asked for).  found = false (everything else empty / zero): the graph does not accept the channel's
// frames.  status: WFST_OK or the channel's own error code.  The doubles are reproducible to rounding, not bit for bit.
struct GraphPosteriors {
  int status = 0;
  bool found = false;
  int n_frames = 0;
  double log_like = 0.0;
  std::vector<int> frame_off, classes, n_distinct;
  std::vector<double> posts, frame_mass, arc_occ;
};
// What GraphPosteriors is asked with.  label_map and the dense output (grad .. consumer_stream) as SequenceStatsOptions has them;
// the scales are finite and >= 0.
struct GraphPosteriorsOptions {
  double graph_scale = 1.0, acoustic_scale = 1.0, min_post = 0.0;
  bool arc_occupancy = false;
  std::vector<int> label_map;
  std::vector<void *> grad;
  std::vector<long long> grad_pitch;
  std::vector<int> grad_frames;
  int n_cols = 0;
  double grad_scale = 1.0;
  void *consumer_stream = WFST_STREAM_NONE;
  long long max_cells = 0;
};

// The path of a channel's raw lattice nearest a reference word sequence (wfst_decoder_nearest_words): least word edit distance, the
// cheapest among those.  errors = sub + ins + del; words / frames[j] = the path's own words with (begin, end) as WordAlignment has
// them; ref_hyp[k] = the index in `words` that reference word k was matched or substituted with, -1: deleted; tot / lm =
// LatticeToVector's two scores of the path.  found = false (everything else empty / zero): the channel has no lattice, or no final
// state of it is reached.
struct NearestPath {
  bool found = false;
  int errors = 0, cor = 0, sub = 0, ins = 0, del = 0, n_arcs = 0;
  float tot = 0.0f, lm = 0.0f;
  std::vector<int> words, ref_hyp;
  std::vector<std::pair<int, int> > frames;
};

// A setting of RescaledWords: the graph (LM) scale, the acoustic scale and the word insertion penalty the best path is picked under.
struct RescaleSetting {
  double graph_scale = 1.0, acoustic_scale = 1.0, word_penalty = 0.0;
};

// The best path of a channel's raw lattice under a RescaleSetting (wfst_decoder_rescaled_words; Kaldi's lattice-best-path-score):
// words / frames[j] = its words with (begin, end) as WordAlignment has them; tids = its transition-ids (the alignment), where asked
// for; scaled_cost = its cost at the setting, float64, bit for bit reproducible; tot / lm = LatticeToVector's two scores of the path,
// UNSCALED.  found = false (everything else empty / zero): the channel has no lattice, or no final state of it is reached.
struct RescaledWords {
  bool found = false;
  int n_arcs = 0;
  double scaled_cost = 0.0;
  float tot = 0.0f, lm = 0.0f;
  std::vector<int> words, tids;
  std::vector<std::pair<int, int> > frames;
};

// A phrase of a bias list: 1..16 word ids and the bonus every occurrence of it in a path's words earns (finite, >= 0).
struct BiasPhrase {
  std::vector<int> words;
  double bonus = 0.0;
};
// A set of bias lists resident on one device (wfst_bias_lists), for BiasedWords.
class BiasLists {
 public:
  BiasLists() : _b(nullptr), _n(0) {}
  ~BiasLists();
  bool Set(const std::vector<std::vector<BiasPhrase> > &lists, int device = 0);  // false (with a message on stderr) on failure
  int Size() const { return _n; }
  const wfst_bias_lists *Handle() const { return _b; }

 private:
  BiasLists(const BiasLists &);
  BiasLists &operator=(const BiasLists &);
  wfst_bias_lists *_b;
  int _n;
};
// A set of books -- bias lists of up to 65 536 nodes -- resident on one device (wfst_bias_books), for BiasedWordsSparse.
class BiasBooks {
 public:
  BiasBooks() : _b(nullptr), _n(0) {}
  ~BiasBooks();
  bool Set(const std::vector<std::vector<BiasPhrase> > &books, int device = 0);  // false (with a message on stderr) on failure
  int Size() const { return _n; }
  const wfst_bias_books *Handle() const { return _b; }

 private:
  BiasBooks(const BiasBooks &);
  BiasBooks &operator=(const BiasBooks &);
  wfst_bias_books *_b;
  int _n;
};
// A setting of BiasedWords: RescaleSetting's three and the scale of the phrases' bonuses.
struct BiasSetting {
  double graph_scale = 1.0, acoustic_scale = 1.0, word_penalty = 0.0, boost_scale = 1.0;
};
// The best path of a channel's raw lattice under a BiasSetting and the channel's bias list (wfst_decoder_biased_words): words /
// frames[j] as RescaledWords has them; biased_cost = its cost, the bonuses taken off, and bonus = their sum, float64, bit for bit
// reproducible; tot / lm UNSCALED; hits[k] = (phrase's index in the list, index in words of the occurrence's last word), by word,
// the longest phrase first.  found = false (everything else empty / zero): the channel has no lattice, or no final state is reached.
// n_cells: BiasedWordsSparse's count of the channel's reachable (state, node) pairs (0 from BiasedWords, -1 beyond max_cells).
struct BiasedWords {
  bool found = false;
  int n_arcs = 0;
  long long n_cells = 0;
  double biased_cost = 0.0, bonus = 0.0;
  float tot = 0.0f, lm = 0.0f;
  std::vector<int> words;
  std::vector<std::pair<int, int> > frames, hits;
};

class GpuLatticeDecoder : public DecoderItf {
 public:
  GpuLatticeDecoder(Fst *graph, const LatticeFasterDecoderConfig &config, const wfst_limits *limits = nullptr);
  // OnlineLatticeDecoderMempoolBiglm(fst, config, oldlm, newlm) (biglm.h:21-30): on-the-fly LM rescoring
  GpuLatticeDecoder(Fst *graph, const LatticeFasterDecoderConfig &config, ArpaLm *oldlm, ArpaLm *newlm,
                    const wfst_limits *limits = nullptr);
  // a channel of the pool's decoder (graph, config, LMs and limits are the pool's); waits for a free channel
  explicit GpuLatticeDecoder(GpuChannelPool *pool);
  // THE ONE-LINE DROP-IN AT SERVICE SCALE.  After ShareDevice(n), decoder objects constructed the reference's way -- (graph, config
  // [, oldlm, newlm][, limits]), one per worker thread (v2-asr/v2-asr-work-thread.h:66) -- lease channels of a SHARED n-channel device
  // decoder per distinct (graph, config, LMs, limits) instead of creating a private 1-channel decoder each: the service's code does not
  // change, its threads' calls are batched (GpuChannelPool).  An object constructed when all n channels are leased opens a further
  // shared decoder.  ShareDevice(0): objects constructed from then on are private again (shared decoders live until their last
  // object is gone).  Call it once at start-up, before the worker threads construct their decoders.
  static void ShareDevice(int n_channels, int linger_us = 50);
  ~GpuLatticeDecoder() override;
  // Page-locked room for `frames` rows of a decodable with `num_indices` indices, allocated NOW: a service calls it when it
  // creates its decoders (it knows its model and its longest utterance).  Without it the buffer is allocated when the first rows
  // arrive and grows by doubling -- page-locking memory costs milliseconds and is serialised by the driver.
  void ReserveRows(int frames, int num_indices);
  void InitDecoding() override;
  void AdvanceDecoding(AmInterface *decodable, int32 max_num_frames = -1) override;
  void FinalizeDecoding() override;
  int32 NumFramesDecoded() const override;
  // The device frame step fuses ProcessEmitting and ProcessNonemitting: ProcessEmitting decodes
  // exactly one frame (emitting arcs + epsilon closure) and returns the cutoff it used for the
  // closure; ProcessNonemitting is then a no-op.
  BaseFloat ProcessEmitting(AmInterface *decodable) override;
  void ProcessNonemitting(BaseFloat) override {}
  // InitDecoding + all ready frames + FinalizeDecoding.  (The reference's Decode() reads one frame
  // past the end, base-inl.h:615; that landmine is not reproduced.)
  bool Decode(AmInterface *decodable) override;
  bool GetBestPath(Lattice *ofst, bool use_final_probs = true) override;
  // after FinalizeDecoding, decoder created with wfst_limits.lattice_links > 0 (else: warning + false)
  bool GetRawLattice(Lattice *ofst, bool use_final_probs = true) override;
  // GetLattice (online-decoder-base.h:182, base-inl.h:850-866): GetRawLattice + DeterminizeLatticeWrapper, both on
  // the device; arcs carry ilabel 0 / olabel = word, final states have no arcs (the reference's output convention)
  bool GetLattice(Lattice *ofst, bool use_final_probs = true);
  // the same with the service's second LM pass (--use-second, kaldi-nnet3/kaldi-online-nnet3-my-decoder.cc:53-78): the determinized
  // lattice composed with the old LM (rescaled by -1) and with the new one -- ComposeLattice twice (newfst/compose-lat-inl.h), on the device
  bool GetLattice(Lattice *ofst, ArpaLm *oldlm, ArpaLm *newlm, bool use_final_probs = true);
  // OnlineClgLatticeFastDecoder::GetNbest (kaldi-nnet3/kaldi-online-nnet3-my-decoder.cc:97-105): GetLattice + NShortestPath +
  // ConvertNbestToVector (newfst/lattice-to-nbest.cc), on the device: the n (<= 4096) cheapest paths of the determinized lattice,
  // each a linear Lattice with that lattice's own arcs on it (ilabel 0, olabel = word, both costs per arc) between the epsilon
  // arcs the reference's Reverse / AddSuperFinalState leave -- arc for arc what the reference returns.  With LMs: over the
  // second-pass lattice (--use-second).  Same conditions as GetRawLattice.
  bool GetNbest(std::vector<Lattice> &nbest_paths, int n);
  bool GetNbest(std::vector<Lattice> &nbest_paths, int n, ArpaLm *oldlm, ArpaLm *newlm);
  // the short list computed on the raw lattice without determinizing it (n <= 16, every channel of a batch in one launch): the same
  // word sequences and totals; each path's FIRST arc carries its whole weight (graph = lm_score, acoustic = tot - lm), so that
  // LatticeToVector gives words, tot_score and lm_score
  bool GetNbestShortlist(std::vector<Lattice> &nbest_paths, int n);
  // EndpointDetected (kaldi-online-nnet3-my-decoder.h:360-362; Kaldi's online2/online-endpoint.cc) after AdvanceDecoding: the
  // trailing silence of the best path and FinalRelativeCost on the device, the rules on the host.  *rule: the rule that fired
  // (1..5, 0: none).  Needs the graph's SetTid2Phone; throws for a biglm decoder, before InitDecoding or after FinalizeDecoding.
  // Over a pool, the requests of many threads go to the device as one call per batcher pass.
  bool EndpointDetected(const OnlineEndpointConfig &config, int *rule = nullptr);
  // The words of the partial result after AdvanceDecoding -- what the reference's services hand to their per-chunk callback
  // (gpu-asr/v1-gpu-asr-task.h:70-76; GetBestPathTxt, kaldi-nnet3/kaldi-online-nnet3-my-decoder.cc:122-137): *words = the words of
  // GetBestPath(use_final_probs = false) now, the first *n_stable of them a prefix of every later result of the utterance
  // (wfst_decoder_get_partial).  The device work follows the frames since the last commit, not the utterance.  false: no frame
  // decoded yet, or no token.  Throws for a biglm decoder, before InitDecoding or after FinalizeDecoding, and for a result of more
  // words than the decoder's max_frames (the call is retried once with the size it asks for; that limit no size satisfies).  Over a pool, the
  // requests of many threads go to the device as one list per batcher pass, and the batcher goes on feeding the device meanwhile.
  bool GetPartialWords(std::vector<int> *words, int *n_stable = nullptr);
  // The best path as words with times, mid-utterance or after FinalizeDecoding, any decoder kind (wfst_decoder_get_words: one
  // launch, no hop list) -- OnebestLatticeToString's words, tot_score and lm_score (kaldi-nnet3/kaldi-online-nnet3-my-decoder.cc:
  // 107-121) and the (start, end) of every word that AlignStruct carries (gpu-asr/gpu-worker-pool-itf.h:85-97), in frames, end
  // exclusive: (*frames)[k].first is the frame of the arc that carries word k's label, .second the next word's begin -- or, after
  // SetSilencePhones, one past the word's last frame that is not silence.  false: no path (no frame decoded, or no token).  Over a
  // pool the same result is derived on the host from the channel's pooled GetBestPath (no silence list there).
  bool GetWords(std::vector<int> *words, std::vector<std::pair<int, int> > *frames, float *tot, float *lm, bool use_final_probs = true);
  void SetSilencePhones(const std::vector<int> &phones);   // needs the graph's SetTid2Phone; empty: none
  // The service's per-chunk GetNbestTxt (kaldi-nnet3/kaldi-online-nnet3-my-decoder.cc:139-150), mid-utterance or after
  // FinalizeDecoding: the words, tot_score and lm_score of the n (<= 64) cheapest paths of GetLattice's lattice (with LMs: of its
  // second pass), the text made on the device (wfst_decoder_get_nbest_words).  false: no path.  The channel's own failure (a lattice
  // beyond the batch's bounds ...) throws, or with `status` given is returned there (WFST_OK otherwise).  Over a pool, the requests
  // of many threads go to the device as one list per batcher pass and distinct (n, use_final_probs, LM pair).
  bool GetNbestWords(std::vector<std::vector<int> > *words, std::vector<float> *tot, std::vector<float> *lm, int n, bool use_final_probs = true,
                     ArpaLm *oldlm = nullptr, ArpaLm *newlm = nullptr, int *status = nullptr);
  // Word times for any word sequence of the lattice -- an n-best path, the rescored 1-best a --use-second service returns
  // (kaldi-nnet3/kaldi-online-nnet3-my-decoder.cc:122-130), an outside transcript: the cheapest path of the channel's RAW lattice
  // that spells `words` (wfst_decoder_align_words), mid-utterance or after FinalizeDecoding; (*frames)[k] as GetWords has them
  // (SetSilencePhones included), *tot / *lm that path's scores.  false: the sequence is not in the lattice (or there is none).  The
  // channel's own failure throws.  Over a pool the call runs in the batcher thread, like GetNbest.
  bool AlignWords(const std::vector<int> &words, std::vector<std::pair<int, int> > *frames, float *tot, float *lm, bool use_final_probs = true);
  // ... of every path GetNbestWords returned, in one device call: (*out)[k] for nbest[k]
  void GetNbestWordTimes(const std::vector<std::vector<int> > &nbest, std::vector<WordAlignment> *out, bool use_final_probs = true);
  // ... with the confidence of every word (wfst_decoder_word_confidence), in one device call: (*out)[k] for seqs[k] (at most 64).
  // The channel's own failure throws.  Over a pool the call runs in the batcher thread, like AlignWords.
  void WordConfidences(const std::vector<std::vector<int> > &seqs, std::vector<WordConfidence> *out, bool use_final_probs = true,
                       double graph_scale = 1.0, double acoustic_scale = 1.0);
  // ... and with the alternatives of every word's slot, the n_alts (1..16) first words of its cell and the cell's "no word" mass
  // (wfst_decoder_word_alternatives), in one device call: (*out)[k] for seqs[k] (at most 64).  The channel's own failure throws.  Over
  // a pool the call runs in the batcher thread, like AlignWords.
  void WordAlternatives(const std::vector<std::vector<int> > &seqs, std::vector<struct WordAlternatives> *out, int n_alts = 5,
                        bool use_final_probs = true, double graph_scale = 1.0, double acoustic_scale = 1.0);
  // How sure the decoder is of each of `seqs` (at most 64) as a WHOLE -- the sum over every path of the RAW lattice that spells it,
  // where WordConfidence::path_logpost is one path's -- or, with phrase = true, how often and when a path says each of them as a
  // phrase (at least one word each; hit_mass: with the per-frame rows), in one device call (wfst_decoder_sequence_posterior):
  // (*out)[k] for seqs[k].  The channel's own failure throws.  Over a pool the call runs in the batcher thread, like AlignWords.
  void SequencePosteriors(const std::vector<std::vector<int> > &seqs, std::vector<SequencePosterior> *out, bool phrase = false,
                          bool use_final_probs = true, double graph_scale = 1.0, double acoustic_scale = 1.0, bool hit_mass = false);
  // What the channel's RAW lattice says at every frame, mid-utterance or after FinalizeDecoding: the posterior of each transition-id,
  // or of each class of label_map (n_tid + 1 entries >= 0, entry 0 unused; empty: none), in one device call
  // (wfst_decoder_frame_posteriors).  The channel's own failure throws.  Over a pool the call runs in the batcher thread, like AlignWords.
  void FramePosteriors(struct FramePosteriors *out, const std::vector<int> &label_map = std::vector<int>(), double min_post = 0.0,
                       bool use_final_probs = true, double graph_scale = 1.0, double acoustic_scale = 1.0);
  // The sMBR / MMI statistics of the channel's RAW lattice against `ref`, the numerator alignment's class per frame (< 0 or beyond its
  // end: unlabelled), mid-utterance or after FinalizeDecoding, in one device call (wfst_decoder_sequence_stats); opt.grad holds at most
  // one pointer.  The channel's own failure throws.  Over a pool the call runs in the batcher thread, like AlignWords.
  void SequenceStats(const std::vector<int> &ref, struct SequenceStats *out, const SequenceStatsOptions &opt = SequenceStatsOptions());
  // The forced alignment of the channel's scores -- the frames handed over so far -- against graph `graph` of `graphs`, mid-utterance
  // or after FinalizeDecoding, in one device call (wfst_decoder_force_align); label_map as FramePosteriors takes it.  The channel's
  // own failure throws.  Over a pool the call runs in the batcher thread, like AlignWords.
  void ForceAlign(const AlignGraphs &graphs, int graph, ForcedAlignment *out, const std::vector<int> &label_map = std::vector<int>());
  // The forward-backward pass of the channel's scores over graph `graph` of `graphs`, mid-utterance or after FinalizeDecoding, in one
  // device call (wfst_decoder_graph_posteriors); opt.grad holds at most one pointer.  The channel's own failure throws.  Over a pool the
  // call runs in the batcher thread, like ForceAlign.
  void GraphPosteriors(const AlignGraphs &graphs, int graph, struct GraphPosteriors *out,
                       const GraphPosteriorsOptions &opt = GraphPosteriorsOptions());
  // The lattice path nearest each of `refs` (at most 64) -- a transcript with a wrong word, a caption file, another system's
  // hypothesis -- on the channel's RAW lattice, mid-utterance or after FinalizeDecoding (wfst_decoder_nearest_words): (*out)[q] for
  // refs[q]; out->errors of a correct transcript is the lattice's oracle error (kaldi-bin/bin/nbest-compute-wer.cc:111-167 counts the
  // 1-best's).  The channel's own failure throws.  Over a pool the call runs in the batcher thread, like AlignWords.
  void NearestWords(const std::vector<std::vector<int> > &refs, std::vector<NearestPath> *out, bool use_final_probs = true);
  // The channel's best path again under each of `settings` (at most 64) -- another LM weight, another acoustic scale, a word
  // penalty -- on its RAW lattice, mid-utterance or after FinalizeDecoding, without decoding again (wfst_decoder_rescaled_words):
  // (*out)[q] for settings[q]; alignment: also the paths' transition-ids.  The channel's own failure throws.  Over a pool the call
  // runs in the batcher thread, like AlignWords.
  void RescaledWords(const std::vector<RescaleSetting> &settings, std::vector<struct RescaledWords> *out, bool use_final_probs = true,
                     bool alignment = false);
  // Phrase boosting: the channel's best path again under each of `settings` (at most 16) with list `list` of `lists` (-1: none) -- on
  // its RAW lattice, mid-utterance or after FinalizeDecoding, without decoding again (wfst_decoder_biased_words): (*out)[q] for
  // settings[q].  The channel's own failure throws.  Over a pool the call runs in the batcher thread, like AlignWords.
  void BiasedWords(const BiasLists &lists, int list, const std::vector<BiasSetting> &settings, std::vector<struct BiasedWords> *out,
                   bool use_final_probs = true);
  // The same answers for a book, a bias list of up to 65 536 nodes, from the cells a path can reach
  // (wfst_decoder_biased_words_sparse); for a list of at most 256 nodes every byte is BiasedWords'.
  void BiasedWordsSparse(const BiasBooks &books, int book, const std::vector<BiasSetting> &settings, std::vector<struct BiasedWords> *out,
                         bool use_final_probs = true);
  // Pruned live lattices (see GpuChannelPool::SetLiveLatticePrune) for this object's device decoder: the private one, or -- over a
  // pool, and so under ShareDevice -- the shared decoder of every object on it (set it before the other threads decode).
  void SetLiveLatticePrune(bool on);

 private:
  void Pull(AmInterface *decodable);
  static void SetEndpointConfig(wfst_decoder *dec, const OnlineEndpointConfig &config, std::string *key);
  template <class F> void OnDevice(F &&f);   // f(): C-ABI calls on (_dec, _chan) -- in the pool's batcher thread where there is a pool
  wfst_decoder *_dec;
  void Share(Fst *graph, const LatticeFasterDecoderConfig &config, ArpaLm *oldlm, ArpaLm *newlm, const wfst_limits *limits);
  std::shared_ptr<GpuChannelPool> _shared;   // ShareDevice: keeps the shared decoder alive
  GpuChannelPool *_pool;     // nullptr: the private decoder
  int _chan;                 // 0, or the leased channel
  int _decoded;              // pool: NumFramesDecoded as of the last request
  float *_rows;              // host history [frames][stride], page-locked (wfst_host_alloc) where the device grants it
  size_t _rows_cap;          // floats
  bool _rows_pinned;
  bool _rows_in_pool = false;   // _rows is the channel's slot of the pool's slab (not this object's to free)
  void GrowRows(size_t floats);
  void SetColumns(const Fst *graph);   // the graph's tid2pdf -> one representative transition-id per pdf (Pull)
  std::vector<int32_t> _rep;           // [pdf] a transition-id of that pdf; empty: the rows are indexed by the decodable's own indices
  std::string _ep_key;                 // private decoder: the endpoint config last set
  int _stride, _rows_ready;
  bool _inited;
};

// Batch shape: n_channels utterances per call, device-resident matrices.
class GpuBatchDecoder {
 public:
  GpuBatchDecoder(Fst *graph, const LatticeFasterDecoderConfig &config, int n_channels,
                  const wfst_limits *limits = nullptr, void *hip_stream = nullptr);
  GpuBatchDecoder(Fst *graph, const LatticeFasterDecoderConfig &config, ArpaLm *oldlm, ArpaLm *newlm, int n_channels,
                  const wfst_limits *limits = nullptr, void *hip_stream = nullptr);  // biglm
  ~GpuBatchDecoder();
  void InitDecoding(const std::vector<int> &channels = std::vector<int>());
  void AdvanceDecoding(const std::vector<int> &channels, const std::vector<const float *> &device_loglikes,
                       const std::vector<int> &num_frames_ready, int stride, int max_num_frames = -1);
  void AdvanceDecodingHost(const std::vector<int> &channels, const std::vector<const float *> &host_loglikes,
                           const std::vector<int> &num_frames_ready, int stride, int max_num_frames = -1);
  // Chunks of the acoustic model's raw output, on the device and in its own precision (wfst_decoder_advance_chunk): entry i appends
  // num_new_frames[i] rows of n_cols elements of dtype (WFST_DTYPE_*) starting at device_rows[i], row_pitch[i] elements apart (empty:
  // n_cols), to the channel's utterance as (x - log_priors[j]) * acoustic_scale -- SetScoreTransform, the reference's
  // --acoustic-scale and prior layer (kaldi-nnet3bin/kaldi-hclg-my-decoder.cc:37-41,107; nnet/nnet-layer.cc:30) -- and decodes.
  // producer_stream: the hipStream_t whose work writes the rows (nullptr: the default stream; WFST_STREAM_NONE: they are complete).
  void SetScoreTransform(float acoustic_scale, const std::vector<float> &log_priors = std::vector<float>());
  void AdvanceDecodingChunk(const std::vector<int> &channels, const std::vector<const void *> &device_rows,
                            const std::vector<int> &num_new_frames, int dtype, int n_cols, void *producer_stream = nullptr,
                            const std::vector<int64_t> &row_pitch = std::vector<int64_t>(), int max_num_frames = -1);
  void FinalizeDecoding(const std::vector<int> &channels = std::vector<int>());
  int NumFramesDecoded(int channel) const;
  bool GetBestPath(int channel, Lattice *ofst, bool use_final_probs = true);
  bool GetRawLattice(int channel, Lattice *ofst, bool use_final_probs = true);
  // the raw lattices of many channels: one device fetch, then the per-lattice host work on
  // `threads` host threads (0: up to 16)
  void GetRawLattices(const std::vector<int> &channels, std::vector<Lattice> *ofsts, std::vector<bool> *ok,
                      bool use_final_probs = true, int threads = 0);
  bool GetNbest(int channel, std::vector<Lattice> &nbest_paths, int n);
  bool GetNbest(int channel, std::vector<Lattice> &nbest_paths, int n, ArpaLm *oldlm, ArpaLm *newlm);
  bool GetNbestShortlist(int channel, std::vector<Lattice> &nbest_paths, int n);   // (n <= 16; see GpuLatticeDecoder)
  // GetLattice ahead of its request: the finalized channels go to the determinizer now, on a side stream; GetBestPaths / GetNbest
  // run beside it and the first GetLattice finds the work done or waits (wfst_decoder_prefetch_determinized)
  void PrefetchLattices();
  // ... detached: the channels go on to their next utterances beside the determinizer (wfst_decoder_prefetch_determinized_detached);
  // the lattices of the utterances finalized at that call are fetched with GetPrefetchedLattice once harvested -- by the next
  // PrefetchLatticesDetached, or by HarvestPrefetchedLattices (which waits)
  void PrefetchLatticesDetached();
  void HarvestPrefetchedLattices();
  bool GetPrefetchedLattice(int channel, Lattice *ofst);
  // GetLattice of one channel; the first call after FinalizeDecoding determinizes every finalized channel in one launch
  bool GetLattice(int channel, Lattice *ofst, bool use_final_probs = true);
  bool GetLattice(int channel, Lattice *ofst, ArpaLm *oldlm, ArpaLm *newlm, bool use_final_probs = true);   // with the second LM pass
  void GetBestPaths(const std::vector<int> &channels, std::vector<Lattice> *ofsts, std::vector<bool> *ok,
                    bool use_final_probs = true);
  // The service's post-processing for MANY finalized channels at once -- GetLattice under --use-second and GetNbest, which the
  // reference runs per utterance on one worker thread each (kaldi-nnet3/kaldi-online-nnet3-my-decoder.cc:50-105,
  // v2-asr/v2-asr-work-thread.h:66): every stage is one launch for the whole list (wfst_decoder_rescore_lattices /
  // wfst_decoder_nbest_paths_batch), the results come back once.  (*ok)[i] = what the per-channel call would return.
  void GetLattices(const std::vector<int> &channels, std::vector<Lattice> *ofsts, std::vector<bool> *ok, ArpaLm *oldlm, ArpaLm *newlm,
                   bool use_final_probs = true);
  void GetNbests(const std::vector<int> &channels, std::vector<std::vector<Lattice> > *nbests, std::vector<bool> *ok, int n,
                 ArpaLm *oldlm = nullptr, ArpaLm *newlm = nullptr);
  // EndpointDetected of many channels in one device call ((*rule)[i]: 1..5, 0 none); the one-channel form
  void EndpointDetected(const std::vector<int> &channels, const OnlineEndpointConfig &config, std::vector<bool> *detected,
                        std::vector<int> *rule = nullptr);
  bool EndpointDetected(int channel, const OnlineEndpointConfig &config, int *rule = nullptr);
  // GetPartialWords (see GpuLatticeDecoder) of many channels in one device call; the one-channel form
  void GetPartialWords(const std::vector<int> &channels, std::vector<std::vector<int> > *words, std::vector<int> *n_stable = nullptr,
                       std::vector<int> *stable_frame = nullptr);
  bool GetPartialWords(int channel, std::vector<int> *words, int *n_stable = nullptr);
  // GetWords (see GpuLatticeDecoder) of many channels (none listed: all) in one device call; (*ok)[i]: the channel has a path
  void GetWords(const std::vector<int> &channels, std::vector<std::vector<int> > *words,
                std::vector<std::vector<std::pair<int, int> > > *frames, std::vector<float> *tot, std::vector<float> *lm,
                std::vector<bool> *ok = nullptr, bool use_final_probs = true);
  void SetSilencePhones(const std::vector<int> &phones);
  // GetNbestWords (see GpuLatticeDecoder) of many channels (none listed: all), live and finalized mixed, one launch per stage:
  // (*words)[i][k], (*tot)[i][k], (*lm)[i][k] of listed channel i's path k; (*status)[i]: WFST_OK or the channel's own error code
  void GetNbestWords(const std::vector<int> &channels, int n, ArpaLm *oldlm, ArpaLm *newlm, bool use_final_probs,
                     std::vector<std::vector<std::vector<int> > > *words, std::vector<std::vector<float> > *tot,
                     std::vector<std::vector<float> > *lm, std::vector<int> *status = nullptr);
  // AlignWords (see GpuLatticeDecoder) of many channels (none listed: all), live and finalized mixed, one launch per stage:
  // seqs[i] = the word sequences for listed channel i (at most 64), (*out)[i][q] the answer for seqs[i][q]; (*status)[i]: WFST_OK or
  // the channel's own error code (nothing of it is found then; without `status` it throws).  max_cells: see wfst_decoder_align_words.
  void AlignWords(const std::vector<int> &channels, const std::vector<std::vector<std::vector<int> > > &seqs, bool use_final_probs,
                  std::vector<std::vector<WordAlignment> > *out, std::vector<int> *status = nullptr, long long max_cells = 0);
  // WordConfidences (see GpuLatticeDecoder) of many channels (none listed: all), live and finalized mixed, one launch per stage;
  // the arguments and the status rule are AlignWords'
  void WordConfidences(const std::vector<int> &channels, const std::vector<std::vector<std::vector<int> > > &seqs, bool use_final_probs,
                       double graph_scale, double acoustic_scale, std::vector<std::vector<WordConfidence> > *out,
                       std::vector<int> *status = nullptr, long long max_cells = 0);
  // WordAlternatives (see GpuLatticeDecoder) of many channels (none listed: all), live and finalized mixed, one launch per stage;
  // the arguments and the status rule are AlignWords'
  void WordAlternatives(const std::vector<int> &channels, const std::vector<std::vector<std::vector<int> > > &seqs, int n_alts,
                        bool use_final_probs, double graph_scale, double acoustic_scale, std::vector<std::vector<struct WordAlternatives> > *out,
                        std::vector<int> *status = nullptr, long long max_cells = 0);
  // SequencePosteriors (see GpuLatticeDecoder) of many channels (none listed: all), live and finalized mixed, one launch per stage;
  // the arguments and the status rule are AlignWords'.  The hit_mass rows are given the room the lattices need.
  void SequencePosteriors(const std::vector<int> &channels, const std::vector<std::vector<std::vector<int> > > &seqs, bool phrase,
                          bool use_final_probs, double graph_scale, double acoustic_scale, std::vector<std::vector<SequencePosterior> > *out,
                          std::vector<int> *status = nullptr, long long max_cells = 0, bool hit_mass = false);
  // FramePosteriors (see GpuLatticeDecoder) of many channels (none listed: all), live and finalized mixed, one launch per stage:
  // (*out)[i] for listed channel i, its own error code in (*out)[i].status (without `status` it throws); the rows are given the room
  // the lattices need.  max_cells: see wfst_decoder_frame_posteriors.
  void FramePosteriors(const std::vector<int> &channels, bool use_final_probs, double graph_scale, double acoustic_scale,
                       const std::vector<int> &label_map, double min_post, std::vector<struct FramePosteriors> *out,
                       std::vector<int> *status = nullptr, long long max_cells = 0);
  // SequenceStats (see GpuLatticeDecoder) of many channels (none listed: all), live and finalized mixed, one launch per stage:
  // refs[i] and (*out)[i] for listed channel i, its own error code in (*out)[i].status (without `status` it throws); the rows are
  // given the room the lattices need.
  void SequenceStats(const std::vector<int> &channels, const std::vector<std::vector<int> > &refs, const SequenceStatsOptions &opt,
                     std::vector<struct SequenceStats> *out, std::vector<int> *status = nullptr);
  // ForceAlign (see GpuLatticeDecoder) of many channels (none listed: all) in one launch: graph_of[i] = the graph of listed channel i
  // (empty: graph i), (*out)[i] its answer, its own error code in (*out)[i].status (without `status` it throws); the rows are given
  // the room the paths need.  max_cells: see wfst_decoder_force_align.
  void ForceAlign(const std::vector<int> &channels, const AlignGraphs &graphs, const std::vector<int> &graph_of,
                  const std::vector<int> &label_map, std::vector<ForcedAlignment> *out, std::vector<int> *status = nullptr,
                  long long max_cells = 0);
  // GraphPosteriors (see GpuLatticeDecoder) of many channels (none listed: all) in one launch per stage: graph_of[i] = the graph of
  // listed channel i (empty: graph i), (*out)[i] its answer, its own error code in (*out)[i].status (without `status` it throws); the
  // rows are given the room the lists need.
  void GraphPosteriors(const std::vector<int> &channels, const AlignGraphs &graphs, const std::vector<int> &graph_of,
                       const GraphPosteriorsOptions &opt, std::vector<struct GraphPosteriors> *out, std::vector<int> *status = nullptr);
  // NearestWords (see GpuLatticeDecoder) of many channels (none listed: all), live and finalized mixed, one launch per stage:
  // refs[i] = the references for listed channel i (at most 64), (*out)[i][q] the answer for refs[i][q]; (*status)[i]: WFST_OK or the
  // channel's own error code (without `status` it throws).  max_cells: see wfst_decoder_nearest_words.
  void NearestWords(const std::vector<int> &channels, const std::vector<std::vector<std::vector<int> > > &refs, bool use_final_probs,
                    std::vector<std::vector<NearestPath> > *out, std::vector<int> *status = nullptr, long long max_cells = 0);
  // RescaledWords (see GpuLatticeDecoder) of many channels (none listed: all), live and finalized mixed, one launch per stage: the
  // settings (at most 64) are shared by the listed channels, (*out)[i][q] is the answer of listed channel i under settings[q];
  // (*status)[i]: WFST_OK or the channel's own error code (without `status` it throws).  max_cells: see wfst_decoder_rescaled_words.
  void RescaledWords(const std::vector<int> &channels, const std::vector<RescaleSetting> &settings, bool use_final_probs,
                     std::vector<std::vector<struct RescaledWords> > *out, std::vector<int> *status = nullptr, bool alignment = false,
                     long long max_cells = 0);
  // BiasedWords (see GpuLatticeDecoder) of many channels (none listed: all), live and finalized mixed, one launch per stage:
  // list_of[i] = the list of listed channel i (-1: none; empty: none has one), the settings (at most 16) are shared, (*out)[i][q] is
  // the answer of listed channel i under settings[q]; (*status)[i]: WFST_OK or the channel's own error code (without `status` it
  // throws).  max_cells: see wfst_decoder_biased_words.
  void BiasedWords(const std::vector<int> &channels, const BiasLists &lists, const std::vector<int> &list_of,
                   const std::vector<BiasSetting> &settings, bool use_final_probs, std::vector<std::vector<struct BiasedWords> > *out,
                   std::vector<int> *status = nullptr, long long max_cells = 0);
  // BiasedWordsSparse (see GpuLatticeDecoder) of many channels: BiasedWords' arguments with books; max_cells bounds ONE channel's
  // reachable cells, round_cells the cost cells of one round (see wfst_decoder_biased_words_sparse; 0: the defaults).
  void BiasedWordsSparse(const std::vector<int> &channels, const BiasBooks &books, const std::vector<int> &book_of,
                         const std::vector<BiasSetting> &settings, bool use_final_probs, std::vector<std::vector<struct BiasedWords> > *out,
                         std::vector<int> *status = nullptr, long long max_cells = 0, long long round_cells = 0);
  void SetLiveLatticePrune(bool on);   // pruned live lattices for every channel (see GpuChannelPool::SetLiveLatticePrune)
  wfst_decoder *Handle() { return _dec; }

 private:
  wfst_decoder *_dec;
  int _n;
  std::string _ep_key;
};

// the reference's name for the biglm decoder (biglm.h:570): `OnlineLatticeDecoderMempoolBiglm decode(&fst, opt, &lm1, &lm2);`
typedef GpuLatticeDecoder OnlineLatticeDecoderMempoolBiglm;

}  // namespace datemoon
#endif
