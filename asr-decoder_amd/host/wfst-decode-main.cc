// wfst-decode: offline batch decode of precomputed log-likelihood matrices on an MI355X.
// Same job and call sequence as the reference CLI kaldi-nnet3bin/kaldi-hclg-my-decoder.cc
// (graph + decoder config + per-utterance matrices -> word ids, scores, real-time factor), with
// plain files instead of Kaldi tables:
//
//   wfst-decode [--tid2pdf=FILE] [--batch=N] [--single-stream] [--lattice-out=FILE [--lattice-links=N] [--determinize]]
//               [--lm-old=FILE --lm-new=FILE]
//   --lm-old/--lm-new  biglm (kaldi-hclg-my-decoder-biglm.cc): rescore on the fly with new LM - old LM; the files
//                  are the reference's binary LMs (arpa2fsa-bin); the old one is rescaled by -1 as the reference CLI does
//               CONFIG GRAPH LOGLIKES [WORDS_OUT]
//   --second-lm-old/--second-lm-new  the service's --use-second: GetLattice (--determinize) and GetNbest (--nbest) run the second LM pass
//                  (ComposeLattice with the old LM rescaled by -1, then with the new one) on the determinized lattice, on the device
//   --nbest-lattice-out  also write every n-best path as the linear lattice GetNbest returns (NShortestPath + ConvertNbestToVector)
//   --lattice-out  also write GetRawLattice of every utterance, in utterance order, in the
//                  reference's on-disk lattice format (Lattice::Write, newfst/lattice-fst.cc:38-64;
//                  lattice mode: N forward links kept per utterance).  An utterance without a
//                  lattice is written as an empty one (0 states, start -1).
//   --determinize  the lattices written are GetLattice's (determinized on the device, base-inl.h:850-866) instead of
//                  GetRawLattice's
//   --chunk=N      single-stream only: the streaming caller's shape (OnlineClgLatticeFastDecoder::ProcessData,
//                  kaldi-nnet3/kaldi-online-nnet3-my-decoder.cc:10-48): NumFramesReady() grows by N frames per
//                  AdvanceDecoding call; after every call the partial result GetBestPath(use_final_probs = false) is
//                  printed as "KEY@frames word-ids..." (GetBestPathTxt(..., false), :122-137); with --nbest also the
//                  partial n-best (lattice mode serves GetNbest mid-utterance)
//   --partial-words  with --chunk=N (and --single-stream or --threads=N): the partial result after every chunk comes from
//                  GetPartialWords -- the incremental form, whose device work follows the frames since the last commit, not the
//                  utterance -- and is printed as "KEY@frames n_stable word-ids...": the first n_stable words are final (the partial
//                  n-best lines of --nbest follow it as they follow the plain partial line)
//   --partial-nbest=K  with --chunk=N, in every shape (--single-stream, --threads=N [--pool=M], the batch shape): after every chunk
//                  but the last, per stream, the service's per-chunk GetNbestTxt (GetNbestWords: wfst_decoder_get_nbest_words, one
//                  list call for the streams that ask together) as "KEY@frames nbest k: word-ids... tot=.. lm=.." per path, over the
//                  second-pass lattice with --second-lm-old/--second-lm-new; a stream's own failure: "KEY@frames nbest status=code"
//   --live-lattice-prune  with --chunk=N --partial-nbest=K, in every shape: the per-chunk n-best comes from the PRUNED live lattice
//                  (SetLiveLatticePrune: the lattice the stream would hold if the utterance ended at this frame -- FinalizeDecoding's
//                  pruning on a snapshot, the stream decodes on untouched) instead of from everything alive, which at service sizes
//                  is mostly beyond the determinizer's bounds; the line format is the same
//   --word-times [--silence-phones=a:b:c]  batch shape and --single-stream: after an utterance's "KEY word-ids..." line one line
//                  "KEY#k word begin end" per word -- the frames of GetWords (wfst_decoder_get_words: the word's label-carrying
//                  arc, and the next word's begin or, with silence phones and --tid2phone=FILE, one past the word's last frame
//                  that is not silence; end exclusive): the (start, end) per word of the reference's AlignStruct
//                  (gpu-asr/gpu-worker-pool-itf.h:85-97)
//   --nbest-word-times  with --nbest=N and/or --partial-nbest=K, batch shape and --single-stream: after every path's line one line
//                  "KEY-k#j word begin end" per word ("KEY@frames nbest k#j word begin end" behind a --partial-nbest line) -- the
//                  path's words aligned on the utterance's RAW lattice (AlignWords: wfst_decoder_align_words), frames as --word-times
//                  has them; a path whose words the raw lattice does not hold prints "... notfound"
//   --align-words=FILE  batch shape and --single-stream: FILE holds lines "KEY w1 w2 ..." (several per KEY, at most 64); after the
//                  utterance's lines, per sequence "KEY align q found=0|1 arcs=N tot=.. lm=.." and "KEY align q#j word begin end"
//   --word-confidence[=GRAPH_SCALE,ACOUSTIC_SCALE]  with --nbest-word-times and/or --align-words=FILE: the confidence of every aligned
//                  word from the posteriors of the RAW lattice (WordConfidences: wfst_decoder_word_confidence; scales default 1,1) --
//                  every "...#j word begin end" line gains a fourth column conf (min(1, the posterior mass of the arcs that say the
//                  word at about that time)), and every path line ("KEY-k ...", "KEY@frames nbest k: ...", "KEY align q ...") of a
//                  path that was found gains " logpost=.." (the log posterior of the aligned path itself)
//   --sentence-posterior  with --nbest-word-times and/or --align-words=FILE: every path line of a path that was found gains
//                  " sentpost=..", the log posterior of the path's WORD SEQUENCE over all paths of the RAW lattice that spell it
//                  (SequencePosteriors: wfst_decoder_sequence_posterior), where logpost is one path's; the scales are
//                  --word-confidence=GS,AS's when given, else 1,1
//   --word-alternatives[=K]  with --nbest-word-times and/or --align-words=FILE: a confusion network pinned to every aligned sequence
//                  (WordAlternatives: wfst_decoder_word_alternatives; K = 1..16, default 5) -- every "...#j word begin end" line gains
//                  " none=.." (the share of the RAW lattice's weight on the paths that say nothing in the word's slot) and
//                  " alts=word:post,..." (the K first words of the slot by posterior mass; "alts=-": the slot has none); the scales
//                  are --word-confidence=GS,AS's when given, else 1,1
//   --phrase-posterior=FILE  batch shape and --single-stream: FILE has --align-words' format, its lines being phrases of at least one
//                  word; after the utterance's lines, per phrase "KEY phrase q found=0|1 count=.. conf=.. peak=FRAME": the expected
//                  number of times a path of the RAW lattice says the phrase, min(1, count), and the lowest frame with the most of
//                  that mass (the begin frame of the phrase's last word; -1: not found); scales as --sentence-posterior
//   --frame-post=FILE [--frame-post-class=tid|pdf|phone] [--frame-post-scales=GS,AS] [--frame-post-min=X]  batch shape and
//                  --single-stream: FILE gets one line per utterance in Kaldi's text posterior form, "KEY [ c p c p ] [ ... ]", one
//                  bracket per frame: the classes of the frame's emitting lattice arcs with their posterior mass, by class ascending
//                  (FramePosteriors: wfst_decoder_frame_posteriors) -- the transition-ids (lattice-to-post), or their pdfs
//                  (--tid2pdf=FILE) or phones (--tid2phone=FILE); the arcs cost GS * graph + AS * acoustic (default 1,1); X: only
//                  the classes with a mass >= X.  The other output is what it is without the flag.
//   --seq-stats=FILE --seq-ref=FILE [--seq-criterion=smbr|mmi] [--seq-class=tid|pdf|phone] [--seq-scales=GS,AS] [--seq-silence=a:b:c]
//                  [--seq-drop-frames]  batch shape and --single-stream: the sequence-training statistics of every utterance's RAW
//                  lattice (SequenceStats: wfst_decoder_sequence_stats; Kaldi's lattice-to-smbr-post / lattice-to-mpe-post and the
//                  MMI occupation difference).  --seq-ref=FILE holds one line "KEY c c c ..." per utterance, the numerator alignment's
//                  class per frame (< 0: unlabelled; an utterance without a line is unlabelled throughout).  FILE gets two lines per
//                  utterance: "KEY [ c v c v ] [ ... ]", Kaldi's text posterior form with the SIGNED values (17 digits), one bracket
//                  per frame, by class ascending, and "KEY seq-stats criterion=.. tot_acc=.. n_frames=.. n_ref_frames=..
//                  n_dropped=.. log_z=..".  Classes as --frame-post-class has them; the arcs cost GS * graph + AS * acoustic
//                  (default 1,1); --seq-silence: classes that never count as correct (sMBR); --seq-drop-frames: MMI's
//                  --drop-frames.  The other output is what it is without the flag.
//   --force-align=DIR [--force-align-class=tid|pdf|phone]  batch shape and --single-stream: after the utterance's other lines the
//                  forced alignment of its scores against its own graph DIR/KEY.fst, in any format the decoding graph may have
//                  (ForceAlign: wfst_decoder_force_align; Kaldi's align-compiled-mapped), as "KEY forced found=0|1 cost=.. ali=t0 t1
//                  ..." -- cost the path's cost (float32, 9 digits), one class per frame: transition-ids, or pdfs (--tid2pdf=FILE)
//                  or phones (--tid2phone=FILE) -- and "KEY forced-words w@frame ...", every word with the frame it begins at.
//                  The other output is what it is without the flag.
//   --graph-post=DIR [--graph-post-class=tid|pdf|phone] [--graph-post-scales=GS,AS] [--graph-post-out=FILE]  batch shape and
//                  --single-stream: after the utterance's other lines the forward-backward pass of its scores over its own graph
//                  DIR/KEY.fst (GraphPosteriors: wfst_decoder_graph_posteriors), as "KEY graph-post found=0|1 loglike=.. frames=..
//                  entries=.." -- loglike the log of the sum over the graph's paths (9 digits) at arc costs GS * graph + AS *
//                  acoustic (default 1,1); with --graph-post-out the per-frame class posteriors go to FILE in --frame-post's format.
//                  The other output is what it is without the flag.
//   --rescale=GS,AS,WIP[:GS,AS,WIP...]  batch shape and --single-stream: after the utterance's other lines, per setting (at most 64:
//                  graph scale, acoustic scale, word insertion penalty) the best path of the RAW lattice picked again under it,
//                  without decoding again (RescaledWords: wfst_decoder_rescaled_words; Kaldi's lattice-best-path-score), as
//                  "KEY rescale q gs=.. as=.. wip=.. found=0|1 cost=.. tot=.. lm=.. : word(begin,end) ..." -- cost the path's cost
//                  at the setting (float64, 17 digits), tot / lm its unscaled LatticeToVector scores.  The other output is what it
//                  is without the flag.
//   --bias=FILE [--bias-settings=GS,AS,WIP,BS[:GS,AS,WIP,BS...]]  batch shape and --single-stream: phrase boosting.  FILE holds lines
//                  "KEY bonus w1 w2 ..." (a bonus >= 0, 1..16 word ids); the phrases of KEY "*" go into every utterance's list, in
//                  front of its own.  After the utterance's other lines, per setting (at most 16: graph scale, acoustic scale, word
//                  penalty, boost scale; without the flag one setting 1,1,0,1) the best path of the RAW lattice picked again with
//                  boost scale x bonus taken off for every occurrence of a phrase (BiasedWords: wfst_decoder_biased_words), as
//                  "KEY bias q gs=.. as=.. wip=.. bs=.. found=0|1 cost=.. bonus=.. tot=.. lm=.. hits=phrase@word,... : word(begin,end) ..."
//                  -- cost and bonus float64 at 17 digits, phrase the phrase's index in the utterance's list, word the index of the
//                  occurrence's last word.  The other output is what it is without the flag.
//   --bias-sparse  with --bias=FILE: the lines come from BiasedWordsSparse (wfst_decoder_biased_words_sparse: the cells a path can
//                  reach, lists of up to 65 536 nodes) whatever the lists' sizes -- the same lines, byte for byte.  Without the flag
//                  that call is taken only where a list of FILE has more than 256 nodes, which BiasedWords refuses.
//   --nearest-words=FILE  batch shape and --single-stream: FILE has --align-words' format, its lines being references (transcripts
//                  that need not be in the lattice); after the utterance's lines, per reference the lattice path nearest it
//                  (NearestWords: wfst_decoder_nearest_words) as "KEY nearest q err=E cor=C sub=S ins=I del=D arcs=N tot=.. lm=.."
//                  and "KEY nearest q#j word begin end" per word of that path ("KEY nearest q notfound": no lattice); behind the
//                  last utterance one line "nearest %WER p [ errors / reference words, I ins, D del, S sub ]" over all of them --
//                  with correct transcripts the lattices' oracle error, in the form kaldi-bin/bin/nbest-compute-wer.cc:166-167
//                  prints the 1-best's
//   --device-chunks --chunk=N [--acoustic-scale=S] [--log-priors=FILE] [--score-dtype=f32|f16|bf16]  batch shape only: the matrices
//                  on disk are the acoustic model's RAW output; N frames at a time every utterance's rows are converted to the
//                  dtype on the host, put into a staging buffer the device reads, and handed over where they lie
//                  (GpuBatchDecoder::AdvanceDecodingChunk): the device makes (x - log_prior) * acoustic_scale of them -- the
//                  reference CLI's --acoustic-scale (default 0.1 there; 1 here) and DecodableMatrixScaledMapped
//                  (kaldi-nnet3bin/kaldi-hclg-my-decoder.cc:37-41,107), the prior layer of its own network (nnet/nnet-layer.cc:30).
//                  FILE: binary float32 array, one log prior per column
//   --inflight=K   batch shape only: K batches in flight, each on its own GpuBatchDecoder (own HIP
//                  stream) driven by its own host thread -- the reference service's model of one
//                  decoder object per thread (v2-asrbin/v2-asr-service.cc:95-105); the GPU overlaps
//                  independent batches.  Output order is unchanged.
//   --devices=a,b,...  batch shape only: the node's GPUs: the graph (and the LMs) are uploaded once per listed device, each
//                  device gets `inflight` GpuBatchDecoders of its own, each driven by its own host thread; batch b goes to device
//                  b mod n -- utterances share nothing but the read-only graph, so there is no exchange between devices, and the
//                  results are merged in input order on the host (the reference's model of N worker threads over one shared
//                  graph, v2-asrbin/v2-asr-service.cc:95-105, with one graph replica per device).  A device may be listed twice.
//   --threads=N    the reference SERVICE's shape (v2-asr/v2-asr-work-thread.h:66, v2-asrbin/v2-asr-service.cc:95-105): N worker threads, each
//                  with its own DecoderItf object, take the utterances in turn -- InitDecoding, AdvanceDecoding in chunks of
//                  --chunk frames (all at once without it), FinalizeDecoding, GetBestPath.  The objects are GpuLatticeDecoders
//                  over private 1-channel device decoders, or
//   --pool=C       over ONE GpuChannelPool of C channels (C >= N): the threads' requests are batched into one device call per
//                  kind (gpu-asr/v1-gpu-kaldi-worker-pool.h:20-204: the dynamic batcher's shape); --linger-us=U: how long the
//                  batcher waits for the other leased channels' requests (50)
//   --repeat=K     --threads only: the utterance list is decoded K times over (a steady-state measurement: the first utterances of a
//                  run pay the decoder's graph captures and buffer allocations); the output is the first pass's
//   --warm=W       with --repeat: the first W passes over the list run BEFORE the clock (bench.py's warm-up steps, for the service's
//                  shape): every thread waits until the last warm-up utterance is done, the clock starts there, and the frames
//                  reported ("LOG Timed passes: ...") are those of the K - W passes behind it
//   --ragged=P     the utterances are cut to pseudo-random lengths between P % and 100 % of their frames (a fixed function of their
//                  position in the list) before anything is decoded: utterance boundaries that do not fall together, as a service
//                  sees them
//   --share=C      the ONE-LINE drop-in at service scale: GpuLatticeDecoder::ShareDevice(C) once, then every thread constructs its decoder
//                  the reference's way -- (graph, config) -- and the objects lease channels of shared C-channel device decoders
//   --pull         the decodable is a plain DecodableInterface: every score goes through LogLikelihood(frame, index) (without it
//                  the rows are taken in one piece, MatrixDecodable)
//   --tid2phone=FILE --endpoint.silence-phones=a:b:c [--endpoint.ruleN.{must-contain-nonsilence,min-trailing-silence,
//                  max-relative-cost,min-utterance-length}=..] [--endpoint.frame-shift=S] [--print-endpoints]
//                  endpointing, with --chunk=N and --single-stream or --threads=N [--pool=C]: after every chunk EndpointDetected
//                  (Kaldi's online2/online-endpoint.cc); on an endpoint the segment is finalized and printed as
//                  "KEY[t_beg,t_end] word-ids..." (frames of the stream), and the decoder starts again on the stream's next rows, as
//                  the reference's service loop does (v1-asr/asr-source.h:280-287); the stream's end ends its last segment.
//                  --print-endpoints: "KEY@t endpoint ruleK" before each segment an endpoint ended.  tid2phone: binary int32 array,
//                  entry 0 unused (TransitionIdToPhone)
//   --nbest=N      also print the N-best word sequences of every utterance (the service's
//                  GetNbestTxt, kaldi-online-nnet3-my-decoder.cc:139-150) as "KEY-k w1 w2 ..." to
//                  stdout and "LOG KEY-k tot_score .. lm_score .." to stderr (lattice mode)
//   --lattice-text same lattices as text: "KEY", one line "src dst ilabel olabel graph_cost
//                  acoustic_cost" per arc, one line "state" per final state, then an empty line
//
//   CONFIG    text file of --beam=.. --max-active=.. lines (reference option names)
//   GRAPH     flat graph in the reference format (Fst::ReadFst)
//   LOGLIKES  binary: repeated { int32 key_len, key bytes, int32 frames, int32 cols,
//             float32[frames*cols] }, cols = pdfs (with --tid2pdf) or NumIndices()+1
//   tid2pdf   binary int32 array, entry 0 unused
//
// Output lines "key word-ids..." like the reference's words_writer (:126-129); the log at the end
// prints the reference's "real-time factor assuming 100 frames/sec" (:189-192).
#include <atomic>
#include <chrono>
#include <cmath>
#include <thread>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <mutex>

#include <map>
#include <sstream>

#include "wfst-host.h"

using namespace datemoon;

namespace {
struct Utt {
  std::string key;
  int frames, cols;
  std::vector<float> m;
};
// an aligned sequence as the lines take it: the alignment, under --word-confidence the confidences, under --word-alternatives the
// slots' alternatives, under --sentence-posterior the posterior of the whole word sequence
struct TimedSeq : WordAlternatives {
  bool sent_found = false;
  double sentpost = 0.0;
};
bool ReadUtt(std::ifstream &in, Utt *u) {
  int32_t kl;
  if (!in.read((char *)&kl, 4)) return false;
  u->key.resize(kl);
  in.read(&u->key[0], kl);
  in.read((char *)&u->frames, 4);
  in.read((char *)&u->cols, 4);
  u->m.resize((size_t)u->frames * u->cols);
  in.read((char *)u->m.data(), u->m.size() * 4);
  return (bool)in;
}
// float32 -> IEEE binary16 / bfloat16 bits, round to nearest even (--score-dtype: what a half-precision model would have written)
uint16_t ToBf16(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);   // NaN stays NaN
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
uint16_t ToF16(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  const uint32_t sign = (u >> 16) & 0x8000u, a = u & 0x7fffffffu;
  if (a > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);
  if (a >= 0x47800000u) return (uint16_t)(sign | 0x7c00u);   // >= 65536 (65520 .. 65536 is rounded below): infinity
  if (a < 0x33000000u) return (uint16_t)sign;                 // < 2^-25: zero
  uint32_t mant = (a & 0x7fffffu) | 0x800000u;
  const int e = (int)(a >> 23) - 127;                         // value = mant * 2^(e - 23)
  const int shift = e >= -14 ? 13 : 13 + (-14 - e);           // normal: 10 mantissa bits; denormal: fewer
  const uint32_t q = mant >> shift, rem = mant & ((1u << shift) - 1u), half = 1u << (shift - 1);
  uint32_t h = e >= -14 ? (uint32_t)((e + 15) << 10) + (q - 0x400u) : q;
  if (rem > half || (rem == half && (h & 1u))) ++h;           // (a carry runs into the exponent, up to infinity, as it should)
  return (uint16_t)(sign | h);
}
// DecodableInterface over a host matrix: the shape every reference caller has.
class HostMatrixDecodable : public MatrixDecodable {
 public:
  // begin: the stream's rows from this frame on (a segment after an endpoint); frame numbers are relative to it
  explicit HostMatrixDecodable(const Utt &u, int begin = 0) : _u(u), _begin(begin), _ready(u.frames - begin) {}
  float LogLikelihood(int f, int i) override { return _u.m[(size_t)(_begin + f) * _u.cols + i]; }
  bool IsLastFrame(int f) const override { return _begin + f == _u.frames - 1; }
  int NumFramesReady() const override { return _ready; }
  void SetFramesReady(int n) { _ready = std::min(n, _u.frames) - _begin; }  // streaming: frames of the stream that have "arrived"
  int NumIndices() const override { return _u.cols - 1; }
  const float *HostRows() const override { return _u.m.data() + (size_t)_begin * _u.cols; }
  int Stride() const override { return _u.cols; }

 private:
  const Utt &_u;
  int _begin, _ready;
};
// ... and as the reference's callers see a decodable: LogLikelihood(frame, index) only, the index a 1-based TRANSITION-ID.  With
// --tid2pdf it is Kaldi's DecodableMatrixScaledMapped as the reference CLI builds it (kaldi-nnet3bin/kaldi-hclg-my-decoder.cc:107):
// LogLikelihood(frame, tid) = M(frame, TransitionIdToPdf(tid)), NumIndices() = the number of transition-ids -- the map belongs to
// the decodable; the graph carries the same map (Fst::SetTid2Pdf), so the decoder pulls one score per PDF through a representative
// transition-id.  Without --tid2pdf: M's columns are the indices themselves.
class PullDecodable : public DecodableInterface {
 public:
  PullDecodable(const Utt &u, const std::vector<int32_t> *tid2pdf, int begin = 0) : _u(u), _map(tid2pdf), _begin(begin), _ready(u.frames - begin) {}
  float LogLikelihood(int f, int i) override { return _u.m[(size_t)(_begin + f) * _u.cols + (_map ? (*_map)[(size_t)i] : i)]; }
  bool IsLastFrame(int f) const override { return _begin + f == _u.frames - 1; }
  int NumFramesReady() const override { return _ready; }
  void SetFramesReady(int n) { _ready = std::min(n, _u.frames) - _begin; }
  int NumIndices() const override { return _map ? (int)_map->size() - 1 : _u.cols - 1; }

 private:
  const Utt &_u;
  const std::vector<int32_t> *_map;   // entry 0 unused
  int _begin, _ready;
};
}  // namespace

int main(int argc, char **argv) {
  try {
    std::string tid2pdf_file, lm_old_file, lm_new_file, second_old_file, second_new_file, nbest_lattice_file;
    int batch = 128;
    bool single = false, determinize = false;
    std::string lattice_file, lattice_text;
    long long lattice_links = 1ll << 22;
    int nbest = 0, partial_nbest = 0, inflight = 1, chunk = 0, n_threads = 0, pool_channels = 0, linger_us = 50;
    bool pull = false, partial_words = false, word_times = false, live_prune = false, nbest_times = false;
    std::string align_file, nearest_file, phrase_file;
    std::string frame_post_file, fp_class = "tid";
    double fp_gs = 1.0, fp_as = 1.0, fp_min = 0.0;
    bool fp_opts = false, fp_bad = false;
    std::string seq_stats_file, seq_ref_file, seq_class = "tid", seq_criterion = "smbr";   // --seq-stats
    SequenceStatsOptions seq_opt;
    bool seq_opts = false, seq_bad = false;
    std::string force_dir, force_class = "tid";   // --force-align
    std::string gpost_dir, gpost_class = "tid", gpost_file;   // --graph-post
    double gpost_gs = 1.0, gpost_as = 1.0;
    bool gpost_opts = false, gpost_bad = false;
    bool force_opts = false;
    std::vector<RescaleSetting> rescale_set;   // --rescale
    bool rescale_bad = false;
    std::string bias_file;                     // --bias
    std::vector<BiasSetting> bias_set;         // --bias-settings
    bool bias_given = false, bias_set_given = false, bias_bad = false, bias_sparse = false;
    bool word_conf = false, sent_post = false;
    int word_alts = 0;   // --word-alternatives[=K]: K, 0 = off
    double conf_gs = 1.0, conf_as = 1.0;
    std::vector<int> wt_silence;
    long long max_tokens_per_frame = 0, arena_tokens = 0;
    int max_frames = 0, repeat = 1, share_channels = 0, warm = 0, ragged = 0;
    std::vector<int> devices(1, 0);
    std::vector<std::string> pos;
    std::string tid2phone_file;
    bool device_chunks = false, scale_given = false;
    float acoustic_scale = 1.0f;
    std::string log_priors_file;
    int score_dtype = WFST_DTYPE_F32;
    OnlineEndpointConfig ep_opt;
    bool endpointing = false, print_endpoints = false;
    for (int i = 1; i < argc; ++i) {
      std::string a = argv[i];
      if (ep_opt.ParseOption(a)) endpointing = true;
      else if (a.compare(0, 12, "--tid2phone=") == 0) tid2phone_file = a.substr(12);
      else if (a == "--print-endpoints") print_endpoints = true;
      else if (a.compare(0, 10, "--tid2pdf=") == 0) tid2pdf_file = a.substr(10);
      else if (a.compare(0, 8, "--batch=") == 0) batch = atoi(a.c_str() + 8);
      else if (a == "--single-stream") single = true;
      else if (a == "--determinize") determinize = true;
      else if (a.compare(0, 14, "--lattice-out=") == 0) lattice_file = a.substr(14);
      else if (a.compare(0, 15, "--lattice-text=") == 0) lattice_text = a.substr(15);
      else if (a.compare(0, 16, "--lattice-links=") == 0) lattice_links = atoll(a.c_str() + 16);
      else if (a.compare(0, 8, "--nbest=") == 0) nbest = atoi(a.c_str() + 8);
      else if (a.compare(0, 11, "--inflight=") == 0) inflight = std::max(1, atoi(a.c_str() + 11));
      else if (a.compare(0, 8, "--chunk=") == 0) chunk = std::max(0, atoi(a.c_str() + 8));
      else if (a.compare(0, 10, "--threads=") == 0) n_threads = std::max(0, atoi(a.c_str() + 10));
      else if (a.compare(0, 7, "--pool=") == 0) pool_channels = std::max(0, atoi(a.c_str() + 7));
      else if (a.compare(0, 12, "--linger-us=") == 0) linger_us = std::max(0, atoi(a.c_str() + 12));
      else if (a == "--pull") pull = true;
      else if (a == "--device-chunks") device_chunks = true;
      else if (a.compare(0, 17, "--acoustic-scale=") == 0) { acoustic_scale = (float)atof(a.c_str() + 17); scale_given = true; }
      else if (a.compare(0, 13, "--log-priors=") == 0) log_priors_file = a.substr(13);
      else if (a.compare(0, 14, "--score-dtype=") == 0) {
        const std::string v = a.substr(14);
        if (v == "f32") score_dtype = WFST_DTYPE_F32;
        else if (v == "f16") score_dtype = WFST_DTYPE_F16;
        else if (v == "bf16") score_dtype = WFST_DTYPE_BF16;
        else { std::cerr << "--score-dtype is f32, f16 or bf16\n"; return 1; }
      }
      else if (a == "--partial-words") partial_words = true;
      else if (a.compare(0, 16, "--partial-nbest=") == 0) partial_nbest = atoi(a.c_str() + 16);
      else if (a == "--live-lattice-prune") live_prune = true;
      else if (a == "--word-times") word_times = true;
      else if (a == "--nbest-word-times") nbest_times = true;
      else if (a.compare(0, 14, "--align-words=") == 0) align_file = a.substr(14);
      else if (a == "--word-confidence") word_conf = true;
      else if (a.compare(0, 18, "--word-confidence=") == 0) {
        char *end = nullptr;
        conf_gs = strtod(a.c_str() + 18, &end);
        if (end == a.c_str() + 18 || *end != ',') { std::cerr << "--word-confidence=GRAPH_SCALE,ACOUSTIC_SCALE\n"; return 1; }
        const char *second_at = end + 1;
        conf_as = strtod(second_at, &end);
        if (end == second_at || *end != 0) { std::cerr << "--word-confidence=GRAPH_SCALE,ACOUSTIC_SCALE\n"; return 1; }
        word_conf = true;
      }
      else if (a.compare(0, 16, "--nearest-words=") == 0) nearest_file = a.substr(16);
      else if (a == "--sentence-posterior") sent_post = true;
      else if (a == "--word-alternatives") word_alts = 5;
      else if (a.compare(0, 20, "--word-alternatives=") == 0) {
        char *end = nullptr;
        const long k = strtol(a.c_str() + 20, &end, 10);
        if (end == a.c_str() + 20 || *end != 0 || k < 1 || k > 16) { std::cerr << "--word-alternatives=K, 1 <= K <= 16\n"; return 1; }
        word_alts = (int)k;
      }
      else if (a.compare(0, 19, "--phrase-posterior=") == 0) phrase_file = a.substr(19);
      else if (a.compare(0, 13, "--frame-post=") == 0) frame_post_file = a.substr(13);
      else if (a.compare(0, 19, "--frame-post-class=") == 0) { fp_class = a.substr(19); fp_opts = true; }
      else if (a.compare(0, 20, "--frame-post-scales=") == 0) {
        char tail = 0;
        fp_opts = true;
        if (sscanf(a.c_str() + 20, "%lf,%lf%c", &fp_gs, &fp_as, &tail) != 2 || !(fp_gs >= 0.0) || !(fp_as >= 0.0) || std::isinf(fp_gs) || std::isinf(fp_as)) fp_bad = true;
      } else if (a.compare(0, 17, "--frame-post-min=") == 0) {
        char tail = 0;
        fp_opts = true;
        if (sscanf(a.c_str() + 17, "%lf%c", &fp_min, &tail) != 1 || !(fp_min >= 0.0 && fp_min <= 1.0)) fp_bad = true;
      }
      else if (a.compare(0, 14, "--force-align=") == 0) force_dir = a.substr(14);
      else if (a.compare(0, 20, "--force-align-class=") == 0) { force_class = a.substr(20); force_opts = true; }
      else if (a.compare(0, 13, "--graph-post=") == 0) gpost_dir = a.substr(13);
      else if (a.compare(0, 19, "--graph-post-class=") == 0) { gpost_class = a.substr(19); gpost_opts = true; }
      else if (a.compare(0, 17, "--graph-post-out=") == 0) { gpost_file = a.substr(17); gpost_opts = true; }
      else if (a.compare(0, 20, "--graph-post-scales=") == 0) {
        char tail = 0;
        gpost_opts = true;
        if (sscanf(a.c_str() + 20, "%lf,%lf%c", &gpost_gs, &gpost_as, &tail) != 2 || !(gpost_gs >= 0.0) || !(gpost_as >= 0.0) || std::isinf(gpost_gs) || std::isinf(gpost_as)) gpost_bad = true;
      }
      else if (a.compare(0, 12, "--seq-stats=") == 0) seq_stats_file = a.substr(12);
      else if (a.compare(0, 10, "--seq-ref=") == 0) { seq_ref_file = a.substr(10); seq_opts = true; }
      else if (a.compare(0, 16, "--seq-criterion=") == 0) { seq_criterion = a.substr(16); seq_opts = true; }
      else if (a.compare(0, 12, "--seq-class=") == 0) { seq_class = a.substr(12); seq_opts = true; }
      else if (a == "--seq-drop-frames") { seq_opt.drop_frames = true; seq_opts = true; }
      else if (a.compare(0, 13, "--seq-scales=") == 0) {
        char tail = 0;
        seq_opts = true;
        if (sscanf(a.c_str() + 13, "%lf,%lf%c", &seq_opt.graph_scale, &seq_opt.acoustic_scale, &tail) != 2 || !(seq_opt.graph_scale >= 0.0) ||
            !(seq_opt.acoustic_scale >= 0.0) || std::isinf(seq_opt.graph_scale) || std::isinf(seq_opt.acoustic_scale))
          seq_bad = true;
      } else if (a.compare(0, 14, "--seq-silence=") == 0) {
        // a:b:c, every class whole and >= 0, strictly ascending, at most 64
        seq_opts = true;
        if (a.size() == 14) seq_bad = true;
        for (size_t p0 = 14; p0 < a.size() && !seq_bad;) {
          const size_t p1 = std::min(a.find(':', p0), a.size());
          char *end = nullptr;
          const std::string tok = a.substr(p0, p1 - p0);
          const long v = strtol(tok.c_str(), &end, 10);
          if (tok.empty() || *end != 0 || v < 0 || v > 0x7FFFFFFF || p1 + 1 == a.size() ||
              (!seq_opt.sil_classes.empty() && v <= seq_opt.sil_classes.back()) || seq_opt.sil_classes.size() >= 64)
            seq_bad = true;
          seq_opt.sil_classes.push_back((int)v);
          p0 = p1 + 1;
        }
      }
      else if (a.compare(0, 10, "--rescale=") == 0) {
        // GS,AS,WIP[:GS,AS,WIP...]: every number whole, the scales finite and >= 0, the penalty finite
        if (a.size() == 10) rescale_bad = true;
        for (size_t p0 = 10; p0 < a.size() && !rescale_bad;) {
          const size_t p1 = std::min(a.find(':', p0), a.size());
          RescaleSetting r;
          char tail = 0;
          if (sscanf(a.substr(p0, p1 - p0).c_str(), "%lf,%lf,%lf%c", &r.graph_scale, &r.acoustic_scale, &r.word_penalty, &tail) != 3 ||
              !(r.graph_scale >= 0.0) || !(r.acoustic_scale >= 0.0) || std::isinf(r.graph_scale) || std::isinf(r.acoustic_scale) ||
              !std::isfinite(r.word_penalty) || p1 + 1 == a.size())
            rescale_bad = true;
          rescale_set.push_back(r);
          p0 = p1 + 1;
        }
      }
      else if (a.compare(0, 7, "--bias=") == 0) { bias_file = a.substr(7); bias_given = true; }
      else if (a == "--bias-sparse") bias_sparse = true;
      else if (a.compare(0, 16, "--bias-settings=") == 0) {
        // GS,AS,WIP,BS[:GS,AS,WIP,BS...]: every number whole, the scales finite and >= 0, the penalty finite
        bias_set_given = true;
        if (a.size() == 16) bias_bad = true;
        for (size_t p0 = 16; p0 < a.size() && !bias_bad;) {
          const size_t p1 = std::min(a.find(':', p0), a.size());
          BiasSetting r;
          char tail = 0;
          if (sscanf(a.substr(p0, p1 - p0).c_str(), "%lf,%lf,%lf,%lf%c", &r.graph_scale, &r.acoustic_scale, &r.word_penalty, &r.boost_scale, &tail) != 4 ||
              !(r.graph_scale >= 0.0) || !(r.acoustic_scale >= 0.0) || !(r.boost_scale >= 0.0) || std::isinf(r.graph_scale) ||
              std::isinf(r.acoustic_scale) || std::isinf(r.boost_scale) || !std::isfinite(r.word_penalty) || p1 + 1 == a.size())
            bias_bad = true;
          bias_set.push_back(r);
          p0 = p1 + 1;
        }
      }
      else if (a.compare(0, 17, "--silence-phones=") == 0) {
        for (size_t p0 = 17; p0 <= a.size();) {
          const size_t p1 = std::min(a.find(':', p0), a.size());
          if (p1 > p0) wt_silence.push_back(atoi(a.substr(p0, p1 - p0).c_str()));
          p0 = p1 + 1;
        }
      }
      else if (a.compare(0, 9, "--repeat=") == 0) repeat = std::max(1, atoi(a.c_str() + 9));
      else if (a.compare(0, 7, "--warm=") == 0) warm = std::max(0, atoi(a.c_str() + 7));
      else if (a.compare(0, 9, "--ragged=") == 0) ragged = std::min(100, std::max(1, atoi(a.c_str() + 9)));
      else if (a.compare(0, 8, "--share=") == 0) share_channels = std::max(0, atoi(a.c_str() + 8));
      else if (a.compare(0, 13, "--max-tokens=") == 0) max_tokens_per_frame = atoll(a.c_str() + 13);
      else if (a.compare(0, 15, "--arena-tokens=") == 0) arena_tokens = atoll(a.c_str() + 15);
      else if (a.compare(0, 13, "--max-frames=") == 0) max_frames = atoi(a.c_str() + 13);
      else if (a.compare(0, 10, "--devices=") == 0) {
        devices.clear();
        for (size_t p0 = 10; p0 <= a.size();) {
          const size_t p1 = std::min(a.find(',', p0), a.size());
          if (p1 > p0) devices.push_back(atoi(a.substr(p0, p1 - p0).c_str()));
          p0 = p1 + 1;
        }
        if (devices.empty()) { std::cerr << "--devices needs a list of device ordinals\n"; return 1; }
      }
      else if (a.compare(0, 9, "--lm-old=") == 0) lm_old_file = a.substr(9);
      else if (a.compare(0, 9, "--lm-new=") == 0) lm_new_file = a.substr(9);
      else if (a.compare(0, 16, "--second-lm-old=") == 0) second_old_file = a.substr(16);
      else if (a.compare(0, 16, "--second-lm-new=") == 0) second_new_file = a.substr(16);
      else if (a.compare(0, 20, "--nbest-lattice-out=") == 0) nbest_lattice_file = a.substr(20);
      else pos.push_back(a);
    }
    if (pos.size() < 3) {
      std::cerr << "usage: wfst-decode [--tid2pdf=FILE] [--batch=N] [--single-stream [--chunk=N [--partial-words] [--partial-nbest=K [--live-lattice-prune]]]] [--word-times [--silence-phones=a:b:c]] [--nbest-word-times] [--align-words=FILE] [--word-confidence[=GS,AS]] [--sentence-posterior] [--phrase-posterior=FILE] [--word-alternatives[=K]] [--nearest-words=FILE] [--frame-post=FILE [--frame-post-class=tid|pdf|phone] [--frame-post-scales=GS,AS] [--frame-post-min=X]] [--rescale=GS,AS,WIP[:GS,AS,WIP...]] [--bias=FILE [--bias-settings=GS,AS,WIP,BS[:GS,AS,WIP,BS...]]] [--bias-sparse] [--force-align=DIR [--force-align-class=tid|pdf|phone]] [--graph-post=DIR [--graph-post-class=tid|pdf|phone] [--graph-post-scales=GS,AS] [--graph-post-out=FILE]] [--seq-stats=FILE --seq-ref=FILE [--seq-criterion=smbr|mmi] [--seq-class=tid|pdf|phone] [--seq-scales=GS,AS] [--seq-silence=a:b:c] [--seq-drop-frames]] [--inflight=K] [--devices=a,b,...] [--nbest=N] [--lattice-out=FILE] [--determinize] "
                   "[--lattice-text=FILE] [--lattice-links=N] [--lm-old=FILE --lm-new=FILE] [--second-lm-old=FILE --second-lm-new=FILE] [--nbest-lattice-out=FILE] "
                   "[--tid2phone=FILE --endpoint.silence-phones=a:b:c [--endpoint.*=..] [--print-endpoints]] "
                   "[--device-chunks --chunk=N [--acoustic-scale=S] [--log-priors=FILE] [--score-dtype=f32|f16|bf16]] CONFIG GRAPH LOGLIKES [WORDS_OUT]\n";
      return 1;
    }
    if ((scale_given || !log_priors_file.empty() || score_dtype != WFST_DTYPE_F32) && !device_chunks) {
      std::cerr << "--acoustic-scale / --log-priors / --score-dtype go with --device-chunks (without it the matrices are finished scores)\n";
      return 1;
    }
    if (device_chunks && (chunk <= 0 || single || n_threads > 0)) { std::cerr << "--device-chunks goes with --chunk=N and the batch shape\n"; return 1; }
    if (word_times && n_threads > 0) { std::cerr << "--word-times goes with the batch shape or --single-stream\n"; return 1; }
    if (!wt_silence.empty() && (!word_times || tid2phone_file.empty())) { std::cerr << "--silence-phones goes with --word-times and --tid2phone=FILE\n"; return 1; }
    if (nbest_times && ((nbest == 0 && partial_nbest == 0) || n_threads > 0)) { std::cerr << "--nbest-word-times goes with --nbest=N or --partial-nbest=K, in the batch shape or --single-stream\n"; return 1; }
    if (!align_file.empty() && n_threads > 0) { std::cerr << "--align-words goes with the batch shape or --single-stream\n"; return 1; }
    if (word_conf && !nbest_times && align_file.empty()) { std::cerr << "--word-confidence goes with --nbest-word-times or --align-words=FILE\n"; return 1; }
    if (!nearest_file.empty() && n_threads > 0) { std::cerr << "--nearest-words goes with the batch shape or --single-stream\n"; return 1; }
    if (sent_post && !nbest_times && align_file.empty()) { std::cerr << "--sentence-posterior goes with --nbest-word-times or --align-words=FILE\n"; return 1; }
    if (!phrase_file.empty() && n_threads > 0) { std::cerr << "--phrase-posterior goes with the batch shape or --single-stream\n"; return 1; }
    if (word_alts && !nbest_times && align_file.empty()) { std::cerr << "--word-alternatives goes with --nbest-word-times or --align-words=FILE\n"; return 1; }
    const bool frame_post = !frame_post_file.empty();
    if (frame_post_file.empty() && (fp_opts || fp_bad)) { std::cerr << "--frame-post-class / --frame-post-scales / --frame-post-min go with --frame-post=FILE\n"; return 1; }
    if (frame_post && n_threads > 0) { std::cerr << "--frame-post goes with the batch shape or --single-stream\n"; return 1; }
    if (fp_bad) { std::cerr << "--frame-post-scales=GS,AS: two finite numbers >= 0; --frame-post-min=X: 0 <= X <= 1\n"; return 1; }
    if (frame_post && fp_class != "tid" && fp_class != "pdf" && fp_class != "phone") { std::cerr << "--frame-post-class=tid|pdf|phone\n"; return 1; }
    if (frame_post && fp_class == "pdf" && tid2pdf_file.empty()) { std::cerr << "--frame-post-class=pdf needs --tid2pdf=FILE\n"; return 1; }
    if (frame_post && fp_class == "phone" && tid2phone_file.empty()) { std::cerr << "--frame-post-class=phone needs --tid2phone=FILE\n"; return 1; }
    const bool seq_stats = !seq_stats_file.empty();
    if (!seq_stats && (seq_opts || seq_bad)) { std::cerr << "--seq-ref / --seq-criterion / --seq-class / --seq-scales / --seq-silence / --seq-drop-frames go with --seq-stats=FILE\n"; return 1; }
    if (seq_stats && seq_ref_file.empty()) { std::cerr << "--seq-stats=FILE needs --seq-ref=FILE\n"; return 1; }
    if (seq_stats && n_threads > 0) { std::cerr << "--seq-stats goes with the batch shape or --single-stream\n"; return 1; }
    if (seq_bad) { std::cerr << "--seq-scales=GS,AS: two finite numbers >= 0; --seq-silence=a:b:c: at most 64 classes >= 0, ascending\n"; return 1; }
    if (seq_stats && seq_criterion != "smbr" && seq_criterion != "mmi") { std::cerr << "--seq-criterion=smbr|mmi\n"; return 1; }
    if (seq_stats && seq_class != "tid" && seq_class != "pdf" && seq_class != "phone") { std::cerr << "--seq-class=tid|pdf|phone\n"; return 1; }
    if (seq_stats && seq_class == "pdf" && tid2pdf_file.empty()) { std::cerr << "--seq-class=pdf needs --tid2pdf=FILE\n"; return 1; }
    if (seq_stats && seq_class == "phone" && tid2phone_file.empty()) { std::cerr << "--seq-class=phone needs --tid2phone=FILE\n"; return 1; }
    seq_opt.mmi = seq_criterion == "mmi";
    if (rescale_bad) { std::cerr << "--rescale=GS,AS,WIP[:GS,AS,WIP...]: per setting two finite scales >= 0 and a finite word penalty\n"; return 1; }
    if (rescale_set.size() > 64) { std::cerr << "--rescale: more than 64 settings\n"; return 1; }
    const bool rescale = !rescale_set.empty();
    if (rescale && n_threads > 0) { std::cerr << "--rescale goes with the batch shape or --single-stream\n"; return 1; }
    if (bias_set_given && !bias_given) { std::cerr << "--bias-settings goes with --bias=FILE\n"; return 1; }
    if (bias_sparse && !bias_given) { std::cerr << "--bias-sparse goes with --bias=FILE\n"; return 1; }
    if (bias_given && bias_file.empty()) { std::cerr << "--bias=FILE: the file of the phrases, lines KEY bonus w1 w2 ...\n"; return 1; }
    if (bias_bad) { std::cerr << "--bias-settings=GS,AS,WIP,BS[:GS,AS,WIP,BS...]: per setting two finite scales >= 0, a finite word penalty and a finite boost scale >= 0\n"; return 1; }
    if (bias_set.size() > 16) { std::cerr << "--bias-settings: more than 16 settings\n"; return 1; }
    const bool bias = bias_given;
    if (bias && n_threads > 0) { std::cerr << "--bias goes with the batch shape or --single-stream\n"; return 1; }
    if (bias && bias_set.empty()) bias_set.push_back(BiasSetting());
    const bool force_align = !force_dir.empty();
    if (!force_align && force_opts) { std::cerr << "--force-align-class goes with --force-align=DIR\n"; return 1; }
    if (force_align && n_threads > 0) { std::cerr << "--force-align goes with the batch shape or --single-stream\n"; return 1; }
    if (force_align && force_class != "tid" && force_class != "pdf" && force_class != "phone") { std::cerr << "--force-align-class=tid|pdf|phone\n"; return 1; }
    if (force_align && force_class == "pdf" && tid2pdf_file.empty()) { std::cerr << "--force-align-class=pdf needs --tid2pdf=FILE\n"; return 1; }
    if (force_align && force_class == "phone" && tid2phone_file.empty()) { std::cerr << "--force-align-class=phone needs --tid2phone=FILE\n"; return 1; }
    const bool graph_post = !gpost_dir.empty();
    if (!graph_post && gpost_opts) { std::cerr << "--graph-post-class / --graph-post-scales / --graph-post-out go with --graph-post=DIR\n"; return 1; }
    if (graph_post && n_threads > 0) { std::cerr << "--graph-post goes with the batch shape or --single-stream\n"; return 1; }
    if (gpost_bad) { std::cerr << "--graph-post-scales=GS,AS: two finite numbers >= 0\n"; return 1; }
    if (graph_post && gpost_class != "tid" && gpost_class != "pdf" && gpost_class != "phone") { std::cerr << "--graph-post-class=tid|pdf|phone\n"; return 1; }
    if (graph_post && gpost_class == "pdf" && tid2pdf_file.empty()) { std::cerr << "--graph-post-class=pdf needs --tid2pdf=FILE\n"; return 1; }
    if (graph_post && gpost_class == "phone" && tid2phone_file.empty()) { std::cerr << "--graph-post-class=phone needs --tid2phone=FILE\n"; return 1; }
    const bool phones_for_frame_post = (frame_post && fp_class == "phone") || (seq_stats && seq_class == "phone") || (force_align && force_class == "phone") || (graph_post && gpost_class == "phone");   // (--tid2phone given for this alone is no endpointing)
    // --align-words / --nearest-words / --phrase-posterior: the sequences to align, the references and the phrases, by utterance key
    std::map<std::string, std::vector<std::vector<int> > > align_seqs, nearest_refs, phrases;
    for (int which = 0; which < 3; ++which) {
      const std::string &file = which == 2 ? phrase_file : which ? nearest_file : align_file;
      const std::string flag = which == 2 ? "--phrase-posterior" : which ? "--nearest-words" : "--align-words";
      std::map<std::string, std::vector<std::vector<int> > > &into = which == 2 ? phrases : which ? nearest_refs : align_seqs;
      if (file.empty()) continue;
      std::ifstream af(file.c_str());
      if (!af) { std::cerr << "cannot read " << file << "\n"; return 1; }
      std::string line;
      while (std::getline(af, line)) {
        std::istringstream ls(line);
        std::string key;
        if (!(ls >> key)) continue;
        std::vector<int> w;
        for (int x; ls >> x;) w.push_back(x);
        if (which == 2 && w.empty()) { std::cerr << flag << ": a phrase has at least one word (" << key << ")\n"; return 1; }
        into[key].push_back(w);
        if (into[key].size() > 64) { std::cerr << flag << ": more than 64 sequences for " << key << "\n"; return 1; }
      }
    }
    // --bias: the phrases by utterance key, "*": of every utterance (they come first in an utterance's list)
    std::map<std::string, std::vector<BiasPhrase> > bias_phrases;
    if (bias) {
      std::ifstream bf(bias_file.c_str());
      if (!bf) { std::cerr << "cannot read " << bias_file << "\n"; return 1; }
      std::string line;
      for (int ln = 1; std::getline(bf, line); ++ln) {
        std::istringstream ls(line);
        std::string key;
        if (!(ls >> key)) continue;
        BiasPhrase ph;
        bool ok = static_cast<bool>(ls >> ph.bonus) && std::isfinite(ph.bonus) && ph.bonus >= 0.0;
        for (int x; ok && ls >> x;) { ok = x > 0; ph.words.push_back(x); }
        if (!ok || !ls.eof() || ph.words.empty() || ph.words.size() > 16) {
          std::cerr << "--bias: line " << ln << " of " << bias_file << ": KEY bonus w1 w2 ... (a finite bonus >= 0, 1..16 word ids > 0)\n";
          return 1;
        }
        bias_phrases[key].push_back(ph);
      }
    }
    // a list of more than 256 nodes is a book: the whole run then goes through BiasedWordsSparse (the node count is host work)
    for (auto it = bias_phrases.begin(); it != bias_phrases.end() && !bias_sparse; ++it) {
      std::vector<BiasPhrase> list;
      if (it->first != "*" && bias_phrases.count("*")) list = bias_phrases["*"];
      list.insert(list.end(), it->second.begin(), it->second.end());
      std::vector<int32_t> len, words;
      std::vector<double> bonus;
      for (const BiasPhrase &ph : list) { len.push_back((int32_t)ph.words.size()); words.insert(words.end(), ph.words.begin(), ph.words.end()); bonus.push_back(ph.bonus); }
      int32_t nodes = 0;
      (void)wfst_bias_book_compile((int32_t)len.size(), len.data(), words.data(), bonus.data(), WFST_BIAS_BOOK_MAX_NODES, &nodes, nullptr, nullptr, nullptr, nullptr, nullptr);
      bias_sparse = nodes > WFST_BIAS_MAX_NODES;
    }
    auto bias_list_of = [&](const Utt &u) {
      std::vector<BiasPhrase> list;
      for (const char *key : {"*", u.key.c_str()}) {
        auto it = bias_phrases.find(key);
        if (it != bias_phrases.end() && (key[0] != '*' || key[1] != 0 || u.key != "*")) list.insert(list.end(), it->second.begin(), it->second.end());
      }
      return list;
    };
    if (live_prune && partial_nbest == 0) { std::cerr << "--live-lattice-prune goes with --chunk=N --partial-nbest=K\n"; return 1; }
    LatticeFasterDecoderConfig opt;
    opt.ReadConfigFile(pos[0]);
    if (endpointing || print_endpoints || (!tid2phone_file.empty() && wt_silence.empty() && !phones_for_frame_post)) {
      // endpointing (v1-asr/asr-source.h:280-287): --tid2phone and --endpoint.silence-phones, a streaming shape, a search without LMs
      if (tid2phone_file.empty() || ep_opt.silence_phones.empty()) { std::cerr << "endpointing needs --tid2phone=FILE and --endpoint.silence-phones\n"; return 1; }
      if (chunk <= 0 || !(single || n_threads > 0)) { std::cerr << "endpointing goes with --chunk=N and --single-stream or --threads=N\n"; return 1; }
      if (!lm_old_file.empty() || !lm_new_file.empty()) { std::cerr << "endpointing is not supported with --lm-old/--lm-new (biglm)\n"; return 1; }
      ep_opt.SilencePhones();   // (checked here, before any device work)
      endpointing = true;
    }
    if (partial_words && (!(single || n_threads > 0) || chunk <= 0 || endpointing || !lm_old_file.empty())) {
      std::cerr << "--partial-words goes with --chunk=N and --single-stream or --threads=N (no endpointing, no --lm-old/--lm-new)\n";
      return 1;
    }
    if (partial_nbest != 0 && (partial_nbest < 1 || partial_nbest > 64 || chunk <= 0 || endpointing || device_chunks || !lm_old_file.empty())) {
      std::cerr << "--partial-nbest=K (1..64) goes with --chunk=N (no endpointing, no --device-chunks, no --lm-old/--lm-new)\n";
      return 1;
    }
    if (single && devices.size() > 1) { std::cerr << "--devices lists several devices: batch shape only\n"; return 1; }
    // one graph replica per listed device (fsts[0] also serves --single-stream)
    std::vector<std::unique_ptr<Fst> > fsts;
    for (size_t di = 0; di < devices.size(); ++di) {
      fsts.emplace_back(new Fst());
      if (!fsts.back()->ReadFst(pos[1].c_str(), devices[di])) return 1;
    }
    Fst &fst = *fsts[0];
    std::vector<int32_t> tid2pdf;
    if (!tid2pdf_file.empty()) {
      std::ifstream t(tid2pdf_file.c_str(), std::ios::binary | std::ios::ate);
      if (!t) { std::cerr << "cannot open " << tid2pdf_file << "\n"; return 1; }
      tid2pdf.resize((size_t)t.tellg() / 4);
      t.seekg(0);
      t.read((char *)tid2pdf.data(), tid2pdf.size() * 4);
      // the graph's rows read the pdf columns (what DecodableMatrixScaledMapped does with the transition model); --pull: the
      // decodable ALSO maps, as the reference's does -- the decoder then asks it for one transition-id per pdf (Fst::SetTid2Pdf)
      for (auto &f : fsts) f->SetTid2Pdf(tid2pdf);
    }
    std::vector<int32_t> tid2phone;
    if (!tid2phone_file.empty()) {   // TransitionModel::TransitionIdToPhone as a table (binary int32, entry 0 unused)
      std::ifstream t(tid2phone_file.c_str(), std::ios::binary | std::ios::ate);
      if (!t) { std::cerr << "cannot open " << tid2phone_file << "\n"; return 1; }
      tid2phone.resize((size_t)t.tellg() / 4);
      t.seekg(0);
      t.read((char *)tid2phone.data(), tid2phone.size() * 4);
      for (auto &f : fsts) f->SetTid2Phone(tid2phone);
    }
    // --frame-post: the class of a transition-id, and the file
    std::vector<int> fp_map;
    if (frame_post && fp_class == "pdf") fp_map.assign(tid2pdf.begin(), tid2pdf.end());
    if (frame_post && fp_class == "phone") fp_map.assign(tid2phone.begin(), tid2phone.end());
    std::ofstream fp_out;
    if (frame_post) {
      fp_out.open(frame_post_file.c_str());
      if (!fp_out) { std::cerr << "cannot write " << frame_post_file << "\n"; return 1; }
    }
    // "KEY [ c p c p ] [ ... ]": an utterance's line of --frame-post (a channel without a lattice: the key alone)
    auto emit_frame_post = [&](const Utt &u, const FramePosteriors &fp) {
      std::string o = u.key;
      char buf[48];
      for (int f = 0; f < fp.n_frames; ++f) {
        o += " [";
        for (int e = fp.frame_off[(size_t)f]; e < fp.frame_off[(size_t)f + 1]; ++e) {
          snprintf(buf, sizeof(buf), " %d %.9g", fp.classes[(size_t)e], fp.posts[(size_t)e]);
          o += buf;
        }
        o += " ]";
      }
      fp_out << o << "\n";
    };
    // --seq-stats: the class of a transition-id, the references by utterance key, and the file
    if (seq_stats && seq_class == "pdf") seq_opt.label_map.assign(tid2pdf.begin(), tid2pdf.end());
    if (seq_stats && seq_class == "phone") seq_opt.label_map.assign(tid2phone.begin(), tid2phone.end());
    std::map<std::string, std::vector<int> > seq_refs;
    std::ofstream seq_out;
    if (seq_stats) {
      std::ifstream rf(seq_ref_file.c_str());
      if (!rf) { std::cerr << "cannot read " << seq_ref_file << "\n"; return 1; }
      std::string line;
      while (std::getline(rf, line)) {
        std::istringstream ls(line);
        std::string key;
        if (!(ls >> key)) continue;
        std::vector<int> &r = seq_refs[key];
        r.clear();
        for (int x; ls >> x;) r.push_back(x);
      }
      seq_out.open(seq_stats_file.c_str());
      if (!seq_out) { std::cerr << "cannot write " << seq_stats_file << "\n"; return 1; }
    }
    auto seq_ref_of = [&](const Utt &u) {
      auto it = seq_refs.find(u.key);
      return it == seq_refs.end() ? std::vector<int>() : it->second;
    };
    // "KEY [ c v c v ] [ ... ]" and "KEY seq-stats ...": an utterance's two lines of --seq-stats
    auto emit_seq_stats = [&](const Utt &u, const SequenceStats &ss) {
      std::string o = u.key;
      char buf[192];
      for (int f = 0; f < ss.n_frames; ++f) {
        o += " [";
        for (int e = ss.frame_off[(size_t)f]; e < ss.frame_off[(size_t)f + 1]; ++e) {
          snprintf(buf, sizeof(buf), " %d %.17g", ss.classes[(size_t)e], ss.values[(size_t)e]);
          o += buf;
        }
        o += " ]";
      }
      snprintf(buf, sizeof(buf), " seq-stats criterion=%s tot_acc=%.17g n_frames=%d n_ref_frames=%d n_dropped=%d log_z=%.17g", seq_criterion.c_str(),
               ss.tot_acc, ss.n_frames, ss.n_ref_frames, ss.n_dropped, ss.log_z);
      seq_out << o << "\n" << u.key << buf << "\n";
    };
    std::ifstream in(pos[2].c_str(), std::ios::binary);
    if (!in) { std::cerr << "cannot open " << pos[2] << "\n"; return 1; }
    std::ofstream fout;
    if (pos.size() > 3) fout.open(pos[3].c_str());
    std::ostream &out = pos.size() > 3 ? (std::ostream &)fout : std::cout;

    std::ofstream lat_out;
    if (!lattice_text.empty()) {
      lat_out.open(lattice_text.c_str());
      lat_out.precision(9);
    }
    if (!lattice_file.empty()) remove(lattice_file.c_str());  // Lattice::Write(file) appends
    if (!nbest_lattice_file.empty()) remove(nbest_lattice_file.c_str());
    const bool want_lattice = !lattice_file.empty() || !lattice_text.empty() || nbest > 0 || partial_nbest > 0 || !align_file.empty() || !nearest_file.empty() || !phrase_file.empty() || frame_post || rescale || bias || seq_stats;
    // "HEAD#j word begin end" per word of an aligned sequence, or "HEAD notfound"
    // (--word-confidence: a fourth column conf; --word-alternatives: " none=.. alts=word:post,...")
    auto time_lines = [&](const std::string &head, const std::vector<int> &words, const TimedSeq &a) {
      std::string o;
      if (!a.found) return head + " notfound\n";
      for (size_t j = 0; j < words.size(); ++j) {
        o += head + "#" + std::to_string(j + 1) + " " + std::to_string(words[j]) + " " + std::to_string(a.frames[j].first) + " " + std::to_string(a.frames[j].second);
        if (word_conf) {
          char buf[32];
          snprintf(buf, sizeof(buf), " %.9g", a.conf[j]);
          o += buf;
        }
        if (word_alts) {
          char buf[48];
          snprintf(buf, sizeof(buf), " none=%.9g alts=", a.none_post[j]);
          o += buf;
          if (a.alts[j].empty()) o += "-";
          for (size_t i = 0; i < a.alts[j].size(); ++i) {
            snprintf(buf, sizeof(buf), "%s%d:%.9g", i ? "," : "", a.alts[j][i].first, a.alts[j][i].second);
            o += buf;
          }
        }
        o += "\n";
      }
      return o;
    };
    // " logpost=.." of a path line under --word-confidence
    // (--sentence-posterior: and " sentpost=..", the log posterior of the path's word sequence over all paths that spell it)
    auto logpost_of = [&](const TimedSeq &a) {
      std::string o;
      char buf[40];
      if (word_conf && a.found) {
        snprintf(buf, sizeof(buf), " logpost=%.9g", a.path_logpost);
        o += buf;
      }
      if (sent_post && a.found && a.sent_found) {
        snprintf(buf, sizeof(buf), " sentpost=%.9g", a.sentpost);
        o += buf;
      }
      return o;
    };
    // AlignWords' / WordConfidences' answers as the lines take them, with the sentence posteriors where there are any
    auto lift = [](const auto &a, const std::vector<SequencePosterior> &sp) {
      std::vector<TimedSeq> o(a.size());
      for (size_t i = 0; i < a.size(); ++i) {
        static_cast<typename std::decay<decltype(a[i])>::type &>(o[i]) = a[i];
        if (i < sp.size()) { o[i].sent_found = sp[i].found; o[i].sentpost = sp[i].logpost; }
      }
      return o;
    };
    // the word times of one stream's sequences (GetNbestWordTimes), under --word-confidence with the confidences (WordConfidences),
    // under --word-alternatives with the slots' alternatives as well (WordAlternatives),
    // under --sentence-posterior with the sequences' posteriors (SequencePosteriors)
    auto stream_times = [&](GpuLatticeDecoder &decode, const std::vector<std::vector<int> > &seqs, std::vector<TimedSeq> *o, bool use_final_probs) {
      std::vector<SequencePosterior> sp;
      if (sent_post) decode.SequencePosteriors(seqs, &sp, false, use_final_probs, conf_gs, conf_as);
      if (word_alts) {   // (the confidences come with them)
        std::vector<WordAlternatives> a;
        decode.WordAlternatives(seqs, &a, word_alts, use_final_probs, conf_gs, conf_as);
        *o = lift(a, sp);
        return;
      }
      if (word_conf) {
        std::vector<WordConfidence> a;
        decode.WordConfidences(seqs, &a, use_final_probs, conf_gs, conf_as);
        *o = lift(a, sp);
        return;
      }
      std::vector<WordAlignment> a;
      decode.GetNbestWordTimes(seqs, &a, use_final_probs);
      *o = lift(a, sp);
    };
    // ... and of a batch's channels (AlignWords / WordConfidences / SequencePosteriors)
    auto batch_times = [&](GpuBatchDecoder &decode, const std::vector<int> &ch, const std::vector<std::vector<std::vector<int> > > &seqs, bool use_final_probs,
                           std::vector<std::vector<TimedSeq> > *o, std::vector<int> *status) {
      std::vector<std::vector<SequencePosterior> > sp;
      std::vector<int> sp_status;   // (a channel's own failure shows in the alignment's status; here its posteriors are left out)
      if (sent_post) decode.SequencePosteriors(ch, seqs, false, use_final_probs, conf_gs, conf_as, &sp, &sp_status);
      const std::vector<SequencePosterior> none;
      o->clear();
      if (word_alts) {
        std::vector<std::vector<WordAlternatives> > a;
        decode.WordAlternatives(ch, seqs, word_alts, use_final_probs, conf_gs, conf_as, &a, status);
        for (size_t i = 0; i < a.size(); ++i) o->push_back(lift(a[i], i < sp.size() ? sp[i] : none));
        return;
      }
      if (word_conf) {
        std::vector<std::vector<WordConfidence> > a;
        decode.WordConfidences(ch, seqs, use_final_probs, conf_gs, conf_as, &a, status);
        for (size_t i = 0; i < a.size(); ++i) o->push_back(lift(a[i], i < sp.size() ? sp[i] : none));
        return;
      }
      std::vector<std::vector<WordAlignment> > a;
      decode.AlignWords(ch, seqs, use_final_probs, &a, status);
      for (size_t i = 0; i < a.size(); ++i) o->push_back(lift(a[i], i < sp.size() ? sp[i] : none));
    };
    // the words of every path of an n-best list (none where LatticeToVector fails: emit_nbest skips such a path)
    auto path_words = [](std::vector<Lattice> &paths) {
      std::vector<std::vector<int> > w(paths.size());
      for (size_t k = 0; k < paths.size(); ++k) {
        std::vector<int> phones;
        float tot = 0, lm = 0;
        if (!LatticeToVector(paths[k], w[k], phones, tot, lm)) w[k].clear();
      }
      return w;
    };
    // --align-words: the lines of one utterance
    auto emit_align = [&](const Utt &u, const std::vector<TimedSeq> &al) {
      auto it = align_seqs.find(u.key);
      if (it == align_seqs.end()) return;
      for (size_t q = 0; q < it->second.size() && q < al.size(); ++q) {
        char buf[96];
        snprintf(buf, sizeof(buf), " found=%d arcs=%d tot=%.9g lm=%.9g", al[q].found ? 1 : 0, al[q].n_arcs, (double)al[q].tot, (double)al[q].lm);
        const std::string head = u.key + " align " + std::to_string(q + 1);
        out << head << buf << logpost_of(al[q]) << "\n";
        if (al[q].found) out << time_lines(head, it->second[q], al[q]);
      }
    };
    // --phrase-posterior: the lines of one utterance
    auto emit_phrases = [&](const Utt &u, const std::vector<SequencePosterior> &sp) {
      auto it = phrases.find(u.key);
      if (it == phrases.end()) return;
      for (size_t q = 0; q < it->second.size() && q < sp.size(); ++q) {
        char buf[128];
        snprintf(buf, sizeof(buf), " found=%d count=%.9g conf=%.9g peak=%d\n", sp[q].found ? 1 : 0, sp[q].count, sp[q].conf, sp[q].peak);
        out << u.key << " phrase " << (q + 1) << buf;
      }
    };
    // --nearest-words: the lines of one utterance, and the sums of the closing line
    long long nr_err = 0, nr_words = 0, nr_ins = 0, nr_del = 0, nr_sub = 0;
    auto emit_nearest = [&](const Utt &u, const std::vector<NearestPath> &np) {
      auto it = nearest_refs.find(u.key);
      if (it == nearest_refs.end()) return;
      for (size_t q = 0; q < it->second.size() && q < np.size(); ++q) {
        const NearestPath &a = np[q];
        const std::string head = u.key + " nearest " + std::to_string(q + 1);
        if (!a.found) { out << head << " notfound\n"; continue; }
        char buf[160];
        snprintf(buf, sizeof(buf), " err=%d cor=%d sub=%d ins=%d del=%d arcs=%d tot=%.9g lm=%.9g\n", a.errors, a.cor, a.sub, a.ins, a.del, a.n_arcs,
                 (double)a.tot, (double)a.lm);
        out << head << buf;
        for (size_t j = 0; j < a.words.size(); ++j)
          out << head << "#" << (j + 1) << " " << a.words[j] << " " << a.frames[j].first << " " << a.frames[j].second << "\n";
        nr_err += a.errors; nr_words += (long long)it->second[q].size(); nr_ins += a.ins; nr_del += a.del; nr_sub += a.sub;
      }
    };
    // --force-align: the class of a transition-id, an utterance's graph file and its two lines
    std::vector<int> force_map;
    if (force_align && force_class == "pdf") force_map.assign(tid2pdf.begin(), tid2pdf.end());
    if (force_align && force_class == "phone") force_map.assign(tid2phone.begin(), tid2phone.end());
    auto force_file = [&](const Utt &u) { return force_dir + "/" + u.key + ".fst"; };
    auto emit_forced = [&](const Utt &u, const ForcedAlignment &fa) {
      char buf[96];
      snprintf(buf, sizeof(buf), " forced found=%d cost=%.9g ali=", fa.found ? 1 : 0, (double)fa.path_cost);
      out << u.key << buf;
      for (size_t f = 0; f < fa.alignment.size(); ++f) out << (f ? " " : "") << fa.alignment[f];
      out << '\n' << u.key << " forced-words";
      for (size_t k = 0; k < fa.words.size(); ++k) out << ' ' << fa.words[k] << '@' << fa.word_frame[k];
      out << '\n';
    };
    // --graph-post: the class of a transition-id, an utterance's graph file, its line and, with --graph-post-out, its lists in
    // --frame-post's format
    GraphPosteriorsOptions gpost_opt;
    gpost_opt.graph_scale = gpost_gs;
    gpost_opt.acoustic_scale = gpost_as;
    if (graph_post && gpost_class == "pdf") gpost_opt.label_map.assign(tid2pdf.begin(), tid2pdf.end());
    if (graph_post && gpost_class == "phone") gpost_opt.label_map.assign(tid2phone.begin(), tid2phone.end());
    std::ofstream gpost_out;
    if (graph_post && !gpost_file.empty()) {
      gpost_out.open(gpost_file.c_str());
      if (!gpost_out) { std::cerr << "cannot write " << gpost_file << "\n"; return 1; }
    }
    auto gpost_graph = [&](const Utt &u) { return gpost_dir + "/" + u.key + ".fst"; };
    auto emit_graph_post = [&](const Utt &u, const GraphPosteriors &gp) {
      char buf[128];
      snprintf(buf, sizeof(buf), " graph-post found=%d loglike=%.9g frames=%d entries=%d\n", gp.found ? 1 : 0, gp.log_like, gp.n_frames, (int)gp.classes.size());
      out << u.key << buf;
      if (gpost_file.empty()) return;
      std::string o = u.key;
      for (int f = 0; f < gp.n_frames; ++f) {
        o += " [";
        for (int e = gp.frame_off[(size_t)f]; e < gp.frame_off[(size_t)f + 1]; ++e) {
          snprintf(buf, sizeof(buf), " %d %.9g", gp.classes[(size_t)e], gp.posts[(size_t)e]);
          o += buf;
        }
        o += " ]";
      }
      gpost_out << o << "\n";
    };
    // --rescale: an utterance's lines, one per setting
    auto emit_rescale = [&](const Utt &u, const std::vector<RescaledWords> &rw) {
      for (size_t q = 0; q < rescale_set.size() && q < rw.size(); ++q) {
        const RescaledWords &a = rw[q];
        char buf[256];
        snprintf(buf, sizeof(buf), " gs=%.9g as=%.9g wip=%.9g found=%d cost=%.17g tot=%.9g lm=%.9g :", rescale_set[q].graph_scale,
                 rescale_set[q].acoustic_scale, rescale_set[q].word_penalty, a.found ? 1 : 0, a.scaled_cost, (double)a.tot, (double)a.lm);
        out << u.key << " rescale " << (q + 1) << buf;
        for (size_t j = 0; j < a.words.size(); ++j) out << ' ' << a.words[j] << '(' << a.frames[j].first << ',' << a.frames[j].second << ')';
        out << '\n';
      }
    };
    // --bias: an utterance's lines, one per setting
    auto emit_bias = [&](const Utt &u, const std::vector<BiasedWords> &bw) {
      for (size_t q = 0; q < bias_set.size() && q < bw.size(); ++q) {
        const BiasedWords &a = bw[q];
        char buf[320];
        snprintf(buf, sizeof(buf), " gs=%.9g as=%.9g wip=%.9g bs=%.9g found=%d cost=%.17g bonus=%.17g tot=%.9g lm=%.9g hits=", bias_set[q].graph_scale,
                 bias_set[q].acoustic_scale, bias_set[q].word_penalty, bias_set[q].boost_scale, a.found ? 1 : 0, a.biased_cost, a.bonus, (double)a.tot,
                 (double)a.lm);
        out << u.key << " bias " << (q + 1) << buf;
        for (size_t k = 0; k < a.hits.size(); ++k) out << (k ? "," : "") << a.hits[k].first << '@' << a.hits[k].second;
        out << " :";
        for (size_t j = 0; j < a.words.size(); ++j) out << ' ' << a.words[j] << '(' << a.frames[j].first << ',' << a.frames[j].second << ')';
        out << '\n';
      }
    };
    auto emit_nbest = [&](const Utt &u, std::vector<Lattice> &paths, const std::vector<TimedSeq> *times = nullptr) {
      for (size_t k = 0; k < paths.size(); ++k) {
        std::vector<int> words, phones;
        float tot = 0, lm = 0;
        if (!nbest_lattice_file.empty() && !paths[k].Write(nbest_lattice_file)) throw std::runtime_error("cannot write " + nbest_lattice_file);
        if (!LatticeToVector(paths[k], words, phones, tot, lm)) continue;
        out << u.key << '-' << (k + 1);
        for (int w : words) out << ' ' << w;
        if (times && k < times->size()) out << logpost_of((*times)[k]);
        out << '\n';
        if (times && k < times->size()) out << time_lines(u.key + "-" + std::to_string(k + 1), words, (*times)[k]);
        std::cerr << "LOG " << u.key << '-' << (k + 1) << " tot_score " << tot << " lm_score " << lm << "\n";
      }
    };
    // biglm (kaldi-nnet3bin/kaldi-hclg-my-decoder-biglm.cc:55-60,80): both LM files, the old one rescaled by -1
    const bool biglm = !lm_old_file.empty() || !lm_new_file.empty();
    struct LmPair { ArpaLm a, b; };
    std::vector<std::unique_ptr<LmPair> > lms, slms;   // [device index]: the search's LMs, the second pass's
    auto load_pairs = [&](const std::string &f_old, const std::string &f_new, std::vector<std::unique_ptr<LmPair> > *v) -> bool {
      for (size_t di = 0; di < devices.size(); ++di) {
        v->emplace_back(new LmPair());
        if (!v->back()->a.Read(f_old.c_str(), devices[di]) || !v->back()->b.Read(f_new.c_str(), devices[di])) return false;
        v->back()->a.Rescale(-1.0);
        v->back()->a.Handle();   // both automata go to HBM here, once, before any worker thread asks for them
        v->back()->b.Handle();
      }
      return true;
    };
    if (biglm) {
      if (lm_old_file.empty() || lm_new_file.empty()) { std::cerr << "--lm-old and --lm-new go together\n"; return 1; }
      if (!load_pairs(lm_old_file, lm_new_file, &lms)) return 1;
    }
    ArpaLm *lm1p = biglm ? &lms[0]->a : nullptr, *lm2p = biglm ? &lms[0]->b : nullptr;
    // the service's second pass (--use-second, kaldi-nnet3/kaldi-online-nnet3-my-decoder.cc:53-78): GetLattice / GetNbest compose the
    // determinized lattice with the old LM (rescaled by -1) and with the new one
    const bool second = !second_old_file.empty() || !second_new_file.empty();
    if (second) {
      if (second_old_file.empty() || second_new_file.empty()) { std::cerr << "--second-lm-old and --second-lm-new go together\n"; return 1; }
      if (!load_pairs(second_old_file, second_new_file, &slms)) return 1;
    }
    ArpaLm *slm1p = second ? &slms[0]->a : nullptr, *slm2p = second ? &slms[0]->b : nullptr;
    // exact n-best (NShortestPath on the determinized lattice) where its lattices are asked for, a second pass runs or the list is long
    const bool exact_nbest = !nbest_lattice_file.empty() || second || nbest > 16;
    wfst_limits limits = {0, 0, 0, 0, 0};  // zeros = the library defaults
    limits.lattice_links = want_lattice ? lattice_links : 0;
    // --partial-nbest: "key@frames nbest k: w1 w2 ... tot=.. lm=.." per path, or "key@frames nbest status=code" for a channel's own failure
    auto nbest_lines = [&](const std::string &key, int frames, int status, const std::vector<std::vector<int> > &w, const std::vector<float> &t,
                           const std::vector<float> &l, const std::vector<TimedSeq> *times = nullptr) {
      std::string o;
      const std::string head = key + "@" + std::to_string(frames) + " nbest ";
      if (status != WFST_OK) o += head + "status=" + std::to_string(status) + "\n";
      for (size_t k = 0; k < w.size(); ++k) {
        o += head + std::to_string(k + 1) + ":";
        for (int x : w[k]) o += " " + std::to_string(x);
        char buf[64];
        snprintf(buf, sizeof(buf), " tot=%.9g lm=%.9g", (double)t[k], (double)l[k]);
        o += buf;
        if (times && k < times->size()) o += logpost_of((*times)[k]);
        o += "\n";
        if (times && k < times->size()) o += time_lines(head + std::to_string(k + 1), w[k], (*times)[k]);
      }
      return o;
    };
    // (--max-frames / --max-tokens / --arena-tokens: wfst_limits as the caller sizes them; 0 = the library's defaults)
    limits.max_frames = max_frames;
    limits.max_tokens_per_frame = (int32_t)max_tokens_per_frame;
    limits.arena_tokens = arena_tokens;
    auto emit_lattice = [&](const Utt &u, Lattice &lat, bool ok) {
      if (!ok) lat.DeleteStates();
      if (!lattice_file.empty() && !lat.Write(lattice_file)) throw std::runtime_error("cannot write " + lattice_file);
      if (!lat_out.is_open()) return;
      lat_out << u.key << '\n';
      if (ok)
        for (StateId s = 0; s < lat.NumStates(); ++s) {
          LatticeState *st = lat.GetState(s);
          for (size_t i = 0; i < st->GetArcSize(); ++i) {
            LatticeArc *a = st->GetArc(i);
            lat_out << s << ' ' << a->_to << ' ' << a->_input << ' ' << a->_output << ' ' << a->_w.Value1() << ' '
                    << a->_w.Value2() << '\n';
          }
          if (st->IsFinal()) lat_out << s << '\n';
        }
      lat_out << '\n';
    };

    std::vector<Utt> utts;
    for (Utt u; ReadUtt(in, &u);) utts.push_back(u);
    std::vector<float> log_priors;   // --log-priors
    if (!log_priors_file.empty()) {
      std::ifstream pf(log_priors_file, std::ios::binary);
      if (!pf) throw std::runtime_error("cannot open " + log_priors_file);
      for (float v; pf.read((char *)&v, 4);) log_priors.push_back(v);
      if (log_priors.empty()) throw std::runtime_error(log_priors_file + ": no log priors");
    }
    if (ragged > 0)
      for (size_t i = 0; i < utts.size(); ++i) {
        const unsigned h = (unsigned)(i * 2654435761u) >> 8;   // (Knuth's multiplicative hash of the position)
        const int keep = std::max(1, (int)((long long)utts[i].frames * (ragged + (int)(h % (unsigned)(101 - ragged))) / 100));
        utts[i].frames = keep;
        utts[i].m.resize((size_t)keep * utts[i].cols);
      }
    int num_success = 0, num_fail = 0;
    long long frame_count = 0, repeat_frames = 0, timed_frames = 0;
    double tot_like = 0;
    auto t0 = std::chrono::steady_clock::now();
    // --word-times: the words and frames of the utterance emit() is called for next (GetWords), or nullptr
    struct WordTimes { std::vector<int> words; std::vector<std::pair<int, int> > frames; };
    const WordTimes *emit_times = nullptr;
    auto emit = [&](const Utt &u, Lattice &best, bool ok) {
      std::vector<int> words, phones;
      float tot = 0, lm = 0;
      if (!ok || !LatticeToVector(best, words, phones, tot, lm)) {
        std::cerr << "WARNING Did not successfully decode utterance " << u.key << ", len = " << u.frames << "\n";
        ++num_fail;
        return;
      }
      out << u.key;
      for (int w : words) out << ' ' << w;
      out << '\n';
      if (emit_times) {
        if (emit_times->words != words) throw std::runtime_error("GetWords and GetBestPath disagree on the words of " + u.key);
        for (size_t k = 0; k < words.size(); ++k)
          out << u.key << '#' << (k + 1) << ' ' << words[k] << ' ' << emit_times->frames[k].first << ' ' << emit_times->frames[k].second << '\n';
      }
      std::cerr << "LOG " << u.key << " tot_score " << tot << " lm_score " << lm << " over " << u.frames << " frames.\n";
      tot_like += -tot;
      frame_count += u.frames;
      ++num_success;
    };
    // One stream decoded as the reference's service loop with endpointing does it (v1-asr/asr-source.h:280-287): the rows arrive
    // --chunk frames at a time; after every AdvanceDecoding, EndpointDetected -- on an endpoint FinalizeDecoding, the segment's
    // words "KEY[t_beg,t_end] w1 w2 ..." (frames of the stream), InitDecoding, and the decoder goes on with the stream's next rows.
    // The end of the stream ends the last segment.  --print-endpoints: also "KEY@t endpoint ruleK" at each endpoint.
    // Returns the lines; *ok: every segment had a path.
    auto decode_segmented = [&](GpuLatticeDecoder &dec, const Utt &u, bool pull_rows, bool *ok) {
      std::string text;
      *ok = true;
      int begin = 0;
      while (begin < u.frames) {
        HostMatrixDecodable md(u, begin);
        PullDecodable pd(u, tid2pdf.empty() ? nullptr : &tid2pdf, begin);
        AmInterface *am = pull_rows ? (AmInterface *)&pd : (AmInterface *)&md;
        dec.InitDecoding();
        int end = u.frames, rule = 0;
        for (int ready = (begin / chunk + 1) * chunk;; ready += chunk) {   // (the rows arrive at multiples of --chunk of the stream)
          md.SetFramesReady(ready);
          pd.SetFramesReady(ready);
          dec.AdvanceDecoding(am);
          if (ready >= u.frames) break;
          if (dec.EndpointDetected(ep_opt, &rule)) { end = ready; break; }
        }
        dec.FinalizeDecoding();
        Lattice best;
        std::vector<int> words, phones;
        float tot = 0, lm = 0;
        const bool seg_ok = dec.GetBestPath(&best) && LatticeToVector(best, words, phones, tot, lm);
        *ok = *ok && seg_ok;
        if (rule > 0 && print_endpoints) text += u.key + "@" + std::to_string(end) + " endpoint rule" + std::to_string(rule) + "\n";
        text += u.key + "[" + std::to_string(begin) + "," + std::to_string(end) + "]";
        for (int w : words) text += " " + std::to_string(w);
        text += "\n";
        begin = end;
      }
      return text;
    };
    auto count_segmented = [&](const Utt &u, bool ok) {
      if (!ok) { std::cerr << "WARNING Did not successfully decode every segment of utterance " << u.key << ", len = " << u.frames << "\n"; ++num_fail; return; }
      frame_count += u.frames;
      ++num_success;
    };
    if (pull && n_threads == 0) { std::cerr << "--pull goes with --threads\n"; return 1; }
    if (n_threads > 0) {
      // the service's shape: N worker threads, one DecoderItf object each, over a pool's channels or private device decoders
      if (devices.size() > 1) { std::cerr << "--threads: one device\n"; return 1; }
      if (pool_channels > 0 && pool_channels < n_threads) { std::cerr << "--pool must hold a channel per thread\n"; return 1; }
      if (share_channels > 0) GpuLatticeDecoder::ShareDevice(share_channels, linger_us);
      std::unique_ptr<GpuChannelPool> pool;
      if (pool_channels > 0)
        pool.reset(biglm ? new GpuChannelPool(&fst, opt, lm1p, lm2p, pool_channels, &limits, linger_us)
                         : new GpuChannelPool(&fst, opt, pool_channels, &limits, linger_us));
      struct Res { Lattice best; bool ok = false; Lattice lat; bool lat_ok = false; std::vector<Lattice> nbest; std::string segments, partials; };
      std::vector<Res> res(utts.size());
      int max_utt_frames = 0, max_utt_cols = 0;
      for (const Utt &u : utts) { max_utt_frames = std::max(max_utt_frames, u.frames); max_utt_cols = std::max(max_utt_cols, u.cols); }
      std::vector<std::string> errors((size_t)n_threads);
      std::atomic<size_t> next(0);
      std::atomic<int> ready_threads(0);
      std::atomic<long long> extra_frames(0);   // frames of the repeat passes (--repeat)
      if (warm >= repeat) { std::cerr << "--warm must leave a timed pass (--repeat)\n"; return 1; }
      const size_t warm_n = (size_t)warm * utts.size();   // utterances decoded before the clock
      std::atomic<size_t> warm_done(0);
      std::atomic<int> clock_started(warm_n == 0 ? 1 : 0);
      std::atomic<long long> clocked_frames(0);
      auto worker = [&](int k) {
        try {
          std::unique_ptr<GpuLatticeDecoder> dp(pool ? new GpuLatticeDecoder(pool.get())
                                                     : biglm ? new OnlineLatticeDecoderMempoolBiglm(&fst, opt, lm1p, lm2p, &limits)
                                                             : new GpuLatticeDecoder(&fst, opt, &limits));
          DecoderItf &decode = *dp;   // (the reference's interface is all the loop below uses, results aside)
          if (live_prune) dp->SetLiveLatticePrune(true);   // (over a pool: the shared decoder's, set by every thread before any of them decodes)
          dp->ReserveRows(max_utt_frames, pull && !tid2pdf.empty() ? (int)tid2pdf.size() - 1 : max_utt_cols - 1);
          // every thread has its decoder before the first utterance starts (the service creates them at start-up)
          ready_threads.fetch_add(1);
          while (ready_threads.load() < n_threads) std::this_thread::yield();
          if (k == 0) t0 = std::chrono::steady_clock::now();   // (the clock starts when every thread holds its decoder)
          for (;;) {
            const size_t uj = next.fetch_add(1);
            if (uj >= utts.size() * (size_t)repeat) return;
            const size_t ui = uj % utts.size();
            const bool first_pass = uj < utts.size();
            const Utt &u = utts[ui];
            // (--warm: the timed passes start together, behind the last warm-up utterance)
            if (uj >= warm_n) while (!clock_started.load()) std::this_thread::yield();
            struct Count {   // whatever way the utterance ends
              std::atomic<size_t> &done; std::atomic<int> &started; std::chrono::steady_clock::time_point &t0; bool is_warm; size_t n;
              ~Count() { if (is_warm && done.fetch_add(1) + 1 == n) { t0 = std::chrono::steady_clock::now(); started.store(1); } }
            } count{warm_done, clock_started, t0, uj < warm_n, warm_n};
            HostMatrixDecodable md(u);
            PullDecodable pd(u, tid2pdf.empty() ? nullptr : &tid2pdf);
            AmInterface *am = pull ? (AmInterface *)&pd : (AmInterface *)&md;
            // an utterance that fails (a capacity limit: the reference's LOG_ERR -> exception) is this utterance's failure, as in the
            // reference CLI (kaldi-hclg-my-decoder.cc:131-136 counts it and goes on): the thread's decoder takes the next one
            try {
            if (endpointing) {
              Res scratch;
              Res &r = first_pass ? res[ui] : scratch;
              r.segments = decode_segmented(*dp, u, pull, &r.ok);
              if (uj >= warm_n && warm_n > 0) clocked_frames.fetch_add(r.ok ? u.frames : 0);
              if (!first_pass) extra_frames.fetch_add(r.ok ? u.frames : 0);
              continue;
            }
            decode.InitDecoding();
            if (chunk > 0) {
              for (int ready = chunk;; ready += chunk) {
                md.SetFramesReady(ready);
                pd.SetFramesReady(ready);
                decode.AdvanceDecoding(am);
                if (ready >= u.frames) break;
                if (partial_words) {   // (over the pool: one list per batcher pass for all the threads that ask)
                  std::vector<int> w;
                  int n_stable = 0;
                  dp->GetPartialWords(&w, &n_stable);
                  if (first_pass) {
                    std::string &o = res[ui].partials;
                    o += u.key + "@" + std::to_string(decode.NumFramesDecoded()) + " " + std::to_string(n_stable);
                    for (size_t q = 0; q < w.size(); ++q) o += " " + std::to_string(w[q]);
                    o += "\n";
                  }
                }
                if (partial_nbest > 0) {   // (over the pool: one list call per batcher pass for all the threads that ask the same)
                  std::vector<std::vector<int> > w;
                  std::vector<float> t, l;
                  int st = WFST_OK;
                  dp->GetNbestWords(&w, &t, &l, partial_nbest, false, slm1p, slm2p, &st);
                  if (first_pass) res[ui].partials += nbest_lines(u.key, decode.NumFramesDecoded(), st, w, t, l);
                }
              }
            } else {
              decode.AdvanceDecoding(am);
            }
            decode.FinalizeDecoding();
            Res scratch;
            Res &r = first_pass ? res[ui] : scratch;
            r.ok = decode.GetBestPath(&r.best);
            if (uj >= warm_n && warm_n > 0) clocked_frames.fetch_add(r.ok ? u.frames : 0);
            if (!first_pass) { extra_frames.fetch_add(r.ok ? u.frames : 0); continue; }
            if (want_lattice && (!lattice_file.empty() || !lattice_text.empty()))
              r.lat_ok = determinize ? dp->GetLattice(&r.lat) : decode.GetRawLattice(&r.lat);
            if (nbest > 0) {
              if (exact_nbest) dp->GetNbest(r.nbest, nbest);
              else dp->GetNbestShortlist(r.nbest, nbest);
            }
            } catch (const std::runtime_error &e) {
              {   // (one stdio call per line: the worker threads share stderr)
                const std::string line = "WARNING utterance " + u.key + " failed: " + e.what() + "\n";
                fputs(line.c_str(), stderr);
              }
              if (first_pass) res[ui].ok = false;
            }
          }
        } catch (const std::exception &e) {
          errors[(size_t)k] = e.what();
          ready_threads.fetch_add(1);   // (a constructor that failed must not leave the others waiting)
        }
      };
      std::vector<std::thread> threads;
      for (int k = 1; k < n_threads; ++k) threads.emplace_back(worker, k);
      worker(0);
      for (std::thread &t : threads) t.join();
      for (const std::string &e : errors)
        if (!e.empty()) throw std::runtime_error(e);
      for (size_t i = 0; i < utts.size(); ++i) {
        if (endpointing) { out << res[i].segments; count_segmented(utts[i], res[i].ok); continue; }
        out << res[i].partials;
        emit(utts[i], res[i].best, res[i].ok);
        if (want_lattice && (!lattice_file.empty() || !lattice_text.empty())) emit_lattice(utts[i], res[i].lat, res[i].lat_ok);
        if (nbest > 0) emit_nbest(utts[i], res[i].nbest);
      }
      repeat_frames = extra_frames.load();
      timed_frames = clocked_frames.load();
      if (pool) {
        const GpuChannelPool::Stats st = pool->GetStats();
        std::cerr << "LOG pool: " << pool_channels << " channels, " << n_threads << " threads, " << st.batches << " batcher passes, " << st.requests
                  << " requests, " << st.advance_calls << " advance calls for " << st.advance_requests << " AdvanceDecoding requests (mean batch "
                  << (st.advance_calls ? (double)st.advance_requests / st.advance_calls : 0.0) << "), " << st.frames << " frames; batcher ms: init "
                  << st.ms_by_kind[0] << " advance " << st.ms_by_kind[1] << " finalize " << st.ms_by_kind[2] << " best-path " << st.ms_by_kind[3]
                  << " calls " << st.ms_by_kind[4] << " waiting " << st.ms_waiting << "\n";
      }
    } else if (single) {  // the reference's shape: one decoder object, one utterance at a time
      std::unique_ptr<GpuLatticeDecoder> decode_p(biglm ? new OnlineLatticeDecoderMempoolBiglm(&fst, opt, lm1p, lm2p, &limits)
                                                        : new GpuLatticeDecoder(&fst, opt, &limits));
      GpuLatticeDecoder &decode = *decode_p;
      if (word_times) decode.SetSilencePhones(wt_silence);
      if (live_prune) decode.SetLiveLatticePrune(true);
      for (const Utt &u : utts) {
        if (endpointing) {
          bool ok = false;
          out << decode_segmented(decode, u, false, &ok);
          count_segmented(u, ok);
          continue;
        }
        HostMatrixDecodable decodable(u);
        decode.InitDecoding();
        if (chunk > 0) {  // the service's loop: data arrives, AdvanceDecoding, partial result
          for (int ready = chunk; ; ready += chunk) {
            decodable.SetFramesReady(ready);
            decode.AdvanceDecoding(&decodable);
            if (ready >= u.frames) break;
            Lattice part;
            std::vector<int> w, ph;
            float tot = 0, lm = 0;
            if (partial_words) {   // key@frames n_stable w1 w2 ...: the incremental partial result, its first n_stable words final
              int n_stable = 0;
              decode.GetPartialWords(&w, &n_stable);
              out << u.key << "@" << decode.NumFramesDecoded() << " " << n_stable;
              for (size_t k = 0; k < w.size(); ++k) out << " " << w[k];
              out << "\n";
            } else {
              out << u.key << "@" << decode.NumFramesDecoded();
              if (decode.GetBestPath(&part, false) && LatticeToVector(part, w, ph, tot, lm))
                for (size_t k = 0; k < w.size(); ++k) out << " " << w[k];
              out << "\n";
            }
            if (nbest > 0) {
              // (partial lists come from the raw lattice: its unpruned last frames make the mid-utterance lattice expensive to
              // determinize, for the reference as much as here)
              std::vector<Lattice> paths;
              decode.GetNbestShortlist(paths, std::min(nbest, 16));
              for (size_t k = 0; k < paths.size(); ++k) {
                std::vector<int> nw, nph;
                float t2 = 0, l2 = 0;
                LatticeToVector(paths[k], nw, nph, t2, l2);
                out << u.key << "@" << decode.NumFramesDecoded() << "-" << (k + 1);
                for (size_t q = 0; q < nw.size(); ++q) out << " " << nw[q];
                out << "\n";
              }
            }
            if (partial_nbest > 0) {
              std::vector<std::vector<int> > pw;
              std::vector<float> pt, pl;
              int st = WFST_OK;
              decode.GetNbestWords(&pw, &pt, &pl, partial_nbest, false, slm1p, slm2p, &st);
              std::vector<TimedSeq> al;
              if (nbest_times && !pw.empty()) stream_times(decode, pw, &al, false);
              out << nbest_lines(u.key, decode.NumFramesDecoded(), st, pw, pt, pl, nbest_times ? &al : nullptr);
            }
          }
        } else {
          decode.AdvanceDecoding(&decodable);
        }
        decode.FinalizeDecoding();
        Lattice best;
        bool ok = decode.GetBestPath(&best);
        WordTimes wt;
        if (word_times && ok) {
          decode.GetWords(&wt.words, &wt.frames, nullptr, nullptr);
          emit_times = &wt;
        }
        emit(u, best, ok);
        emit_times = nullptr;
        if (want_lattice) {
          Lattice lat;
          bool lok = determinize ? (second ? decode.GetLattice(&lat, slm1p, slm2p) : decode.GetLattice(&lat)) : decode.GetRawLattice(&lat);
          emit_lattice(u, lat, lok);
        }
        if (nbest > 0) {
          std::vector<Lattice> paths;
          if (!exact_nbest) decode.GetNbestShortlist(paths, nbest);
          else if (second) decode.GetNbest(paths, nbest, slm1p, slm2p);
          else decode.GetNbest(paths, nbest);
          std::vector<TimedSeq> al;
          if (nbest_times && !paths.empty()) stream_times(decode, path_words(paths), &al, true);
          emit_nbest(u, paths, nbest_times ? &al : nullptr);
        }
        if (align_seqs.count(u.key)) {
          std::vector<TimedSeq> al;
          stream_times(decode, align_seqs[u.key], &al, true);
          emit_align(u, al);
        }
        if (phrases.count(u.key)) {
          std::vector<SequencePosterior> sp;
          decode.SequencePosteriors(phrases[u.key], &sp, true, true, conf_gs, conf_as, true);
          emit_phrases(u, sp);
        }
        if (nearest_refs.count(u.key)) {
          std::vector<NearestPath> np;
          decode.NearestWords(nearest_refs[u.key], &np);
          emit_nearest(u, np);
        }
        if (frame_post) {
          FramePosteriors fp;
          decode.FramePosteriors(&fp, fp_map, fp_min, true, fp_gs, fp_as);
          emit_frame_post(u, fp);
        }
        if (seq_stats) {
          SequenceStats ss;
          decode.SequenceStats(seq_ref_of(u), &ss, seq_opt);
          emit_seq_stats(u, ss);
        }
        if (rescale) {
          std::vector<RescaledWords> rw;
          decode.RescaledWords(rescale_set, &rw);
          emit_rescale(u, rw);
        }
        if (bias) {
          const std::vector<BiasPhrase> list = bias_list_of(u);
          BiasLists bl;
          BiasBooks bk;
          const std::vector<std::vector<BiasPhrase> > one(1, list);
          if (!list.empty() && !(bias_sparse ? bk.Set(one, devices[0]) : bl.Set(one, devices[0]))) throw std::runtime_error("--bias: the phrases of " + u.key + " make no list");
          std::vector<BiasedWords> bw;
          if (bias_sparse) decode.BiasedWordsSparse(bk, list.empty() ? -1 : 0, bias_set, &bw);
          else decode.BiasedWords(bl, list.empty() ? -1 : 0, bias_set, &bw);
          emit_bias(u, bw);
        }
        if (force_align) {
          AlignGraphs ag;
          if (!ag.Read(std::vector<std::string>(1, force_file(u)), devices[0])) throw std::runtime_error("--force-align: cannot load " + force_file(u));
          ForcedAlignment fa;
          decode.ForceAlign(ag, 0, &fa, force_map);
          emit_forced(u, fa);
        }
        if (graph_post) {
          AlignGraphs ag;
          if (!ag.Read(std::vector<std::string>(1, gpost_graph(u)), devices[0])) throw std::runtime_error("--graph-post: cannot load " + gpost_graph(u));
          GraphPosteriors gp;
          decode.GraphPosteriors(ag, 0, &gp, gpost_opt);
          emit_graph_post(u, gp);
        }
      }
    } else {  // the MI355X shape: `batch` utterances per pass, `inflight` passes at a time
      struct BatchOut {
        std::vector<Lattice> best, lats;
        std::vector<bool> ok, lat_ok;
        std::vector<std::vector<Lattice> > nbest;
        std::vector<std::vector<int> > wt_words;                      // --word-times
        std::vector<std::vector<std::pair<int, int> > > wt_frames;
        std::string partials;                                         // --partial-nbest
        std::vector<std::vector<TimedSeq> > nb_times, al_times;  // --nbest-word-times, --align-words
        std::vector<std::vector<SequencePosterior> > phrase_post;     // --phrase-posterior
        std::vector<std::vector<NearestPath> > nearest;               // --nearest-words
        std::vector<FramePosteriors> frame_post;                      // --frame-post
        std::vector<std::vector<RescaledWords> > rescaled;            // --rescale
        std::vector<std::vector<BiasedWords> > biased;                // --bias
        std::vector<SequenceStats> seq_stats;                         // --seq-stats
        std::vector<ForcedAlignment> forced;                          // --force-align
        std::vector<GraphPosteriors> graph_post;                      // --graph-post
      };
      const size_t n_batches = (utts.size() + batch - 1) / batch;
      std::vector<BatchOut> outs(n_batches);
      std::atomic<size_t> next(0);
      const int n_dev = (int)devices.size(), n_workers = inflight * n_dev;
      std::vector<std::string> errors((size_t)n_workers);
      std::vector<std::atomic<size_t> > next_of_dev((size_t)n_dev);
      for (auto &x : next_of_dev) x = 0;
      auto worker = [&](int k) {
        try {
          // worker k drives a decoder on device k mod n_dev, over that device's graph replica (and LMs)
          const int di = k % n_dev;
          Fst *wf = fsts[(size_t)di].get();
          ArpaLm *lm1 = biglm ? &lms[(size_t)di]->a : nullptr, *lm2 = biglm ? &lms[(size_t)di]->b : nullptr;
          ArpaLm *slm1 = second ? &slms[(size_t)di]->a : nullptr, *slm2 = second ? &slms[(size_t)di]->b : nullptr;
          std::unique_ptr<GpuBatchDecoder> decode_p(biglm ? new GpuBatchDecoder(wf, opt, lm1, lm2, batch, &limits)
                                                          : new GpuBatchDecoder(wf, opt, batch, &limits));  // its own stream
          GpuBatchDecoder &decode = *decode_p;
          if (word_times) decode.SetSilencePhones(wt_silence);
          if (live_prune) decode.SetLiveLatticePrune(true);
          if (device_chunks) decode.SetScoreTransform(acoustic_scale, log_priors);
          // --device-chunks: a chunk of every channel's rows in the score dtype, page-locked (the device reads it where it lies)
          const size_t elem = score_dtype == WFST_DTYPE_F32 ? 4 : 2;
          std::unique_ptr<void, void (*)(void *)> stage(nullptr, wfst_host_free);
          size_t stage_per = 0;
          for (;;) {
            // one device: the next batch nobody has taken; several: batch b belongs to device b mod n_dev (its workers share them)
            const size_t b = n_dev == 1 ? next.fetch_add(1) : (size_t)di + (size_t)n_dev * next_of_dev[(size_t)di].fetch_add(1);
            if (b >= n_batches) return;
            const size_t b0 = b * (size_t)batch;
            const int n = (int)std::min<size_t>(batch, utts.size() - b0);
            std::vector<int> ch(n), ready(n);
            std::vector<const float *> rows(n);
            const int stride = utts[b0].cols;
            for (int i = 0; i < n; ++i) {
              ch[i] = i;
              ready[i] = utts[b0 + i].frames;
              rows[i] = utts[b0 + i].m.data();
              if (utts[b0 + i].cols != stride) throw std::runtime_error("all matrices of a batch must have the same width");
            }
            BatchOut &o = outs[b];
            decode.InitDecoding(ch);
            if (device_chunks) {
              if (!log_priors.empty() && (int)log_priors.size() != stride) throw std::runtime_error("--log-priors: one prior per column of the matrices");
              if ((size_t)chunk * stride * elem > stage_per) {
                stage_per = (((size_t)chunk * stride * elem) + 15) & ~(size_t)15;
                stage.reset(wfst_host_alloc(stage_per * (size_t)batch));
                if (!stage) throw std::runtime_error("--device-chunks: no page-locked staging buffer");
              }
              int longest = 0;
              for (int i = 0; i < n; ++i) longest = std::max(longest, ready[i]);
              std::vector<const void *> ptrs(n);
              std::vector<int> fresh(n);
              for (int have = 0; have < longest; have += chunk) {
                for (int i = 0; i < n; ++i) {
                  fresh[i] = std::max(0, std::min(chunk, ready[i] - have));
                  char *dst = (char *)stage.get() + stage_per * (size_t)i;
                  ptrs[i] = fresh[i] ? dst : nullptr;
                  const float *src = rows[i] + (size_t)have * stride;
                  const size_t cnt = (size_t)fresh[i] * stride;
                  if (score_dtype == WFST_DTYPE_F32) memcpy(dst, src, cnt * 4);
                  else for (size_t e = 0; e < cnt; ++e) ((uint16_t *)dst)[e] = score_dtype == WFST_DTYPE_F16 ? ToF16(src[e]) : ToBf16(src[e]);
                }
                decode.AdvanceDecodingChunk(ch, ptrs, fresh, score_dtype, stride, WFST_STREAM_NONE);
                if (wfst_decoder_sync(decode.Handle()) != WFST_OK) throw std::runtime_error(wfst_last_error());   // (the staging buffer is the next chunk's)
              }
            } else if (partial_nbest > 0) {
              // the streaming shape over the batch: every channel's next chunk, then ONE n-best text call for the channels still running
              int longest = 0;
              for (int i = 0; i < n; ++i) longest = std::max(longest, ready[i]);
              std::vector<int> upto(n);
              for (int have = chunk;; have += chunk) {
                for (int i = 0; i < n; ++i) upto[i] = std::min(ready[i], have);
                decode.AdvanceDecodingHost(ch, rows, upto, stride);
                if (have >= longest) break;
                std::vector<int> live;
                for (int i = 0; i < n; ++i)
                  if (have < ready[i]) live.push_back(i);
                std::vector<std::vector<std::vector<int> > > w;
                std::vector<std::vector<float> > t, l;
                std::vector<int> st;
                decode.GetNbestWords(live, partial_nbest, slm1, slm2, false, &w, &t, &l, &st);
                std::vector<std::vector<TimedSeq> > al;
                std::vector<int> ast;
                if (nbest_times && !live.empty()) batch_times(decode, live, w, false, &al, &ast);   // (one call for the channels still running)
                for (size_t q = 0; q < live.size(); ++q)
                  o.partials += nbest_lines(utts[b0 + (size_t)live[q]].key, decode.NumFramesDecoded(live[q]), st[q], w[q], t[q], l[q],
                                            nbest_times && ast[q] == WFST_OK ? &al[q] : nullptr);
              }
            } else {
              decode.AdvanceDecodingHost(ch, rows, ready, stride);
            }
            decode.FinalizeDecoding(ch);
            if (want_lattice && determinize && !second) decode.PrefetchLattices();   // the determinizer runs beside the best paths
            decode.GetBestPaths(ch, &o.best, &o.ok);
            if (word_times) decode.GetWords(ch, &o.wt_words, &o.wt_frames, nullptr, nullptr);
            if (want_lattice && determinize) {
              o.lats.assign(n, Lattice());
              o.lat_ok.assign(n, false);
              for (int i = 0; i < n; ++i) o.lat_ok[i] = second ? decode.GetLattice(i, &o.lats[i], slm1, slm2) : decode.GetLattice(i, &o.lats[i]);
            } else if (want_lattice) {
              decode.GetRawLattices(ch, &o.lats, &o.lat_ok);
            }
            if (nbest > 0) {
              o.nbest.resize(n);
              // (short lists for the whole batch come from one launch on the raw lattices; longer ones are NShortestPath per channel)
              for (int i = 0; i < n; ++i) {
                if (!exact_nbest) decode.GetNbestShortlist(i, o.nbest[i], nbest);
                else if (second) decode.GetNbest(i, o.nbest[i], nbest, slm1, slm2);
                else decode.GetNbest(i, o.nbest[i], nbest);
              }
              if (nbest_times) {   // every path of every channel in one call
                std::vector<std::vector<std::vector<int> > > seqs(n);
                for (int i = 0; i < n; ++i) seqs[i] = path_words(o.nbest[i]);
                batch_times(decode, ch, seqs, true, &o.nb_times, nullptr);
              }
            }
            if (!align_seqs.empty()) {
              std::vector<std::vector<std::vector<int> > > seqs(n);
              for (int i = 0; i < n; ++i) {
                auto it = align_seqs.find(utts[b0 + i].key);
                if (it != align_seqs.end()) seqs[i] = it->second;
              }
              batch_times(decode, ch, seqs, true, &o.al_times, nullptr);
            }
            if (!phrases.empty()) {   // every phrase of every channel in one call
              std::vector<std::vector<std::vector<int> > > seqs(n);
              for (int i = 0; i < n; ++i) {
                auto it = phrases.find(utts[b0 + i].key);
                if (it != phrases.end()) seqs[i] = it->second;
              }
              decode.SequencePosteriors(ch, seqs, true, true, conf_gs, conf_as, &o.phrase_post, nullptr, 0, true);
            }
            if (!nearest_refs.empty()) {   // every reference of every channel in one call
              std::vector<std::vector<std::vector<int> > > refs(n);
              for (int i = 0; i < n; ++i) {
                auto it = nearest_refs.find(utts[b0 + i].key);
                if (it != nearest_refs.end()) refs[i] = it->second;
              }
              decode.NearestWords(ch, refs, true, &o.nearest);
            }
            if (frame_post) decode.FramePosteriors(ch, true, fp_gs, fp_as, fp_map, fp_min, &o.frame_post);   // every channel in one call
            if (rescale) decode.RescaledWords(ch, rescale_set, true, &o.rescaled);                           // every channel and setting in one call
            if (bias) {                                                                                      // every channel and setting in one call
              std::vector<std::vector<BiasPhrase> > lists;
              std::vector<int> list_of(n, -1);
              for (int i = 0; i < n; ++i) {
                const std::vector<BiasPhrase> list = bias_list_of(utts[b0 + i]);
                if (list.empty()) continue;
                list_of[i] = (int)lists.size();
                lists.push_back(list);
              }
              BiasLists bl;
              BiasBooks bk;
              if (!lists.empty() && !(bias_sparse ? bk.Set(lists, devices[(size_t)di]) : bl.Set(lists, devices[(size_t)di])))
                throw std::runtime_error("--bias: the phrases of " + bias_file + " make no lists");
              if (bias_sparse) decode.BiasedWordsSparse(ch, bk, list_of, bias_set, true, &o.biased);
              else decode.BiasedWords(ch, bl, list_of, bias_set, true, &o.biased);
            }
            if (seq_stats) {                                                                                 // every channel in one call
              std::vector<std::vector<int> > refs(n);
              for (int i = 0; i < n; ++i) refs[i] = seq_ref_of(utts[b0 + i]);
              decode.SequenceStats(ch, refs, seq_opt, &o.seq_stats);
            }
            if (force_align) {                                                                               // every channel in one launch
              std::vector<std::string> files(n);
              for (int i = 0; i < n; ++i) files[i] = force_file(utts[b0 + i]);
              AlignGraphs ag;
              if (!ag.Read(files, devices[(size_t)di])) throw std::runtime_error("--force-align: cannot load the graphs of " + force_dir);
              decode.ForceAlign(ch, ag, std::vector<int>(), force_map, &o.forced);
            }
            if (graph_post) {                                                                                // every channel in one launch
              std::vector<std::string> files(n);
              for (int i = 0; i < n; ++i) files[i] = gpost_graph(utts[b0 + i]);
              AlignGraphs ag;
              if (!ag.Read(files, devices[(size_t)di])) throw std::runtime_error("--graph-post: cannot load the graphs of " + gpost_dir);
              decode.GraphPosteriors(ch, ag, std::vector<int>(), gpost_opt, &o.graph_post);
            }
          }
        } catch (const std::exception &e) {
          errors[(size_t)k] = e.what();
        }
      };
      std::vector<std::thread> threads;
      for (int k = 1; k < n_workers; ++k) threads.emplace_back(worker, k);
      worker(0);
      for (std::thread &t : threads) t.join();
      for (const std::string &e : errors)
        if (!e.empty()) throw std::runtime_error(e);
      for (size_t b = 0; b < n_batches; ++b) {  // results in input order
        const size_t b0 = b * (size_t)batch;
        BatchOut &o = outs[b];
        const int n = (int)o.best.size();
        out << o.partials;
        for (int i = 0; i < n; ++i) {
          WordTimes wt;
          if (word_times && o.ok[i]) {
            wt.words = o.wt_words[i];
            wt.frames = o.wt_frames[i];
            emit_times = &wt;
          }
          emit(utts[b0 + i], o.best[i], o.ok[i]);
          emit_times = nullptr;
        }
        for (int i = 0; i < n && want_lattice; ++i) emit_lattice(utts[b0 + i], o.lats[i], o.lat_ok[i]);
        for (int i = 0; i < n && nbest > 0; ++i) emit_nbest(utts[b0 + i], o.nbest[i], nbest_times ? &o.nb_times[i] : nullptr);
        for (int i = 0; i < n && !o.al_times.empty(); ++i) emit_align(utts[b0 + i], o.al_times[i]);
        for (int i = 0; i < n && !o.phrase_post.empty(); ++i) emit_phrases(utts[b0 + i], o.phrase_post[i]);
        for (int i = 0; i < n && !o.nearest.empty(); ++i) emit_nearest(utts[b0 + i], o.nearest[i]);
        for (int i = 0; i < n && !o.frame_post.empty(); ++i) emit_frame_post(utts[b0 + i], o.frame_post[i]);
        for (int i = 0; i < n && !o.rescaled.empty(); ++i) emit_rescale(utts[b0 + i], o.rescaled[i]);
        for (int i = 0; i < n && !o.biased.empty(); ++i) emit_bias(utts[b0 + i], o.biased[i]);
        for (int i = 0; i < n && !o.seq_stats.empty(); ++i) emit_seq_stats(utts[b0 + i], o.seq_stats[i]);
        for (int i = 0; i < n && !o.forced.empty(); ++i) emit_forced(utts[b0 + i], o.forced[i]);
        for (int i = 0; i < n && !o.graph_post.empty(); ++i) emit_graph_post(utts[b0 + i], o.graph_post[i]);
      }
    }
    if (!nearest_refs.empty()) {   // errors over reference words, as nbest-compute-wer prints them
      char buf[160];
      snprintf(buf, sizeof(buf), "nearest %%WER %.2f [ %lld / %lld, %lld ins, %lld del, %lld sub ]\n", nr_words ? 100.0 * (double)nr_err / (double)nr_words : 0.0,
               nr_err, nr_words, nr_ins, nr_del, nr_sub);
      out << buf;
    }
    double elapsed = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (timed_frames) {   // (--warm: the clock started behind the warm-up passes)
      std::cerr << "LOG Time taken " << elapsed << "s: real-time factor assuming 100 frames/sec is " << elapsed * 100.0 / timed_frames << "\n";
      std::cerr << "LOG Timed passes: " << timed_frames << " frames in " << elapsed << " s behind " << warm << " warm-up passes over the list\n";
    } else {
      std::cerr << "LOG Time taken " << elapsed << "s: real-time factor assuming 100 frames/sec is "
                << (frame_count ? elapsed * 100.0 / (frame_count + repeat_frames) : 0.0) << "\n";
      if (repeat_frames) std::cerr << "LOG Frames decoded in all passes: " << (frame_count + repeat_frames) << "\n";
    }
    std::cerr << "LOG Done " << num_success << " utterances, failed for " << num_fail << "\n";
    std::cerr << "LOG Overall log-likelihood per frame is " << (frame_count ? tot_like / frame_count : 0.0) << " over "
              << frame_count << " frames.\n";
    return num_success != 0 ? 0 : 1;
  } catch (const std::exception &e) {
    std::cerr << "ERROR " << e.what() << "\n";
    return 2;
  }
}
