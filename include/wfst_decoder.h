/*
 * wfst_decoder.h -- C ABI of the MI355X-native batched WFST token-passing decoder.
 *
 * This is the drop-in boundary for ONE path of datemoon/ASR-decoder: the frame-synchronous
 * token-passing search of src/my-decoder (ProcessEmitting / ProcessNonemitting / beam pruning
 * over the flat HCLG of src/newfst), precomputed log-likelihoods in; best path, raw lattice and
 * n-best out.
 * Plain pointers and sizes only; no C++ or torch types.  Every entry point names the reference
 * interface it replaces (paths relative to the reference's src/).
 *
 * Threading: one wfst_decoder per host thread (like one reference decoder object per worker
 * thread, v2-asr/v2-asr-work-thread.h:66); a wfst_graph is immutable after creation and may be
 * shared by any number of decoders on the same device (like the shared read-only Fst,
 * kaldi-nnet3/kaldi-online-nnet3-my-decoder.h:121).
 *
 * Errors: every function returning int returns WFST_OK (0) or a negative WFST_E_* code;
 * wfst_last_error() gives the message of the calling thread's last failure.  There is no CPU
 * fallback: without a usable HIP device every call that needs one fails with WFST_E_DEVICE.
 */
#ifndef WFST_DECODER_H_
#define WFST_DECODER_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WFST_OK 0
#define WFST_E_ARG (-1)      /* bad argument                                              */
#define WFST_E_IO (-2)       /* graph file unreadable / truncated                         */
#define WFST_E_DEVICE (-3)   /* HIP error (no device, out of memory, launch failure)      */
#define WFST_E_CAPACITY (-4) /* a per-channel limit of wfst_limits was exceeded on device */
#define WFST_E_STATE (-5)    /* call sequence violated (e.g. advance before init)         */
#define WFST_E_FORMAT (-6)   /* graph violates a layout limit (see wfst_graph_from_arrays) */

typedef struct wfst_graph wfst_graph;     /* HCLG resident in HBM; replaces `Fst` (newfst/optimize-fst.h:53-307) */
typedef struct wfst_decoder wfst_decoder; /* a batch of decoding channels; one channel replaces one
                                             OnlineLatticeDecoderMempool (my-decoder/online-decoder-mempool-base.h:77) */
typedef struct wfst_lm wfst_lm;           /* a back-off n-gram LM automaton resident in HBM; replaces `ArpaLm`
                                             (newlm/arpa2fsa.h:249-441) for the biglm decoder */

/* Field-for-field LatticeFasterDecoderConfig (my-decoder/lattice-faster-decoder-conf.h:21-44);
 * wfst_config_default() fills the reference defaults (conf.h:35-44).  hash_ratio is accepted for
 * compatibility (the device hash tables are sized by wfst_limits and wfst_options).  Best-path decoders keep
 * no forward-link lists to back-prune: prune_interval and lattice_beam there only decide which of several
 * parallel arcs GetBestPath reports, exactly as in the reference.  In LATTICE MODE
 * (wfst_limits.lattice_links > 0) the reference's PruneActiveTokens runs on the device: every prune_interval
 * frames the recorded links are pruned backwards by lattice_beam, walking back while a frame's extra costs
 * move by more than lattice_beam * prune_scale (base-inl.h:439-607, 660-661), and the token arena and link
 * store are compacted, so that memory stays bounded whatever the utterance length; FinalizeDecoding prunes
 * with delta 0 like the reference's PruneActiveTokens(0) (base-inl.h:541-607). */
typedef struct wfst_config {
  float beam;
  int32_t max_active;
  int32_t min_active;
  float lattice_beam;
  int32_t prune_interval;
  float beam_delta;
  float hash_ratio;
  float prune_scale;
} wfst_config;

/* Per-channel device capacities (0 = default).  Exceeding one makes the affected call return
 * WFST_E_CAPACITY -- with ONE exception, max_tokens_per_frame of a best-path decoder on the fused rows,
 * which degrades the search instead (below) and says so through wfst_decoder_get_degraded_frames; the
 * C++ mirror's GetBestPath(s) warn when that count is not 0.  Nothing is dropped without one of the two. */
typedef struct wfst_limits {
  int32_t max_frames;           /* frames per utterance                     (default 4096)    */
  int32_t max_tokens_per_frame; /* distinct states reached in one frame     (default 65536, or 4 x a finite max_active, at most 262144).
                                   Best-path decoders on the fused rows do not fail at it: it acts as a max_active
                                   (the frame goes on from its limit-th cheapest token; wfst_decoder_get_degraded_frames
                                   counts such frames).  Such a frame may HOLD several times the limit (the arrivals of
                                   limit expanded tokens), while the token collection is sized for limit tokens a frame:
                                   an utterance that stays over the limit frame after frame can still exhaust the arena
                                   between two collections and then fails loudly with WFST_E_CAPACITY (arena full) --
                                   size arena_tokens for it or raise the limit.  Lattice and biglm decoders return
                                   WFST_E_CAPACITY at the limit itself */
  int64_t arena_tokens;         /* token arena of one utterance, 16 bytes a token.  BEST-PATH decoders keep every
                                   token of the utterance for the traceback (there are no link lists to prune
                                   them by): an utterance of T frames with n tokens alive per frame needs about
                                   T x n IF nothing is reclaimed; when less than an eighth of the arena (a quarter: two-launch decoders) is left
                                   the decoder collects it (keeps what the frontier's backpointers reach, a percent or two,
                                   and moves it down), so that what the arena must hold is the raw tokens of the
                                   frames between two collections plus the surviving history -- a few hundred
                                   frames' worth is plenty for any utterance length; WFST_E_CAPACITY only if one
                                   collection cannot free half of it.  A collection costs ~5 ms per million
                                   tokens in the arena: size it so that collections are rare.  Arenas of at most 4194304
                                   tokens (the default) leave room in a token's backpointer for its state's degree
                                   code: the expansion then skips the row-header reads (a third of its fetches).  LATTICE-MODE decoders reclaim it every
                                   prune_interval frames (see wfst_config) and need ~3x the tokens
                                   FinalizeDecoding keeps + prune_interval frames of raw tokens.
                                   Default: max_frames x max(256, max_tokens_per_frame / 64), at least 4194304,
                                   i.e. room for the default max_frames at 1024 tokens per frame             */
  int64_t lattice_links;        /* > 0: LATTICE MODE -- record every forward link (capacity per
                                   utterance) so that FinalizeDecoding can prune by lattice_beam and
                                   GetRawLattice can be served; 0 (default): best path only        */
  int64_t lm_pairs;             /* biglm decoders: distinct (old-LM state, new-LM state) pairs one
                                   utterance may reach (default 262144; rounded up to a power of two) */
  int32_t det_raw_states;       /* GetLattice (wfst_decoder_get_determinized_lattice): the largest raw lattice the on-device
                                   determinizer takes, in states (default 65536) ...                                    */
  int32_t det_raw_arcs;         /* ... and arcs (default 2 x det_raw_states).  The determinizer's workspace is allocated by
                                   the first GetLattice call: about 1.2 KB per raw state and lattice (79 MB at the default),
                                   for as many lattices at a time as det_workspace_bytes allows                          */
  int64_t det_workspace_bytes;  /* upper bound of that workspace (default: room for every channel of the decoder, at most an
                                   eighth of the device's memory).  Lattices beyond it are determinized in further launches:
                                   a speed knob, never a refusal (at least one lattice's workspace is always allocated)   */
} wfst_limits;

/* Scheduling choices of a decoder (NULL / wfst_options_default() = the measured defaults).  None of
 * them changes a result bit; they replace what a CPU decoder has no use for.  Values out of range are
 * WFST_E_ARG.  (The library reads no environment variables.) */
typedef struct wfst_options {
  int32_t channel_groups;      /* 1..8: channel groups, each with its own stream and hipGraph; 0 = automatic
                                  (2 groups from 64 channels up, 3 from 96 up, else 1)           (0)    */
  int32_t use_hip_graph;       /* replay the frame loop of an advance call as a hipGraph        (1)    */
  int32_t log2_partitions;     /* 0..6: hash partitions (candidate buckets) per channel; -1 = by the
                                  decoder's kind: 5, lattice decoders 6                          (-1)   */
  int32_t log2_lds_slots;      /* 8..13: LDS hash slots of one insert workgroup                 (12)   */
  int32_t joint_max;           /* records a group of partitions may hold to share a workgroup   (1536) */
  int32_t expand_workgroups;   /* grid of the expansion kernel; 0 = by the decoder's kind: 2048,
                                  lattice decoders 3072                                          (0)    */
  int32_t insert_workgroups;   /* grid of the insert kernel                                     (768)  */
  int32_t upload_slice_frames; /* wfst_decoder_advance_host: frames per upload slice, 0 = copy
                                  everything before decoding                                    (48)   */
  int32_t tile_tokens;         /* 64..256: frontier tokens per tile of the staged expansion     (256)  */
  int32_t debug;               /* kernel phase timers (32 closure / 64 insert / 128 expansion, printed when the
                                  decoder is freed)                                              (0)    */
                               /* (0x1000: lattice decoders run the iterated epsilon-closure pass instead of
                                  the fused rows + flat epsilon-link pass; same results, for comparison.
                                  0x800: a running back-pruning pass prices the never-priced frames of EVERY
                                  channel on several workgroups (by default only channels with 800 k such links
                                  or more: the LDS walk is faster below); same results, for the tests.
                                  0x400: with 0x800, one workgroup of every such channel stays away from the
                                  first meeting -- the pass is abandoned after its 40 ms time-out and done over
                                  by the one-workgroup walk; same results, for the tests.
                                  0x100 / 0x200 / 0x300: a lattice decoder's closure launches run 1 / 2 / 8
                                  workgroups per channel instead of 4 (they share the frame's epsilon links);
                                  same results, for the tests.
                                  Further bits are A/B switches of timing experiments, honoured only by a
                                  library built with -DWFST_AB_SWITCHES) */
} wfst_options;

/* Graph upload choices (NULL / wfst_graph_options_default() = defaults). */
typedef struct wfst_graph_options {
  int32_t row_align_slots;     /* rows are placed so that they touch as few lines of this many 16-byte
                                  slots as possible (8 slots = the 128-byte line a random gather
                                  costs on MI355X); 1 = packed                                  (8)    */
  int32_t flatten_closures;    /* precompute each state's whole epsilon closure (<= 4 paths)     (1)    */
  int32_t fuse_closures;       /* fold the epsilon closures into the expansion (pseudo arcs behind
                                  each state's emitting arcs) where the graph allows: no epsilon
                                  cycle, closures of <= 48 paths and <= 8 hops, no negative epsilon
                                  weight; best-path and lattice decoders then run no separate closure
                                  pass (lattice mode keeps one flat pass that lists the epsilon links) (1)    */
} wfst_graph_options;

/* Original on-disk / in-memory graph records of the reference format. */
typedef struct wfst_arc { int32_t ilabel, olabel; float weight; int32_t nextstate; } wfst_arc;   /* StdArc, newfst/arc.h:17-26 */
typedef struct wfst_state_info { uint32_t num_arcs, niepsilons, noepsilons; } wfst_state_info;   /* Fst::StateInfo, newfst/optimize-fst.h:220-225 */

void wfst_config_default(wfst_config *cfg);
void wfst_options_default(wfst_options *opt);
void wfst_graph_options_default(wfst_graph_options *opt);
const char *wfst_last_error(void);
int wfst_device_count(void);

/* ---- graph ------------------------------------------------------------------------------- */

/* Fst::ReadFst(const char*) (newfst/optimize-fst.h:208-280): reads the flat format
 * {start, final_state, total_states, total_arcs, total_niepsilons, total_noepsilons} int32,
 * StateInfo x S, StdArc x A and uploads it as CSR to `device`.
 * The same call also takes the OpenFst binary files the reference ingests (detected by the OpenFst
 * magic number): a CONST fst (ConstFst<StdArc,int>::Read + Fst(ConstFst), newfst/const-fst.h:118-245,
 * newfst/optimize-fst.h:82-134 -- what the service loads with --constfst=true) and a VECTOR fst
 * (fst_format_convert_tool/read_fst.c:11-187), both with the reference's super-final construction
 * (final weight on a leading <eps>:<eps> arc to one extra state).  WFST_E_FORMAT for embedded
 * symbol tables, non-"standard" arcs or other fst types (the reference readers misread those). */
int wfst_graph_load(const char *path, int device, wfst_graph **out);
int wfst_graph_load_ex(const char *path, int device, const wfst_graph_options *opt, wfst_graph **out);

/* convert_fst IN OUT (fst_format_convert_tool/convert_fst.c:5-27): read a graph file in any format
 * wfst_graph_load takes and write the flat format.  Host only -- needs no device. */
int wfst_graph_convert_file(const char *in_path, const char *flat_out_path);

/* Same from host arrays (what Fst holds after ReadFst or after Fst(ConstFst),
 * newfst/optimize-fst.h:82-134).  Requirements, checked: every state's input-epsilon arcs precede
 * its other arcs (the reference format guarantees it, fst_format_convert_tool/read_fst.c:110-135);
 * <= 4095 input-epsilon arcs and < 2^20 emitting arcs per state (WFST_E_FORMAT otherwise). */
int wfst_graph_from_arrays(int32_t start, int32_t final_state, int32_t n_states, int32_t n_arcs,
                           const wfst_state_info *states, const wfst_arc *arcs, int device,
                           wfst_graph **out);
int wfst_graph_from_arrays_ex(int32_t start, int32_t final_state, int32_t n_states, int32_t n_arcs,
                              const wfst_state_info *states, const wfst_arc *arcs, int device,
                              const wfst_graph_options *opt, wfst_graph **out);

/* Optional transition-id -> pdf map (Kaldi DecodableMatrixScaledMapped as used by
 * kaldi-nnet3bin/kaldi-hclg-my-decoder.cc:107; hmm/transition-model.h:52-61):
 * LogLikelihood(f, ilabel) = loglikes[f][tid2pdf[ilabel]].  tid2pdf has n_tid+1 entries, entry 0
 * unused.  Without a map, column = ilabel (a matrix with NumIndices()+1 columns). */
int wfst_graph_set_tid2pdf(wfst_graph *g, const int32_t *tid2pdf, int32_t n_tid);

int wfst_graph_info(const wfst_graph *g, int32_t *start, int32_t *final_state, int32_t *n_states,
                    int32_t *n_arcs, int64_t *device_bytes);
void wfst_graph_free(wfst_graph *g);

/* ---- language models (biglm: on-the-fly LM rescoring, BASELINE configs[3]) ----------------- */

/* Records of the reference's LM automaton (newlm/arpa2fsa.h:22-40,80-91 and arpa2fsa.cc:62-67). */
typedef struct wfst_lm_state { int32_t arc_num; float backoff_prob; int32_t backoff_id; } wfst_lm_state;
typedef struct wfst_lm_arc { int32_t wordid; float weight; int32_t tostateid; } wfst_lm_arc;

/* ArpaLm::Read (newlm/arpa2fsa.h:355-397 + Fsa::Read, newlm/arpa2fsa.cc:68-176) followed by
 * ArpaLm::Rescale(scale) (arpa2fsa.cc:264-275): reads the binary LM file arpa2fsa-bin writes
 * {i32 bos, eos, unk; u64 orders; i32 count[orders]; i32 n_states; {i32 arc_num, f32 backoff, i32
 * backoff_id} x n_states; i32 n_arcs; {i32 wordid, f32 weight, i32 tostate} x n_arcs} and uploads it
 * to `device`.  The biglm CLI loads the OLD LM (the one compiled into the HCLG) with scale -1 and the
 * NEW one with scale 1 (kaldi-nnet3bin/kaldi-hclg-my-decoder-biglm.cc:55-60).  Checked, WFST_E_FORMAT
 * otherwise: counts consistent with the file size, arcs of a state sorted by word id, state 0 holding
 * arc k for word id k, destinations in range, every back-off chain ending in state 0. */
int wfst_lm_load(const char *path, float scale, int device, wfst_lm **out);
int wfst_lm_from_arrays(int32_t bos, int32_t eos, int32_t unk, int32_t n_states, const wfst_lm_state *states,
                        int32_t n_arcs, const wfst_lm_arc *arcs, float scale, int device, wfst_lm **out);
int wfst_lm_info(const wfst_lm *lm, int32_t *bos, int32_t *eos, int32_t *n_states, int32_t *n_arcs,
                 int32_t *n_words /* arcs of the empty-history state */, int64_t *device_bytes);
/* The shape of the LM's device look-up table, as the upload left it: every arc of a state other than the empty history sits in one
 * open-addressed (state, word) table with linear probing.  table_size slots (a power of two), `used` of them occupied; longest_run
 * = the longest cyclic run of occupied slots; max_displacement = the farthest an entry sits past its home slot; wraps = 1 if an
 * occupied run covers both the last slot and slot 0.  Computed on the host at upload; any output pointer may be NULL.  For tests
 * and tuning: nothing a result depends on. */
int wfst_lm_table_stats(const wfst_lm *lm, int64_t *table_size, int32_t *used, int32_t *longest_run, int32_t *max_displacement,
                        int32_t *wraps);
void wfst_lm_free(wfst_lm *lm);

/* ---- decoder ----------------------------------------------------------------------------- */

/* Decoder(Fst*, const LatticeFasterDecoderConfig&) (my-decoder/online-decoder-base.h:95,
 * base-inl.h:22-30) for n_channels independent utterance slots.  `hip_stream` is a hipStream_t
 * (NULL = a stream owned by the decoder); all work is enqueued on it. */
int wfst_decoder_create(const wfst_graph *g, const wfst_config *cfg, int32_t n_channels,
                        const wfst_limits *limits, void *hip_stream, wfst_decoder **out);
/* Same with explicit scheduling options (at most 32767 channels per decoder). */
int wfst_decoder_create_ex(const wfst_graph *g, const wfst_config *cfg, int32_t n_channels,
                           const wfst_limits *limits, const wfst_options *options, void *hip_stream,
                           wfst_decoder **out);
/* OnlineLatticeDecoderMempoolBiglm(fst, config, oldlm, newlm) (my-decoder/online-decoder-mempool-base-
 * biglm.h:21-30): every arc with an output label is rescored on the fly with cost_new(word | history) -
 * cost_old(word | history); a token is identified by (graph state, LM pair state) (:77-90).  Both LMs must
 * be on the graph's device and stay alive as long as the decoder.  Each LM is walked from its OWN state
 * (DiffArpaLm with the pair's components; the reference text hands the pair id to both LMs,
 * newlm/diff-lm.h:80,86 -- see DESIGN.md).  With limits->lattice_links > 0 it is the LATTICE decoder it is in the reference
 * (the service asks a `biglm-hclg` decoder for GetRawLattice / GetLattice / n-best, kaldi-nnet3/kaldi-online-nnet3-my-decoder.cc:
 * 58,81,97-105): forward links carry graph cost = arc weight + LM difference (:377-392, :448-458), FinalizeDecoding prunes with
 * the LM's final costs (:160-215, 469-560), and -- as in the reference's GetRawLattice (base-inl.h:930-966) -- a raw lattice only
 * FLAGS its final states: the LM's final cost of a final token is not part of the lattice.
 * WFST_E_FORMAT if the graph has an output label the LMs' empty-history state has no arc for (the
 * reference indexes that state without a bounds check, newlm/arpa2fsa.h:211-214). */
int wfst_decoder_create_biglm(const wfst_graph *g, const wfst_config *cfg, int32_t n_channels,
                              const wfst_limits *limits, const wfst_options *options, const wfst_lm *old_lm,
                              const wfst_lm *new_lm, void *hip_stream, wfst_decoder **out);
void wfst_decoder_free(wfst_decoder *d);

/* InitDecoding() (base-inl.h:40-67) for the listed channels (channels == NULL: all). */
int wfst_decoder_init(wfst_decoder *d, const int32_t *channels, int32_t n);

/* AdvanceDecoding(decodable, max_num_frames) (base-inl.h:630-668) for the listed channels at
 * once.  For channel channels[i]: loglikes[i] is a DEVICE pointer to row 0 of the utterance's
 * row-major float32 matrix [frames][stride] of already-scaled log-likelihoods (what
 * LogLikelihood(frame, index) returns, itf/decodable-itf.h:71), n_frames_ready[i] is
 * NumFramesReady(); rows [0, n_frames_ready[i]) must stay valid and unchanged until the
 * channel's next wfst_decoder_init (GetBestPath reads acoustic costs back from them).
 * max_num_frames < 0: decode everything ready.  Returns after the work is ENQUEUED on the stream;
 * use wfst_decoder_sync or any result getter to wait. */
int wfst_decoder_advance(wfst_decoder *d, const int32_t *channels, int32_t n,
                         const float *const *loglikes, const int32_t *n_frames_ready,
                         int32_t stride, int32_t max_num_frames);

/* Same with HOST matrices: rows [NumFramesDecoded, n_frames_ready) are copied into a device
 * history buffer owned by the channel (the shape a DecodableInterface-pulling caller needs).
 * PAGEABLE buffers are consumed when the call returns; a long hand-over is uploaded and decoded in
 * slices, so that the copy of one slice overlaps the search over the previous one.
 * PAGE-LOCKED buffers (wfst_host_alloc; every listed channel's): the rows go up by DMA and the call
 * returns when copies and frames are ENQUEUED, like wfst_decoder_advance -- the rows handed over must
 * stay valid and unchanged until they are decoded (wfst_decoder_sync or any result getter of the
 * channel); a host that hands over chunk after chunk keeps enqueueing while the device decodes.
 * Page-locked matrices of CONSECUTIVE listed channels that lie equally spaced in host memory (one block of utterances; slots of one
 * allocation) and hand over the same frames go up as ONE 2-D copy per run of such channels: list the channels in ascending order.
 * (The device histories of all channels are one allocation, n_channels x the longest hand-over so far, at most max_frames rows.) */
int wfst_decoder_advance_host(wfst_decoder *d, const int32_t *channels, int32_t n,
                              const float *const *loglikes_host, const int32_t *n_frames_ready,
                              int32_t stride, int32_t max_num_frames);

/* Page-locked host memory for the matrices handed to wfst_decoder_advance_host: rows in it go to the device at the link's rate
 * and without a staging copy (pageable rows work too, at a fraction of it).  NULL when the allocation fails.  The host mirror's
 * GpuLatticeDecoder keeps the rows it pulls from a DecodableInterface in such a buffer. */
void *wfst_host_alloc(size_t bytes);
void wfst_host_free(void *p);

/* FinalizeDecoding() (base-inl.h:829-847): marks the channels finalized (afterwards advance is an
 * error and get_best_path requires use_final_probs != 0, as in the reference). */
int wfst_decoder_finalize(wfst_decoder *d, const int32_t *channels, int32_t n);

/* Blocks until everything enqueued so far has run; returns WFST_E_CAPACITY / WFST_E_DEVICE if a
 * channel hit a limit or the device faulted. */
int wfst_decoder_sync(wfst_decoder *d);

/* 1 while work enqueued on the decoder's stream has not finished, 0 when it is idle (never blocks); < 0: error. */
int wfst_decoder_busy(wfst_decoder *d);

/* How many of the decoder's enqueued wfst_decoder_advance[_host] calls -- calls that brought frames; an init or finalize between two
 * of them is not counted -- have not finished yet (0 ... 16: the marks of the newest sixteen calls are looked at; never blocks);
 * < 0: error.  The depth of the device's backlog, for a batching host that hands over chunk after chunk (the host mirror's
 * GpuChannelPool): with three calls outstanding the next one would wait inside the library for the device (the staging sets of the
 * targets and row pointers are used in rotation), and while the device has work behind the call it is running, requests that arrive
 * can still join the next call for nothing; with one or none outstanding it is about to run dry. */
int wfst_decoder_calls_in_flight(wfst_decoder *d);

/* NumFramesDecoded() (my-decoder/online-decoder-base.h:139). */
int wfst_decoder_num_frames_decoded(wfst_decoder *d, int32_t channel);

/* GetBestPath(Lattice*, use_final_probs) (base-inl.h:1071-1094) for every listed channel at once.
 * The linear best-path lattice is returned hop by hop in start->final order, exactly the arcs the
 * reference's Lattice holds (first hop is the (0,0,One) arc of the root token): for channel
 * channels[i], hops are written to ilabel/olabel/graph_cost/acoustic_cost + i*cap, their number
 * to n_hops[i] (0 = the reference's `return false`: no frames decoded or no surviving token).
 * If a path is longer than cap, n_hops[i] is the needed size and WFST_E_CAPACITY is returned. */
int wfst_decoder_get_best_path(wfst_decoder *d, const int32_t *channels, int32_t n,
                               int32_t use_final_probs, int32_t cap, int32_t *ilabel,
                               int32_t *olabel, float *graph_cost, float *acoustic_cost,
                               int32_t *n_hops);

/* GetBestPath of a channel LIST in two halves, for a host that batches many decoder objects over one decoder (the C++ mirror's
 * GpuChannelPool): _enqueue puts the traceback and the copies on the decoder's results stream behind the listed channels' own
 * enqueued work and returns at once; _ready says (never blocks) whether the results have landed; _fetch waits if need be and
 * writes them out -- same outputs, for the enqueued list and capacity, as wfst_decoder_get_best_path, which for a list is the two
 * halves one behind the other.  One request may be outstanding per decoder (a second _enqueue: WFST_E_STATE); the listed channels
 * must not be advanced or initialised in between.  A device error of another channel's utterance does not fail the request. */
int wfst_decoder_best_path_enqueue(wfst_decoder *d, const int32_t *channels, int32_t n, int32_t use_final_probs, int32_t cap);
int wfst_decoder_best_path_ready(wfst_decoder *d);
int wfst_decoder_best_path_fetch(wfst_decoder *d, int32_t *ilabel, int32_t *olabel, float *graph_cost, float *acoustic_cost,
                                 int32_t *n_hops);

/* LatticeToVector (newfst/lattice-functions.cc:179-217) on one hop list: nonzero olabels ->
 * words, nonzero ilabels -> transition-ids, lm = sum graph, tot = sum (graph + acoustic), float
 * accumulation in forward order.  Host-only helper; returns the counts through n_words/n_tids. */
int wfst_lattice_to_vector(const int32_t *ilabel, const int32_t *olabel, const float *graph_cost,
                           const float *acoustic_cost, int32_t n_hops, int32_t *words,
                           int32_t max_words, int32_t *n_words, int32_t *tids, int32_t max_tids,
                           int32_t *n_tids, float *tot_score, float *lm_score);

/* The same for a batch of hop lists laid out as wfst_decoder_get_best_path returns them ([n_paths][cap] arrays, n_hops per
 * path): tot_score / lm_score of every path (the sequential float sums of LatticeToVector) and the number of words and
 * transition-ids in it.  Host-only. */
int wfst_lattice_to_vector_batch(const int32_t *ilabel, const int32_t *olabel, const float *graph_cost,
                                 const float *acoustic_cost, const int32_t *n_hops, int32_t n_paths, int32_t cap,
                                 float *tot_score, float *lm_score, int32_t *n_words, int32_t *n_tids);

/* The label half of LatticeToVector for the same batch layout: the nonzero olabels (words) and ilabels (transition-ids) of
 * every path in hop order, packed path after path -- path p's words are words[word_off[p] .. word_off[p + 1]).  words / tids
 * hold the sums of wfst_lattice_to_vector_batch's n_words / n_tids (at most n_paths * cap), the offset arrays n_paths + 1
 * entries.  Host-only. */
int wfst_lattice_labels_batch(const int32_t *ilabel, const int32_t *olabel, const int32_t *n_hops, int32_t n_paths, int32_t cap,
                              int32_t *words, int32_t *word_off, int32_t *tids, int32_t *tid_off);

/* Per-channel work counters since the last init: {frames, N tokens expanded, E emitting arcs
 * traversed, Z epsilon arcs traversed, tokens kept, peak tokens per frame, candidate records
 * bucketed, forward links recorded (lattice mode) / token collections run (best-path mode)}.  N and E follow the
 * definitions of the reference loop (base-inl.h:311-347). */
int wfst_decoder_get_stats(wfst_decoder *d, int32_t channel, int64_t stats[8]);

/* GetRawLattice(Lattice*, use_final_probs) (base-inl.h:869-975) of a channel of a decoder created in
 * lattice mode (wfst_limits.lattice_links > 0).  After FinalizeDecoding: the state-level lattice that is
 * left after its lattice_beam pruning (base-inl.h:725-847).  MID-UTTERANCE (any time after InitDecoding, as
 * the service asks for it: kaldi-nnet3/kaldi-online-nnet3-my-decoder.cc:58,81): everything alive right now
 * -- the history as the last PruneActiveTokens pass left it plus the raw frames since.  One documented
 * deviation there: the running passes judge "extra costs moved by more than lattice_beam * prune_scale" on
 * each frame's exact fixpoint, the reference sweep by sweep over its token list, so a pass may stop walking
 * back at another frame than the reference's and a mid-utterance lattice may hold a few links more or fewer
 * than the reference's at that moment (it equals the order-free oracle's, DESIGN.md section 4 deviation 7);
 * after FinalizeDecoding (delta 0 in the reference too) the lattices are identical.  States are numbered frame
 * by frame in a topological order (every arc goes to a higher id; state 0 is the start), like the
 * reference's TopSortTokens; the numbering inside a frame is implementation defined there too.
 * Per state: final flag, frame, graph state id, forward cost; per arc (sorted by source):
 * source, destination, ilabel, olabel, graph cost, acoustic cost.  If a capacity is too small the
 * needed sizes are returned in n_states/n_arcs with WFST_E_CAPACITY.  n_states == 0 with WFST_OK is
 * the reference's `return false` (no frames decoded, no token alive, or use_final_probs == 0 after
 * FinalizeDecoding). */
int wfst_decoder_get_raw_lattice(wfst_decoder *d, int32_t channel, int32_t use_final_probs,
                                 int32_t cap_states, int32_t cap_arcs, int32_t *n_states,
                                 int32_t *n_arcs, int32_t *st_final, int32_t *st_frame,
                                 int32_t *st_state, float *st_cost, int32_t *a_src, int32_t *a_dst,
                                 int32_t *a_ilabel, int32_t *a_olabel, float *a_graph, float *a_acoustic);

/* GetLattice ahead of its request: sends the finalized channels that have no determinized lattice yet to the determinizer
 * NOW, on a side stream, and returns at once (the determinizer is one lane per lattice and a launch lasts as long as its
 * largest lattice -- tens of milliseconds during which the device is all but idle).  wfst_decoder_get_best_path and
 * wfst_decoder_get_nbest served meanwhile run beside it; the first wfst_decoder_get_determinized_lattice (or batched
 * post-processing call) finds the work done or waits for it.  Results and errors are those of the calls that fetch: this
 * call changes when the work is done, not what it gives (kaldi-online-nnet3-my-decoder.cc:50-105 asks for the best path,
 * the n-best list and the lattice of a finished utterance one after the other).  One launch's worth of channels
 * (wfst_limits.det_workspace_bytes); the rest are determinized on request.  wfst_decoder_init / _advance / _finalize wait for
 * a prefetch in flight. */
int wfst_decoder_prefetch_determinized(wfst_decoder *d);

/* ... DETACHED: for a service that refills its channels at once.  The part of the determinizer that reads the channels' state
 * (a fraction of a millisecond) runs on the decoder's stream; the subset construction runs on a stream of its own, on the
 * determinizer's workspace alone, and wfst_decoder_init / _advance / _finalize do NOT wait for it: the channels decode their next
 * utterances beside it.  The lattices -- those of the utterances the channels had finalized at this call -- are kept per
 * channel and fetched with wfst_decoder_get_prefetched_lattice once harvested (by the next prefetch call, or by
 * wfst_decoder_harvest_prefetched), until the harvest after that; a channel that still holds the very utterance also serves them through
 * wfst_decoder_get_determinized_lattice.  The side stream is one more HIP stream of the process: with the runtime's default of
 * four hardware queues it can end up sharing a queue with a channel group's stream, whose launches then wait behind the
 * determinizer. */
int wfst_decoder_prefetch_determinized_detached(wfst_decoder *d);
/* GetLattice AND GetNbest ahead of their requests, as the service runs them one behind the other (kaldi-nnet3/kaldi-online-nnet3-
 * my-decoder.cc:97-105: NShortestPath on the lattice DeterminizeLatticeWrapper returned): like wfst_decoder_prefetch_determinized
 * (detached = 0) / _detached (detached != 0), with the n_paths (<= 64) cheapest paths of every lattice computed right behind the
 * determinizer on its stream.  detached = 0: wfst_decoder_get_nbest_paths(channel, n_paths, 1, NULL, NULL, ...) then finds the work
 * done; detached: wfst_decoder_get_prefetched_nbest_paths once harvested (same outputs; WFST_E_STATE where the channel's lattice
 * was not covered or was larger than the prefetch's n-best takes -- 4096 states / 8192 arcs: ask for it alone then). */
int wfst_decoder_prefetch_nbest(wfst_decoder *d, int32_t n_paths, int32_t detached);
int wfst_decoder_get_prefetched_nbest_paths(wfst_decoder *d, int32_t channel, int32_t cap_paths, int32_t cap_arcs, int32_t *n_paths,
                                            int32_t *total_arcs, int32_t *path_off, float *path_tot, int32_t *a_olabel, float *a_graph,
                                            float *a_acoustic);

/* Waits for a prefetch in flight and takes its lattices over -- what the next prefetch (or any other use of the determinizer)
 * does by itself; for the last utterance of a stream of them.  wfst_decoder_get_prefetched_lattice returns the lattices of the
 * last HARVESTED detached prefetch and never waits: right behind the call that started utterance k's determinization it returns
 * utterance k - 1's. */
int wfst_decoder_harvest_prefetched(wfst_decoder *d);
int wfst_decoder_get_prefetched_lattice(wfst_decoder *d, int32_t channel, int32_t cap_states, int32_t cap_arcs,
                                        int32_t *n_states, int32_t *n_arcs, int32_t *st_final, int32_t *a_src, int32_t *a_dst,
                                        int32_t *a_ilabel, int32_t *a_olabel, float *a_graph, float *a_acoustic);

/* GetLattice(Lattice*, use_final_probs) (base-inl.h:850-866) = GetRawLattice + DeterminizeLatticeWrapper
 * (newfst/lattice-determinize-api.cc:5-21: Invert, ArcSort, LatticeDeterminizer::Determinize in the (graph,
 * acoustic) lattice semiring, OutputNoolabel, Invert): the word-level deterministic lattice, built on the
 * device from the raw lattice resident there.  Lattice-mode decoders; finalized channels (the first call
 * determinizes every finalized channel of the batch at once) or mid-utterance.  State 0 is the start; arcs
 * carry ilabel 0 and olabel = word; a final weight is an <eps>:<eps> arc into a final state of its own
 * (OutputNoolabel, lattice-determinize.h:307-377).  Arc for arc (as a multiset: labels and float costs bit for
 * bit) what the reference's determinizer makes of the same raw lattice.  n_states == 0 with WFST_OK: no
 * lattice (as wfst_decoder_get_raw_lattice).  WFST_E_CAPACITY: output larger than the given capacities (sizes
 * returned), or the subset construction outgrew its workspace (the reference's unpruned determinizer has no
 * bound either: DeterminizeLatticeOptions::_max_mem). */
int wfst_decoder_get_determinized_lattice(wfst_decoder *d, int32_t channel, int32_t use_final_probs,
                                          int32_t cap_states, int32_t cap_arcs, int32_t *n_states, int32_t *n_arcs,
                                          int32_t *st_final, int32_t *a_src, int32_t *a_dst, int32_t *a_ilabel,
                                          int32_t *a_olabel, float *a_graph, float *a_acoustic);

/* GetLattice of the service with --use-second (OnlineClgLatticeFastDecoder::GetLattice, kaldi-nnet3/kaldi-online-nnet3-my-decoder.cc:
 * 50-78): the determinized lattice composed with the OLD LM (loaded with scale -1: its scores are taken out) and then with the NEW
 * one -- ComposeLattice twice (newfst/compose-lat-inl.h:15-130: pairs (lattice state, LM state) breadth first, a word-labelled arc
 * steps ComposeArpaLm and adds its cost, an arc into a final state adds the LM's final cost and makes the composed state final),
 * each followed by Connect -- on the device, over the determinized lattice resident there and the LM automata in HBM.  Outputs as
 * wfst_decoder_get_determinized_lattice (st_final here marks the composed final states).  One channel per call.
 * THE LABEL CHECK of every call that takes an LM pair for the second pass (this one, wfst_decoder_get_nbest_paths,
 * wfst_decoder_rescore_lattices, wfst_decoder_nbest_paths_batch, wfst_decoder_get_nbest_words): the rule of
 * wfst_decoder_create_biglm -- the decoder's graph has no negative output label and its largest one is below the arc count of both
 * LMs' empty-history states (wfst_lm_info's n_words); WFST_E_FORMAT otherwise, before any device work, and what the decoder holds
 * for the channel stays as it was.  (The empty-history state is indexed by word id without a bound, arpa2fsa.cc:253-254.) */
int wfst_decoder_get_rescored_lattice(wfst_decoder *d, int32_t channel, int32_t use_final_probs, const wfst_lm *old_lm,
                                      const wfst_lm *new_lm, int32_t cap_states, int32_t cap_arcs, int32_t *n_states,
                                      int32_t *n_arcs, int32_t *st_final, int32_t *a_src, int32_t *a_dst, int32_t *a_ilabel,
                                      int32_t *a_olabel, float *a_graph, float *a_acoustic);

/* GetNbest of the service as it is defined (OnlineClgLatticeFastDecoder::GetNbest, kaldi-nnet3/kaldi-online-nnet3-my-decoder.cc:97-105):
 * NShortestPath (newfst/lattice-to-nbest.cc:15-147) over the lattice GetLattice returns -- the determinized lattice, or with
 * old_lm / new_lm (both or neither) its second-pass rescoring -- each path with the lattice's own arcs on it, as
 * ConvertNbestToVector (:149-199) hands them out: path i = arcs path_off[i] .. path_off[i + 1] of a_olabel / a_graph /
 * a_acoustic, front to back (word or 0, and both costs, of every arc; the last arc of a path is the final weight's
 * <eps>:<eps> arc), path_tot[i] its cost (arc costs added front to back in float, as NShortestPath adds them), paths in
 * ascending cost.  On the device: a k-best dynamic program over the lattice resident there; any n up to 4096 (the reference has
 * no bound; wfst_decoder_get_nbest above is the batched short-list form on the raw lattice, n <= 16, words and totals only).
 * A determinized lattice has one path per word sequence, so the paths are distinct word sequences.  One channel per call;
 * finalized channels or mid-utterance.  *n_paths == 0 with WFST_OK: no lattice.  WFST_E_CAPACITY: more paths / arcs than the
 * given capacities (the sizes are returned), or n paths over this lattice outgrow the path workspace. */
int wfst_decoder_get_nbest_paths(wfst_decoder *d, int32_t channel, int32_t n, int32_t use_final_probs, const wfst_lm *old_lm,
                                 const wfst_lm *new_lm, int32_t cap_paths, int32_t cap_arcs, int32_t *n_paths, int32_t *total_arcs,
                                 int32_t *path_off, float *path_tot, int32_t *a_olabel, float *a_graph, float *a_acoustic);

/* The service's post-processing as a BATCH.  The reference runs GetLattice (+ the second LM pass under --use-second) and GetNbest per
 * utterance, one worker thread each, concurrently (kaldi-nnet3/kaldi-online-nnet3-my-decoder.cc:50-105, v2-asr/v2-asr-work-thread.h:66);
 * here the listed FINALIZED channels (NULL: every finalized channel) are determinized, composed with the two LMs
 * (newfst/compose-lat-inl.h:15-130, twice) and -- the second call -- searched for their n cheapest paths (newfst/lattice-to-nbest.cc)
 * in ONE launch each, a workgroup per lattice, and the results are fetched once: the per-channel calls
 * wfst_decoder_get_rescored_lattice / wfst_decoder_get_nbest_paths with the same arguments then return them without device work
 * (until the channel is initialised again).  old_lm / new_lm of the second call: both NULL = the paths of the determinized lattice.
 * WFST_E_STATE for a channel that is not finalized (mid-utterance requests: the per-channel calls). */
int wfst_decoder_rescore_lattices(wfst_decoder *d, const int32_t *channels, int32_t n, int32_t use_final_probs, const wfst_lm *old_lm,
                                  const wfst_lm *new_lm);
int wfst_decoder_nbest_paths_batch(wfst_decoder *d, const int32_t *channels, int32_t n, int32_t n_paths, int32_t use_final_probs,
                                   const wfst_lm *old_lm, const wfst_lm *new_lm);

/* ---- n-best TEXT of a channel list, mid-utterance included -----------------------------------------------------------------
 * The service's per-chunk GetNbestTxt (kaldi-nnet3/kaldi-online-nnet3-my-decoder.cc:139-150, called with end_of_utterance = false
 * from v2-asr/v2-asr-task.h:298-319): GetLattice (raw lattice, DeterminizeLatticeWrapper, under --use-second ComposeLattice x 2),
 * NShortestPath, then OnebestLatticeToString per path -- for a LIST of channels, live (initialised, not finalized) and finalized
 * ones mixed, in one launch per stage: the live channels' lattices emitted, all determinized, composed with the LM pair if one is
 * given, their n cheapest paths found, and the paths turned into text on the device (nbest_words_kernel), so that words and three
 * floats per path cross the link instead of every arc of every path.
 *
 * For listed channel i and path k, with P = what wfst_decoder_get_nbest_paths(channels[i], n_paths, use_final_probs, old_lm, new_lm,
 * ...) returns at this moment: got_paths[i] = P's *n_paths; path_tot[i][k] = P's path_tot[k], bit for bit; words[i][k][..] = the
 * non-zero a_olabel of path k in order, n_words[i][k] of them; tot_score / lm_score[i][k] = bit for bit what wfst_lattice_to_vector
 * returns for path k's arcs (float sums in arc order).  A finalized channel with use_final_probs == 0 has no lattice (got_paths 0,
 * status WFST_OK, as GetRawLattice has it); so has a channel with no frame decoded.  Entries of paths k >= got_paths[i] are zero.
 *
 * A failure of ONE channel does not fail the list: the call returns WFST_OK and status[i] carries the channel's own error code with
 * got_paths[i] = 0 (wfst_last_error() then holds the message of the last such channel, although the call succeeded) -- a lattice beyond the determinizer's, the composition's or the n-best search's batch limits (WFST_E_CAPACITY),
 * a device error of that channel's utterance.  More words on a path than cap_words: status[i] = WFST_E_CAPACITY, n_words[i][k] is
 * the needed size and the first cap_words words are written (got_paths[i] stays).
 * The call itself fails, before any device work, with WFST_E_ARG (n_paths outside 1..64, one LM without the other, an LM on
 * another device, a bad or duplicate list, cap_words <= 0) or WFST_E_STATE (a decoder without lattice_links, a listed channel never
 * initialised).  Any output pointer may be NULL.  Lists longer than the determinizer's workspace slots are taken in rounds.
 * What the per-channel getters and the prefetch keep for the same channels is untouched: they answer afterwards what they would
 * have answered without this call.
 * Synchronous, and deliberately without enqueue / ready / fetch halves: the stages exchange their sizes through the host (the
 * determinizer's result words size the composition's and the search's workspaces), and unpicking that is a change of its own. */
int wfst_decoder_get_nbest_words(wfst_decoder *d, const int32_t *channels, int32_t n, int32_t n_paths /* 1..64 */,
                                 int32_t use_final_probs, const wfst_lm *old_lm, const wfst_lm *new_lm, int32_t cap_words,
                                 int32_t *status /* [n] */, int32_t *got_paths /* [n] */, int32_t *n_words /* [n][n_paths] */,
                                 int32_t *words /* [n][n_paths][cap_words] */, float *tot_score, float *lm_score /* [n][n_paths] */,
                                 float *path_tot /* [n][n_paths] */);

/* How many lattices ONE launch of the determinizer (and of the stages behind it) takes -- the workspace slots that
 * wfst_limits.det_workspace_bytes buys, at most one per channel -- and the bytes one slot takes; a longer list goes in rounds.
 * Allocates the workspace if no call has yet.  Either output may be NULL.  WFST_E_STATE: a decoder without lattice_links. */
int wfst_decoder_get_determinizer_slots(wfst_decoder *d, int32_t *slots, int64_t *bytes_per_slot);

/* ---- pruned live lattices: FinalizeDecoding's pruning on a snapshot ------------------------------------------------------------
 * A live raw lattice is the history as the last PruneActiveTokens pass left it plus up to prune_interval frames of unpruned tokens,
 * of which a percent or two survive any lattice-beam pruning: at the headline configuration it is mostly beyond the determinizer's
 * bounds (wfst_limits.det_raw_states / det_raw_arcs).  mode 1 makes every getter that emits a LIVE channel's lattice --
 * wfst_decoder_get_raw_lattice, _get_determinized_lattice, _get_rescored_lattice, _get_nbest_paths, _get_nbest_words, _get_nbest --
 * work from the SNAPSHOT lattice S(channel, use_final_probs) instead:
 *   use_final_probs != 0: exactly the raw lattice a twin channel fed the same frames holds after wfst_decoder_finalize -- the pruning
 *     of FinalizeDecoding (PruneForwardLinksFinal + PruneForwardLinks + PruneTokensForFrame, my-decoder/online-decoder-base-inl.h:725-847):
 *     the same states (frame, graph state, final flag, forward cost bits), the same arcs (labels and both costs bit for bit), the same
 *     numbering rules;
 *   use_final_probs == 0: the same computation with every token of the newest frame final at cost 0 (what ComputeFinalCosts yields
 *     when no token of that frame is final in the graph); st_final is set on every surviving token of the newest frame.
 * The channel is NOT changed by it: the pruning is priced into scratch of its own and decoding goes on bit for bit as without the
 * query.  Finalized channels are served exactly as with mode 0 (the default: everything alive, as before).
 * The one thing that differs from the reference: its GetLattice(..., false) (kaldi-nnet3/kaldi-online-nnet3-my-decoder.cc:50-89)
 * determinizes the UNPRUNED live lattice; mode 1 determinizes S.
 * The scratch (8 bytes per arena entry of every channel) is allocated when mode 1 is first set and freed with the decoder; if it
 * cannot be allocated the setter returns the error (WFST_E_CAPACITY / WFST_E_DEVICE) and the mode stays 0.  Changing the mode drops
 * what the decoder keeps of live channels' lattices, so that no getter answers from the other mode's lattice; what it keeps of
 * finalized channels stays.  The setting is the decoder's: set it before other threads use the decoder.
 * WFST_E_STATE: a decoder without lattice_links.  WFST_E_ARG: a mode outside {0, 1}, a NULL decoder.
 * 0 (default): live getters serve everything alive, as today.  1: they serve S(c, use_final_probs). */
int wfst_decoder_set_live_lattice_prune(wfst_decoder *d, int32_t mode);
/* Either output may be NULL; scratch_bytes is 0 until mode 1 has been set once. */
int wfst_decoder_get_live_lattice_prune(wfst_decoder *d, int32_t *mode, int64_t *scratch_bytes);

/* ---- lattice-constrained word alignment: word times for any n-best path ---------------------------------------------------------
 * The services hand a client (start, end) per word for the first-pass best path only (AlignStruct, gpu-asr/gpu-worker-pool-itf.h:85-97:
 * wfst_decoder_get_words here).  The determinizer drops the input labels (OutputNoolabel), so the paths of GetNbestTxt
 * (kaldi-nnet3/kaldi-online-nnet3-my-decoder.cc:139-150) and the rescored 1-best a --use-second deployment returns (:122-130) are
 * words and costs without times.  This call puts them back: given a word sequence, the cheapest path of the channel's RAW lattice
 * that spells it, with that path's word times and scores -- for a list of channels, live and finalized ones mixed, n_seqs sequences
 * per channel, one launch per stage (the live channels' lattices emitted, the in-arc index of every lattice built once, one
 * dynamic program per (channel, sequence): align_index_kernel / align_kernel).
 *
 * The lattice R = what wfst_decoder_get_raw_lattice(channel, use_final_probs) returns at this moment (wfst_decoder_set_live_lattice_prune,
 * the use_final_probs rule after FinalizeDecoding and "no lattice" honoured): every arc goes to a higher state id, state 0 is the
 * start, final states are flagged and carry no weight.
 * The recurrence, for a sequence w[0..L) of word ids > 0: d[0][0] = 0.0f; every arc a = (s -> t, ilabel, olabel, graph, acoustic)
 * takes (s, k) to (t, k) if olabel == 0 and to (t, k + 1) if k < L and olabel == w[k] -- no other transition -- with
 *   d[t][k'] = min(d[t][k'], d[s][k] + (graph + acoustic)),
 * all in float32, graph + acoustic rounded first and then added (LatticeToVector's tot += graph + acoustic); a total of zero is +0,
 * and a total that is not finite is no path.  The answer ends in the final state e with the least d[e][L]; found = 0 if no final
 * state has one.  The path is recovered backwards: at (t, k') an in-arc with d[s][k] + (graph + acoustic) == d[t][k'].
 * The tie rule does not depend on the numbering of states or arcs: among several such in-arcs the least wins under (emitting before
 * epsilon, graph state of the source token, ilabel, olabel, bits of graph, bits of acoustic -- the float's 32 bits as an unsigned
 * number); among several best final states the least graph state.  On biglm lattices two tokens of a frame may share a graph
 * state: a tie that survives the rule is unspecified there.
 *
 * Per listed channel i and sequence q (seq_len[i][q] words at seq_words[i][q][..]; -1: skipped, all outputs zero): found[i][q];
 * n_arcs[i][q] arcs on the path; tot_score = d[e][L]; lm_score = the float32 sum of graph along the path in arc order; per word k
 * begin_frame[i][q][k] = the frame of the source state of the arc that carries the word, and end_frame[i][q][k] (exclusive) by
 * wfst_decoder_get_words' own definition with the aligned path's arcs as its hops: the next word's begin, the end state's frame for the
 * last word; with a silence list (wfst_decoder_set_silence_phones) one past the last non-silence emitting arc of the word's span,
 * begin_frame[i][q][k] if there is none.  The empty sequence (seq_len 0) is found where a path without words is.
 *
 * A failure of ONE channel goes into status[i] with found[i][..] = 0 and the call still returns WFST_OK: a sequence whose table of
 * states x (seq_len + 1) cells is beyond max_cells (WFST_E_CAPACITY), a device error of that channel's utterance.  max_cells = 0 is
 * the default, 65 536 states (the determinizer's own default bound) x 65: a table takes 4 bytes per cell and 4 bytes per state of path
 * scratch, 16.5 MiB per sequence at that bound; the index takes 32 bytes per arc and 8 per state of a listed lattice.  The workspace is
 * sized from the emitted lattices and the sequences, allocated by the first call, kept with the decoder; lists whose tables pass
 * 256 MiB together are taken in rounds.
 * The call itself fails, before any device work, with WFST_E_ARG (n_seqs outside 1..64, cap_words <= 0, a seq_len above cap_words, a
 * word id <= 0 inside a sequence, a bad or duplicate channel list, NULL sequences) or WFST_E_STATE (a decoder without lattice_links, a
 * listed channel never initialised).  Any output pointer may be NULL.  The decoder's state is only read: decoding goes on bit for bit
 * as without the call, and what the other getters keep for the same channels answers afterwards what it would have answered.
 * Synchronous, as wfst_decoder_get_nbest_words is and for the same reason: the lattices' sizes pass through the host. */
int wfst_decoder_align_words(wfst_decoder *d, const int32_t *channels, int32_t n, int32_t use_final_probs,
                             int32_t n_seqs /* per channel, 1..64 */, int32_t cap_words,
                             const int32_t *seq_words /* [n][n_seqs][cap_words] */, const int32_t *seq_len /* [n][n_seqs], -1 = skip */,
                             int64_t max_cells /* states x (len + 1) per sequence; 0 = default */,
                             int32_t *status /* [n] */, int32_t *found, int32_t *n_arcs /* [n][n_seqs] */,
                             int32_t *begin_frame, int32_t *end_frame /* [n][n_seqs][cap_words] */,
                             float *tot_score, float *lm_score /* [n][n_seqs] */);

/* ---- lattice edit distance: the lattice path nearest a transcript ----------------------------------------------------------------
 * wfst_decoder_align_words is all or nothing: for a transcript that is nearly in the lattice (a human transcript with one wrong word, a
 * caption file, another system's hypothesis) it answers found = 0.  This call answers with the path of the channel's RAW lattice
 * nearest a reference word sequence: the least word edit distance between any lattice path and the reference -- the lattice's oracle
 * error, Kaldi's lattice-oracle figure beside the 1-best WER that kaldi-bin/bin/nbest-compute-wer.cc:111-167 counts, the measure of what
 * lattice_beam, prune_interval, the live-prune mode or a degraded frame leave in a lattice -- and, among the paths at that distance, the
 * cheapest, with its edit operations and (begin, end) per word: lightly supervised alignment.  For a list of channels, live and
 * finalized ones mixed, n_refs references per channel, one launch per stage (the live channels' lattices emitted, align_index_kernel,
 * one dynamic program per (channel, reference): nearest_kernel).
 *
 * The lattice R = what wfst_decoder_get_raw_lattice(channel, use_final_probs) returns at this moment (wfst_decoder_set_live_lattice_prune,
 * the use_final_probs rule after FinalizeDecoding and "no lattice" honoured exactly as wfst_decoder_align_words states them): every arc
 * goes to a higher state id, state 0 is the start, final states are flagged and carry no weight.
 * The cells, for a reference r[0..L) of word ids > 0: v[s][k] = (e, d), int errors and a float32 cost, ordered lexicographically (e
 * first, then d as floats); a cell not reached is greater than every other.  v[0][0] = (0, +0.0f).  With c(a) = graph + acoustic,
 * rounded first, and d' = (d + c(a)) + 0.0f -- a d' that is not finite is no transition (wfst_decoder_align_words' rules) -- the
 * transitions are, and there are no others:
 *   free                  (s, k) -> (t, k)     over an arc a with olabel == 0:           (e, d')
 *   match / substitution  (s, k) -> (t, k + 1) over an arc a with olabel != 0, k < L:    (e + (olabel != r[k]), d')
 *   insertion             (s, k) -> (t, k)     over an arc a with olabel != 0:           (e + 1, d')   (a lattice word the reference lacks)
 *   deletion              (s, k) -> (s, k + 1) with k < L:                               (e + 1, d)    (a reference word no arc carries)
 * and v[t][k'] is the minimum over all arrivals.  The kinds go by OLABEL, not by ilabel: a word may sit on an epsilon arc.  Float
 * addition is monotone, so v[t][k'] is the minimum over the paths p from (0, 0) of (Levenshtein(words(p), r[0..k')), the sequential
 * float32 sum of c along p).  The answer ends in the final state e with the least v[e][L], the least graph state among equals;
 * found = 0 only if no final state is reached at all.
 * The traceback runs backwards from (e, L) to (0, 0) by exact equality of both halves of the cell.  Among several qualifying
 * predecessors the least key wins; the key's first part is the kind order -- 0: match / substitution, from (s, k - 1); 1: free arc,
 * from (s, k); 2: insertion, from (s, k); 3: the deletion step, from (t, k - 1) -- and for the arc kinds wfst_decoder_align_words' tuple
 * follows: ilabel == 0 last, graph state of the source token, ilabel, olabel, bits of graph, bits of acoustic.  Nothing depends on the
 * numbering of states or arcs.  On biglm lattices two tokens of a frame may share a graph state: a tie that survives the rule is
 * unspecified there.
 *
 * Per listed channel i and reference q (ref_len[i][q] words at ref_words[i][q][..]; -1: skipped, all outputs zero): found; n_err = e;
 * n_cor, n_sub, n_ins, n_del counted along the traceback (sub + ins + del == n_err, cor + sub + del == L, cor + sub + ins == n_hyp);
 * n_arcs; n_hyp and hyp_words[i][q][..], the non-zero olabels of the path in order; begin_frame / end_frame[i][q][j] per HYPOTHESIS word
 * by wfst_decoder_align_words' own definition over the path's arcs (the list of wfst_decoder_set_silence_phones included);
 * ref_hyp[i][q][k], for reference word k the index of the hypothesis word it was matched or substituted with, -1 if it was deleted --
 * strictly increasing over its non-negative entries: how a caller reads the transcript's own word times; tot_score = d; lm_score =
 * the float32 sum of graph along the path in arc order.
 *
 * A failure of ONE channel goes into status[i] and the call still returns WFST_OK: a reference whose table of states x (ref_len + 1)
 * cells is beyond max_cells (WFST_E_CAPACITY, found[i][..] = 0), a device error of that channel's utterance (likewise), or a path with
 * n_hyp > cap_hyp (WFST_E_CAPACITY: n_hyp is the room needed, the first cap_hyp words and times are written as
 * wfst_decoder_get_nbest_words does, and everything else of the channel's answers stands).  max_cells = 0 is
 * wfst_decoder_align_words' default bound, 65 536 states x 65 cells.  A cell is 8 bytes here (errors in the high word, the cost's
 * orderable float bits in the low word: one unsigned 64-bit minimum): 32.5 MiB of table per reference at that bound.  The workspace is
 * the decoder's, shared with wfst_decoder_align_words and grown on demand; lists whose tables pass 256 MiB together are taken in rounds.
 * The call itself fails, before any device work, with WFST_E_ARG (n_refs outside 1..64, cap_words or cap_hyp <= 0, a ref_len above
 * cap_words, a word id <= 0 inside a reference, a bad or duplicate channel list, NULL references) or WFST_E_STATE (a decoder without
 * lattice_links, a listed channel never initialised).  Any output pointer may be NULL.  The decoder's state is only read: decoding goes
 * on bit for bit as without the call.  Synchronous, as wfst_decoder_align_words is and for the same reason. */
int wfst_decoder_nearest_words(wfst_decoder *d, const int32_t *channels, int32_t n, int32_t use_final_probs,
                               int32_t n_refs /* per channel, 1..64 */, int32_t cap_words,
                               const int32_t *ref_words /* [n][n_refs][cap_words] */, const int32_t *ref_len /* [n][n_refs], -1 = skip */,
                               int32_t cap_hyp, int64_t max_cells /* states x (len + 1) per reference; 0 = default */,
                               int32_t *status /* [n] */, int32_t *found, int32_t *n_err, int32_t *n_cor, int32_t *n_sub, int32_t *n_ins,
                               int32_t *n_del, int32_t *n_arcs, int32_t *n_hyp /* [n][n_refs] */,
                               int32_t *hyp_words, int32_t *begin_frame, int32_t *end_frame /* [n][n_refs][cap_hyp] */,
                               int32_t *ref_hyp /* [n][n_refs][cap_words] */, float *tot_score, float *lm_score /* [n][n_refs] */);

/* ---- word confidences from lattice posteriors -----------------------------------------------------------------------------------
 * How sure the decoder is of a word: the posterior mass of the lattice's arcs that say the word at about the time a hypothesis says
 * it.  The sum-over-paths twin of wfst_decoder_align_words, on the same lattice, for a list of channels, live and finalized ones
 * mixed, n_seqs sequences per channel, one launch per stage (the live channels' lattices emitted, align_index_kernel, align_kernel,
 * posterior_kernel, confidence_kernel).
 *
 * The lattice R is exactly wfst_decoder_align_words': what wfst_decoder_get_raw_lattice(channel, use_final_probs) returns at this
 * moment (wfst_decoder_set_live_lattice_prune, the use_final_probs rule after FinalizeDecoding and "no lattice" honoured).  State 0 is
 * the start, every arc goes to a higher state id, final states are flagged and carry no weight, and a final state may have out-arcs.
 * All arithmetic is float64.  For the scales graph_scale and acoustic_scale (finite, >= 0) an arc a = (s -> t, graph, acoustic) costs
 *   c(a) = graph_scale * (double)graph + acoustic_scale * (double)acoustic,
 * and an arc whose float32 graph + acoustic is not finite is no arc (wfst_decoder_align_words' rule: both calls see the same paths).
 *   alpha[0] = 0;   alpha[t] = -log sum over the arcs a: s -> t of exp(-(alpha[s] + c(a)))
 *   beta[s]  = -log([s is final] + sum over the arcs a: s -> t of exp(-(c(a) + beta[t])))
 *   log_z    = -beta[0]
 *   gamma(a) = exp(-(alpha[s] + c(a) + beta[t] + log_z))                                  (the posterior of the arc)
 * Every sum is taken as m - log(sum exp(-(x - m))) with m the least term.  A state without a finite term is +inf, and its arcs have
 * posterior 0, never NaN.  The ORDER in which a state's arcs are summed is free -- it is the order of the device's arc index, which
 * the launch that emits the lattice decides -- so the results are reproducible to rounding (a few ulp of the largest |alpha| or |beta|
 * per level of the lattice), NOT bit for bit.
 *
 * Word confidence, for a sequence w[0..L) of word ids > 0, on top of wfst_decoder_align_words' answer for that sequence -- found,
 * n_arcs, begin_frame, end_frame, tot_score and lm_score are that call's own, unscaled and bit for bit.  With b[k] = begin_frame[k]
 * (the frame of the source state of the arc that carries word k) the time axis is cut at the midpoints of consecutive begin frames:
 *   m[0] = 0;   m[k] = (b[k - 1] + b[k] + 1) >> 1 for 1 <= k < L;   m[L] = +inf;   cell k = the frames m[k] <= f < m[k + 1]
 *   word_post[k] = sum of gamma(a) over the arcs a with olabel(a) == w[k] whose SOURCE state's frame lies in cell k
 * -- emitting and epsilon arcs alike: a word may sit on an epsilon arc.  It is the expected number of times a path says w[k] at about
 * the time the hypothesis does: order-free, without a word-boundary lattice, 1 when every path agrees, and above 1 when paths say a
 * short word twice inside one cell.  The confidence is min(1, word_post[k]); this call returns word_post UNCLAMPED.
 * path_logpost[i][q] = -log_z - sum of c(a) along the aligned path, in arc order: the log posterior of that one path (<= 0), a lower
 * bound of the hypothesis' sentence posterior.  log_z[i] is per channel.  found = 0: word_post and path_logpost are zero.  The empty sequence
 * is found where the alignment finds it and has no words.
 * Limitation: a word's arc sits where the graph put its olabel, so the cells follow label positions, not acoustic word boundaries.
 * Not computed here: a hypothesis' full sentence posterior (a log-semiring table of states x (L + 1)), per-frame transition-id
 * posteriors (lattice-to-post), minimum Bayes risk / confusion networks.  (The sentence posterior is wfst_decoder_sequence_posterior's,
 * below.)  (The confusion network pinned to a hypothesis -- the other words of a slot, and "no word" -- is
 * wfst_decoder_word_alternatives', below; minimum Bayes risk decoding stays out.)
 * (The per-frame transition-id posteriors are wfst_decoder_frame_posteriors', further below.)
 *
 * A failure of ONE channel goes into status[i] with all of that channel's outputs zero, and the call still returns WFST_OK: a
 * sequence whose alignment table of states x (seq_len + 1) cells is beyond max_cells (WFST_E_CAPACITY; 0 = wfst_decoder_align_words'
 * default), a device error of that channel's utterance.  Beside the alignment's workspace (shared with wfst_decoder_align_words, rounds
 * included) the posteriors take 24 bytes per state and 16 per arc of a listed lattice: alpha, beta, the level flags, gamma and a
 * by-source arc table.
 * The call itself fails, before any device work, with WFST_E_ARG (a scale that is negative or not finite, and everything
 * wfst_decoder_align_words names) or WFST_E_STATE (as there).  Any output pointer may be NULL.  The decoder's state is only read:
 * decoding goes on bit for bit as without the call, and the other getters answer afterwards what they would have answered.
 * Synchronous, as wfst_decoder_align_words is and for the same reason. */
int wfst_decoder_word_confidence(wfst_decoder *d, const int32_t *channels, int32_t n, int32_t use_final_probs,
                                 double graph_scale, double acoustic_scale,
                                 int32_t n_seqs /* per channel, 1..64 */, int32_t cap_words,
                                 const int32_t *seq_words /* [n][n_seqs][cap_words] */, const int32_t *seq_len /* [n][n_seqs], -1 = skip */,
                                 int64_t max_cells /* states x (len + 1) per sequence; 0 = default */,
                                 int32_t *status /* [n] */, double *log_z /* [n] */,
                                 int32_t *found, int32_t *n_arcs /* [n][n_seqs] */,
                                 int32_t *begin_frame, int32_t *end_frame /* [n][n_seqs][cap_words] */,
                                 double *word_post /* [n][n_seqs][cap_words] */, double *path_logpost /* [n][n_seqs] */,
                                 float *tot_score, float *lm_score /* [n][n_seqs] */);

/* ---- sentence and phrase posteriors ----------------------------------------------------------------------------------------------
 * How sure the decoder is of a WHOLE hypothesis, and whether a phrase is in the lattice at all, and when.  The raw lattice is not
 * determinized: a word sequence is spelled by many paths, and path_logpost above is the posterior of one of them.  This call sums
 * over all of them -- the log-semiring twin of wfst_decoder_align_words' table -- for a list of channels, live and finalized ones
 * mixed, n_seqs sequences per channel and one mode per call, one launch per stage (the live channels' lattices emitted,
 * align_index_kernel, posterior_kernel, seqpost_kernel).
 *
 * The lattice R, the scales, the arc cost c(a) = graph_scale * (double)graph + acoustic_scale * (double)acoustic in float64, the rule
 * that an arc whose float32 graph + acoustic is not finite is no arc, alpha, beta, log_z and the way every sum is taken (m - log(sum
 * exp(-(x - m))) with m the least term; a cell without a finite term is +inf, never NaN) are exactly wfst_decoder_word_confidence's.
 * A final state may have out-arcs; a complete path is a path from state 0 that ends in a final state.  The kinds go by OLABEL, not by
 * ilabel: a word may sit on an epsilon arc.  The input is a sequence w[0..L) of word ids > 0.
 *
 * mode 0, sentence (L >= 0): a table S[s][k], 0 <= k <= L, with S[0][0] = 0 and every other cell
 *   S[t][k] = -log( sum over the arcs a: s -> t with olabel 0                   of exp(-(S[s][k]     + c(a)))
 *                 + sum over the arcs a: s -> t with olabel == w[k - 1], k >= 1, of exp(-(S[s][k - 1] + c(a))) )
 * and there is no other transition.  seq_cost = -log sum over the final states s of exp(-S[s][L]), and
 *   seq_logpost = -log_z - seq_cost
 * is the log of the share of the lattice's total weight on the paths that spell exactly w (<= 0 up to rounding, >= the path_logpost
 * of any one of them).  found = 0 and seq_logpost = 0 where no such path exists.  The empty sequence is the posterior of saying
 * nothing.  The posteriors of all distinct word sequences of a lattice sum to 1.
 *
 * mode 1, phrase (L >= 1): a table P[s][k], 0 <= k < L.  P[s][0] = alpha[s] for EVERY state: the phrase may start after any prefix.
 * For k >= 1 the recurrence is the one above: an arc with olabel 0 carries k -> k, an arc with olabel == w[k - 1] carries k - 1 -> k,
 * any other word arc carries nothing -- the phrase is contiguous in the path's words.  An occurrence is completed by an arc
 * a: s -> t with olabel == w[L - 1]:
 *   occ(a) = exp(-(P[s][L - 1] + c(a) + beta[t] + log_z)),   count = sum of occ(a)
 * count is the expected number of (path, position) occurrences; overlapping ones count, so it may pass 1, as word_post may.
 * seq_logpost = log(count) and found = (count > 0); the confidence is min(1, count), and this call returns the count UNCLAMPED, as its
 * logarithm.  hit_mass[i][q][f] = the sum of occ(a) over the arcs whose SOURCE state's frame is f -- wfst_decoder_align_words' begin
 * frame of the phrase's last word, the frame wfst_decoder_word_confidence's cells go by; its sum over f is count, and for L = 1
 * occ(a) = gamma(a).  A row has n_frames[i] entries: the state frames 0 .. frames decoded of the channel's lattice.
 *
 * The ORDER of every sum is the order of the device's arc index, which the launch that emits the lattice decides, and the
 * occurrences are added up with atomic adds: the results are reproducible to rounding, NOT bit for bit.
 *
 * Per listed channel i: log_z[i], n_frames[i]; per sequence q (seq_len[i][q] words at seq_words[i][q][..]; -1: skipped, outputs
 * zero): found[i][q], seq_logpost[i][q], and in mode 1, where hit_mass is given, hit_mass[i][q][0 .. n_frames[i]) of a row of
 * cap_frames (hit_mass is not written in mode 0 beyond being zeroed).
 * A failure of ONE channel goes into status[i] and the call still returns WFST_OK: a sequence whose table of states x (seq_len + 1)
 * cells is beyond max_cells (WFST_E_CAPACITY, the channel's outputs zero; 0 = wfst_decoder_align_words' default bound), a device
 * error of that channel's utterance (likewise), or, with hit_mass given, a lattice of more frames than cap_frames (WFST_E_CAPACITY:
 * n_frames[i] is the room needed, the channel's rows stay zero and its other answers stand).  A cell is 8 bytes, 32.5 MiB of table
 * per sequence at the default bound; the workspace is the decoder's, shared with wfst_decoder_align_words and
 * wfst_decoder_word_confidence (24 bytes per state and 16 per arc of posteriors, 4 bytes per state and sequence of level flags) and
 * grown on demand; lists whose tables pass 256 MiB together are taken in rounds.
 * The call itself fails, before any device work, with WFST_E_ARG (a scale that is negative or not finite, mode outside 0..1, a
 * seq_len of 0 in mode 1, cap_frames < 0, hit_mass given with cap_frames == 0, and everything wfst_decoder_align_words names) or
 * WFST_E_STATE (as there).  Any output pointer may be NULL.  The decoder's state is only read: decoding goes on bit for bit as without
 * the call, and the other getters answer afterwards what they would have answered.  Synchronous, as wfst_decoder_align_words is and
 * for the same reason.
 * Not computed here: minimum Bayes risk decoding and confusion networks, per-frame transition-id posteriors (lattice-to-post).
 * (The confusion network pinned to a hypothesis is wfst_decoder_word_alternatives', below.)
 * (The per-frame transition-id posteriors are wfst_decoder_frame_posteriors', further below.) */
int wfst_decoder_sequence_posterior(wfst_decoder *d, const int32_t *channels, int32_t n, int32_t use_final_probs,
                                    double graph_scale, double acoustic_scale, int32_t mode /* 0 sentence, 1 phrase */,
                                    int32_t n_seqs /* per channel, 1..64 */, int32_t cap_words,
                                    const int32_t *seq_words /* [n][n_seqs][cap_words] */, const int32_t *seq_len /* [n][n_seqs], -1 = skip */,
                                    int64_t max_cells /* states x (len + 1) per sequence; 0 = default */,
                                    int32_t cap_frames /* row length of hit_mass; 0 with hit_mass NULL */,
                                    int32_t *status /* [n] */, double *log_z /* [n] */,
                                    int32_t *n_frames /* [n]: frames of the lattice = room hit_mass needs */,
                                    int32_t *found, double *seq_logpost /* [n][n_seqs] */,
                                    double *hit_mass /* [n][n_seqs][cap_frames], mode 1, may be NULL */);

/* ---- word alternatives per slot: a confusion network pinned to a hypothesis ---------------------------------------------------------
 * What else could have been said in a word's slot, and how likely it is that nothing was said there.  The pivot construction of a
 * confusion network (Hakkani-Tur & Riccardi, "A general algorithm for word graph matrix decomposition", 2003), first half: the
 * hypothesis is the pivot, its time cells are the slots, and every other word of the lattice falls into the slot its time lies in.
 * For a list of channels, live and finalized ones mixed, n_seqs sequences per channel, one launch per stage (the live channels'
 * lattices emitted, align_index_kernel, align_kernel, posterior_kernel, confidence_kernel, slot_mass_kernel, slot_none_kernel).
 *
 * Taken as it is from wfst_decoder_word_confidence: the lattice R, the scales, c(a), the rule that an arc whose float32 graph +
 * acoustic is not finite is no arc, alpha, beta, log_z, gamma(a) and the way every sum is taken.  For a sequence w[0..L) of word ids
 * > 0 the alignment runs first; found, n_arcs, begin_frame, end_frame, tot_score and lm_score are wfst_decoder_align_words' own, bit
 * for bit; the cells are that call's: m[0] = 0, m[k] = (b[k - 1] + b[k] + 1) >> 1, m[L] = +inf, cell k = the frames m[k] <= f <
 * m[k + 1]; word_post[k], path_logpost and log_z are that call's values.
 * A state has a frame.  An arc with ilabel 0 stays inside its frame; every other arc goes from frame f to f + 1.
 *
 * mass and alternatives.  For a cell k and a word v > 0
 *   mass(k, v) = the sum of gamma(a) over the arcs a with olabel(a) == v whose SOURCE state's frame lies in cell k
 * -- emitting and epsilon arcs alike -- so mass(k, w[k]) = word_post[k].  The alternatives of slot k are the words with mass(k, v) > 0,
 * ordered by mass DESCENDING and then by word id ASCENDING.  alt_word[k][0 .. n_alts) and alt_post[k][..] are the first n_alts of them
 * (1 <= n_alts <= WFST_ALTERN_MAX_ALTS), alt_post UNCLAMPED as word_post is; n_distinct[k] is how many such words there are in all;
 * the unused entries are zero.  The hypothesis' own word is one of them wherever it is among the first n_alts; word_post[k] beside
 * the list says where it stands.  The order is taken on the device's own sums: a list is strictly ordered, and where two masses
 * differ by less than their rounding, which of the two comes first (or falls off the list's end) is the device's.
 *
 * none_post[k] = the share of the lattice's weight on the complete paths that have NO word-carrying arc whose source state's frame
 * lies in cell k: the slot's "no word" entry, none_post[k] + P(some word in the cell) = 1.  With lo = m[k], hi = m[k + 1]:
 * an empty cell (lo >= hi: two words that begin at one frame make one) has none_post[k] = 1.  Otherwise, over the states of the
 * cell's frames, A_k[start] = 0 if lo == 0, and
 *   A_k[t] = -log( sum over a: s -> t with frame(s) < lo                          of exp(-(alpha[s] + c(a)))
 *                + sum over a: s -> t with lo <= frame(s) < hi and olabel(a) == 0 of exp(-(A_k[s]   + c(a))) )
 * -- a word on an arc that ENTERS the cell belongs to the cell before -- and none_post[k] is the sum of
 *   exp(-(A_k[s] + c(a) + beta[t] + log_z))  over the arcs a: s -> t that leave the cell (frame(s) in it, frame(t) >= hi), olabel 0,
 *   exp(-(A_k[s] + log_z))                   over the final states s in the cell,
 *   exp(-(alpha[s] + log_z))                 over the final states s with frame(s) < lo: the paths that ended before the cell began.
 * A state without a finite term is +inf; a result is never NaN.  For L = 1 the one cell is the whole time axis and none_post[0] is
 * the posterior of saying nothing at all: exp of wfst_decoder_sequence_posterior's sentence posterior of the empty sequence.
 * 1 - none_post[k] <= the sum of mass(k, v) over v, with equality where no path says two words inside the cell.
 *
 * found = 0: every new output is zero.  The empty sequence has no slots.  The ORDER of every sum is the order of the device's arc
 * index and of its atomic adds: the results are reproducible to rounding, NOT bit for bit.
 *
 * The (cell, word) sums of a sequence are kept in an on-chip table where its distinct (cell, word) pairs number at most
 * WFST_ALTERN_LDS_KEYS, and in the decoder's workspace otherwise; the answers do not depend on which.
 * A failure of ONE channel goes into status[i] with all of that channel's outputs zero, and the call still returns WFST_OK, as
 * wfst_decoder_word_confidence has it.  Beside that call's workspace (rounds included) this one takes, per sequence, 8 bytes per
 * state (A), 8 per word, and 16 bytes per slot of a table with a power of two of slots above the arcs of the round's largest lattice.
 * The call itself fails, before any device work, with WFST_E_ARG (n_alts outside 1..16, a scale that is negative or not finite, and
 * everything wfst_decoder_word_confidence names) or WFST_E_STATE (as there).  Any output pointer may be NULL.  The decoder's state is
 * only read: decoding goes on bit for bit as without the call.  Synchronous, as wfst_decoder_align_words is and for the same reason.
 * Not computed here: minimum Bayes risk decoding, the merging of slots or new slots between the hypothesis' words (the pivot
 * algorithm's second half), per-frame transition-id posteriors.
 * (The per-frame transition-id posteriors are wfst_decoder_frame_posteriors', right below.) */
#define WFST_ALTERN_MAX_ALTS 16
#define WFST_ALTERN_LDS_KEYS 1024 /* distinct (cell, word) pairs of a sequence the on-chip table takes */
int wfst_decoder_word_alternatives(wfst_decoder *d, const int32_t *channels, int32_t n, int32_t use_final_probs,
                                   double graph_scale, double acoustic_scale, int32_t n_alts /* per slot, 1..16 */,
                                   int32_t n_seqs /* per channel, 1..64 */, int32_t cap_words,
                                   const int32_t *seq_words /* [n][n_seqs][cap_words] */, const int32_t *seq_len /* [n][n_seqs], -1 = skip */,
                                   int64_t max_cells /* states x (len + 1) per sequence; 0 = default */,
                                   int32_t *status /* [n] */, double *log_z /* [n] */,
                                   int32_t *found, int32_t *n_arcs /* [n][n_seqs] */,
                                   int32_t *begin_frame, int32_t *end_frame /* [n][n_seqs][cap_words] */,
                                   double *word_post, double *none_post /* [n][n_seqs][cap_words] */,
                                   int32_t *n_distinct /* [n][n_seqs][cap_words] */,
                                   int32_t *alt_word, double *alt_post /* [n][n_seqs][cap_words][n_alts] */,
                                   double *path_logpost /* [n][n_seqs] */, float *tot_score, float *lm_score /* [n][n_seqs] */);

/* ---- frame posteriors: transition-id, pdf or phone per frame ------------------------------------------------------------------------
 * What the lattice says at every FRAME: the posterior mass of each transition-id of the frame's emitting arcs (Kaldi's
 * lattice-to-post), or of each pdf or phone where the caller maps the transition-ids -- state and phone occupancies for adaptation,
 * phone-level confidences, the frame-level confidence trace of a hypothesis, "which pdfs was the decoder torn between at frame t".
 * For a list of channels, live and finalized ones mixed, one launch per stage (the live channels' lattices emitted,
 * align_index_kernel, posterior_kernel, frame_post_kernel, frame_pack_kernel), the results back in one copy per round.
 *
 * Taken as it is from wfst_decoder_word_confidence: the lattice R, the scales, c(a), the rule that an arc whose float32 graph +
 * acoustic is not finite is no arc, alpha, beta, log_z, gamma(a) and the way every sum is taken.
 * A state has a frame.  An arc with ilabel 0 stays inside its frame; every other arc goes from frame f to f + 1.
 *   class(a)      = ilabel(a) where label_map is NULL, label_map[ilabel(a)] otherwise (n_tid + 1 entries >= 0, entry 0 unused)
 *   post(f, v)    = the sum of gamma(a) over the emitting arcs a (ilabel > 0) whose SOURCE state's frame is f and whose class is v
 *   frame_mass[f] = the sum of post(f, v) over all v, before any threshold: 1 minus the weight of the complete paths that ended
 *                   before frame f + 1 (a final state may have out-arcs), so 1 to rounding wherever every path runs to the end
 *   n_distinct[f] = the number of classes with post(f, v) > 0
 * The entries of frame f are the classes with post(f, v) > 0 and post(f, v) >= min_post (0 <= min_post <= 1, taken on the device's own
 * sum), by class id ASCENDING: the order does not depend on the sums, so near ties cannot reorder a list.  An arc with ilabel 0 is
 * in no frame's list, whatever word it carries; an arc on no complete path has gamma 0 and counts nowhere.
 * n_frames[i] = the frames the lattice spans (the frames decoded); an empty lattice, or a finalized channel asked without
 * final-probs, has n_frames = 0, log_z = 0 and no entries, as the sibling calls report "no lattice".
 *
 * Per listed channel i: log_z[i], n_frames[i], n_entries[i]; frame_off[i][0 .. n_frames[i]] (frame f's entries are
 * frame_off[i][f] .. frame_off[i][f + 1] of the channel's rows, frame_off[i][n_frames[i]] = n_entries[i]); n_distinct[i][f] and
 * frame_mass[i][f] for f < n_frames[i]; entry_class[i][e] and entry_post[i][e] (UNCLAMPED, in (0, 1] up to rounding) for
 * e < n_entries[i].  What lies beyond is zero.
 * The ORDER of a class' sum follows the device's arc index, which the launch that emits the lattice decides: the results are
 * reproducible to rounding, NOT bit for bit.  A frame's (class, gamma) pairs are sorted and summed on chip where the frame has at
 * most WFST_FRAMEPOST_LDS_RECS emitting arcs, and in the decoder's workspace otherwise; the answers do not depend on which.
 *
 * A failure of ONE channel goes into status[i] with that channel's lists zero, and the call still returns WFST_OK: a device error of
 * that channel's utterance, a lattice of more than max_cells states (WFST_E_CAPACITY; 0 = wfst_decoder_word_confidence's default
 * bound), or a lattice with n_frames[i] > cap_frames or n_entries[i] > cap_entries (WFST_E_CAPACITY: n_frames[i] and n_entries[i] are
 * the room needed, so that the call can be repeated once; log_z[i] stands).  Beside wfst_decoder_word_confidence's posterior
 * workspace the call takes 24 bytes per arc of a listed lattice (the staged lists and the sort's workspace) and 16 per frame.
 * The call itself fails, before any device work, with WFST_E_ARG (a NULL decoder or channel list, a scale that is negative or not
 * finite, min_post that is NaN or outside 0..1, cap_frames < 1, cap_entries < 1, max_cells < 0, label_map given with n_tid < 1 or with
 * a negative entry, label_map shorter than the graph's largest ilabel -- from the graph's host copy, as wfst_graph_set_tid2phone
 * checks its map -- a bad or duplicate channel list) or WFST_E_STATE (a decoder without lattice_links, a listed channel never
 * initialised).  Any output pointer may be NULL.  The decoder's state is only read: decoding goes on bit for bit as without the call.
 * Synchronous, as wfst_decoder_align_words is and for the same reason.
 * Not computed here: minimum Bayes risk decoding and the pivot algorithm's second half. */
#define WFST_FRAMEPOST_LDS_RECS 1024 /* emitting arcs of one frame that are sorted and summed on chip */
int wfst_decoder_frame_posteriors(wfst_decoder *d, const int32_t *channels, int32_t n, int32_t use_final_probs,
                                  double graph_scale, double acoustic_scale,
                                  const int32_t *label_map /* NULL, or n_tid + 1 entries, entry 0 unused */, int32_t n_tid,
                                  double min_post, int64_t max_cells /* lattice states; 0 = default */,
                                  int32_t cap_frames, int32_t cap_entries,
                                  int32_t *status /* [n] */, double *log_z /* [n] */, int32_t *n_frames /* [n] */,
                                  int32_t *n_entries /* [n] */, int32_t *frame_off /* [n][cap_frames + 1] */,
                                  int32_t *n_distinct /* [n][cap_frames] */, double *frame_mass /* [n][cap_frames] */,
                                  int32_t *entry_class /* [n][cap_entries] */, double *entry_post /* [n][cap_entries] */);

/* ---- sequence-training statistics: MMI and sMBR on the raw lattice ----------------------------------------------------------------------
 * The way back from the lattice to the acoustic model: per frame the derivative of the MMI or the sMBR criterion with respect to the
 * scores of the frame's classes, for discriminative (sequence) training -- Kaldi's LatticeForwardBackwardMpeVariants with criterion
 * "smbr" (kaldi/src/lat/lattice-functions.cc), the expectation-semiring pass, and the occupation difference of
 * LatticeForwardBackwardMmi with --drop-frames.  For a list of channels, live and finalized ones mixed, one launch per stage (the live
 * channels' lattices emitted, align_index_kernel, posterior_kernel, acc_kernel, seqstat_frame_kernel, seqstat_pack_kernel and, with
 * dense rows, seqstat_dense_kernel), the lists back in one copy per round.
 *
 * The lattice is exactly wfst_decoder_frame_posteriors': the live-prune mode, use_final_probs, the rule that an arc whose float32
 * graph + acoustic is not finite is no arc, c(a) = graph_scale * graph + acoustic_scale * acoustic, alpha, beta, log_z, gamma(a) and
 * class(a) of an emitting arc (its transition-id, or label_map[tid]) are taken from there unchanged.  Float64 throughout.
 * The caller gives ref[i][f] for f < n_ref[i], the numerator alignment's class per frame (ref[i][f] < 0 and f >= n_ref[i]: the frame is
 * unlabelled), and sil_classes, up to WFST_SEQSTAT_MAX_SIL class ids >= 0, strictly ascending.
 *   acc(a)     = 1 if a is an emitting arc out of frame f, ref[f] >= 0, class(a) == ref[f] and the class is not in sil_classes;
 *                0 otherwise, and for every arc with ilabel 0
 *   p_in(a)    = exp(-(alpha[s] + c(a) - alpha[t])),   p_out(a) = exp(-(c(a) + beta[t] - beta[s]))      (0 where not finite)
 *   fa[0] = 0, fa[t] = sum over in-arcs  a: s -> t of p_in(a)  * (fa[s] + acc(a))
 *              fb[s] = sum over out-arcs a: s -> t of p_out(a) * (fb[t] + acc(a))      (a final state's "stop here" term adds 0)
 *   tot_acc    = fb[0]: the expected number of correct frames
 *   w(a)       = gamma(a) * (fa[s] + acc(a) + fb[t] - tot_acc), signed
 * level by level, as posterior_kernel orders a frame with arcs between its own states.  Per frame f and class v of an emitting arc
 * out of f:
 *   post(f, v)  = the sum of gamma(a)                     (wfst_decoder_frame_posteriors' number)
 *   value(f, v) = the sum of w(a)                         under WFST_SEQ_SMBR
 *   value(f, v) = [v == ref[f]] - post(f, v)              under WFST_SEQ_MMI, 0 everywhere on an unlabelled frame
 * The list of frame f holds the classes with post(f, v) > 0 by class id ASCENDING (frame_posteriors' membership at min_post = 0),
 * each entry (class, post, value).  Under MMI a labelled frame whose ref[f] is no such class gets one more entry (ref[f], 0, 1) at
 * its place in the order; with drop_frames != 0 (Kaldi's --drop-frames) it gets none, every value of that frame is 0 and the frame
 * counts in n_dropped.  drop_frames is not looked at under sMBR.  tot_acc is 0 under MMI.
 *
 * Per listed channel i: log_z, tot_acc, n_frames, n_ref_frames (the labelled frames below n_frames), n_dropped, n_entries,
 * frame_off[i][0 .. n_frames[i]], entry_class / entry_post / entry_value[i][e] for e < n_entries[i].  What lies beyond is zero.
 * cap_frames = cap_entries = 0: no lists are handed out (the channels' numbers and the dense rows only) and none can be too small.
 * The dense output: grad NULL, or per listed channel a DEVICE pointer (NULL: none) to float32 [grad_frames[i]][n_cols] with a row
 * pitch of grad_pitch[i] floats (grad_pitch NULL: n_cols).  Rows 0 .. min(n_frames[i], grad_frames[i]) - 1 are written: n_cols
 * zeros, then float32(grad_scale * value(f, v)) at column v for every entry of the frame's list.  Nothing beyond n_cols in a row and
 * no other row is touched.  A class is a column: a label_map entry or a ref class >= n_cols is refused, and without a map n_cols
 * must exceed the graph's largest transition-id.  The writes run on the decoder's stream, ordered against consumer_stream (a
 * hipStream_t, NULL: the legacy default stream) both ways, as wfst_decoder_advance_chunk orders a chunk against its producer_stream: the
 * writes wait for what that stream was given before the call (a fill of the rows, the previous step's read of them), and the stream
 * waits on an event recorded behind the writes.  WFST_STREAM_NONE: the rows are free to be written when the call is made, and the
 * call returns with them complete (it does in either case today: the call is synchronous).
 * The ORDER of a sum follows the device's arc index: the results are reproducible to rounding, NOT bit for bit.  A frame's triples
 * are sorted and summed on chip where the frame has at most WFST_SEQSTAT_LDS_RECS emitting arcs, and in the decoder's workspace
 * otherwise; the answers do not depend on which.
 *
 * A failure of ONE channel goes into status[i] with that channel's outputs zero and its dense rows untouched, and the call still
 * returns WFST_OK: a device error of that channel's utterance, a lattice of more than max_cells states (WFST_E_CAPACITY; 0 =
 * wfst_decoder_word_confidence's default bound), or n_frames[i] > cap_frames or n_entries[i] > cap_entries (WFST_E_CAPACITY: n_frames[i]
 * and n_entries[i] are the room needed, so that the call can be repeated once; log_z[i] stands, and so do the dense rows).  Beside
 * wfst_decoder_word_confidence's posterior workspace the call takes 48 bytes per arc, 16 per state and 32 per frame of a listed lattice
 * (fa, fb, w, the staged lists and the sort's workspace).
 * The call itself fails, before any device work, with WFST_E_ARG (everything wfst_decoder_frame_posteriors names; an unknown
 * criterion; sil_classes negative, not strictly ascending or more than WFST_SEQSTAT_MAX_SIL; n_ref[i] < 0 or above cap_ref; a
 * grad_scale that is not finite; grad without grad_frames, n_cols < 1, a negative grad_frames, a pitch below n_cols, a grad pointer not
 * aligned to 4 bytes, a class beyond n_cols as above) or WFST_E_STATE as there.  Any output pointer may be NULL.  The decoder's state
 * is only read: decoding goes on bit for bit as without the call.
 * Not computed here: minimum Bayes risk decoding and the pivot algorithm's second half, Kaldi's one_silence_class variant, a
 * half-precision dense output.  (The MMI numerator's log-probability: wfst_decoder_graph_posteriors' log_like.)
 * (The numerator alignment `ref` and its cost come from wfst_decoder_force_align with label_map = the same map.) */
#define WFST_SEQ_MMI 0
#define WFST_SEQ_SMBR 1
#define WFST_SEQSTAT_LDS_RECS 1024 /* emitting arcs of one frame that are sorted and summed on chip */
#define WFST_SEQSTAT_MAX_SIL 64    /* silence classes */
int wfst_decoder_sequence_stats(wfst_decoder *d, const int32_t *channels, int32_t n, int32_t criterion, int32_t use_final_probs,
                                double graph_scale, double acoustic_scale,
                                const int32_t *label_map /* NULL, or n_tid + 1 entries, entry 0 unused */, int32_t n_tid,
                                const int32_t *ref /* [n][cap_ref] */, const int32_t *n_ref /* [n] */, int32_t cap_ref,
                                const int32_t *sil_classes, int32_t n_sil, int32_t drop_frames,
                                int64_t max_cells /* lattice states; 0 = default */, int32_t cap_frames, int32_t cap_entries,
                                void *const *grad /* NULL, or [n] device pointers */, const int64_t *grad_pitch /* [n], floats */,
                                const int32_t *grad_frames /* [n] */, int32_t n_cols, double grad_scale, void *consumer_stream,
                                int32_t *status /* [n] */, double *log_z /* [n] */, double *tot_acc /* [n] */,
                                int32_t *n_frames, int32_t *n_ref_frames, int32_t *n_dropped, int32_t *n_entries /* [n] each */,
                                int32_t *frame_off /* [n][cap_frames + 1] */, int32_t *entry_class /* [n][cap_entries] */,
                                double *entry_post, double *entry_value /* [n][cap_entries] */);

/* ---- best paths under new scales: the 1-best again at another LM weight, acoustic scale and word penalty -----------------------------
 * Everything above is decided at the scales the search ran with.  This call picks the best path of a channel's RAW lattice again under
 * another graph (LM) scale, another acoustic scale and a word insertion penalty, without decoding again: Kaldi's
 * lattice-best-path-score (kaldi-bin/bin/lattice-best-path-score.cc:93-116: ScaleLattice(LatticeScale(lm_scale, acoustic_scale)), then
 * the shortest path, then the words, the alignment and (graph, acoustic, sum)), the tool every scoring script sweeps over LMWT x word
 * penalty.  With wfst_decoder_nearest_words for the error count, tuning both on a development set is one decode plus two lattice
 * calls; and the posterior calls, which take scales already, can be asked about the hypothesis that is best AT those scales.  For a
 * list of channels, live and finalized ones mixed, and n_set (1..64) settings shared by all listed channels, settings[q] =
 * (graph_scale gs, acoustic_scale as, word_penalty wip), one launch per stage (the live channels' lattices emitted,
 * align_index_kernel, one dynamic program per (channel, setting): rescale_kernel).
 *
 * The lattice R is exactly wfst_decoder_align_words': what wfst_decoder_get_raw_lattice(channel, use_final_probs) returns at this
 * moment, wfst_decoder_set_live_lattice_prune, the use_final_probs rule after FinalizeDecoding and "no lattice" honoured as there.
 * State 0 is the start, every arc goes to a higher state id, final states are flagged and carry no weight, and an arc whose float32
 * graph + acoustic is not finite is no arc, so that all the word queries see the same paths.
 * The cost of an arc a under setting q, in float64:
 *   c_q(a) = (gs * (double)graph + as * (double)acoustic) + (olabel(a) != 0 ? wip : 0.0)
 * with every product and every sum rounded on its own -- no fused multiply-add; the kernel switches the compiler's contraction off
 * for this expression, and that is why the result is reproducible: it is numpy's arithmetic.  The penalty goes by OLABEL, as
 * everywhere here: a word may sit on an epsilon arc.  gs and as are finite and >= 0; wip is finite and of either sign.
 * The cells: v[0] = +0.0; v[t] = the minimum over the in-arcs a: s -> t of (v[s] + c_q(a)) + 0.0; a sum that is not finite is no
 * transition; a state not reached is greater than every other.  Float addition is monotone, so v[t] is the minimum over the paths
 * from state 0 to t of the sequential float64 sum of c_q along the path.  A minimum does not depend on the order it is taken in, so
 * the result is bit for bit the same whatever the order of the device's arc index.
 * The answer ends in the final state e with the least v[e], the least graph state among equals; found = 0 only if no final state is
 * reached at all.  The traceback runs backwards from e to state 0 by exact equality, (v[s] + c_q(a)) + 0.0 == v[t]; among several
 * qualifying arcs the least key wins, the key being wfst_decoder_align_words' tuple: ilabel == 0 last, graph state of the source
 * token, ilabel, olabel, bits of graph, bits of acoustic.  Nothing depends on the numbering of states or arcs.  On biglm lattices two
 * tokens of a frame may share a graph state: a tie that survives the rule is unspecified there.
 *
 * Per listed channel i and setting q: found[i][q]; n_arcs; n_hyp and hyp_words[i][q][..], the non-zero olabels of the path in
 * order; begin_frame / end_frame[i][q][j] per word by wfst_decoder_align_words' own definition over the path's arcs (the list of
 * wfst_decoder_set_silence_phones included); scaled_cost = v[e]; tot_score = the float32 sequential sum of graph + acoustic along the
 * path, each arc's own sum rounded first, and lm_score = the float32 sequential sum of graph, both UNSCALED: LatticeToVector's, as the
 * other calls define them.  Where tids is given, n_tids and tids[i][q][..], the non-zero ilabels in path order (the alignment); with
 * tids NULL the alignment is skipped and cap_tids is not looked at beyond its sign.
 * The lattice was PRUNED at scales (1, 1): a path that lattice_beam dropped is not found again however good it would be under the
 * new scales -- Kaldi's own caveat for its lattices.  Keep lattice_beam wide enough for the range that is swept.
 *
 * A failure of ONE channel goes into status[i] and the call still returns WFST_OK: a device error of that channel's utterance
 * (found[i][..] = 0), a lattice of more than max_cells states (WFST_E_CAPACITY, found[i][..] = 0; 0 = 65 536 states x 65, the
 * bound wfst_decoder_align_words has by default), or a path with n_hyp > cap_words or, where tids is given, n_tids > cap_tids
 * (WFST_E_CAPACITY: the counts are the room needed, the first cap_words words and times and the first cap_tids transition-ids are
 * written as wfst_decoder_nearest_words does, and everything else of the channel's answers stands).  The call takes 8 bytes per state
 * and setting for the cells and 4 for the traced path, beside the index (32 bytes per arc and 8 per state of a listed lattice); the
 * workspace is the decoder's, shared with wfst_decoder_align_words and grown on demand; lists whose cells pass 256 MiB together are
 * taken in rounds.
 * The call itself fails, before any device work, with WFST_E_ARG (a NULL decoder or channel list, n_set outside 1..64, NULL
 * settings, a scale that is negative or not finite, a penalty that is not finite, cap_words <= 0, cap_tids < 0, max_cells < 0, a
 * bad or duplicate channel list) or WFST_E_STATE (a decoder without lattice_links, a listed channel never initialised).  Any output
 * pointer may be NULL.  The decoder's state is only read: decoding goes on bit for bit as without the call.  Synchronous, as
 * wfst_decoder_align_words is and for the same reason.
 * Not computed here: n-best lists under new scales, a second LM, and pruning the search itself with other scales. */
int wfst_decoder_rescaled_words(wfst_decoder *d, const int32_t *channels, int32_t n, int32_t use_final_probs,
                                int32_t n_set /* 1..64, shared by the listed channels */,
                                const double *settings /* [n_set][3]: graph_scale, acoustic_scale, word_penalty */,
                                int32_t cap_words, int32_t cap_tids, int64_t max_cells /* lattice states; 0 = default */,
                                int32_t *status /* [n] */, int32_t *found, int32_t *n_arcs, int32_t *n_hyp,
                                int32_t *n_tids /* [n][n_set] */,
                                int32_t *hyp_words, int32_t *begin_frame, int32_t *end_frame /* [n][n_set][cap_words] */,
                                int32_t *tids /* [n][n_set][cap_tids], or NULL */,
                                double *scaled_cost /* [n][n_set] */, float *tot_score, float *lm_score /* [n][n_set] */);

/* ---- phrase boosting: biased best paths of the raw lattice, a list of phrases per channel -----------------------------------------------
 * Contextual biasing: a caller brings a short list of phrases per stream -- contact names, product names, a meeting's attendees --
 * and wants the answer to prefer them.  This call picks the best path of a channel's RAW lattice again as
 * wfst_decoder_rescaled_words does, under a graph scale, an acoustic scale and a word penalty, and with a bonus for every occurrence
 * of a listed phrase in the path's word sequence: the product of that call's sweep and a phrase automaton (bias_kernel behind
 * align_index_kernel, one workgroup per (channel, setting)).  It finds only what the lattice holds: a phrase that lattice_beam
 * pruned away is not brought back, however large its bonus -- the accepted shape of lattice-rescoring biasing.  Keep lattice_beam
 * wide enough for the bonuses in use.
 *
 * A bias list is P >= 0 phrases; phrase p is 1..WFST_BIAS_MAX_WORDS word ids (> 0) with a bonus b_p, a float64 that is finite and
 * >= 0; no two phrases of one list are equal.  The phrases of a list form a trie of J nodes including the root, J <=
 * WFST_BIAS_MAX_NODES.  The nodes are numbered in breadth-first order, root 0, ordered by (depth, parent's number, word id)
 * ascending; the numbering is part of the definition because the tie rule uses it.  str(j) is the word string that leads from the
 * root to node j.
 * The automaton: fail(j) is the node of the longest proper suffix of str(j) that is a node (the root for depth 1); delta(i, w) is
 * the node of the longest suffix of str(i) . w that is a node, the root if none is; own(j) = b_p where str(j) is phrase p, else 0.0;
 * beta(0) = 0.0 and beta(j) = own(j) + beta(fail(j)), computed in node order in float64 (a list whose beta is not finite is
 * refused).  So every occurrence of every phrase as a contiguous run of the path's word sequence earns its bonus: overlapping and
 * nested occurrences each count, and nothing is retracted.
 *
 * settings[q] = (graph_scale gs, acoustic_scale as, word_penalty wip, boost_scale bs), n_set = 1..16 of them shared by the listed
 * channels; gs, as and bs are finite and >= 0, wip is finite.  The lattice R, "no arc", c_q(a) and the + 0.0 are exactly
 * wfst_decoder_rescaled_words'.  Along a path the node track is j_0 = 0, then j_k = delta(j_{k-1}, olabel(a_k)) on a word arc
 * (olabel != 0), else j_{k-1}.  An arc costs
 *   d = c_q(a) - r,   r = bs * beta(j_k) on a word arc and 0.0 otherwise,
 * the product and the difference each rounded on its own, under the same contraction-off pragma: no fused multiply-add.
 * The cells: v[0][0] = +0.0; v[t][j] = the minimum over the in-arcs a: s -> t and the source nodes i whose step over a gives j of
 * (v[s][i] + d) + 0.0; a sum that is not finite is no transition.  Float addition is monotone for costs of either sign and R is a
 * DAG (every arc goes to a higher state id), so v[t][j] is the minimum over the paths of the sequential float64 sum, whatever the
 * order of the arc index: the result is bit for bit reproducible.  Totals may be negative.
 * The end: the pair (final state e, node j) with the least v, then the least graph state, then the least node; found = 0 only if
 * no final state is reached.  The traceback runs backwards by exact equality, (v[s][i] + d) + 0.0 == v[t][j]; among several
 * qualifying (arc, source node) the least wfst_decoder_align_words arc tuple wins, then the least source node.  On biglm lattices
 * two tokens of a frame may share a graph state: a tie that survives the rule is unspecified there.
 *
 * Per listed channel i and setting q: found[i][q]; n_arcs; n_hyp and hyp_words[i][q][..]; begin_frame / end_frame by
 * wfst_decoder_rescaled_words' definitions (the list of wfst_decoder_set_silence_phones included); biased_cost = v[e][j]; bonus =
 * the float64 sequential sum of r in hop order; tot_score and lm_score UNSCALED, LatticeToVector's, unchanged by the bias; n_hits
 * with hit_phrase[i][q][..] (the phrase's index in the channel's list) and hit_word[i][q][..] (the index in hyp_words of the
 * occurrence's last word), ordered by hit_word ascending, then along the chain j, fail(j), ..., so that the longest phrase comes
 * first.  list_of[i] maps listed channel i to a list of the set, -1 (or list_of NULL) means no list: J = 1, only the root.  With
 * J = 1, or with bs = 0, biased_cost is bit for bit wfst_decoder_rescaled_words' scaled_cost at (gs, as, wip), and the whole answer
 * equals it wherever no decision was a tie.
 *
 * A failure of ONE channel goes into status[i] and the call still returns WFST_OK: a device error of that channel's utterance, a
 * table of lattice states x J cells beyond max_cells (WFST_E_CAPACITY, found[i][..] = 0; 0 = 65 536 states x 256), or a path with
 * n_hyp > cap_words or, where hit_phrase or hit_word is given, n_hits > cap_hits (WFST_E_CAPACITY: the counts are the room needed,
 * the first entries are written, and everything else of the channel's answers stands).  The call takes 8 bytes per cell; the
 * workspace is the decoder's, shared with wfst_decoder_align_words and grown on demand; lists of channels whose cells pass 256 MiB
 * together are taken in rounds.  The call itself fails, before any device work, with WFST_E_ARG (a NULL decoder or channel list,
 * n_set outside 1..16, NULL settings, a scale that is negative or not finite, a penalty that is not finite, cap_words <= 0,
 * cap_hits < 0, max_cells < 0, a bad or duplicate channel list, a list_of outside the set or a list where lists is NULL, lists of
 * another device) or WFST_E_STATE (a decoder without lattice_links, a listed channel never initialised).  Any output pointer may be NULL.
 * The decoder's state is only read: decoding goes on bit for bit as without the call.  Synchronous, as wfst_decoder_align_words is.
 *
 * wfst_bias_compile is host only: from one list's phrases (phrase_words: the phrases' words one after the other) it returns the
 * nodes' parent (-1: the root), word (0: the root), fail, phrase (index or -1) and beta, so that the automaton can be looked at
 * without a device; n_nodes is set even where it exceeds cap_nodes or WFST_BIAS_MAX_NODES (WFST_E_CAPACITY both).
 * wfst_bias_lists_create validates on the host before any device is touched (phrase_len / phrase_bonus: the lists' phrases one
 * list after the other): a word id <= 0, a length outside 1..16, a bonus that is negative or not finite or a duplicate phrase is
 * WFST_E_ARG and the message names list and phrase; more than 256 nodes is WFST_E_CAPACITY; no device is WFST_E_DEVICE.
 * Not computed here: biasing the first-pass search; lists beyond 256 nodes or a sparse table; n-best lists under a bias;
 * transition-id output; class or subword biasing. */
#define WFST_BIAS_MAX_NODES 256
#define WFST_BIAS_MAX_WORDS 16
#define WFST_BIAS_MAX_SETTINGS 16
typedef struct wfst_bias_lists wfst_bias_lists;
int wfst_bias_compile(int32_t n_phrases, const int32_t *phrase_len /* [n_phrases] */, const int32_t *phrase_words,
                      const double *phrase_bonus /* [n_phrases] */, int32_t cap_nodes, int32_t *n_nodes,
                      int32_t *parent, int32_t *word, int32_t *fail, int32_t *phrase, double *beta /* [cap_nodes] each, or NULL */);
int wfst_bias_lists_create(int32_t n_lists, const int32_t *n_phrases /* [n_lists] */, const int32_t *phrase_len,
                           const int32_t *phrase_words, const double *phrase_bonus, int device, wfst_bias_lists **out);
int wfst_bias_lists_info(const wfst_bias_lists *b, int32_t *n_lists, int64_t *total_phrases, int64_t *total_nodes,
                         int32_t *n_phrases, int32_t *n_nodes, int32_t *n_words /* [n_lists] each */, int64_t *device_bytes);
void wfst_bias_lists_free(wfst_bias_lists *b);
int wfst_decoder_biased_words(wfst_decoder *d, const int32_t *channels, int32_t n, int32_t use_final_probs,
                              const wfst_bias_lists *lists, const int32_t *list_of /* [n], -1: no list; NULL: none has one */,
                              int32_t n_set /* 1..16, shared by the listed channels */,
                              const double *settings /* [n_set][4]: graph_scale, acoustic_scale, word_penalty, boost_scale */,
                              int32_t cap_words, int32_t cap_hits, int64_t max_cells /* cells of one table; 0 = default */,
                              int32_t *status /* [n] */, int32_t *found, int32_t *n_arcs, int32_t *n_hyp,
                              int32_t *n_hits /* [n][n_set] */,
                              int32_t *hyp_words, int32_t *begin_frame, int32_t *end_frame /* [n][n_set][cap_words] */,
                              int32_t *hit_phrase, int32_t *hit_word /* [n][n_set][cap_hits] */,
                              double *biased_cost, double *bonus /* [n][n_set] */, float *tot_score, float *lm_score /* [n][n_set] */);

/* ---- phrase boosting for large lists: sparse cells over reachable nodes ------------------------------------------------------------------
 * wfst_decoder_biased_words keeps a cell for every (lattice state, node) pair and so serves lists of at most 256 nodes.  The lists
 * the feature exists for -- a phone's contacts, a product catalogue -- run to thousands of phrases.  Along one path the automaton is
 * in exactly one node and most lattice words are in no phrase, so almost all of those cells are +inf.  This call keeps only the
 * cells a path can reach; its cost follows the lattice, not the list.
 *
 * A BOOK is a bias list without the 256-node cap: P >= 0 phrases of 1..WFST_BIAS_MAX_WORDS word ids > 0, each with a bonus that is
 * finite and >= 0, no two phrases equal; its trie has J <= WFST_BIAS_BOOK_MAX_NODES = 65 536 nodes.  The numbering, fail, delta, own
 * and beta are exactly wfst_decoder_biased_words': breadth first, root 0, by (depth, parent's number, word id).  The settings,
 * c_q(a), d = c_q(a) - r, the + 0.0, the end rule, the traceback's tie rule (the wfst_decoder_align_words arc tuple, then the least
 * source node) and every output are that call's, word for word.  So for a list of <= 256 nodes this call's answer equals that
 * call's in every byte.
 *
 * New in the definition is the reachable set, which does not depend on the settings:
 *   R(0) = {0};
 *   for every in-arc a: s -> t that is an arc (its float32 graph + acoustic sum is finite), R(t) contains R(s) if olabel(a) == 0,
 *   and {delta(i, olabel(a)) : i in R(s)} otherwise;
 *   R is the least fixed point of these rules (the lattice is a DAG, so R is well defined).
 * By induction over the DAG, v[t][j] finite implies j in R(t): the table restricted to {(t, j) : j in R(t)}, with the same
 * recurrence, holds the same bits as the dense one.  A cell inside R may still be +inf (a float64 sum that overflows).
 * n_cells[i] = the sum over t of |R(t)|, an exact integer, is a per-channel output.
 *
 * bias_reach_kernel (one workgroup per channel, once per call, shared by the settings) builds R and the product graph's edges over
 * align_index_kernel's index; bias_sparse_kernel (one workgroup per (channel, setting)) sweeps the cells, picks the end, walks back
 * and reads the path forwards, recomputing the node track from the automaton itself: a hop that differs from the traced cell is
 * reported as an internal error (WFST_E_DEVICE), never answered.  On the device a book is its nodes' word, fail, phrase, first
 * child and child count, beta and the distinct words; goto(i, w) is a binary search among i's children (consecutive numbers in
 * ascending word order), delta(i, w) tries goto along i, fail(i), ... down to the root.
 *
 * max_cells bounds ONE channel's n_cells (0 = 4 Mi cells; at most 2^30); a channel beyond it gets status[i] = WFST_E_CAPACITY, zeroed
 * answers and n_cells[i] = -1, the others' answers stand.  The same holds for a channel whose product graph has more than
 * min(16 x max_cells, 2^30) edges.  The sets live in per-channel regions that start at max(1024, 4 x states) cells and
 * max(4096, 8 x arcs) edges; a region that overflows is made four times as large and the reach stage runs again, at most
 * log4(max_cells / first size) + 1 times for each of the two.  round_cells is the number of cost cells (8 bytes each) of the
 * (channel, setting) pairs taken together in one round of the sweep (0 = 32 Mi cells = 256 MiB); a channel whose own settings need
 * more runs in a round of its own.  The answers do not depend on max_cells, round_cells or the growth.
 * Every other failure, argument error and state error is wfst_decoder_biased_words', and round_cells < 0 is WFST_E_ARG.  Any output
 * pointer may be NULL.  The decoder's state is only read.  Synchronous.
 *
 * wfst_bias_book_compile is wfst_bias_compile under the book's cap: host only, n_nodes is set even on WFST_E_CAPACITY.
 * wfst_bias_books_create validates on the host before any device is touched; its argument errors are wfst_bias_lists_create's, with
 * "bias book K phrase P" in the message; more than 65 536 nodes is WFST_E_CAPACITY.
 * Measured on one MI355X (profiles/bias_sparse_probe.json: 64 live channels at frame 150 of the headline lattice configuration, four
 * settings): 5.1 .. 6.6 ms per call from 2 to 65 536 nodes beside the dense call's 3.1 / 3.9 / 6.9 / 78 ms at 2 / 16 / 64 / 256 nodes,
 * n_cells / states 1.004 at the median.  Not measured: an idle card, a service end to end, sets of hundreds of nodes per state.
 * Not computed here: biasing the first-pass search; n-best lists under a bias; transition-id output; class or subword biasing. */
#define WFST_BIAS_BOOK_MAX_NODES 65536
typedef struct wfst_bias_books wfst_bias_books;
int wfst_bias_book_compile(int32_t n_phrases, const int32_t *phrase_len /* [n_phrases] */, const int32_t *phrase_words,
                           const double *phrase_bonus /* [n_phrases] */, int32_t cap_nodes, int32_t *n_nodes,
                           int32_t *parent, int32_t *word, int32_t *fail, int32_t *phrase, double *beta /* [cap_nodes] each, or NULL */);
int wfst_bias_books_create(int32_t n_books, const int32_t *n_phrases /* [n_books] */, const int32_t *phrase_len,
                           const int32_t *phrase_words, const double *phrase_bonus, int device, wfst_bias_books **out);
int wfst_bias_books_info(const wfst_bias_books *b, int32_t *n_books, int64_t *total_phrases, int64_t *total_nodes,
                         int32_t *n_phrases, int32_t *n_nodes, int32_t *n_words /* [n_books] each */, int64_t *device_bytes);
void wfst_bias_books_free(wfst_bias_books *b);
int wfst_decoder_biased_words_sparse(wfst_decoder *d, const int32_t *channels, int32_t n, int32_t use_final_probs,
                                     const wfst_bias_books *books, const int32_t *book_of /* [n], -1: no book; NULL: none has one */,
                                     int32_t n_set /* 1..16, shared by the listed channels */,
                                     const double *settings /* [n_set][4]: graph_scale, acoustic_scale, word_penalty, boost_scale */,
                                     int32_t cap_words, int32_t cap_hits, int64_t max_cells /* reachable cells of one channel; 0 = default */,
                                     int64_t round_cells /* cost cells of one round; 0 = default */,
                                     int32_t *status /* [n] */, int64_t *n_cells /* [n] */, int32_t *found, int32_t *n_arcs, int32_t *n_hyp,
                                     int32_t *n_hits /* [n][n_set] */,
                                     int32_t *hyp_words, int32_t *begin_frame, int32_t *end_frame /* [n][n_set][cap_words] */,
                                     int32_t *hit_phrase, int32_t *hit_word /* [n][n_set][cap_hits] */,
                                     double *biased_cost, double *bonus /* [n][n_set] */, float *tot_score, float *lm_score /* [n][n_set] */);

/* ---- forced alignment: exact Viterbi of a channel's scores against the utterance's own graph -----------------------------------------
 * Everything above reads the lattice the search left behind; a transcript that is not in the lattice is not found there.  This call
 * aligns a channel's SCORES against a small graph the caller brings per utterance -- a compiled training graph, a transcript
 * acceptor -- as Kaldi's align-compiled-mapped does: the numerator alignment and its cost for MMI / sMBR (wfst_decoder_sequence_stats'
 * `ref`), word and phone times of a known transcript, "does this transcript fit this audio at all", realignment between training
 * stages.  The scores are the ones the decoder holds on the device; one launch per round (forced_align_kernel), one workgroup per
 * listed channel.
 *
 * A graph G is given in the reference format, exactly as wfst_graph_from_arrays takes it: start, ONE final_state, wfst_state_info x S,
 * wfst_arc x A, every state's input-epsilon arcs first.  An arc's INDEX is its position in G's arc array.  ll(f, tid) is row f of the
 * channel's scores at column tid2pdf[tid] of the DECODER's own graph (wfst_graph_set_tid2pdf), column tid without a map: what the
 * search itself reads.  T is the number of frames aligned.
 * The table V[f][s], 0 <= f <= T, float32, every operation rounded on its own (no fused multiply-add):
 *   V[0][start] has the seed 0.
 *   an emitting arc a: s -> t (ilabel != 0) out of frame f < T offers (V[f][s] + (-ll(f, ilabel))) + w(a) to V[f + 1][t]: the acoustic
 *     cost first, then the graph cost (cur_cost + ac_cost + graph_cost, as the search adds them);
 *   an epsilon arc a: s -> t (ilabel 0) offers V[f][s] + w(a) to V[f][t], inside frame f;
 *   a candidate x that is not finite (x - x != 0: NaN or an infinity) is no candidate;
 *   V[f][t] is the least candidate, +inf without one.
 * Epsilon weights may be negative.  A graph whose epsilon arcs form a cycle, of any weight, is refused when the set is created, so a
 * frame is a DAG and V is well defined.
 * The backpointer of a reached (f, t): the seed at (0, start); everywhere else, among the candidates that equal V[f][t] exactly, an
 * emitting arc before an epsilon arc, then the least arc index: the oracle's tie rule 1 for arrivals.  It does not depend on any
 * order in which the device visits arcs.
 * found = V[T][final_state] is finite; path_cost = V[T][final_state]; the path follows the backpointers from (T, final_state) to the
 * seed.  With the path's arcs in order: hop_arc[0 .. n_hops) their arc indices; alignment[f] the ilabel of the emitting arc out of
 * frame f, or label_map[ilabel] where the caller gives a map (n_tid + 1 entries >= 0, entry 0 unused, as
 * wfst_decoder_frame_posteriors takes it: the row is wfst_decoder_sequence_stats' ref as it stands); words[0 .. n_words) the non-zero
 * olabels in path order; word_frame[k] the frame of the SOURCE state of the arc that carries word k (wfst_decoder_align_words' begin
 * frame); tot_score and lm_score wfst_lattice_to_vector's two sums over the hop list: sequential float32 sums of graph + acoustic and
 * of graph, epsilon hops included, the acoustic cost being -ll(f, ilabel), 0 on an epsilon hop.  found = 0 zeroes every output of
 * that channel with status OK.  T = 0 is legal: the path is epsilon arcs from start to final_state, or nothing if they are one state.
 * Min-plus in float32 with a fixed tie rule: the results are bit for bit reproducible.
 *
 * wfst_align_graphs: n_graphs graphs uploaded together; states and arcs are the graphs' arrays one behind the other.  Creation
 * validates on the host BEFORE it touches a device: everything wfst_graph_from_arrays checks of the format, labels >= 0, nextstate in
 * range, no epsilon cycle (WFST_E_FORMAT, the graph and a state of the cycle named in wfst_last_error).  It then builds an in-arc
 * index by destination state (emitting records first, arc index ascending: the first exact minimum in record order is the tie
 * rule's winner), every state's level in the epsilon DAG (a frame's epsilon arcs are settled in `depth` ordered passes) and the list
 * of distinct ilabels of each graph: 32 bytes per arc and 8 to 12 per state on the device.  wfst_align_graphs_info: the totals, per graph
 * (arrays of n_graphs, any may be NULL) n_states, n_arcs, the largest ilabel, the epsilon depth and the distinct ilabels, and the
 * device bytes.
 *
 * wfst_decoder_force_align works on best-path, lattice and biglm decoders alike and on every initialised channel -- live, finalized,
 * or fed with max_num_frames = 0 and never decoded -- because it reads scores only.  The frames: those a library-held history holds
 * (wfst_decoder_advance_host, wfst_decoder_advance_chunk); for a channel fed through wfst_decoder_advance the frames DECODED of the
 * caller's matrix, whose rows that call's contract keeps valid.  n_frames_in[i] (NULL: all -1) may ask for fewer, -1 = all; more is
 * WFST_E_ARG.  graph_of[i] is the graph of listed channel i.  The call runs behind the channels' ingests, as wfst_decoder_get_scores
 * does, and is synchronous, as wfst_decoder_align_words is.  The decoder's state is only read: decoding goes on bit for bit as
 * without the call.  Any output pointer may be NULL; a capacity is looked at only where its rows are given.
 * A failure of ONE channel goes into status[i] and the call still returns WFST_OK: a table of (T + 1) x n_states cells beyond
 * max_cells (WFST_E_CAPACITY, n_frames[i] = T, everything else zero; 0 = wfst_decoder_align_words' default bound, 65 536 x 65), or
 * T > cap_frames, n_hops > cap_hops or n_words > cap_words (WFST_E_CAPACITY: n_frames / n_hops / n_words are the room needed, so that
 * the call can be repeated once; what fits is written and the scores stand).
 * The call itself fails, before any device work, with WFST_E_ARG (a NULL decoder, channel list, graph set or graph_of; a graph_of
 * out of range; a graph whose largest ilabel lies beyond the tid2pdf map or whose transition-ids read a column beyond the score
 * stride; n_frames_in below -1 or above the frames held; a negative capacity or max_cells; label_map given with n_tid < 1, with a
 * negative entry or shorter than a listed graph's largest ilabel; a bad or duplicate channel list; a graph set on another device)
 * or WFST_E_STATE (a listed channel never initialised).
 * The workspace is the decoder's, grown on demand: 4 bytes per (frame, state) cell for the backpointers, 4 per possible hop for the
 * traced path, and 8 per state for the two cost rows of a graph of more than WFST_FALIGN_LDS_STATES states -- up to that size the rows
 * live on chip, and the answers do not depend on which.  Lists whose cells pass 256 MiB together are taken in rounds; an explicit
 * max_cells bounds the cells of one round as well (at least one channel per round), and with them the workspace.
 * wfst_decoder_force_align_workspace: the bytes held.
 * Not computed here: a beam (the table is dense), graphs compiled from transcripts and lexicons, Kaldi table I/O, device-resident
 * outputs.  (Per-arc posteriors of the numerator graph: wfst_decoder_graph_posteriors.) */
#define WFST_FALIGN_LDS_STATES 4096 /* states of a graph whose two float32 cost rows live in LDS (32 KiB of a workgroup's 64) */
typedef struct wfst_align_graphs wfst_align_graphs;
int wfst_align_graphs_create(int32_t n_graphs, const int32_t *start, const int32_t *final_state, const int32_t *n_states,
                             const int32_t *n_arcs /* [n_graphs] each */, const wfst_state_info *states /* concatenated */,
                             const wfst_arc *arcs /* concatenated */, int device, wfst_align_graphs **out);
/* The same from files, one graph each, in any format wfst_graph_load reads (WFST_E_IO / WFST_E_FORMAT with the file named). */
int wfst_align_graphs_load(int32_t n_graphs, const char *const *paths, int device, wfst_align_graphs **out);
int wfst_align_graphs_info(const wfst_align_graphs *g, int32_t *n_graphs, int64_t *total_states, int64_t *total_arcs,
                           int32_t *n_states, int32_t *n_arcs, int32_t *max_ilabel, int32_t *eps_depth,
                           int32_t *n_labels /* [n_graphs] each */, int64_t *device_bytes);
void wfst_align_graphs_free(wfst_align_graphs *g);
int wfst_decoder_force_align(wfst_decoder *d, const int32_t *channels, int32_t n, const wfst_align_graphs *graphs,
                             const int32_t *graph_of /* [n] */, const int32_t *n_frames_in /* [n], -1 = all; NULL: all */,
                             const int32_t *label_map /* NULL, or n_tid + 1 entries, entry 0 unused */, int32_t n_tid,
                             int64_t max_cells /* (T + 1) x states; 0 = default */,
                             int32_t cap_frames, int32_t cap_hops, int32_t cap_words,
                             int32_t *status /* [n] */, int32_t *found, int32_t *n_frames /* [n] */,
                             float *path_cost, float *tot_score, float *lm_score /* [n] */,
                             int32_t *n_hops /* [n] */, int32_t *hop_arc /* [n][cap_hops] */, int32_t *alignment /* [n][cap_frames] */,
                             int32_t *n_words /* [n] */, int32_t *words, int32_t *word_frame /* [n][cap_words] */);
int wfst_decoder_force_align_workspace(wfst_decoder *d, int64_t *bytes);

/* ---- graph posteriors: forward-backward of a channel's scores over the utterance's own graph ------------------------------------------
 * wfst_decoder_force_align gives the BEST path through a per-utterance graph; this call sums over ALL of them, in the log semiring:
 * the log-likelihood of the graph given the scores (the numerator term of MMI: objective = log_like - log_z, with log_z from
 * wfst_decoder_sequence_stats), per frame the posterior of every class (soft numerators: CTC-style graphs, lattice-free MMI numerators,
 * flat-start training, transcripts with alternative pronunciations or optional silence; how sure an alignment is) and per arc its
 * expected count.  One launch per stage and round (graphpost_kernel, graphpost_pack_kernel and, with dense rows,
 * graphpost_dense_kernel), one workgroup per listed channel.
 *
 * The graph G, ll(f, tid) (the column through the DECODER's tid2pdf), T, the frames a channel holds, n_frames_in, graph_of, "runs
 * behind the channels' ingests" and "the decoder's state is only read" are wfst_decoder_force_align's, unchanged.  Everything below is
 * float64.  graph_scale gs and acoustic_scale as are finite and >= 0.
 *   An epsilon arc a costs c(a) = gs * (double)w(a); an emitting arc out of frame f costs c(f, a) = as * (double)x + gs * (double)w(a)
 *   with x = float32(-ll(f, ilabel)): two products and one sum, each rounded on its own (no fused multiply-add).  An arc whose w(a) is
 *   not finite is no arc; an emitting arc whose x is not finite (NaN or either infinity) is no arc at that frame.
 *   Forward: alpha[0][start] has the seed 0; alpha[f][t] is -log sum exp(-x) over its terms: the seed where it applies,
 *   alpha[f - 1][s] + c(f - 1, a) over its emitting in-arcs and alpha[f][s] + c(a) over its epsilon in-arcs.  A state has its terms
 *   complete before a state with an epsilon path from it reads it (the graph set's epsilon levels).  A sum is m - log(sum exp(-(x - m)))
 *   with m the least term, +inf without a finite term.
 *   Backward: beta[T][final_state] has the term 0; beta[f][s] is the same sum over its out-arcs: c(f, a) + beta[f + 1][t] for emitting
 *   arcs while f < T, c(a) + beta[f][t] for epsilon arcs; the levels -- the longest epsilon path OUT of a state -- ascending.
 *   tot = alpha[T][final_state]; found = tot is finite; log_like = -tot.  found = 0 zeroes every output of that channel with status OK
 *   and leaves its dense rows untouched.
 *   gamma(f, a) = exp(-(alpha[f][s] + c + beta[f'][t] - tot)), f' = f + 1 for an emitting arc and f for an epsilon arc; 0 where the
 *   exponent is not finite.
 * Per frame f < T and class v -- the ilabel of an emitting arc out of f, or label_map[ilabel] exactly as wfst_decoder_frame_posteriors
 * takes a map -- post(f, v) is the sum of gamma(f, a) over the arcs of that class.  The list of frame f holds the classes with
 * post > 0 and post >= min_post by class id ASCENDING; n_distinct[f] counts the classes with post > 0 before the threshold and
 * frame_mass[f] sums them all: 1 to rounding on a found channel.  frame_off, entry_class, entry_post, n_entries and the cap_frames /
 * cap_entries answers have wfst_decoder_frame_posteriors' format; cap_frames = cap_entries = 0: no lists are handed out, as in
 * wfst_decoder_sequence_stats.
 * arc_occ (NULL: none) gets per listed channel arc_occ[i][a] for a < n_arcs[i], the arcs of its graph by arc index: the expected
 * number of times a path takes arc a, the sum of gamma(f, a) over f < T for an emitting arc and over f <= T for an epsilon arc.
 * The dense output: grad, grad_pitch, grad_frames, n_cols, grad_scale and consumer_stream are exactly
 * wfst_decoder_sequence_stats'.  Rows 0 .. min(T, grad_frames[i]) - 1 get n_cols zeros, then float32(grad_scale * post(f, v)) at column
 * v for every class with post > 0; min_post does not thin the dense rows; nothing else is touched.  A label_map class >= n_cols is
 * refused, without a map n_cols must exceed the largest ilabel of every listed graph, and the writes are ordered against
 * consumer_stream both ways, as there.
 * The ORDER of a sum follows the device's records: results are reproducible to rounding, NOT bit for bit against another
 * implementation.  No float is accumulated by an atomic: two identical calls return identical bytes.
 * Beside wfst_decoder_force_align: at scales (1, 1) and with finite scores and weights found is that call's, except that force_align
 * drops a path whose float32 running sum overflows, while here the "no arc" rule is per arc, in float64.
 *
 * A failure of ONE channel goes into status[i] and the call still returns WFST_OK: a table of (T + 1) x n_states cells beyond
 * max_cells (WFST_E_CAPACITY, n_frames[i] = T, everything else zero; 0 = wfst_decoder_force_align's default bound), T > cap_frames or
 * n_entries > cap_entries (WFST_E_CAPACITY: n_frames[i] and n_entries[i] are the room needed, the lists stay zero, log_like, the
 * occupancies and the dense rows stand), or arc_occ given with n_arcs[i] > cap_arcs (WFST_E_CAPACITY: n_arcs[i] is the room needed,
 * that row stays zero and everything else stands), so that the call can be repeated once.
 * The call itself fails, before any device work, with WFST_E_ARG (everything wfst_decoder_force_align names; a scale that is
 * negative or not finite; min_post that is NaN or outside 0..1; cap_frames or cap_entries < 1 unless both are 0; cap_arcs < 0; a
 * grad_scale that is not finite; grad without grad_frames, n_cols < 1, a negative grad_frames, a pitch below n_cols, a grad pointer
 * not aligned to 4 bytes, a class beyond n_cols as above) or WFST_E_STATE (a listed channel never initialised).  Any output pointer
 * may be NULL.
 * The workspace is the decoder's, grown on demand: 8 bytes per (frame, state) cell for alpha, 24 per arc, 8 per (frame, class of the
 * graph), and 16 per state for the two rolling rows of a graph of more than WFST_GPOST_LDS_STATES states -- up to that size the rows
 * live on chip, and the answers do not depend on which.  Lists whose cells pass 256 MiB together are taken in rounds; an explicit
 * max_cells bounds the cells of one round as well.  The by-source tables of a graph set are built on the set's first call, under
 * a lock (a set may be shared between decoders and threads), take 16 bytes per arc and 12 per state on the device, and go with
 * wfst_align_graphs_free; wfst_align_graphs_info answers what it did before.  wfst_decoder_graph_posteriors_workspace: the bytes held.
 * Not computed here: a beam (the table is dense), an "add into the rows" dense mode and a soft-numerator MMI in one call (the caller
 * combines the tensors of this call and wfst_decoder_sequence_stats), a half-precision dense output, graph compilation. */
#define WFST_GPOST_LDS_STATES 2048 /* states of a graph whose two float64 rows live in LDS (32 KiB of a workgroup's 64) */
int wfst_decoder_graph_posteriors(wfst_decoder *d, const int32_t *channels, int32_t n, const wfst_align_graphs *graphs,
                                  const int32_t *graph_of /* [n] */, const int32_t *n_frames_in /* [n], -1 = all; NULL: all */,
                                  const int32_t *label_map /* NULL, or n_tid + 1 entries, entry 0 unused */, int32_t n_tid,
                                  double graph_scale, double acoustic_scale, double min_post,
                                  int64_t max_cells /* (T + 1) x states; 0 = default */,
                                  int32_t cap_frames, int32_t cap_entries, int32_t cap_arcs,
                                  void *const *grad /* NULL, or [n] device pointers */, const int64_t *grad_pitch /* [n], floats */,
                                  const int32_t *grad_frames /* [n] */, int32_t n_cols, double grad_scale, void *consumer_stream,
                                  int32_t *status /* [n] */, int32_t *found, int32_t *n_frames /* [n] */, double *log_like /* [n] */,
                                  int32_t *n_entries, int32_t *n_arcs /* [n] */, int32_t *frame_off /* [n][cap_frames + 1] */,
                                  int32_t *n_distinct /* [n][cap_frames] */, double *frame_mass /* [n][cap_frames] */,
                                  int32_t *entry_class /* [n][cap_entries] */, double *entry_post /* [n][cap_entries] */,
                                  double *arc_occ /* [n][cap_arcs], or NULL */);
int wfst_decoder_graph_posteriors_workspace(wfst_decoder *d, int64_t *bytes);

/* The service's n-best (OnlineClgLatticeFastDecoder::GetNbest, kaldi-nnet3/kaldi-online-nnet3-my-
 * decoder.cc:50-105: GetRawLattice -> DeterminizeLatticeWrapper -> NShortestPath ->
 * ConvertNbestToVector, then LatticeToVector per path) of channels of a lattice-mode decoder, finalized
 * or mid-utterance (the service's partial n-best; what is alive now, see wfst_decoder_get_raw_lattice): the n (<= 16) lowest-cost DISTINCT word sequences of the pruned lattice, cheapest first,
 * each with tot_score = sum(graph + acoustic) and lm_score = sum(graph) of its best path.
 * Computed on the device by a k-best search over the raw lattice (no determinized lattice is
 * materialised).  Outputs for the i-th listed channel: n_paths[i]; n_words[i*n + k];
 * words[(i*n + k)*max_words ...] (first max_words ids); tot_score / lm_score [i*n + k].
 * n_paths[i] == 0: no lattice (see wfst_decoder_get_raw_lattice).  WFST_E_CAPACITY if a lattice is
 * larger than the search's working set (32768 .. 262144 states depending on the channel count;
 * the message gives the numbers). */
int wfst_decoder_get_nbest(wfst_decoder *d, const int32_t *channels, int32_t n_channels, int32_t n,
                           int32_t max_words, int32_t *n_paths, int32_t *n_words, int32_t *words,
                           float *tot_score, float *lm_score);

/* Kernel timing for the roofline report: while enabled, every expand / boundary launch of
 * wfst_decoder_advance is bracketed by HIP events recorded on the decoder's own stream.
 * wfst_decoder_get_profile waits for the stream and returns, since the last enable:
 * [0] expand kernel (ProcessEmitting inner loop -> candidate buckets), [1] insert kernel
 * (FindOrAddToken in LDS hash tables -> tokens), [2] closure kernel (ProcessNonemitting fixpoint +
 * GetCutoff + next_cutoff seed).  Leave it off in production runs. */
int wfst_decoder_set_profiling(wfst_decoder *d, int32_t enable);
int wfst_decoder_get_profile(wfst_decoder *d, double ms[3], int64_t launches[3]);
/* The time during which at least one launch of each kernel class was executing (union of the launches'
 * intervals): with several channel groups the launches of different groups overlap, and the sum of their
 * durations (wfst_decoder_get_profile) counts the shared time once per group. */
int wfst_decoder_get_profile_busy(wfst_decoder *d, double busy_ms[3]);
/* Which of the library's kernel paths this decoder runs (for benchmarks and tests: the N > 1 ranks of a sharded run must report
 * what the N = 1 run does): {staged expansion, two launches per frame, frames between two token-collection checks (gc_stride),
 * degree codes in the tokens, log-likelihood row staged in LDS (known after the first advance), best token found by the
 * expansion, the per-frame limit degrades (soft limit), channel groups}. */
int wfst_decoder_get_path_flags(wfst_decoder *d, int32_t flags[8]);
/* The number of channel groups the decoder runs with (wfst_options.channel_groups, resolved). */
int wfst_decoder_channel_groups(wfst_decoder *d);

/* Lattice-mode work counters of a channel since its last init, for the byte model of the back-pruning (bench.py): {forward links
 * recorded, links priced by the PruneActiveTokens / FinalizeDecoding walks (one per link and sweep), tokens priced by them,
 * tokens + links scanned by the compactions, tokens + links the compactions moved}. */
int wfst_decoder_get_lattice_stats(wfst_decoder *d, int32_t channel, int64_t stats[5]);

/* How long the device took to determinize the lattice of `channel` that the decoder holds (the last wfst_decoder_get_determinized_lattice
 * / prefetch of it), in milliseconds of the device's constant clock: the time of that lattice's own workgroup, not of the launch
 * (which lasts as long as its largest lattice).  Beside the reference's DeterminizeLatticeWrapper timed on a host core (bench.py).
 * WFST_E_STATE if no determinized lattice of the channel is held. */
int wfst_decoder_get_determinizer_ms(wfst_decoder *d, int32_t channel, float *ms);

/* Running back-pruning passes (PruneActiveTokens, base-inl.h:439-607) of the channel since its last init whose several-workgroup
 * pricing of the never-priced frames was ABANDONED -- a workgroup waited 40 ms for its siblings (a chip shared with other
 * processes) -- and done over by the one-workgroup walk: the same lattice, later; never an error.  -1: the several-workgroup pass is
 * off on this device (its grid would not be resident at once). */
int wfst_decoder_get_prune_raw_abandoned(wfst_decoder *d, int32_t channel, int32_t *n_passes);

/* Frames of the channel's utterance (since its last init) on which the per-frame token limit BOUND: best-path decoders on
 * the fused graph rows treat wfst_limits.max_tokens_per_frame as a max_active, not as a capacity -- a frame that reaches
 * more distinct states keeps every token (the arena permitting) and the search goes on from the limit-th cheapest, exactly
 * what the reference does at that max_active (GetCutoff, base-inl.h:188-203) where it grows its hash and pools instead
 * (base-inl.h:237-244, util/mem-pool.h:17-65).  0 = the result is the one the caller's config alone defines.  Lattice and
 * biglm decoders report 0 and keep WFST_E_CAPACITY for that limit. */
int wfst_decoder_get_degraded_frames(wfst_decoder *d, int32_t channel, int32_t *n_frames);

/* Frontier of a channel after the last decoded frame (states and costs, unordered); for tests.
 * Returns the number of tokens (may exceed cap; only cap are written). */
int wfst_decoder_get_frontier(wfst_decoder *d, int32_t channel, int32_t cap, int32_t *states,
                              float *costs);

/* ---- endpoint detection (streaming) --------------------------------------------------------------------------------------
 * Kaldi's online2/online-endpoint.{h,cc}, which the reference's online decoder calls after every AdvanceDecoding
 * (EndpointDetected(const OnlineEndpointConfig&), kaldi-nnet3/kaldi-online-nnet3-my-decoder.h:360-362; the service loop:
 * v1-asr/asr-source.h:280-287).  A rule fires iff
 *   (utterance_length > trailing_silence || !must_contain_nonsilence) && trailing_silence >= min_trailing_silence &&
 *   relative_cost <= max_relative_cost && utterance_length >= min_utterance_length
 * with utterance_length = num_frames_decoded * frame_shift and trailing_silence = trailing_silence_frames * frame_shift (f32);
 * rules 1..5 are tried in order, the first that fires is reported.  No frames decoded: not detected. */
typedef struct {                  /* OnlineEndpointRule */
  int32_t must_contain_nonsilence;
  float min_trailing_silence;     /* seconds */
  float max_relative_cost;        /* +inf: no limit */
  float min_utterance_length;     /* seconds */
} wfst_endpoint_rule;

typedef struct {                  /* OnlineEndpointConfig (--endpoint.*) */
  wfst_endpoint_rule rule[5];     /* rule1 .. rule5 */
  float frame_shift;              /* seconds per decoded frame: 0.01, or 0.03 for frame-subsampled chain models */
  int32_t n_silence_phones;       /* --endpoint.silence-phones=a:b:c -- non-empty, no duplicates, every phone > 0 */
  const int32_t *silence_phones;  /* (copied by the calls that take a config) */
} wfst_endpoint_config;

/* Kaldi's defaults: rule1 {0, 5.0, inf, 0}, rule2 {1, 0.5, 2.0, 0}, rule3 {1, 1.0, 8.0, 0}, rule4 {1, 2.0, inf, 0},
 * rule5 {0, 0, inf, 20.0}; frame_shift 0.01; no silence phones (the caller must name them). */
void wfst_endpoint_config_default(wfst_endpoint_config *cfg);

/* TransitionModel::TransitionIdToPhone as a table: tid2phone[tid] for tid 1..n_tid (entry 0 unused, the layout of
 * wfst_graph_set_tid2pdf).  WFST_E_ARG if an arc's ilabel exceeds n_tid or a phone is negative.  Host-side only. */
int wfst_graph_set_tid2phone(wfst_graph *g, const int32_t *tid2phone, int32_t n_tid);

/* The endpoint configuration of a decoder: checked (WFST_E_ARG: empty or duplicate silence list, a phone <= 0,
 * frame_shift <= 0), then the silence set is turned into a bitmap over transition-ids (through the graph's tid2phone) in
 * device memory.  WFST_E_STATE: the graph has no tid2phone; WFST_E_ARG: a biglm decoder (not supported). */
int wfst_decoder_set_endpoint_config(wfst_decoder *d, const wfst_endpoint_config *cfg);

/* EndpointDetected (kaldi-online-nnet3-my-decoder.h:360-362) for a LIST of channels mid-utterance, one launch: per listed
 * channel trailing_frames[i] = TrailingSilenceLength (the silence hops at the end of the best path GetBestPath(use_final_probs =
 * false) reports, epsilon hops skipped), relative_cost[i] = FinalRelativeCost (ComputeFinalCosts, base-inl.h:670-720: cost of
 * the best token on the final state - cost of the best token, +inf without one), rule[i] = the rule that fired (1..5, 0: none)
 * and detected[i] = rule[i] != 0.  Enqueued behind the listed channels' own work (as wfst_decoder_best_path_enqueue), then
 * waited for.  WFST_E_ARG: a biglm decoder (not supported); WFST_E_STATE: no endpoint config set, or a listed channel not
 * initialised or already finalized.  A channel with no frame decoded yet has no path (trailing_frames[i] = -1, relative_cost[i] = +inf,
 * not detected, as Kaldi's EndpointDetected returns false there).  A channel whose utterance ended in a device error has no path: trailing_frames[i] = -1,
 * relative_cost[i] = +inf, not detected -- the others' results stand and the call returns WFST_OK (the error itself is
 * reported by the channel's next advance / sync / best path).  Any output pointer may be NULL. */
int wfst_decoder_endpoint_detected(wfst_decoder *d, const int32_t *channels, int32_t n, int32_t *detected, int32_t *rule,
                                   int32_t *trailing_frames, float *relative_cost);

/* The rules alone, on the host (no device): *rule = the first of rules 1..5 that fires for these inputs, 0 if none (and 0 for
 * num_frames_decoded == 0).  The config is checked as wfst_decoder_set_endpoint_config checks it; WFST_E_ARG also for
 * trailing_frames outside [0, num_frames_decoded]. */
int wfst_endpoint_rules(const wfst_endpoint_config *cfg, int32_t num_frames_decoded, int32_t trailing_frames, float relative_cost,
                        int32_t *rule);

/* ---- partial results with a stable word prefix (streaming) ------------------------------------------------------------------
 * What the reference's services hand to their per-chunk callback (best_str, partial, endpoint_detected)
 * (gpu-asr/v1-gpu-asr-task.h:70-76, option print-partial-hypotheses, gpu-asr/gpu-worker-pool-itf.h:19-48; the CPU service after
 * every AdvanceDecoding: GetBestPathTxt, kaldi-nnet3/kaldi-online-nnet3-my-decoder.cc:122-137) -- without a traceback of the
 * whole utterance per chunk, and with the part of it that can no longer change told apart.
 *
 * For every listed channel (initialised, not finalized), with nd frames decoded:
 *   words[i * cap_words .. + n_words[i])  the non-zero olabels of the path wfst_decoder_get_best_path(use_final_probs = 0) reports
 *                       now, start -> end: wfst_lattice_to_vector's words on that call's hops;
 *   n_stable[i] <= n_words[i]: the first n_stable[i] words are a prefix of the words of every later partial result of the utterance
 *                       and of its best path after FinalizeDecoding, with either value of use_final_probs;
 *   stable_frame[i]     the frame of the commit token (0: none yet): the newest token below the last PruneActiveTokens pass
 *                       ((nd - 1) / prune_interval * prune_interval) that every token of the frontier descends from.
 * n_stable and stable_frame never decrease within an utterance; wfst_decoder_init starts a channel from zero.  The device work of a
 * call follows nd - stable_frame, not nd.
 *
 * wfst_decoder_partial_enqueue puts the work on the results stream behind the listed channels' own enqueued work and returns at
 * once; _ready says (never blocks) whether the results have landed; _fetch waits if need be and writes them out;
 * wfst_decoder_get_partial is the halves in a row.  One partial request may be outstanding per decoder (a second _enqueue:
 * WFST_E_STATE), beside an outstanding best-path request or none; the listed channels must not be advanced or initialised in
 * between.  WFST_E_ARG: a biglm decoder (not supported), cap_words <= 0, a bad list; WFST_E_STATE: a listed channel not initialised
 * or already finalized; WFST_E_CAPACITY: a result longer than cap_words (n_words[i] is then the needed size, the first cap_words
 * words are written), or longer than the decoder's max_frames words -- the per-channel workspace's limit: no word of that
 * channel is written then, n_words[i] exceeds max_frames and no cap_words helps; the channel's commit state stays as it was.  No frame decoded: n_words[i] = n_stable[i] = 0.  A channel whose
 * utterance ended in a device error reports n_words[i] = 0; the others' results stand and the call returns WFST_OK.  Any output
 * pointer may be NULL. */
int wfst_decoder_partial_enqueue(wfst_decoder *d, const int32_t *channels, int32_t n, int32_t cap_words);
int wfst_decoder_partial_ready(wfst_decoder *d);
int wfst_decoder_partial_fetch(wfst_decoder *d, int32_t *words /* [n][cap_words] */, int32_t *n_words, int32_t *n_stable,
                               int32_t *stable_frame);
int wfst_decoder_get_partial(wfst_decoder *d, const int32_t *channels, int32_t n, int32_t cap_words, int32_t *words,
                             int32_t *n_words, int32_t *n_stable, int32_t *stable_frame);

/* ---- an utterance's result in one launch: words, word times and scores ----------------------------------------------------
 * What the reference's services deliver per utterance, without the hop list: OnebestLatticeToString's word string, tot_score and
 * lm_score (kaldi-nnet3/kaldi-online-nnet3-my-decoder.cc:107-121) and the (start, end) time of every word that the GPU service's
 * BestPathAndAlignCallback(const std::string &, AlignStruct &, bool, bool) hands over (AlignStruct =
 * vector<pair<string, pair<float, float>>>, gpu-asr/gpu-worker-pool-itf.h:85-97) -- times here are frames; the caller multiplies
 * by its frame shift.  Any decoder kind, biglm included; mid-utterance or after FinalizeDecoding.
 *
 * Let h_0 .. h_{H-1} be the hops wfst_decoder_get_best_path(channel, use_final_probs) would return now, F(j) the number of hops
 * i < j with ilabel_i != 0 (the frame hop j consumes if it is emitting) and E = F(H).  For listed channel i:
 *   n_hops[i] = H (0: the reference's "no path" -- n_words[i] = 0, both scores 0);
 *   words[i * cap_words .. + n_words[i])  the non-zero olabels in hop order; word k sits at hop j_k;
 *   begin_frame[.. k] = F(j_k);
 *   end_frame[.. k]   (exclusive) with L_k = begin_frame of word k + 1, or E for the last word:
 *                     without a silence list L_k; with one, 1 + the largest F(i) over the emitting hops i in [j_k, j_{k+1})
 *                     ([j_k, H) for the last word) whose phone tid2phone[ilabel_i] is not a silence phone, and begin_frame[k] if
 *                     there is none;
 *   tot_score[i], lm_score[i]  bit for bit what wfst_lattice_to_vector_batch returns for those hops (float sums of
 *                     graph + acoustic and of graph, in hop order).
 * Where an HCLG places a word's olabel relative to the word's phones is a property of the graph, so begin_frame is the frame of
 * the label-carrying arc, not of the word's first phone.
 *
 * Errors and state follow wfst_decoder_get_best_path and its halves: the same use_final_probs rule after FinalizeDecoding
 * (WFST_E_STATE), a device error of another channel's utterance does not fail the request, one words request may be outstanding
 * per decoder (a second _enqueue: WFST_E_STATE) beside an outstanding best-path or partial request, and the listed channels must
 * not be advanced or initialised in between.  WFST_E_CAPACITY: a channel has more words than cap_words -- n_words[i] is the
 * needed size, the first cap_words words and times are written, scores and n_hops are valid.  There is no hop capacity: the
 * library sizes the walk's scratch itself, and when a path outgrows it _fetch grows it and runs the list again.  Any output
 * pointer may be NULL. */
int wfst_decoder_words_enqueue(wfst_decoder *d, const int32_t *channels, int32_t n, int32_t use_final_probs, int32_t cap_words);
int wfst_decoder_words_ready(wfst_decoder *d);
int wfst_decoder_words_fetch(wfst_decoder *d, int32_t *words /* [n][cap_words] */, int32_t *begin_frame, int32_t *end_frame,
                             int32_t *n_words, int32_t *n_hops, float *tot_score, float *lm_score);
int wfst_decoder_get_words(wfst_decoder *d, const int32_t *channels, int32_t n, int32_t use_final_probs, int32_t cap_words,
                           int32_t *words, int32_t *begin_frame, int32_t *end_frame, int32_t *n_words, int32_t *n_hops,
                           float *tot_score, float *lm_score);

/* The silence phones that word end times skip (the silence list of the reference's word alignment and of
 * --endpoint.silence-phones): any decoder kind, biglm included.  The list is checked as wfst_decoder_set_endpoint_config checks
 * its own (WFST_E_ARG: a phone <= 0 or a duplicate) and needs the graph's tid2phone (WFST_E_STATE without); n == 0 clears it.
 * wfst_decoder_set_endpoint_config sets this list too.  WFST_E_STATE while a words request is outstanding. */
int wfst_decoder_set_silence_phones(wfst_decoder *d, const int32_t *phones, int32_t n);

/* ---- acoustic-model chunks ingested on the device: f16 / bf16 / f32 rows, acoustic scale, log priors ---------------------------
 * What the reference's decodable does between the network and the search: the CLI's --acoustic-scale (default 0.1) and
 * DecodableMatrixScaledMapped(trans_model, loglikes, acoustic_scale) (kaldi-nnet3bin/kaldi-hclg-my-decoder.cc:37-41,107); its own
 * network's decodable returns `_acoustic_scale * output[...]` (nnet/nnet-nnet.h:212-232) behind the prior layer's
 * AddVecToRows(out, frames, cols, _log_priors, -1.0, 1.0) (nnet/nnet-layer.cc:30, nnet/nnet-nnet.cc:156-164).  An acoustic model on
 * the same device hands over one chunk of rows per step, in its own precision, and keeps nothing:
 *
 *   hist[have + r][j] = (float(x[r][j]) - log_priors[j]) * acoustic_scale
 *
 * computed in float32 as written (no FMA), where `have` is the number of frames the channel's history held before the call.
 * Without priors nothing is subtracted, with acoustic_scale == 1.0f nothing is multiplied (float32 in, neither: a bit copy);
 * float16 -> float32 and bfloat16 -> float32 are exact, denormals kept.
 *
 * wfst_decoder_set_score_transform: the transform of every later chunk (default: scale 1, no priors).  log_priors (host, n_cols
 * floats) are copied to the device; NULL with n_cols == 0 clears them.  WFST_E_STATE while a channel holds frames of an
 * unfinished utterance in its history (a transform does not change mid-utterance); WFST_E_ARG: n_cols < 0, priors without
 * n_cols > 0 or n_cols without priors, a scale that is not finite.
 *
 * wfst_decoder_advance_chunk: for listed channel channels[i] (NULL: all), rows[i] is a DEVICE pointer to the first of
 * n_new_frames[i] NEW rows of n_cols elements of `dtype`, row_pitch[i] elements apart (NULL: n_cols); 0 rows are allowed and
 * rows[i] may then be NULL.  The rows go into the decoder-owned history wfst_decoder_advance_host fills (same allocation, same
 * regrowth; wfst_decoder_init resets a channel) with a stride of n_cols rounded up to a multiple of 4, pad columns written as 0;
 * a channel may be fed by both calls in one utterance only if the strides agree.  Then AdvanceDecoding(max_num_frames) as in
 * wfst_decoder_advance (0: ingest only).  Returns when everything is ENQUEUED.
 * Ordering: producer_stream is the hipStream_t whose enqueued work writes the rows (NULL: the legacy default stream).  The library
 * records an event on it; the ingest runs behind that event on the decoder's upload stream -- not on the decode stream, so the
 * model's next forward pass never waits for a search -- and both the decode stream and producer_stream wait for the ingest:
 * whatever the caller enqueues on producer_stream after the call may overwrite the chunk buffers (a caller that reuses them from
 * elsewhere synchronises itself).  WFST_STREAM_NONE: the rows are complete and the caller keeps them until wfst_decoder_sync or
 * a getter; no event touches a caller stream.  The chunk buffers are never read again after the ingest: the "rows must stay valid
 * until the next init" contract of wfst_decoder_advance does not apply.
 * WFST_E_ARG, before any device work: unknown dtype; n_cols <= 0, not above the graph's largest log-likelihood column, or not
 * the priors' n_cols; a pitch below n_cols; a negative n_new_frames; a pointer not aligned to its element size; a bad or
 * duplicate channel list; a NULL row pointer with frames to append; a stride other than that of the frames the histories hold.
 * WFST_E_STATE: a channel not initialised or already finalized.  WFST_E_CAPACITY, before any work is enqueued:
 * have + n_new_frames[i] > wfst_limits.max_frames.
 *
 * wfst_decoder_get_scores: rows [first_frame, first_frame + n_frames) of the channel's library-held history, n_cols floats each
 * (the n_cols of the chunk call; the stride of wfst_decoder_advance_host), copied to the host behind the channel's ingests -- for
 * tests and debugging, like wfst_decoder_get_frontier.  WFST_E_STATE: the channel reads the caller's own matrix
 * (wfst_decoder_advance); WFST_E_ARG: a range outside the frames held. */
#define WFST_DTYPE_F32 0
#define WFST_DTYPE_F16 1   /* IEEE binary16 */
#define WFST_DTYPE_BF16 2
#define WFST_STREAM_NONE ((void *)(intptr_t)-1)

int wfst_decoder_set_score_transform(wfst_decoder *d, float acoustic_scale, const float *log_priors /* host, n_cols floats, or NULL */,
                                     int32_t n_cols);
int wfst_decoder_advance_chunk(wfst_decoder *d, const int32_t *channels, int32_t n,
                               const void *const *rows,        /* [n] DEVICE pointer to the first NEW row of entry i */
                               const int32_t *n_new_frames,    /* [n] rows appended to entry i's utterance (0 allowed, rows[i] may then be NULL) */
                               const int64_t *row_pitch,       /* [n] elements between rows; NULL: n_cols */
                               int32_t dtype, int32_t n_cols, void *producer_stream, int32_t max_num_frames);
int wfst_decoder_get_scores(wfst_decoder *d, int32_t channel, int32_t first_frame, int32_t n_frames,
                            float *out /* host, [n_frames][n_cols] */);

#ifdef __cplusplus
}
#endif
#endif /* WFST_DECODER_H_ */
