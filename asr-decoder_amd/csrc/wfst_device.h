// Device-side data layout of the batched WFST token-passing decoder (gfx950 / MI355X).
//
// Everything a kernel touches is described here; wfst_capi.cc owns the allocations and
// wfst_kernels.hip the code.  Reference structures replaced (paths relative to the reference's
// src/): Fst state/arc arrays (newfst/optimize-fst.h:60-61), HashList<StateId,Token*>
// (util/hash-list.h), StdToken + backpointer (my-decoder/online-decoder-base.h:52-84).
#ifndef WFST_DEVICE_H_
#define WFST_DEVICE_H_

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace wfst {

// ---- graph in HBM: CSR with the row header in front of the row ---------------------------
// rows[]: ONE int4 array in "ext" index space.  State s owns slots [pos(s), pos(s)+1+num_arcs(s)),
//   pos(s) increasing in s (rows are packed, with padding slots where a row would otherwise
//   straddle one more 64-byte line than it needs), and IS identified by pos(s) everywhere on the device.
//   rows[pos(s)]      header {(n_emit << 12) | n_eps, original state id, pseudo arcs of s (fused closures),
//                     (first entry in eps_flat[] << 3) | entries, entries = 0: not flattened}
//   rows[pos(s)+1+i]  arc i {ll_col, next_eps(nextstate), weight bits, pos(nextstate)}; epsilon arcs
//                     first.  ll_col = log-likelihood column of the ilabel (tid2pdf applied at
//                     upload), -1 for an input-epsilon arc.
//   One gather finds a token's arcs, and its cache lines hold the arcs themselves (a separate
//   8-byte state table cost one more 64-byte fabric request per expanded token).
//   next_eps word: bit 31 = the state has outgoing epsilon arcs; bits 30..0 = 1 + its ordinal among
//   the graph's epsilon-TARGET states (0 = no epsilon arc enters it).
// eps_flat[]: the WHOLE epsilon closure of a state as a list, for states whose closure has at most
//   kFlatMax paths (nearly all): entry {epsilon-target ordinal of the path's end, last arc (row
//   index), (parent entry + 1) | 8 if the end state has epsilon arcs out, weight bits of the last arc},
//   parents before children.  The closure kernel prices such a state's closure in ONE round
//   (cost of an entry = cost of its parent + weight, in path order, every prefix below the cutoff)
//   instead of one round per epsilon hop.
// FUSED closures (GraphDev::fused, best-path decoders): the epsilon closure folded into the expansion.
//   Behind a state's emitting arcs sit its PSEUDO ARCS, header.z of them: one per (emitting arc i ->
//   s', path p of s''s whole epsilon closure) = {ll_col of arc i, index of p in pseudo[], weight bits of
//   arc i, row of p's end state}.  pseudo[p] = {last arc of the path (row index) | flags of its end
//   state, parent path or -1, weight bits of the last arc, hops}.  Expanding a pseudo arc prices
//   ProcessEmitting's arrival at s' and ProcessNonemitting's walk from it in one go:
//   ((cur + ac) + w_i) + w_1 + ... + w_k, summed in path order; the candidate it yields is an epsilon
//   arrival (kEpsRec: loses an exact cost tie to an emitting arc; its token's predecessor is found at
//   traceback, kPrevUnresolved).  FindOrAddToken is a minimum and float addition is monotone, so
//   taking the minimum over the arrivals of EVERY candidate at s' equals the reference's walk from the
//   final cost of the token at s'.  Needs: no epsilon cycle, closures of <= 48 paths and <=
//   kPseudoDepthMax hops, no negative epsilon weight (a path then never costs less than its prefix, so
//   one cutoff test on the arrival stands for the test at every hop).  Lattice decoders use the fused rows too
//   (the epsilon arrivals come through the insert launch; one flat pass then lists the frame's epsilon links);
//   biglm decoders, and graphs that do not qualify, run the separate closure pass instead and ignore the pseudo arcs.
// arc_ilabel[], arc_olabel[], arc_src[] (source row | bit 31 for an epsilon arc): cold arrays in
//   the same index space.  eps_target_state[k] = row of epsilon-target ordinal k.
struct GraphDev {
  const int4 *arcs;  // rows[]
  const int32_t *arc_ilabel;
  const int32_t *arc_olabel;
  const int32_t *arc_src;
  const int32_t *eps_target_state;
  const int4 *eps_flat;
  const int4 *pseudo;
  const float *pseudo_w;   // [paths][kPseudoDepthMax]: a path's epsilon weights root to leaf (paths of three hops or more read them)
  int32_t fused;
  int32_t col_mask;     // log-likelihood column of an arc = its first word & col_mask (kColMask where the degree codes ride above it)
  int32_t degcode;      // the arcs of the fused rows carry the degree code of their target state (below)
  int32_t start, final_state, n_states, n_arcs;
  uint32_t start_eps;   // next_eps word of the start state
  int32_t n_eps_targets;
};

// ---- LM automaton in HBM (biglm, BASELINE configs[3]): the reference's Fsa (newlm/arpa2fsa.h:216-247) ----
// st[s]    {first arc, arc count, back-off weight bits, back-off state}
// words[a] word id of arc a (the arcs of a state are word-id sorted: binary search, arpa2fsa.h:194-210;
//          state 0, the empty history, is indexed directly by word id, arpa2fsa.cc:253-254)
// wt[a]    {weight bits, destination state}
// Weights are natural-log probabilities, already rescaled (the old LM by -1).
struct LmDev {
  const int4 *st;
  const int32_t *words;
  const int2 *wt;
  int32_t n_states, n_arcs;
  int32_t bos, eos;
  int32_t start;       // ComposeArpaLm::Start(): the state after <s> (compose-arpalm.cc:5-13)
  int32_t start_arcs;  // arcs of state 0 = word ids it can be asked for
  // arcs of every state but the empty history as ONE open-addressed table {state, word, weight bits, destination} (empty: state
  // -1): Fsa::GetArc's binary search over a state's word-sorted arcs (arpa2fsa.h:194-210) is three to five dependent loads,
  // a probe of this table is one -- and an LM step is a chain of such look-ups (back-off by back-off, LM by LM) that a whole
  // wavefront waits for.  Same arcs, same answers.
  const int4 *hash;
  uint32_t hmask;      // table size - 1 (a power of two, at most a quarter full)
};
__host__ __device__ inline uint32_t lm_hash(int32_t state, int32_t word) {
  uint32_t h = (uint32_t)state * 0x9E3779B1u ^ ((uint32_t)word + 0x7F4A7C15u) * 0x85EBCA77u;
  h ^= h >> 15;
  return h * 0x2C1B3C6Du;
}

#if defined(__HIPCC__)
// Fsa::GetArc (newlm/arpa2fsa.cc:244-262): the arc of LM state `id` for `word`, false if the state
// has none (the caller backs off).  State 0 (empty history) is indexed by word id directly
// (SearchStartArc, arpa2fsa.h:211-214; wfst_decoder_create_biglm and, for the second pass, check_lm_pair
// check the graph's labels against its arc count); the others by binary search over their word-id
// sorted arcs (SearchArc, :194-210).
__device__ __forceinline__ bool fsa_getarc(const LmDev &L, int id, int word, float *w, int *to) {
  if (id == 0) {   // (state 0's arcs start the arc array: wfst_lm_from_arrays)
    const int2 x = L.wt[word];
    *w = __int_as_float(x.x);
    *to = x.y;
    return true;
  }
  // every other state: one probe of the LM's (state, word) table instead of a binary search over the state's arcs
  uint32_t slot = lm_hash(id, word) & L.hmask;
  for (;;) {
    const int4 e = L.hash[slot];
    if (e.x == id && e.y == word) { *w = __int_as_float(e.z); *to = e.w; return true; }
    if (e.x < 0) return false;
    slot = (slot + 1) & L.hmask;
  }
}
// ComposeArpaLm::GetArc (newlm/compose-arpalm.cc:52-70): back off until the word is found; the cost
// is minus the sum of the back-off weights and the arc weight, summed in that order.
__device__ __forceinline__ void lm_getarc(const LmDev &L, int s, int word, int *next, float *value1) {
  float weight = 0.0f, w_arc = 0.0f;
  int to = 0;
  while (!fsa_getarc(L, s, word, &w_arc, &to)) {
    const int4 st = L.st[s];
    w_arc = __int_as_float(st.z);
    s = st.w;
    weight += w_arc;
  }
  weight += w_arc;
  *value1 = -1 * weight;
  *next = to;
}
// ComposeArpaLm::Final (compose-arpalm.cc:15-29)
__device__ __forceinline__ float lm_final_cost(const LmDev &L, int s) {
  int next;
  float v;
  lm_getarc(L, s, L.eos, &next, &v);
  return v;
}
#endif

constexpr int kEpsBits = 12;
constexpr int kFlatMax = 4;  // paths of a flattened epsilon closure (3 bits in the header word)
constexpr uint32_t kEpsMask = (1u << kEpsBits) - 1;
constexpr uint32_t kFlagOutEps = 0x80000000u;     // state has outgoing input-epsilon arcs
constexpr uint32_t kFlagEpsTarget = 0x40000000u;  // some input-epsilon arc enters the state
constexpr uint32_t kFlagMask = kFlagOutEps | kFlagEpsTarget;
constexpr uint32_t kEpsWon = 0x80000000u;         // in a packed eps-table value: won by an epsilon arc
constexpr uint32_t kEpsOutBit = 0x40000000u;      // in a packed eps-table value: the state has epsilon arcs out
// token/record flag bits from an arc's next_eps word
// DEGREE CODE (fused best-path decoders): what a token needs to find its arcs WITHOUT reading its row header first --
// the state's epsilon arcs (2 bits, <= 3), emitting arcs (4 bits, <= 15) and pseudo arcs (5 bits, <= 31); kCodeUnknown
// where a count does not fit (the expansion then reads the header, as it always did).  On the graph side it rides in the
// arc's first word above the log-likelihood column (graphs whose ilabels stay below 2^20); in a candidate record -- and so,
// verbatim, in the token the insert kernel writes -- in bits nothing else uses: its two low bits in bits 30..31 of the arc
// word (the closure pass's flags, idle without a closure pass), the rest above the source-token index (arenas of up to
// 2^22 tokens leave 9 bits), or, for an epsilon arrival, in the unresolved-backpointer sentinel: z = kPrevUnresolved - rest.
// The row-header loads it saves are a fifth of the expansion (10 of 51 us per launch, measured by replay).
constexpr int kColBits = 20;
constexpr int32_t kColMask = (1 << kColBits) - 1;
constexpr uint32_t kCodeUnknown = 0x7FFu;
constexpr int kCodeRestBits = 9;   // code >> 2
__host__ __device__ inline uint32_t pack_code(uint32_t n_eps, uint32_t n_emit, uint32_t n_pseudo) {
  if (n_eps > 3u || n_emit > 15u || n_pseudo > 31u) return kCodeUnknown;
  const uint32_t c = n_eps | (n_emit << 2) | (n_pseudo << 6);
  return c == kCodeUnknown ? kCodeUnknown : c;   // (3, 15, 31) itself reads as unknown: the header path is always right
}

__host__ __device__ inline uint32_t flags_of(uint32_t next_eps) {
  return (next_eps & kFlagOutEps) | ((next_eps & 0x7FFFFFFFu) ? kFlagEpsTarget : 0u);
}
// THE TIE RULE (deviation 3).  Of the arrivals at a token that equal its final cost bit for bit the winner is
// the least under (emitting arc before epsilon arrival, then row index of the arc -- of a fused or flattened path: of its last arc);
// rows are in file order (states ascending, a state's arcs as uploaded, epsilon arcs first).  That is the low word of every packed
// (f2o(cost) << 32 | ...) minimum: kEpsRec / kEpsWon sit above the arc index, the other bits beside it depend on the target state
// alone.  The best path ends in the cheapest token, then the lowest row, biglm then the lowest pair_keys[] value (bp_frontier).
// biglm, equal (cost, arc) from several source tokens: the lowest source pair_keys[] value (insert pass 1b, bp_scan_eps_pred).
constexpr uint32_t kEpsRec = 0x20000000u;          // in a candidate record / token: an epsilon arrival (fused closures)
constexpr uint32_t kArcMask = ~(kFlagMask | kEpsRec);  // arc (row) indices are < 2^29
constexpr uint32_t kNoArc = kArcMask;              // "no arc" (root token), flags kept beside it
constexpr int kPseudoDepthMax = 8;                 // hops of a fused closure path
constexpr int32_t kEmptyKey = -1;
constexpr int32_t kPrevUnresolved = -3;  // token won by an epsilon arc: backpointer found at traceback
constexpr unsigned long long kEmptyVal = ~0ull;

// error bits (ChanCtl::error)
constexpr int kErrTableFull = 1, kErrArenaFull = 2, kErrFrontierFull = 4, kErrWorklistFull = 8,
              kErrFramesFull = 16, kErrBucketFull = 32, kErrLinksFull = 64, kErrPairsFull = 128,
              kErrInternal = 256;   // an invariant of the kernels did not hold (never expected; reported, not papered over)

// ---- per-channel control block (one 128-byte line each) ----------------------------------
struct __attribute__((aligned(128))) ChanCtl {
  int32_t n_decoded;     // NumFramesDecoded()
  int32_t front_begin;   // arena index of the current frontier's first token
  int32_t front_count;   // tokens in the current frontier
  int32_t active;        // this frame step processes the channel
  uint32_t bound;        // orderable next_cutoff, tightened during expansion (atomicMin)
  float cur_cutoff;      // GetCutoff() result for the frame being expanded
  float adaptive_beam;
  int32_t peak_tokens;
  unsigned long long best_next;  // min (orderable cost << 32 | arena index) over the new frame (best_row decoders: | graph row; staged
                                 // best_row decoders: set by the EXPANSION -- the cheapest candidate is the cheapest token)
  int32_t eps_occ;       // occupied slots of the epsilon table   } one 8-byte word: the insert
  int32_t wl_n;          // epsilon-closure seeds queued          } workgroups bump both at once
  int32_t error;         // sticky kErr* bits
  int32_t finalized;
  // one 8-byte word: two-launch decoders allocate an item's tokens (add to the low half) and count the item out (subtract from
  // the high half) with 64-bit atomics on it, so the workgroup that counts the LAST item out learns the frame's token count
  // from the same answer (kFrameErrBit: an item of this frame could not write its tokens)
  int32_t new_count;     // tokens of the frame being built (atomicAdd by the insert workgroups)
  int32_t items_left;    // fused best-path decoders: insert work items of the frame not finished yet (the workgroup that
                         // finishes the last one closes the frame and prepares the next: frame_boundary_fused)
  unsigned long long cnt_N, cnt_E, cnt_Z, cnt_tok, cnt_rec;  // work counters since init
  int32_t link_count;    // lattice mode: forward links recorded so far (atomicAdd)
  int32_t lat_arcs;      // lattice mode, after lattice_prune_kernel: surviving links in lat_arcs[]
  int32_t lat_toks;      //   "   surviving tokens in lat_toks[]
  int32_t tiles_left;    // expansion tiles of the frame not finished yet (the last one plans the insert items)
  union {
    int32_t pair_count;  // biglm: LM pair states interned since InitDecoding (atomicAdd)
    int32_t stores_left; // two-launch decoders: insert items of the frame whose token stores have not all landed yet (counted down,
                         // behind every wave's drain, AFTER the item has counted itself out of items_left: the frame boundary waits
                         // for it only where GetCutoff has to look at the frame's tokens)
  };
  int32_t pruned_upto;   // lattice mode: NumFramesDecoded() at the last back-pruning pass (frames below hold extras)
};
static_assert(offsetof(ChanCtl, new_count) % 8 == 0 && offsetof(ChanCtl, items_left) == offsetof(ChanCtl, new_count) + 4, "the {new_count, items_left} word");
constexpr int32_t kRiskyBit = 1 << 29;   // in items_left (plan_channel): the frame's boundary may have to read the frame's tokens
constexpr unsigned long long kFrameErrBit = 1ull << 62;   // in the {new_count, items_left} word (items_left stays below 2^16)
static_assert(sizeof(ChanCtl) == 128, "ChanCtl must be one 128-byte line");

// One 256/512-token tile of a channel's frontier, listed by prep_frame for the expansion: everything
// a workgroup needs to start, in one 32-byte load (instead of tile -> channel -> control block ->
// log-likelihood pointer, three dependent loads).
struct __attribute__((aligned(32))) TileDesc {
  int32_t chan;
  int32_t tok_begin;    // arena index of the tile's first token
  int32_t tok_count;    // tokens in the tile (<= tile size)
  float cutoff;         // GetCutoff() of the frame
  float adaptive_beam;
  int32_t pad;
  const float *llrow;   // log-likelihood row of the frame being decoded
};
static_assert(sizeof(TileDesc) == 32, "TileDesc is one 32-byte load");

// one arc of the pruned lattice (lattice mode)
struct __attribute__((aligned(32))) LatArc {
  int32_t src_tok, dst_tok;  // arena indices
  int32_t ilabel, olabel;
  float graph, acoustic;
  int32_t src_frame, is_eps;
};
static_assert(sizeof(LatArc) == 32, "LatArc is two 16-byte stores");

// per channel-group frame counters, double buffered by step parity
struct FrameCtl {
  int32_t total_tiles[2];  // tiles published by prep_frame for the step of that parity
  int32_t ticket[2];       // dynamic tile dispenser of expand_kernel
  int32_t n_items[2];      // insert work items listed by plan_channel (expand's last tile of a channel)
  int32_t item_ticket[2];  // dynamic item dispenser of insert_kernel
  int32_t n_small[2];      // of those items, the light ones: listed from the END of items[] so that the
                           // insert workgroups take the heavy items first (longest-first keeps the tail short)
  int32_t pad[6];
};

// ---- decoder (batch of channels) ---------------------------------------------------------
// Per channel c:
//   tok[c][arena_cap]           int4 {state, cost bits, prev token (arena index, -1 root),
//                               winning arc | flags of the state}; frame f = tokens
//                               [frame_off[f], frame_off[f+1]); the newest frame is the frontier
//   frame_off[c][max_frames+2], cutoff_hist[c][max_frames+2] (cutoff of frame f's closure)
//   bucket[c][P][bucket_cap]    int4 candidate records {nextstate, cost bits, source token,
//                               arc | flags(nextstate)}, partition = top bits of hash(nextstate)
//   bucket_cnt[c][P]
//   eps table, direct mapped: eps_vals[c][K] (orderable cost << 32 | kEpsWon? | arc) and
//                               eps_toki[c][K] indexed by the epsilon-target ordinal of a state,
//                               eps_occ_list[c][...] = ordinals touched this frame (for clearing)
//   worklist[c][2][wl_cap]      epsilon-closure frontiers (slots of the eps table)
struct DecoderDev {
  GraphDev g;
  ChanCtl *ctl;
  int4 *tok;
  int32_t *frame_off;
  float *cutoff_hist;
  int4 *bucket;
  int32_t *bucket_cnt;
  int32_t prune_raw_min; // ... for channels with at least this many never-priced links (wfst_options.debug 0x800: 0, every channel)
  int32_t closure_slabs; // lattice decoders on the fused rows: workgroups per channel of a closure launch (they share the frame's epsilon links)
  int32_t link_delta;    // lattice decoders on the fused rows: a forward link's 4th word is (link cost - cost of its destination token) -- the float the
                         // back-pruning computes from the two anyway (base-inl.h:524-526), known when the link is recorded: a link is priced from the
                         // destination's extra alone; elsewhere (iterated closures: a token's cost may still improve) the link cost itself
  int32_t prune_raw;     // lattice mode: a running back-pruning pass prices its raw frames with several workgroups per channel (wfst_kernels.hip: lattice_prune_raw_*)
  int32_t *prune_par;    // [c][kPruneParInts]: lattice mode -- what a running back-pruning pass hands to its compaction launches (wfst_kernels.hip: kPrParInts)
  int32_t *emit_cnt;     // [c][32] (a line each): lattice mode on the fused rows -- entries of the channel's emitter list (the tokens of the
                         // frame being built that have epsilon arcs out: listed by the insert launch in the channel's worklist space,
                         // read and reset by the closure launch's epsilon_links)
  unsigned long long *eps_vals;
  int32_t *eps_toki;
  int32_t *eps_occ_list;        // [c][wl_cap] ordinals touched this frame
  int32_t *eps_won_list;        // [c][wl_cap] ordinals whose token an epsilon arc won this frame
  int4 *worklist;               // [c][2][wl_cap] {eps-table slot, state, cost bits, 0}
  // lattice mode (wfst_limits.lattice_links > 0): every forward link the reference would hold after
  // FinalizeDecoding is among links[c][0..link_count): {source token, destination token, arc,
  // cost bits of (source cost + acoustic) + graph}; segment k = links whose destination is on
  // frame k = [link_off[k], link_off[k+1]): the emitting links from frame k-1 first
  // [link_off[k], link_mid[k]), then the epsilon links inside frame k [link_mid[k], link_off[k+1]).
  // extra[c][token] = {orderable extra_cost (base-inl.h:482-572), cost bits of the token}, kept up to
  // date by the back-pruning passes (prune_pass: every prune_interval frames and at FinalizeDecoding),
  // which also REMOVE the dead tokens and links and move the survivors down, so that tok[] / links[]
  // hold the surviving history plus the raw frames since the last pass.  lattice_emit_kernel resolves
  // what is alive into lat_arcs[c][0..ctl.lat_arcs) and lat_toks[c][0..ctl.lat_toks) for GetRawLattice.
  int4 *links;
  int32_t *link_off, *link_mid;  // [c][max_frames+3]
  uint2 *extra;
  int32_t *remap;               // [c][arena_cap] scratch of the back-pruning passes (previous extras, then new indices)
  LatArc *lat_arcs;
  unsigned long long *lat_stats;  // [c][4] since InitDecoding: {forward links recorded, links priced by the back-pruning walks (one per
                                  // link and sweep), tokens priced by them, tokens + links scanned by the compactions | moved << 32 ... see wfst_decoder_get_lattice_stats}
  int4 *lat_toks;               // {arena index, graph state id, cost bits, frame | final << 30}
  int64_t link_cap;
  int32_t lat_arc_cap, lat_tok_cap;
  int32_t lattice;
  FrameCtl *fctl;               // [n_groups]
  TileDesc *tiles;              // [n_groups][tile_cap] tiles of the coming frame
  int32_t tile_cap;
  int32_t tok_idx_bits;         // bits of a token's backpointer that hold the arena index (31: all of them; less: a degree code above)
  int32_t degcode;              // tokens and records carry degree codes (fused rows, packed graph, arena small enough)
  int32_t *items;               // [n_groups][item_cap] channel << 16 | first partition << 8 | group size
  int32_t item_cap;
  int32_t *item_pref;           // [n_groups][item_cap][64]: entry i of an item = records in its first i + 1 buckets (plan_channel writes the
                                // prefix it has in registers; the insert workgroup gets it with the item instead of loading the counters behind it)
  const float *const *ll_base;  // [n_channels] device pointers to row 0 of each utterance matrix
  int32_t n_channels;
  int32_t stride;               // floats per log-likelihood row
  int32_t n_part, log2part;     // hash partitions per channel (power of two, <= 64)
  int32_t lds_slots, log2lds;   // LDS hash slots per partition workgroup (4096 or 8192)
  int32_t bucket_cap;           // records per bucket
  int32_t joint_max;            // insert: most records a group of partitions may hold to share one workgroup
  int32_t ecap;                 // = n_eps_targets (entries of eps_vals / eps_toki per channel)
  int32_t max_tok;              // tokens per frame
  int32_t wl_cap;
  int32_t max_frames;
  int64_t arena_cap;
  int64_t gc_reserve;           // best-path decoders: the token collection's mark lies this far below arena_cap (gc_base_mark)
  // config (LatticeFasterDecoderConfig)
  float beam, lattice_beam, beam_delta, prune_scale;
  int32_t max_active, min_active, prune_interval;
  // biglm mode (wfst_decoder_create_biglm): a token is identified by (graph row, LM pair state), the
  // reference's 64-bit PairId (my-decoder/online-decoder-mempool-base-biglm.h:77-90).
  //   pair_keys[c][pair_cap]  the channel's LM pair-state table, DiffArpaLm's _state_map/_state_vec
  //                           (newlm/diff-lm.h:92-103) as one open-addressed array: slot = pair id,
  //                           value = old-LM state | new-LM state << 32; emptied by InitDecoding
  //                           (DiffArpaLm::Reset)
  //   tok_lm[c][arena_cap]    pair id of each token;  bucket_lm[c][P][bucket_cap] of each candidate record
  //   eps_keys[c][ecap]       the epsilon table is HASHED in this mode (the state alone no longer
  //                           identifies a token): open-addressed keys (row | pair << 32) beside
  //                           eps_vals / eps_toki, ecap a power of two
  int32_t fused;  // the graph's fused closures are in use (best-path, non-biglm decoder on a graph that has them)
  // Two launches per frame (fused best-path decoders whose max_active / min_active can never bind: GetCutoff is then
  // best + beam and needs no look at the tokens): the insert workgroup that finishes a channel's last work item closes the
  // frame and prepares the next one (frame_boundary_fused), so the third launch of a frame disappears -- except on every
  // gc_stride-th frame of an advance call, which runs the classic three launches: the closure kernel there checks whether the
  // token arena wants collecting (the arena's reserve covers gc_stride + 1 frames at the per-frame limit).
  // best_row: ChanCtl::best_next carries the best token's graph ROW in its low word instead of its arena index (all the
  // seeding of next_cutoff needs, with no token read behind other workgroups' stores; ties on the best cost then go to the
  // lowest row: deterministic, where the arena order is not).
  int32_t two_launch, gc_stride, best_row;
  // seed_tiles (best_row decoders): next_cutoff's seed from the best token's arcs (base-inl.h:282-300) is computed by the
  // EXPANSION -- one extra tile per channel, listed first (TileDesc with tok_count 0: tok_begin = the best token's row, cutoff
  // = its cost) -- instead of by the frame boundary, whose serial tail it was three dependent round trips of; the tiles read
  // next_cutoff afresh every round, so the seed (and every other tile's tightening) reaches them as soon as it lands.
  int32_t seed_tiles;
  int32_t staged;   // fused (non-biglm) decoders: expand_kernel_staged (the tile's arcs staged in LDS by gather DMA) instead of expand_kernel_fused
  int32_t soft_limit;   // fused best-path decoders: max_tokens_per_frame is not a capacity but a max_active -- a frame may hold more tokens
                        // (while the arena and the candidate buckets take them); GetCutoff then tightens to the limit-th cheapest
  int32_t *degraded;    // [c] frames of the utterance on which that happened (wfst_decoder_get_degraded_frames)
  int32_t st_tile_tokens;   // staged expansion: frontier tokens per tile (wfst_options.tile_tokens; at most the kernel's 256 threads)
  int32_t best_exp; // staged best_row decoders: ChanCtl::best_next is set by the expansion (the insert launch does not look for the best token)
  int32_t ll_row;   // staged decoders: the tile's whole log-likelihood row is staged in LDS too (rows of at most 3072 columns, a multiple of
                    // four, 16-byte aligned: set by wfst_decoder_advance from the matrices it is handed); 0: one 4-byte gather per arc slot
  int32_t big;
  LmDev lm_old, lm_new;
  unsigned long long *pair_keys;
  int32_t *pair_list;           // [n_channels][pair_cap] the table slots claimed since InitDecoding, in claiming order (clear_pairs_kernel)
  int32_t pair_cap;             // power of two
  int32_t *tok_lm;
  int32_t *bucket_lm;
  unsigned long long *eps_keys;
  // pruned live lattices (wfst_decoder_set_live_lattice_prune): live_prune != 0 -- launch_lattice_emit serves a live channel from its
  // SNAPSHOT, FinalizeDecoding's pruning priced into snap_extra[c][arena_cap] ({orderable extra, cost bits}, as extra[]) by
  // lattice_snapshot_kernel with the channel left as it is; nullptr until the mode is first set
  uint2 *snap_extra;
  int32_t live_prune;
  unsigned long long *dbg_t;  // [64] phase timers (WFST_DBG & 32): sums, maxima, counts
  int32_t dbg;  // WFST_DBG ablation bits (timing experiments only; results are wrong when set)
};

// ---- n-best (wfst_nbest.hip) ---------------------------------------------------------------
struct NbEntry {            // one partial path of a lattice state's k-best list
  float tot, lm;            // sum of (graph + acoustic), sum of graph, in path order
  unsigned long long hash;  // of the word sequence so far
  int32_t prev;             // (source lattice state << 4) | entry, -1 at the start state
  int32_t word;             // olabel of the arc that led here (0: none)
};
static_assert(sizeof(NbEntry) == 24, "NbEntry");
struct NbestDev {
  NbEntry *list;            // [c][tok_cap][K]
  int32_t *scratch;         // [c][scratch_ints]
  int32_t tok_cap, arc_cap, K;
  int64_t scratch_ints;     // 4 * arc_cap (in-arc records) + 3 * tok_cap + 1 + 3 * (max_frames + 2), rounded up to a multiple of 4
  int32_t *out_n;           // [cnt]      paths found, or -1: the lattice exceeds tok_cap / arc_cap
  int32_t *out_nwords;      // [cnt][n]
  int32_t *out_words;       // [cnt][n][max_words]
  float *out_tot, *out_lm;  // [cnt][n]
  int32_t n, max_words;
};
void launch_nbest(const DecoderDev &D, const NbestDev &N, const int32_t *chan_list_dev, int cnt, hipStream_t s);

// ---- lattice determinization (wfst_determinize.hip / wfst_determinize.h) -------------------------------
struct DetCaps;
}  // namespace wfst
#include "wfst_determinize.h"
namespace wfst {
constexpr int kPruneParInts = 64;   // ints of a channel's block of DecoderDev::prune_par
constexpr int kPrRawAbandon = 37;       // ... [37]: the raw launch gave this pass up (a workgroup of the channel waited too long at a meeting): lattice_prune_kernel prices the raw frames itself
constexpr int kPrRawAbandonCount = 38;  // ... [38]: how often since InitDecoding (wfst_decoder_get_prune_raw_abandoned)
constexpr int kClSlabWord = 60;     // ... of which [60, 62), one 64-bit word: the closure launch's meeting of a channel's workgroups (finalize_frame)

struct DetDev {
  int32_t *ws;                  // [c][words_per_channel]: the lattice's CSR, then the determinizer's workspace
  int64_t words_per_channel;
  int32_t raw_states_cap, raw_arcs_cap;   // largest raw lattice taken
  DetCaps caps;
  int32_t *result;              // [cnt][4] {states, arcs, status, determinized states proper}
  int4 *out_a;                  // [cnt][out_cap] {src, dst, word, is-final-arc}
  float2 *out_w;                // [cnt][out_cap] {graph, acoustic}
  int32_t out_cap;
  unsigned long long *ticks;    // [cnt] how long the slot's workgroup ran, in ticks of the constant 100 MHz clock (wfst_decoder_get_determinizer_ms)
};
void launch_determinize(const DecoderDev &D, const DetDev &X, const int32_t *chan_list_dev, int cnt, hipStream_t s, int phase = 0);   // phase: wfst_determinize.hip
void launch_det_pack(const DetDev &X, int cnt, int4 *pack_a, float2 *pack_w, int64_t pack_cap, hipStream_t s);

// ---- n cheapest paths of a determinized / rescored lattice (wfst_nbest.hip: nbest_paths_kernel) --------------------------------
struct NbPathEntry { float cost; int32_t arc, rank, pad; };   // a partial path: its cost, the arc it arrives by (-1: the start), its rank in that arc's source list
struct NbPathsDev {
  const int4 *a;                // the lattice's arcs {src, dst, word, -} ...
  const float2 *w;              // ... and their {graph, acoustic} costs
  const int32_t *res;           // {states, arcs, status, determinized states proper} as determinize_kernel / compose2_kernel leave it
  const int32_t *fin;           // final flag per state, or null: the states from res[3] on
  int64_t in_stride, fin_stride;   // a batch: slot b's lattice sits at a / w + b * in_stride, res + 4 b, fin + b * fin_stride; its workspace,
                                // lists and outputs at b * ws_ints, b * list_cap, out + 4 b, out_off + b (n + 1), out_tot + b n, out_arcs + b out_cap
  int32_t n;                    // paths wanted (<= 4096)
  int32_t *ws;                  // scratch: 7 states + 4 max(states, arcs) + arcs + 16 ints
  int64_t ws_ints;
  NbPathEntry *lists;           // the states' lists, packed
  int64_t list_cap;
  int32_t *out;                 // {paths found, arcs on them, status (0 ok, 1 a capacity, 2 no input, 3 cyclic input), -}
  int32_t *out_off;             // [n + 1] first arc of each path in out_arcs
  float *out_tot;               // [n] cost of each path
  int32_t *out_arcs;            // arc indices (into a / w), path after path, front to back
  int32_t out_cap;
};
void launch_nbest_paths(const NbPathsDev &P, int n_slots, hipStream_t s, int small = 0);   // small: one wave per lattice (lattices of a few hundred states, short lists)
// the text of the paths a launch_nbest_paths over n_slots lattices left in P's buffers (nbest_words_kernel): packed = [n_slots][4] the
// slots' result words (P.out), then per (slot, path) kNbWordsHead ints {n_words, tot bits, lm bits, path cost bits} + cap_words words
constexpr int32_t kNbWordsHead = 4;
void launch_nbest_words(const NbPathsDev &P, int n_slots, int cap_words, int32_t *packed, hipStream_t s);

// ---- lattice-constrained word alignment (wfst_align.hip) -------------------------------------------------------------
// The cheapest path of a channel's raw lattice (lat_toks[] / lat_arcs[] as lattice_emit_kernel left them) that spells a given word
// sequence, for n_seqs sequences per listed channel (slot = position in the list).  align_index_kernel builds a slot's
// by-destination in-arc index once; align_kernel runs one (slot, sequence) pair per workgroup over it.
//   idx[slot][idx_ints]  recA int4[na_cap] {source state | is_eps << 31, olabel, graph bits, acoustic bits}, recB int4[na_cap]
//                        {graph state of the source token, ilabel, source frame, 0} (what the tie rule and the word times need),
//                        head[8] {status (kAln*), states, arcs, frames decoded, ...}, off[ns_cap + 1], cur[ns_cap],
//                        fbeg / fend / feps[fr_cap] (first state, one past the last state, "has epsilon arcs" of a frame)
//   cells[]              the pairs' tables d[state][len + 1] (orderable float bits, kAlnUnreached: no path), pair p at cell_off[p]
//                        (< 0: the pair is not run: seq_len -1, or a table beyond the caller's max_cells)
//   path[p][ns_cap]      the in-arc records of the traced path, last arc first
//   out[p]               kAlignHead ints {found, arcs on the path, tot bits, lm bits, error (kAln*), 0, 0, 0}, begin[cap_words],
//                        end[cap_words]
constexpr int32_t kAlignHead = 8;
constexpr uint32_t kAlnUnreached = 0xFFFFFFFFu;
constexpr int32_t kAlnNoLattice = 1, kAlnTooLarge = 2, kAlnChannelError = 3, kAlnCycle = 4, kAlnInternal = 5;
struct AlignDev {
  int32_t *idx;
  int64_t idx_ints;
  int32_t ns_cap, na_cap, fr_cap;
  const int32_t *seq_words;   // [cnt][n_seqs][cap_words]
  const int32_t *seq_len;     // [cnt][n_seqs]
  const int64_t *cell_off;    // [cnt][n_seqs]
  uint32_t *cells;
  int32_t *path;
  int32_t n_seqs, cap_words;
  const uint32_t *sil_bits;   // the silence bitmap over transition-ids 1..n_tid, or nullptr
  int32_t n_tid;
  int32_t *out;
};
inline int64_t align_idx_ints(int64_t ns_cap, int64_t na_cap, int64_t fr_cap) {
  return (8 * na_cap + 8 + (ns_cap + 1) + ns_cap + 3 * fr_cap + 3) & ~(int64_t)3;
}
void launch_align_index(const DecoderDev &D, const AlignDev &A, const int32_t *chan_list_dev, int cnt, hipStream_t s);
void launch_align(const DecoderDev &D, const AlignDev &A, const int32_t *chan_list_dev, int cnt, hipStream_t s);

// ---- lattice edit distance (wfst_nearest.hip) ---------------------------------------------------------------------------
// The path of a channel's raw lattice nearest a reference word sequence: least (word errors, cost), for n_refs references per listed
// channel, over the in-arc index align_index_kernel built (AlignDev::idx; the other fields of the AlignDev are not read).
//   cells[]              the pairs' tables v[state][len + 1]: errors << 32 | orderable float bits of the cost, kNrUnreached: no path;
//                        pair p at cell_off[p] (< 0: the pair is not run: ref_len -1, or a table beyond the caller's max_cells)
//   path[p][path_cap]    the traceback's steps, last first: kind << 30 | in-arc record (kind 3, the deletion step: no arc);
//                        path_cap >= ns_cap + cap_words
//   out[p]               kNearestHead ints {found, arcs on the path, tot bits, lm bits, error (kAln*), n_err, n_cor, n_sub, n_ins,
//                        n_del, n_hyp, 0}, hyp_words[cap_hyp], begin[cap_hyp], end[cap_hyp], ref_hyp[cap_words]
constexpr int32_t kNearestHead = 12;
constexpr unsigned long long kNrUnreached = ~0ull;
struct NearestDev {
  const int4 *lat_toks;       // DecoderDev::lat_toks, lat_tok_cap entries per channel
  int64_t lat_tok_cap;
  const int32_t *ref_words;   // [cnt][n_refs][cap_words]
  const int32_t *ref_len;     // [cnt][n_refs]
  const int64_t *cell_off;    // [cnt][n_refs], in cells
  unsigned long long *cells;
  int32_t *path;
  int32_t path_cap;
  int32_t n_refs, cap_words, cap_hyp;
  const uint32_t *sil_bits;   // the silence bitmap over transition-ids 1..n_tid, or nullptr
  int32_t n_tid;
  int32_t *out;
};
constexpr int64_t nearest_out_ints(int64_t cap_words, int64_t cap_hyp) { return kNearestHead + 3 * cap_hyp + cap_words; }
void launch_nearest(const AlignDev &A, const NearestDev &N, const int32_t *chan_list_dev, int cnt, hipStream_t s);

// ---- lattice posteriors and word confidences (wfst_posterior.hip) -----------------------------------------------------
// The sum-over-paths twin of the alignment: forward and backward costs of a listed channel's raw lattice in the log semiring, in
// float64, over the in-arc index align_index_kernel built (AlignDev::idx), and the statistic read from them for the sequences
// align_kernel has just placed in time (AlignDev::out, AlignDev::path).  posterior_kernel runs one workgroup per slot,
// confidence_kernel one per (slot, sequence) pair.
//   alpha / beta[slot][ns_cap]  forward / backward cost of a state (+inf: no path from the start / to a final state)
//   gamma[slot][na_cap]         the posterior of an arc, by in-arc record
//   done[slot][ns_cap]          the level rounds' flags: 0, or 1 + the round that summed the state
//   soff[slot][ns_cap]          the by-source table: the out-arcs of state s are sarc[s ? soff[s - 1] : 0 .. soff[s])
//   sarc[slot][na_cap]          {in-arc record, destination state}, grouped by source state
//   log_z[slot]                 -beta[0]; chan_err[slot]: 0 or kAlnCycle
//   out[p][1 + cap_words]       {path_logpost, word_post[cap_words]} of pair p (all zero where align_kernel found nothing)
struct PostDev {
  double *alpha, *beta, *gamma;
  int32_t *done, *soff;
  int2 *sarc;
  double *log_z;
  int32_t *chan_err;
  double graph_scale, acoustic_scale;
  double *out;
};
// bytes of a slot's share of the posterior workspace
inline int64_t post_slot_bytes(int64_t ns_cap, int64_t na_cap) { return 24 * ns_cap + 16 * na_cap; }
void launch_posterior(const DecoderDev &D, const AlignDev &A, const PostDev &P, const int32_t *chan_list_dev, int cnt, hipStream_t s);
void launch_confidence(const AlignDev &A, const PostDev &P, int cnt, hipStream_t s);

// ---- sentence and phrase posteriors (wfst_seqpost.hip) -----------------------------------------------------------------
// The log-semiring twin of align_kernel's table: the weight of ALL paths that spell a word sequence (mode 0), or that say a phrase
// somewhere (mode 1), over the in-arc index (AlignDev::idx) and posterior_kernel's alpha, beta and log_z (PostDev).  seqpost_kernel
// runs one workgroup per (slot, sequence) pair.  Of the AlignDev it reads idx, seq_words, seq_len, cell_off, n_seqs, cap_words and
//   cells[]              the pairs' tables of float64 cells, pair p at cell_off[p] (in cells; < 0: not run): S[state][len + 1] in
//                        mode 0, P[state][len] in mode 1
//   path[p][ns_cap]      the level of a state inside its frame (0, or 1 + the round that sums its row)
//   out[p]               kSeqPostHead ints {found, state frames of the lattice (frames decoded + 1), 0, 0, error (kAln*), 0, 0, 0}
// and of the PostDev alpha, beta, log_z, chan_err and the scales.
//   out[p]               seq_logpost of pair p (0 where nothing is found)
//   hit[p][cap_frames]   mode 1: hit_mass, written where the lattice's state frames fit cap_frames; nullptr: not asked for
constexpr int32_t kSeqPostHead = 8;
struct SeqPostDev {
  const int4 *lat_toks;       // DecoderDev::lat_toks, lat_tok_cap entries per channel
  int64_t lat_tok_cap;
  int32_t mode;               // 0 sentence, 1 phrase
  int32_t cap_frames;
  double *out;
  double *hit;
};
void launch_seqpost(const AlignDev &A, const PostDev &P, const SeqPostDev &Q, const int32_t *chan_list_dev, int cnt, hipStream_t s);

// ---- word alternatives per slot (wfst_altern.hip) ------------------------------------------------------------------------
// A confusion network pinned to the sequences align_kernel has placed in time: per cell of confidence_kernel's time axis the words
// the lattice says there with their posterior mass (slot_mass_kernel) and the mass of the paths that say nothing there
// (slot_none_kernel), over the in-arc index (AlignDev::idx), align_kernel's results (AlignDev::out) and posterior_kernel's alpha, beta,
// gamma, log_z and chan_err (PostDev).  One workgroup per (slot, sequence) pair each.  slot_none_kernel keeps its level flags in
// AlignDev::path[p][ns_cap], behind confidence_kernel's last read of it.
//   none[p][cap_words]             none_post (all zero where align_kernel found nothing)
//   alt_post / alt_word[p][cap_words][n_alts], n_distinct[p][cap_words]
//   acost[p][ns_cap]               A of a state, in the cell its frame lies in
//   early[p][cap_words]            per cell the mass of the complete paths that end in it
//   tab_key / tab_mass[p][tab_slots]  the table of a pair whose (cell, word) keys outgrow LDS: tab_slots a power of two above na_cap
struct AltDev {
  const int4 *lat_toks;       // DecoderDev::lat_toks, lat_tok_cap entries per channel
  int64_t lat_tok_cap;
  int32_t n_alts;
  double *none, *alt_post;
  int32_t *alt_word, *n_distinct;
  double *acost, *early;
  unsigned long long *tab_key;
  double *tab_mass;
  int64_t tab_slots;
};
void launch_slot_mass(const AlignDev &A, const PostDev &P, const AltDev &Q, int cnt, hipStream_t s);
void launch_slot_none(const AlignDev &A, const PostDev &P, const AltDev &Q, const int32_t *chan_list_dev, int cnt, hipStream_t s);

// ---- frame posteriors (wfst_framepost.hip) ---------------------------------------------------------------------------------
// Per frame of a listed channel's raw lattice the posterior mass of every class (the ilabel of an emitting arc, or label_map of it),
// over the in-arc index (AlignDev::idx) and posterior_kernel's gamma and chan_err (PostDev).  frame_post_kernel runs one workgroup
// per (slot, frame), frame_pack_kernel one per slot.
//   ws_key / ws_val[slot][na_cap]     the sort's pairs of a frame with more than kFramePostLdsRecs emitting arcs, at its record offset
//   st_class / st_post[slot][na_cap]  a frame's list, by class ascending, at the frame's record offset
//   st_cnt / st_distinct / st_mass[slot][fr_cap]  the list's length, n_distinct and frame_mass of a frame
//   out[slot]   kFramePostHead ints {n_frames, n_entries, 1: the rows do not hold them, 0, error (kAln*), 0, 0, 0},
//               frame_off[cap_frames + 1], n_distinct[cap_frames], entry_class[cap_entries]
//   dout[slot]  frame_mass[cap_frames], entry_post[cap_entries]
constexpr int32_t kFramePostHead = 8;
constexpr int32_t kFramePostLdsRecs = 1024;   // WFST_FRAMEPOST_LDS_RECS
struct FramePostDev {
  const int32_t *label_map;   // [n_tid + 1], entry 0 unused; nullptr: the class is the ilabel
  int32_t n_tid;
  double min_post;
  int32_t cap_frames, cap_entries;
  uint32_t *ws_key;
  double *ws_val;
  int32_t *st_class;
  double *st_post;
  int32_t *st_cnt, *st_distinct;
  double *st_mass;
  int32_t *out;
  double *dout;
};
constexpr int64_t frame_post_out_ints(int64_t cap_frames, int64_t cap_entries) { return kFramePostHead + 2 * cap_frames + 1 + cap_entries; }
void launch_frame_post(const AlignDev &A, const PostDev &P, const FramePostDev &Q, int cnt, hipStream_t s);

// ---- sequence-training statistics (wfst_seqstat.hip) -------------------------------------------------------------------------
// The expectation-semiring pass behind sMBR and the MMI occupation difference, per frame of a listed channel's raw lattice, over the
// in-arc index (AlignDev::idx) and posterior_kernel's alpha, beta, gamma, log_z, chan_err and by-source table (PostDev), which is
// still resident behind that launch.  acc_kernel runs one workgroup per slot (sMBR only), seqstat_frame_kernel one per
// (slot, frame), seqstat_pack_kernel one per slot, seqstat_dense_kernel one per (slot, frame row).
//   ref[slot][fr_cap]                 the reference class of a frame, -1: unlabelled (the host pads)
//   fa / fb[slot][ns_cap]             the expected accuracy of the partial paths into / out of a state
//   w[slot][na_cap]                   the signed weight of an arc, by in-arc record; tot[slot] = fb[0]
//   ws_key / ws_val / ws_w[slot][na_cap]   the sort's triples of a frame with more than kSeqStatLdsRecs emitting arcs
//   st_class / st_post / st_value[slot][na_cap + fr_cap]  a frame's list, by class ascending, at the frame's record offset + the
//                                     frame's number (every frame before it may hold MMI's one extra entry)
//   st_cnt / st_flag[slot][fr_cap]    the list's length; bit 0 "labelled", bit 1 "dropped"
//   out[slot]   kSeqStatHead ints {n_frames, n_entries, 1: the rows do not hold them, n_ref_frames, error (kAln*), n_dropped, 0, 0},
//               frame_off[cap_frames + 1], entry_class[cap_entries]
//   dout[slot]  tot_acc, entry_post[cap_entries], entry_value[cap_entries]
//   grad / grad_pitch / grad_rows[slot]  the dense rows of a slot (nullptr: none), their pitch in floats and their number
constexpr int32_t kSeqStatHead = 8;
constexpr int32_t kSeqStatLdsRecs = 1024;   // WFST_SEQSTAT_LDS_RECS
constexpr int32_t kSeqStatMaxSil = 64;      // WFST_SEQSTAT_MAX_SIL
constexpr int32_t kSeqMmi = 0, kSeqSmbr = 1;   // WFST_SEQ_MMI, WFST_SEQ_SMBR
struct SeqStatSil { int32_t v[kSeqStatMaxSil]; };   // passed by value: the list reaches the kernel with its arguments
struct SeqStatDev {
  const int32_t *label_map;   // [n_tid + 1], entry 0 unused; nullptr: the class is the ilabel
  int32_t n_tid;
  int32_t criterion, drop_frames, n_sil;
  const int32_t *ref;
  int32_t cap_frames, cap_entries;   // both 0: no lists are handed out
  double *fa, *fb, *w, *tot;
  uint32_t *ws_key;
  double *ws_val, *ws_w;
  int32_t *st_class;
  double *st_post, *st_value;
  int32_t *st_cnt, *st_flag;
  int32_t *out;
  double *dout;
  float *const *grad;
  const int64_t *grad_pitch;
  const int32_t *grad_rows;
  int32_t n_cols;
  double grad_scale;
};
constexpr int64_t seq_stat_out_ints(int64_t cap_frames, int64_t cap_entries) { return kSeqStatHead + cap_frames + 1 + cap_entries; }
constexpr int64_t seq_stat_out_doubles(int64_t cap_entries) { return 1 + 2 * cap_entries; }
void launch_seq_stat(const AlignDev &A, const PostDev &P, const SeqStatDev &Q, const SeqStatSil &sil, int cnt, bool dense, hipStream_t s);

// ---- best paths under new scales (wfst_rescale.hip) -------------------------------------------------------------------------
// The cheapest path of a listed channel's raw lattice at arc costs (gs * graph + as * acoustic) + (olabel != 0 ? wip : 0), float64,
// for n_set settings (gs, as, wip) shared by the listed channels, over the in-arc index align_index_kernel built (AlignDev::idx; the
// other fields of the AlignDev are not read).  rescale_kernel runs one workgroup per (slot, setting) pair.
//   cells[]              the pairs' cells v[state] (float64, +inf: not reached), pair p at cell_off[p] (< 0: the pair is not run)
//   path[p][path_cap]    the in-arc records of the traced path, last arc first; path_cap >= ns_cap
//   out[p]               kRescaleHead ints {found, arcs on the path, tot bits, lm bits, error (kAln*), n_hyp, n_tids, 0, the low and
//                        the high word of scaled_cost's bits, 0, 0}, hyp_words[cap_words], begin[cap_words], end[cap_words],
//                        tids[cap_tids]
constexpr int32_t kRescaleHead = 12;
constexpr int32_t kRescaleMaxSettings = 64;
struct RescaleSet {   // passed by value: the settings reach the kernel with its arguments
  double v[3 * kRescaleMaxSettings];   // {graph_scale, acoustic_scale, word_penalty} per setting
};
struct RescaleDev {
  const int4 *lat_toks;       // DecoderDev::lat_toks, lat_tok_cap entries per channel
  int64_t lat_tok_cap;
  const int64_t *cell_off;    // [cnt][n_set], in cells
  double *cells;
  int32_t *path;
  int32_t path_cap;
  int32_t n_set, cap_words, cap_tids;
  const uint32_t *sil_bits;   // the silence bitmap over transition-ids 1..n_tid, or nullptr
  int32_t n_tid;
  int32_t *out;
};
constexpr int64_t rescale_out_ints(int64_t cap_words, int64_t cap_tids) { return kRescaleHead + 3 * cap_words + cap_tids; }
void launch_rescale(const AlignDev &A, const RescaleDev &Q, const RescaleSet &S, const int32_t *chan_list_dev, int cnt, hipStream_t s);

// ---- phrase boosting: biased best paths (wfst_bias.hip) ------------------------------------------------------------------------
// rescale_kernel's sweep over cells (lattice state, node of the slot's phrase automaton): an arc costs c_q(a) - r, r = bs * beta(node
// reached) on a word arc (olabel != 0) and 0.0 otherwise, float64, for n_set settings (gs, as, wip, bs) shared by the listed channels,
// over the in-arc index align_index_kernel built.  bias_kernel runs one workgroup per (slot, setting) pair.  A list of a
// wfst_bias_lists set, all offsets into the set's concatenated arrays:
//   hdr[l][kBiasHdr]     {nodes J, distinct words W, offset of its ints, of its beta (= of its nodes), of its table, phrases, 0, 0}
//   ints[]               per list: word[J] (a node's last word, 0: the root), fail[J], phrase[J] (index in the list, -1: none),
//                        pred_off[J + 1], words[W] (the distinct word ids, ascending), pred[]: for node j the nodes i with
//                        delta(i, word[j]) = j, ascending, at pred_off[j] .. pred_off[j + 1]
//   beta[]               per node, float64
//   table[]              per list [J][W] bytes: delta(i, words[k]); a word that is not in words[] leads to the root from every node
//   list_of[slot]        the list of a round's slot, -1: none (J = 1)
//   cells[]              the pairs' tables v[state][J] (float64, +inf: not reached), pair p at cell_off[p] (< 0: the pair is not run)
//   path[p][path_cap]    the in-arc records of the traced path, last arc first; path_cap >= ns_cap
//   out[p]               kBiasHead ints {found, arcs on the path, tot bits, lm bits, error (kAln*), n_hyp, n_hits, 0, the low and the
//                        high word of biased_cost's bits, of bonus' bits, 0, 0, 0, 0}, hyp_words[cap_words], begin[cap_words],
//                        end[cap_words], hit_phrase[cap_hits], hit_word[cap_hits]
constexpr int32_t kBiasHead = 16;
constexpr int32_t kBiasHdr = 8;
constexpr int32_t kBiasMaxNodes = 256;      // = WFST_BIAS_MAX_NODES
constexpr int32_t kBiasMaxSettings = 16;
struct BiasSet {   // passed by value: the settings reach the kernel with its arguments
  double v[4 * kBiasMaxSettings];   // {graph_scale, acoustic_scale, word_penalty, boost_scale} per setting
};
struct BiasListsDev {
  const int32_t *hdr, *ints;
  const double *beta;
  const uint8_t *table;
};
struct BiasDev {
  BiasListsDev L;
  const int32_t *list_of;     // [cnt]
  const int4 *lat_toks;       // DecoderDev::lat_toks, lat_tok_cap entries per channel
  int64_t lat_tok_cap;
  const int64_t *cell_off;    // [cnt][n_set], in cells
  double *cells;
  int32_t *path;
  int32_t path_cap;
  int32_t n_set, cap_words, cap_hits;
  const uint32_t *sil_bits;   // the silence bitmap over transition-ids 1..n_tid, or nullptr
  int32_t n_tid;
  int32_t *out;
};
constexpr int64_t bias_out_ints(int64_t cap_words, int64_t cap_hits) { return kBiasHead + 3 * cap_words + 2 * cap_hits; }
void launch_bias(const AlignDev &A, const BiasDev &Q, const BiasSet &S, const int32_t *chan_list_dev, int cnt, hipStream_t s);

// ---- phrase boosting for large lists: sparse cells over reachable nodes (wfst_bias_sparse.hip) ------------------------------------------
// bias_kernel's sweep restricted to the cells (lattice state t, node j) with j in R(t), the nodes a path into t can be in.
// bias_reach_kernel, one workgroup per slot, builds R and the product graph's edges once per call; bias_sparse_kernel, one workgroup
// per (slot, setting), sweeps the cells and never evaluates the automaton's delta except to check its own traced path.  A book of a
// wfst_bias_books set, all offsets into the set's concatenated arrays (no byte table, no predecessor lists):
//   hdr[l][kBookHdr]     {nodes J, distinct words W, offset of its ints, of its beta, phrases, 0, 0, 0}
//   ints[]               per book: word[J], fail[J], phrase[J], first_child[J], n_child[J], words[W].  Breadth-first numbering makes a
//                        node's children consecutive numbers in ascending word order: goto(i, w) is a binary search of
//                        word[first_child[i] .. first_child[i] + n_child[i])
// A slot's region of BiasReachDev::ints, at reg[4 slot] ints, cell_cap = reg[4 slot + 1], edge_cap = reg[4 slot + 2] (0: skip the slot):
//   roff[ns_cap + 1]     the cells of state t are roff[t] .. roff[t + 1], in (state, node) order
//   ncnt[ns_cap]         a round's new set sizes
//   eoff[na_cap + 1]     the edges of in-arc record a are eoff[a] .. eoff[a + 1]: one per cell of the arc's source state (none for
//                        an arc that is no arc)
//   rnode[cell_cap], rstate[cell_cap]   a cell's node and state
//   edge[edge_cap]       the local index in R(destination) of the cell the transition reaches
//   stage[edge_cap + ns_cap]   a frame's sorted sets before they are packed
//   head[slot][kReachHead]     {status (0, kAln* or kReach*), cells, edges, the largest |R(t)|, 0, 0, 0, 0}
constexpr int32_t kBookHdr = 8;
constexpr int32_t kReachHead = 8;
constexpr int32_t kBiasBookMaxNodes = 65536;   // = WFST_BIAS_BOOK_MAX_NODES
constexpr int32_t kReachOverCells = 6, kReachOverEdges = 7, kReachSkipped = 8;   // beside kAln*: a region is too small; not run
struct BiasBooksDev {
  const int32_t *hdr, *ints;
  const double *beta;
};
struct BiasReachDev {
  BiasBooksDev B;
  const int32_t *book_of;     // [cnt], -1: no book (J = 1)
  int32_t *ints;
  const int64_t *reg;         // [cnt][4]
  int32_t *head;              // [cnt][kReachHead]
};
inline int64_t bias_reach_ints(int64_t ns_cap, int64_t na_cap, int64_t cell_cap, int64_t edge_cap) {
  return (ns_cap + 1) + ns_cap + (na_cap + 1) + 2 * cell_cap + 2 * edge_cap + ns_cap;
}
struct BiasSparseDev {
  BiasReachDev R;
  const int32_t *slot_of;     // [cnt of the round]: the slot of the index and of the regions
  const int4 *lat_toks;
  int64_t lat_tok_cap;
  const int64_t *cell_off;    // [cnt of the round][n_set], in cells
  double *cells;
  int32_t *path;              // [pair][2 path_cap]: the in-arc records of the traced path, last arc first, then the nodes they reach
  int32_t path_cap;
  int32_t n_set, cap_words, cap_hits;
  const uint32_t *sil_bits;
  int32_t n_tid;
  int32_t *out;               // [pair][bias_out_ints]: bias_kernel's layout
};
void launch_bias_reach(const AlignDev &A, const BiasReachDev &Q, int cnt, hipStream_t s);
void launch_bias_sparse(const AlignDev &A, const BiasSparseDev &Q, const BiasSet &S, const int32_t *chan_list_dev, int cnt, hipStream_t s);

// ---- forced alignment against per-utterance graphs (wfst_forced.hip) -----------------------------------------------------------
// Exact float32 Viterbi of a listed channel's scores against one small graph of a wfst_align_graphs set (include/wfst_decoder.h,
// wfst_decoder_force_align).  forced_align_kernel runs one workgroup per list entry.  A graph of the set, all offsets into the set's
// concatenated arrays:
//   hdr[g][kFalignHdr]   {start, final state, states S, arcs, epsilon depth, distinct ilabels, offset of in_off, of rec, of lvl_state,
//                         of lvl_off, of labels, of arcs, largest ilabel, 0, 0, 0}
//   in_off[S + 1]        per destination state {its first in-arc record, its first EPSILON record}; the emitting records come first,
//                        each kind by arc index ascending: the first exact minimum in record order is the tie rule's winner
//   rec[]                {source state, slot of the ilabel in labels[] (-1: an epsilon arc), bits of the weight, arc index}
//   lvl_state[], lvl_off[depth + 1]   the states with epsilon in-arcs by level of the epsilon DAG, level L at lvl_off[L - 1] .. lvl_off[L]
//   labels[]             the graph's distinct non-zero ilabels, ascending
//   arcs[]               the caller's arcs {ilabel, olabel, bits of the weight, nextstate}
constexpr int32_t kFalignLdsStates = 4096;   // = WFST_FALIGN_LDS_STATES: the two cost rows of a graph up to this size live in LDS
constexpr int32_t kFalignLdsLabels = 1024;   // distinct ilabels whose scores are staged in LDS one frame ahead (beyond: gathered)
constexpr int32_t kFalignHdr = 16;
struct ForcedGraphsDev {
  const int32_t *hdr;
  const int2 *in_off;
  const int4 *rec;
  const int32_t *lvl_state, *lvl_off, *labels;
  const int4 *arcs;
};
struct ForcedChan {        // one list entry
  const float *ll;         // row 0 of the channel's scores (not read where T == 0)
  int64_t bp_off;          // of its (T + 1) x S backpointers, in cells
  int64_t row_off;         // of its two cost rows in the workspace, in floats (a graph beyond kFalignLdsStates)
  int64_t path_off;        // of its traced path, in ints
  int32_t graph, T, stride, path_cap;
};
//   bp[]                 per (frame, state) the winning in-arc record + 1, 0: the seed or not reached
//   out[i]               falign_out_ints(): kFalignHead ints {found, T, bits of path_cost, of tot_score, of lm_score, n_hops, n_words,
//                        error (1: the walk left the table)}, hop_arc[cap_hops], alignment[cap_frames], words[cap_words],
//                        word_frame[cap_words]; zero-filled by the host before the launch
constexpr int32_t kFalignHead = 8;
struct ForcedDev {
  ForcedGraphsDev G;
  const ForcedChan *chan;
  const int32_t *col_map;     // the decoder graph's tid2pdf (nullptr: the column is the transition-id)
  const int32_t *label_map;   // the caller's class per transition-id (nullptr: none)
  int32_t *bp, *path;
  float *rows;
  int32_t cap_frames, cap_hops, cap_words;
  int32_t *out;
};
constexpr int64_t falign_out_ints(int64_t cap_frames, int64_t cap_hops, int64_t cap_words) {
  return kFalignHead + cap_hops + cap_frames + 2 * cap_words;
}
void launch_forced_align(const ForcedDev &Q, int cnt, hipStream_t s);

// ---- graph posteriors: forward-backward over per-utterance graphs (wfst_graphpost.hip) -------------------------------------------
// The log-semiring pass of a listed channel's scores against one graph of a wfst_align_graphs set (include/wfst_decoder.h,
// wfst_decoder_graph_posteriors), float64.  graphpost_kernel runs one workgroup per list entry, graphpost_pack_kernel one per entry,
// graphpost_dense_kernel one per (entry, frame row).  Beside ForcedGraphsDev the backward pass reads a graph by SOURCE state, built on
// the set's first call (all offsets into the concatenated arrays):
//   bhdr[g][kGpostHdr]   {offset of out_off, of orec, of blvl_state, of blvl_off, the depth counted from the other end, 0, 0, 0}
//   out_off[S + 1]       per source state {its first arc, its first EMITTING arc}: the caller's own order, epsilon arcs first
//   orec[]               per arc, by arc index {destination state, slot of the ilabel in labels[] (-1: epsilon), bits of the weight, 0}
//   blvl_state[], blvl_off[bdepth + 2]   every state by the longest epsilon path OUT of it, level L at blvl_off[L] .. blvl_off[L + 1]
// and, per call and distinct graph of the list, the classes of its emitting arcs as a CSR (cls[] at GpostChan::cls_off):
//   {slot_class[n_slots] ascending, slot_off[n_slots + 1], slot_arc[]: the emitting arcs of a slot, arc index ascending}
constexpr int32_t kGpostLdsStates = 2048;   // = WFST_GPOST_LDS_STATES: the two float64 rows of a graph up to this size live in LDS
constexpr int32_t kGpostHdr = 8;
constexpr int32_t kGpostHead = 8;
struct GpostGraphsDev {
  const int32_t *bhdr;
  const int2 *out_off;
  const int4 *orec;
  const int32_t *blvl_state, *blvl_off;
};
struct GpostChan {         // one list entry
  const float *ll;         // row 0 of the channel's scores (not read where T == 0)
  int64_t tab_off;         // of its (T + 1) x S alpha table, in cells
  int64_t row_off;         // of its two rolling rows in the workspace, in cells (a graph beyond kGpostLdsStates)
  int64_t gam_off;         // of gamma[A] of the frame in hand and occ[A], in cells
  int64_t post_off;        // of its [T][n_slots] class sums, in cells
  int64_t cnt_off;         // of its per-frame list lengths, in ints
  int64_t cls_off;         // of its graph's class CSR, in ints
  float *grad;             // its dense rows (nullptr: none)
  int64_t grad_pitch;      // in floats
  int32_t grad_rows;
  int32_t graph, T, stride, n_slots, want_occ;
};
//   out[i]    gpost_out_ints(): kGpostHead ints {found, T, n_entries, 1: the rows do not hold them, 0, 0, 0, 0},
//             frame_off[cap_frames + 1], n_distinct[cap_frames], entry_class[cap_entries]; zero-filled by the host before the launch
//   dout[i]   gpost_out_doubles(): log_like, frame_mass[cap_frames], entry_post[cap_entries], arc_occ[cap_arcs]
struct GpostDev {
  ForcedGraphsDev G;
  GpostGraphsDev B;
  const GpostChan *chan;
  const int32_t *col_map;     // the decoder graph's tid2pdf (nullptr: the column is the transition-id)
  const int32_t *cls;
  double graph_scale, acoustic_scale, min_post, grad_scale;
  double *tab, *rows, *gam, *post;
  int32_t *cnt;
  int32_t cap_frames, cap_entries, cap_arcs, n_cols;
  int32_t *out;
  double *dout;
};
constexpr int64_t gpost_out_ints(int64_t cap_frames, int64_t cap_entries) { return kGpostHead + 2 * cap_frames + 1 + cap_entries; }
constexpr int64_t gpost_out_doubles(int64_t cap_frames, int64_t cap_entries, int64_t cap_arcs) { return 1 + cap_frames + cap_entries + cap_arcs; }
void launch_graph_post(const GpostDev &Q, int cnt, int max_T, bool dense, hipStream_t s);

// ---- second-pass LM composition on determinized lattices (wfst_compose.hip) ------------------------------------
// ComposeLattice (newfst/compose-lat-inl.h:15-130) of the determinized lattice of workspace slot 0 (DetDev::out_a / out_w, as
// determinize_kernel left it) with ComposeArpaLm(lm1), then of the result with ComposeArpaLm(lm2) -- what the service's GetLattice
// does under --use-second (kaldi-nnet3/kaldi-online-nnet3-my-decoder.cc:53-78) -- each followed by Connect.
struct CmpDev {
  int32_t *ws;            // workspace (ints): see wfst_compose.hip
  int64_t ws_ints;
  int32_t pair_cap;       // composed states per pass (hash slots = 2 x)
  int32_t arc_cap;        // arcs per pass
  int32_t *result;        // {states, arcs, status (0 ok, 1 capacity), -}
  int4 *out_a;            // [arc_cap] {src, dst, olabel, final flag of dst}
  float2 *out_w;          // [arc_cap] {graph, acoustic}
  int32_t *out_fin;       // [pair_cap] final flag per state
};
void launch_compose2(const DetDev &X, const CmpDev &Y, const LmDev &lm1, const LmDev &lm2, int n_slots, hipStream_t s);

// launch wrappers (wfst_kernels.hip)
void launch_init(const DecoderDev &D, const int32_t *chan_list_dev, int n, hipStream_t s);
void launch_expand(const DecoderDev &D, int group, int par, int n_workgroups, hipStream_t s);
// boundary: 0 = the closure kernel follows (classic frame); 1 = the insert launch closes the frame and prepares the next
// (two-launch frame); 2 = closes the frame only (last frame of an advance call)
void launch_insert(const DecoderDev &D, int chan_off, int chan_cnt, const int32_t *target_dev, int boundary, int group, int par,
                   int n_workgroups, hipStream_t s);
// after_insert: the launch closes a frame an insert launch has just built (DecoderDev::closure_slabs workgroups per channel then)
void launch_closure(const DecoderDev &D, int chan_off, int chan_cnt, const int32_t *target_dev, int do_prep,
                    int group, int par, hipStream_t s, int after_insert);
// stage: -1 = the step's four launches; 0..3 = one of them (raw frames, walk, flag sweeps, moves): a profiled step times them one by one
void launch_lattice_prune_step(const DecoderDev &D, int chan_off, int chan_cnt, const int32_t *target_dev, int group, int par, hipStream_t s, int stage);
int prune_raw_resident_workgroups(int device);   // lattice_prune_raw_kernel: workgroups the device holds at once (occupancy x compute units)
int prune_raw_grid(int chan_cnt);                // ... and the grid of one launch over chan_cnt channels
void launch_set_finalized(const DecoderDev &D, const int32_t *chan_list_dev, int n, hipStream_t s);
void launch_delay(int microseconds, hipStream_t s);
void launch_lattice_prune(const DecoderDev &D, const int32_t *chan_list_dev, int n, hipStream_t s);
void launch_lattice_emit(const DecoderDev &D, const int32_t *chan_list_dev, int n, int use_final, hipStream_t s);
void launch_best_path(const DecoderDev &D, const int32_t *chan_list_dev, int n, int use_final,
                      int cap, int32_t *ilabel, int32_t *olabel, float *graph, float *ac,
                      int32_t *n_hops, int32_t *chain_scratch, hipStream_t s);
// words, word times and scores of the listed channels' best paths (words_kernel): out[i] = {n_hops, n_words, tot, lm, 1: the path
// outgrew the scratch, the channel's error word, 0, 0} + cap_words words, begin frames and end frames; chain: cap_chain ints per list entry for the hops
// of the walk beyond words_chain_lds(); sil_bits: the silence bitmap over transition-ids 1..n_tid, or nullptr
constexpr int32_t kWordsHead = 8;
int words_chain_lds();
void launch_words(const DecoderDev &D, const int32_t *chan_list_dev, int n, int use_final, const uint32_t *sil_bits, int n_tid,
                  int cap_words, int cap_chain, int32_t *chain, int32_t *out, hipStream_t s);
// endpoint inputs of the listed channels (endpoint_kernel): out[3 i ..] = {trailing silence frames, final relative cost, error}
void launch_endpoint(const DecoderDev &D, const int32_t *chan_list_dev, int n, const uint32_t *sil_bits, int n_tid, int32_t *out,
                     hipStream_t s);
// partial words with a stable prefix of the listed channels (partial_kernel): list entries may carry kPartialResetBit (the channel's
// commit state starts from zero); ws: partial_ws_ints(max_frames) ints per channel; out[i]: {n_words, n_stable, stable_frame, error}
// and cap_words words
constexpr int32_t kPartialResetBit = 1 << 30;
inline int64_t partial_ws_ints(int32_t max_frames) { return 8 + 2 * (int64_t)max_frames; }
void launch_partial(const DecoderDev &D, const int32_t *chan_list_dev, int n, int32_t *ws, int64_t ws_stride, int cap_words, int32_t *out,
                    hipStream_t s);

}  // namespace wfst
#endif
