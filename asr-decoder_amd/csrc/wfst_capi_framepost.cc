// wfst_decoder_frame_posteriors: per frame of a channel's raw lattice the posterior mass of every class -- the transition-id of an
// emitting arc, or what the caller's map makes of it -- for a channel list (live and finalized channels mixed), one launch per stage
// (lattice_emit_kernel for the live channels, align_index_kernel, posterior_kernel, frame_post_kernel, frame_pack_kernel:
// wfst_align.hip, wfst_posterior.hip, wfst_framepost.hip).  A translation unit of its own -- see wfst_capi_framepost.h.
#include "wfst_capi_framepost.h"

#include <cmath>

using namespace wfst;

namespace {
struct FramePostQuery : WordQuery {
  size_t n, capf, cape;
  double graph_scale, acoustic_scale, min_post;
  const int32_t *label_map;
  int32_t n_tid;
  double *log_z, *frame_mass, *entry_post;
  int32_t *n_frames, *n_entries, *frame_off, *n_distinct, *entry_class;
  FramePostQuery(size_t n_, int32_t cap_frames, int32_t cap_entries)
      : n(n_), capf((size_t)std::max(cap_frames, 0)), cape((size_t)std::max(cap_entries, 0)) {
    name = "frame posteriors"; item = "sequence"; abbr = "seq";
    default_cells = kFramePostDefaultCells; round_cells = kFramePostRoundCells;
    pair_ints = (size_t)frame_post_out_ints((int64_t)capf, (int64_t)cape);
    chan_ints = 1;   // posterior_kernel's error word
    invariant = "an unknown error word";
  }
  std::string workspace_note(const WordRound &R) const override {
    const size_t na = (size_t)R.A.na_cap, fr = (size_t)R.A.fr_cap;
    return ", " + std::to_string(R.cnt * post_slot_bytes(R.A.ns_cap, R.A.na_cap)) + " bytes of posteriors, " +
           std::to_string(R.cnt * (8 * frame_post_slot_doubles(na, fr) + 4 * frame_post_slot_ints(na, fr))) + " bytes of staged lists";
  }
  void clear() override {
    align_zero(log_z, n); align_zero(n_frames, n); align_zero(n_entries, n);
    align_zero(frame_off, n * (capf + 1)); align_zero(n_distinct, n * capf); align_zero(frame_mass, n * capf);
    align_zero(entry_class, n * cape); align_zero(entry_post, n * cape);
  }
  int launch(WordRound &R) override {
    const AlignView &V = *R.V;
    AlignState &S = *V.as;
    const AlignDev A = R.align_dev();
    const size_t cnt = R.cnt, na = (size_t)A.na_cap, fr = (size_t)A.fr_cap, more = cnt * (capf + cape);
    // what comes back beside the packed ints: log_z [cnt], then per slot frame_mass [cap_frames] and entry_post [cap_entries]
    PostDev P;
    const int rc = post_workspace(*this, R, more, graph_scale, acoustic_scale, &P);
    if (rc != WFST_OK) return rc;
    const size_t dbl_n = cnt * frame_post_slot_doubles(na, fr), int_n = cnt * frame_post_slot_ints(na, fr);
    const size_t map_n = label_map ? (size_t)n_tid + 1 : 0;
    if (S.fpost.n < dbl_n || S.fpost_idx.n < int_n || S.fpost_map.n < map_n) {
      ALIGN_TRY(hipStreamSynchronize(V.stream));
      if (align_grow(S.fpost, dbl_n) != hipSuccess || align_grow(S.fpost_idx, int_n) != hipSuccess || align_grow(S.fpost_map, map_n) != hipSuccess) {
        (void)hipGetLastError();
        return word_query_no_memory(*this, R);
      }
    }
    if (label_map) ALIGN_TRY(hipMemcpyAsync(S.fpost_map.p, label_map, map_n * 4, hipMemcpyHostToDevice, V.stream));
    FramePostDev Q = {};
    Q.label_map = label_map ? S.fpost_map.p : nullptr;
    Q.n_tid = n_tid;
    Q.min_post = min_post;
    Q.cap_frames = (int32_t)capf;
    Q.cap_entries = (int32_t)cape;
    Q.st_post = S.fpost.p;
    Q.ws_val = Q.st_post + cnt * na;
    Q.st_mass = Q.ws_val + cnt * na;
    Q.st_class = S.fpost_idx.p;
    Q.ws_key = reinterpret_cast<uint32_t *>(Q.st_class + cnt * na);
    Q.st_cnt = Q.st_class + 2 * cnt * na;
    Q.st_distinct = Q.st_cnt + cnt * fr;
    Q.out = A.out;
    Q.dout = P.out;
    launch_align_index(*V.D, A, R.chan, (int)cnt, V.stream);
    ALIGN_TRY(hipGetLastError());
    launch_posterior(*V.D, A, P, R.chan, (int)cnt, V.stream);
    ALIGN_TRY(hipGetLastError());
    launch_frame_post(A, P, Q, (int)cnt, V.stream);
    ALIGN_TRY(hipGetLastError());
    R.more_dst = S.post_pin.p; R.more_src = P.log_z; R.more_bytes = (cnt + more) * 8;
    return WFST_OK;
  }
  int unpack(const WordRound &R, size_t j, size_t o, int32_t channel) override {
    const int32_t *r = R.landed + j * pair_ints;
    const double *landed = R.V->as->post_pin.p, *dm = landed + R.cnt + j * (capf + cape);
    const int32_t nf = r[0], ne = r[1];
    if (log_z) log_z[o] = landed[j];
    if (n_frames) n_frames[o] = nf;
    if (n_entries) n_entries[o] = ne;
    // the rows do not hold the lattice's frames or entries: n_frames and n_entries are the room they take, the lists stay zero
    if (r[2])
      return capi_fail(WFST_E_CAPACITY, "channel " + std::to_string(channel) + ": frame posteriors: " + std::to_string(nf) + " frames and " +
                                            std::to_string(ne) + " entries, cap_frames is " + std::to_string(capf) + " and cap_entries " +
                                            std::to_string(cape));
    if (nf <= 0) return WFST_OK;   // no lattice: the lists stay zero
    const size_t f = (size_t)nf, e = (size_t)ne;
    const int32_t *r_off = r + kFramePostHead, *r_distinct = r_off + capf + 1, *r_class = r_distinct + capf;
    if (frame_off) memcpy(frame_off + o * (capf + 1), r_off, (f + 1) * 4);
    if (n_distinct) memcpy(n_distinct + o * capf, r_distinct, f * 4);
    if (frame_mass) memcpy(frame_mass + o * capf, dm, f * 8);
    if (entry_class) memcpy(entry_class + o * cape, r_class, e * 4);
    if (entry_post) memcpy(entry_post + o * cape, dm + capf, e * 8);
    return WFST_OK;
  }
};
}  // namespace

int wfst_decoder_frame_posteriors(wfst_decoder *d, const int32_t *channels, int32_t n, int32_t use_final_probs, double graph_scale,
                                  double acoustic_scale, const int32_t *label_map, int32_t n_tid, double min_post, int64_t max_cells,
                                  int32_t cap_frames, int32_t cap_entries, int32_t *status, double *log_z, int32_t *n_frames,
                                  int32_t *n_entries, int32_t *frame_off, int32_t *n_distinct, double *frame_mass, int32_t *entry_class,
                                  double *entry_post) {
  if (!d || !channels) return capi_fail(WFST_E_ARG, "NULL decoder / channel list");
  if (!std::isfinite(graph_scale) || !std::isfinite(acoustic_scale) || graph_scale < 0.0 || acoustic_scale < 0.0)
    return capi_fail(WFST_E_ARG, "graph_scale / acoustic_scale must be finite and >= 0");
  if (!(min_post >= 0.0 && min_post <= 1.0)) return capi_fail(WFST_E_ARG, "min_post must lie in 0..1");
  if (cap_frames < 1 || cap_entries < 1) return capi_fail(WFST_E_ARG, "cap_frames / cap_entries < 1");
  if (max_cells < 0) return capi_fail(WFST_E_ARG, "max_cells < 0");
  if (label_map) {
    if (n_tid < 1) return capi_fail(WFST_E_ARG, "label_map with n_tid < 1");
    for (int32_t t = 1; t <= n_tid; ++t)
      if (label_map[t] < 0) return capi_fail(WFST_E_ARG, "a negative class in label_map");
  }
  // (the channel list's own checks, so that the graph is only looked at through a decoder that stands; the driver repeats them)
  AlignView V;
  const int rc = align_begin(d, channels, n, &V);
  if (rc != WFST_OK) return rc;
  if (label_map && align_max_ilabel(d) > n_tid) return capi_fail(WFST_E_ARG, "arc ilabel outside label_map range");
  FramePostQuery q((size_t)n, cap_frames, cap_entries);
  q.graph_scale = graph_scale; q.acoustic_scale = acoustic_scale; q.min_post = min_post;
  q.label_map = label_map; q.n_tid = n_tid;
  q.log_z = log_z; q.frame_mass = frame_mass; q.entry_post = entry_post;
  q.n_frames = n_frames; q.n_entries = n_entries; q.frame_off = frame_off; q.n_distinct = n_distinct; q.entry_class = entry_class;
  // one empty sequence per channel: a table of states x 1 cells
  const std::vector<int32_t> none((size_t)n, 0);
  return word_query_run(q, d, channels, n, use_final_probs, 1, 1, none.data(), none.data(), max_cells, status);
}
