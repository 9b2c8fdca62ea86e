// wfst_decoder_sequence_stats: the sMBR / MMI statistics of a channel's raw lattice against a reference alignment -- per frame the
// (class, post, value) list, tot_acc, and optionally the values scattered into the caller's dense float32 rows on the device -- for
// a channel list (live and finalized channels mixed), one launch per stage (lattice_emit_kernel for the live channels,
// align_index_kernel, posterior_kernel, acc_kernel, seqstat_frame_kernel, seqstat_pack_kernel, seqstat_dense_kernel: wfst_align.hip,
// wfst_posterior.hip, wfst_seqstat.hip).  A translation unit of its own -- see wfst_capi_seqstat.h.
#include "wfst_capi_seqstat.h"

#include <cmath>
#include <unordered_map>

using namespace wfst;

namespace {
struct SeqStatQuery : WordQuery {
  size_t n, capf, cape;
  bool lists;
  int32_t criterion, drop_frames;
  double graph_scale, acoustic_scale;
  const int32_t *label_map;
  int32_t n_tid;
  const int32_t *ref, *n_ref;
  size_t cap_ref;
  SeqStatSil sil;
  int32_t n_sil;
  void *const *grad;
  const int64_t *grad_pitch;
  const int32_t *grad_frames;
  int32_t n_cols;
  double grad_scale;
  void *consumer;
  std::unordered_map<int32_t, size_t> where;   // a channel's position in the caller's list
  std::vector<int32_t> h_ref;                  // a round's staged inputs (kept until the round's download has landed)
  std::vector<int64_t> h_grad;
  Event free_ev, rows_ev;                      // the caller's stream before the writes, the writes before the caller's stream
  double *log_z, *tot_acc, *entry_post, *entry_value;
  int32_t *n_frames, *n_ref_frames, *n_dropped, *n_entries, *frame_off, *entry_class;
  SeqStatQuery(size_t n_, int32_t cap_frames, int32_t cap_entries)
      : n(n_), capf((size_t)std::max(cap_frames, 0)), cape((size_t)std::max(cap_entries, 0)), lists(cap_frames > 0 || cap_entries > 0) {
    name = "sequence stats"; item = "sequence"; abbr = "seq";
    default_cells = kSeqStatDefaultCells; round_cells = kSeqStatRoundCells;
    pair_ints = (size_t)seq_stat_out_ints((int64_t)capf, (int64_t)cape);
    chan_ints = 1;   // posterior_kernel's error word
    invariant = "an unknown error word";
  }
  std::string workspace_note(const WordRound &R) const override {
    const size_t ns = (size_t)R.A.ns_cap, na = (size_t)R.A.na_cap, fr = (size_t)R.A.fr_cap;
    return ", " + std::to_string(R.cnt * post_slot_bytes(R.A.ns_cap, R.A.na_cap)) + " bytes of posteriors, " +
           std::to_string(R.cnt * (8 * seq_stat_slot_doubles(ns, na, fr) + 4 * seq_stat_slot_ints(na, fr))) + " bytes of accuracies and staged lists";
  }
  void clear() override {
    align_zero(log_z, n); align_zero(tot_acc, n); align_zero(n_frames, n); align_zero(n_ref_frames, n); align_zero(n_dropped, n);
    align_zero(n_entries, n);
    if (!lists) return;
    align_zero(frame_off, n * (capf + 1)); align_zero(entry_class, n * cape); align_zero(entry_post, n * cape); align_zero(entry_value, n * cape);
  }
  int launch(WordRound &R) override {
    const AlignView &V = *R.V;
    AlignState &S = *V.as;
    const AlignDev A = R.align_dev();
    const size_t cnt = R.cnt, ns = (size_t)A.ns_cap, na = (size_t)A.na_cap, fr = (size_t)A.fr_cap, more = cnt * (1 + 2 * cape);
    // what comes back beside the packed ints: log_z [cnt], then per slot tot_acc, entry_post and entry_value [cap_entries]
    PostDev P;
    const int rc = post_workspace(*this, R, more, graph_scale, acoustic_scale, &P);
    if (rc != WFST_OK) return rc;
    const size_t dbl_n = cnt * seq_stat_slot_doubles(ns, na, fr), int_n = cnt * seq_stat_slot_ints(na, fr);
    const size_t map_n = label_map ? (size_t)n_tid + 1 : 0, in_n = 3 * cnt;
    if (S.sstat.n < dbl_n || S.sstat_idx.n < int_n || S.sstat_map.n < map_n || S.sstat_in.n < in_n) {
      ALIGN_TRY(hipStreamSynchronize(V.stream));
      if (align_grow(S.sstat, dbl_n) != hipSuccess || align_grow(S.sstat_idx, int_n) != hipSuccess ||
          align_grow(S.sstat_map, map_n) != hipSuccess || align_grow(S.sstat_in, in_n) != hipSuccess) {
        (void)hipGetLastError();
        return word_query_no_memory(*this, R);
      }
    }
    // the round's channels as word_query_run staged them (the landing place still holds the inputs): slot j is list position o
    const int32_t *h_chan = S.pin.p + 2 * R.pairs;
    h_ref.assign(cnt * fr, -1);
    h_grad.assign(in_n, 0);
    int32_t *h_rows = reinterpret_cast<int32_t *>(h_grad.data() + 2 * cnt);
    bool dense = false;
    for (size_t j = 0; j < cnt; ++j) {
      const size_t o = where.at(h_chan[j]);
      const size_t k = std::min(fr, (size_t)(n_ref ? n_ref[o] : 0));
      for (size_t f = 0; f < k; ++f) h_ref[j * fr + f] = std::max(ref[o * cap_ref + f], -1);
      if (grad && grad[o]) {
        h_grad[j] = (int64_t)reinterpret_cast<intptr_t>(grad[o]);
        h_grad[cnt + j] = grad_pitch ? grad_pitch[o] : (int64_t)n_cols;
        h_rows[j] = grad_frames[o];
        dense = dense || grad_frames[o] > 0;
      }
    }
    SeqStatDev Q = {};
    Q.label_map = label_map ? S.sstat_map.p : nullptr;
    Q.n_tid = n_tid;
    Q.criterion = criterion; Q.drop_frames = drop_frames; Q.n_sil = n_sil;
    Q.cap_frames = (int32_t)capf; Q.cap_entries = (int32_t)cape;
    Q.fa = S.sstat.p;
    Q.fb = Q.fa + cnt * ns;
    Q.w = Q.fb + cnt * ns;
    Q.ws_val = Q.w + cnt * na;
    Q.ws_w = Q.ws_val + cnt * na;
    Q.st_post = Q.ws_w + cnt * na;
    Q.st_value = Q.st_post + cnt * (na + fr);
    Q.tot = Q.st_value + cnt * (na + fr);
    Q.ws_key = reinterpret_cast<uint32_t *>(S.sstat_idx.p);
    Q.st_class = S.sstat_idx.p + cnt * na;
    Q.st_cnt = Q.st_class + cnt * (na + fr);
    Q.st_flag = Q.st_cnt + cnt * fr;
    int32_t *d_ref = Q.st_flag + cnt * fr;
    Q.ref = d_ref;
    Q.out = A.out;
    Q.dout = P.out;
    Q.grad = reinterpret_cast<float *const *>(S.sstat_in.p);
    Q.grad_pitch = S.sstat_in.p + cnt;
    Q.grad_rows = reinterpret_cast<const int32_t *>(S.sstat_in.p + 2 * cnt);
    Q.n_cols = n_cols;
    Q.grad_scale = grad_scale;
    if (label_map) ALIGN_TRY(hipMemcpyAsync(S.sstat_map.p, label_map, map_n * 4, hipMemcpyHostToDevice, V.stream));
    ALIGN_TRY(hipMemcpyAsync(d_ref, h_ref.data(), cnt * fr * 4, hipMemcpyHostToDevice, V.stream));
    ALIGN_TRY(hipMemcpyAsync(S.sstat_in.p, h_grad.data(), in_n * 8, hipMemcpyHostToDevice, V.stream));
    // the dense rows against the caller's stream, both ways, as wfst_decoder_advance_chunk orders a chunk: what that stream was given
    // before the call (a fill, the previous step's read of the rows) is over before the rows are written, and what it is given next
    // comes behind the writes
    const bool linked = dense && consumer != WFST_STREAM_NONE;
    const hipStream_t cons = linked ? static_cast<hipStream_t>(consumer) : nullptr;
    if (linked) {
      if (!free_ev.h) ALIGN_TRY(free_ev.create());
      if (!rows_ev.h) ALIGN_TRY(rows_ev.create());
      ALIGN_TRY(hipEventRecord(free_ev.h, cons));
      ALIGN_TRY(hipStreamWaitEvent(V.stream, free_ev.h, 0));
    }
    launch_align_index(*V.D, A, R.chan, (int)cnt, V.stream);
    ALIGN_TRY(hipGetLastError());
    launch_posterior(*V.D, A, P, R.chan, (int)cnt, V.stream);
    ALIGN_TRY(hipGetLastError());
    launch_seq_stat(A, P, Q, sil, (int)cnt, dense, V.stream);
    ALIGN_TRY(hipGetLastError());
    if (linked) {
      ALIGN_TRY(hipEventRecord(rows_ev.h, V.stream));
      ALIGN_TRY(hipStreamWaitEvent(cons, rows_ev.h, 0));
    }
    R.more_dst = S.post_pin.p; R.more_src = P.log_z; R.more_bytes = (cnt + more) * 8;
    return WFST_OK;
  }
  int unpack(const WordRound &R, size_t j, size_t o, int32_t channel) override {
    const int32_t *r = R.landed + j * pair_ints;
    const double *landed = R.V->as->post_pin.p, *dm = landed + R.cnt + j * (1 + 2 * cape);
    const int32_t nf = r[0], ne = r[1];
    if (log_z) log_z[o] = landed[j];
    if (n_frames) n_frames[o] = nf;
    if (n_entries) n_entries[o] = ne;
    // the rows do not hold the lattice's frames or entries: n_frames and n_entries are the room they take, everything else stays zero
    if (r[2])
      return capi_fail(WFST_E_CAPACITY, "channel " + std::to_string(channel) + ": sequence stats: " + std::to_string(nf) + " frames and " +
                                            std::to_string(ne) + " entries, cap_frames is " + std::to_string(capf) + " and cap_entries " +
                                            std::to_string(cape));
    if (tot_acc) tot_acc[o] = dm[0];
    if (n_ref_frames) n_ref_frames[o] = r[3];
    if (n_dropped) n_dropped[o] = r[5];
    if (nf <= 0 || !lists) return WFST_OK;   // no lattice: the lists stay zero
    const size_t f = (size_t)nf, e = (size_t)ne;
    const int32_t *r_off = r + kSeqStatHead, *r_class = r_off + capf + 1;
    if (frame_off) memcpy(frame_off + o * (capf + 1), r_off, (f + 1) * 4);
    if (entry_class) memcpy(entry_class + o * cape, r_class, e * 4);
    if (entry_post) memcpy(entry_post + o * cape, dm + 1, e * 8);
    if (entry_value) memcpy(entry_value + o * cape, dm + 1 + cape, e * 8);
    return WFST_OK;
  }
};
}  // namespace

int wfst_decoder_sequence_stats(wfst_decoder *d, const int32_t *channels, int32_t n, int32_t criterion, int32_t use_final_probs,
                                double graph_scale, double acoustic_scale, const int32_t *label_map, int32_t n_tid, const int32_t *ref,
                                const int32_t *n_ref, int32_t cap_ref, const int32_t *sil_classes, int32_t n_sil, int32_t drop_frames,
                                int64_t max_cells, int32_t cap_frames, int32_t cap_entries, void *const *grad, const int64_t *grad_pitch,
                                const int32_t *grad_frames, int32_t n_cols, double grad_scale, void *consumer_stream, int32_t *status,
                                double *log_z, double *tot_acc, int32_t *n_frames, int32_t *n_ref_frames, int32_t *n_dropped,
                                int32_t *n_entries, int32_t *frame_off, int32_t *entry_class, double *entry_post, double *entry_value) {
  if (!d || !channels) return capi_fail(WFST_E_ARG, "NULL decoder / channel list");
  if (criterion != WFST_SEQ_MMI && criterion != WFST_SEQ_SMBR) return capi_fail(WFST_E_ARG, "criterion is neither WFST_SEQ_MMI nor WFST_SEQ_SMBR");
  if (!std::isfinite(graph_scale) || !std::isfinite(acoustic_scale) || graph_scale < 0.0 || acoustic_scale < 0.0)
    return capi_fail(WFST_E_ARG, "graph_scale / acoustic_scale must be finite and >= 0");
  const bool lists = cap_frames != 0 || cap_entries != 0;   // (0, 0: no lists, the dense rows and the channels' numbers only)
  if (lists && (cap_frames < 1 || cap_entries < 1)) return capi_fail(WFST_E_ARG, "cap_frames / cap_entries < 1 (both 0: no lists)");
  if (max_cells < 0) return capi_fail(WFST_E_ARG, "max_cells < 0");
  if (label_map) {
    if (n_tid < 1) return capi_fail(WFST_E_ARG, "label_map with n_tid < 1");
    for (int32_t t = 1; t <= n_tid; ++t)
      if (label_map[t] < 0) return capi_fail(WFST_E_ARG, "a negative class in label_map");
  }
  if (n_sil < 0 || n_sil > WFST_SEQSTAT_MAX_SIL || (n_sil > 0 && !sil_classes))
    return capi_fail(WFST_E_ARG, "sil_classes: 0 .. WFST_SEQSTAT_MAX_SIL classes");
  for (int32_t i = 0; i < n_sil; ++i)
    if (sil_classes[i] < 0 || (i && sil_classes[i] <= sil_classes[i - 1])) return capi_fail(WFST_E_ARG, "sil_classes must be >= 0 and strictly ascending");
  if (cap_ref < 0 || (cap_ref > 0 && (!ref || !n_ref))) return capi_fail(WFST_E_ARG, "cap_ref < 0, or NULL ref / n_ref");
  if (n < 0) return capi_fail(WFST_E_ARG, "n < 0");
  for (int32_t i = 0; n_ref && i < n; ++i)
    if (n_ref[i] < 0 || n_ref[i] > cap_ref) return capi_fail(WFST_E_ARG, "n_ref outside 0 .. cap_ref");
  if (!std::isfinite(grad_scale)) return capi_fail(WFST_E_ARG, "grad_scale is not finite");
  if (grad) {
    if (!grad_frames || n_cols < 1) return capi_fail(WFST_E_ARG, "grad without grad_frames, or n_cols < 1");
    for (int32_t i = 0; i < n; ++i) {
      if (!grad[i]) continue;
      if (reinterpret_cast<uintptr_t>(grad[i]) % 4) return capi_fail(WFST_E_ARG, "a grad pointer is not aligned to 4 bytes");
      if (grad_frames[i] < 0) return capi_fail(WFST_E_ARG, "grad_frames < 0");
      if (grad_pitch && grad_pitch[i] < n_cols) return capi_fail(WFST_E_ARG, "a grad_pitch below n_cols");
      for (int32_t f = 0; n_ref && f < n_ref[i]; ++f)
        if (ref[(size_t)i * cap_ref + f] >= n_cols) return capi_fail(WFST_E_ARG, "a ref class >= n_cols");
    }
    if (label_map)
      for (int32_t t = 1; t <= n_tid; ++t)
        if (label_map[t] >= n_cols) return capi_fail(WFST_E_ARG, "a label_map class >= n_cols");
  }
  // (the channel list's own checks, so that the graph is only looked at through a decoder that stands; the driver repeats them)
  AlignView V;
  const int rc = align_begin(d, channels, n, &V);
  if (rc != WFST_OK) return rc;
  if (label_map && align_max_ilabel(d) > n_tid) return capi_fail(WFST_E_ARG, "arc ilabel outside label_map range");
  if (grad && !label_map && align_max_ilabel(d) >= n_cols) return capi_fail(WFST_E_ARG, "n_cols does not exceed the graph's largest transition-id");
  SeqStatQuery q((size_t)n, cap_frames, cap_entries);
  q.criterion = criterion; q.drop_frames = drop_frames != 0;
  q.graph_scale = graph_scale; q.acoustic_scale = acoustic_scale;
  q.label_map = label_map; q.n_tid = n_tid;
  q.ref = ref; q.n_ref = cap_ref > 0 ? n_ref : nullptr; q.cap_ref = (size_t)cap_ref;
  q.sil = SeqStatSil{};
  for (int32_t i = 0; i < n_sil; ++i) q.sil.v[i] = sil_classes[i];
  q.n_sil = n_sil;
  q.grad = grad; q.grad_pitch = grad_pitch; q.grad_frames = grad_frames; q.n_cols = n_cols; q.grad_scale = grad_scale;
  q.consumer = consumer_stream;
  for (int32_t i = 0; i < n; ++i) q.where[channels[i]] = (size_t)i;
  q.log_z = log_z; q.tot_acc = tot_acc; q.entry_post = entry_post; q.entry_value = entry_value;
  q.n_frames = n_frames; q.n_ref_frames = n_ref_frames; q.n_dropped = n_dropped; q.n_entries = n_entries;
  q.frame_off = frame_off; q.entry_class = entry_class;
  // one empty sequence per channel: a table of states x 1 cells
  const std::vector<int32_t> none((size_t)n, 0);
  return word_query_run(q, d, channels, n, use_final_probs, 1, 1, none.data(), none.data(), max_cells, status);
}
