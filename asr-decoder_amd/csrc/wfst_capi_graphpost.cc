// wfst_decoder_graph_posteriors: the forward-backward pass of the listed channels' scores against per-utterance graphs, one launch
// per stage and round (graphpost_kernel, graphpost_pack_kernel, graphpost_dense_kernel: wfst_graphpost.hip).  A translation unit of
// its own -- see wfst_capi_graphpost.h.
#include "wfst_capi_graphpost.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>

#include "wfst_capi_align.h"    // capi_fail, ALIGN_TRY, align_grow, align_zero, cut_round
#include "wfst_capi_forced.h"   // wfst_align_graphs, forced_view, forced_stream, the bounds

namespace wfst {

// What the backward pass reads of a set beside ForcedGraphsDev: the arcs by SOURCE state and every state's level counted from the
// other end (wfst_device.h, GpostGraphsDev).  Built from the set's host copies on the set's first call.
struct GpostTables {
  DevBuf<int32_t> d_bhdr, d_blvl_state, d_blvl_off;
  DevBuf<int2> d_out_off;
  DevBuf<int4> d_orec;
  GpostGraphsDev view() const { return GpostGraphsDev{d_bhdr.p, d_out_off.p, d_orec.p, d_blvl_state.p, d_blvl_off.p}; }
};
void gpost_tables_free(GpostTables *t) { delete t; }

}  // namespace wfst

using namespace wfst;

namespace {

template <class T>
int upload(DevBuf<T> &buf, const std::vector<T> &v) {
  ALIGN_TRY(buf.alloc(v.size()));
  if (!v.empty()) ALIGN_TRY(hipMemcpy(buf.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return WFST_OK;
}

// the set's by-source tables, made by the first caller (the set's device is current)
int gpost_tables(const wfst_align_graphs *gs, const GpostTables **out) {
  std::lock_guard<std::mutex> lock(gs->gpost_mu);
  if (gs->gpost) { *out = gs->gpost; return WFST_OK; }
  std::vector<int32_t> bhdr((size_t)gs->n_graphs * kGpostHdr, 0), blvl_state, blvl_off;
  std::vector<int4> orec(gs->h_arcs.size());
  for (int32_t g = 0; g < gs->n_graphs; ++g) {
    const int32_t *H = gs->hdr.data() + (size_t)g * kFalignHdr;
    const int32_t S = H[2], A = H[3];
    const int2 *oo = gs->h_out_off.data() + H[6];
    const int4 *ar = gs->h_arcs.data() + H[11];
    const int32_t *labs = gs->labels.data() + H[10];
    for (int32_t a = 0; a < A; ++a) {
      const int32_t slot = ar[a].x ? (int32_t)(std::lower_bound(labs, labs + H[5], ar[a].x) - labs) : -1;
      orec[(size_t)H[11] + (size_t)a] = make_int4(ar[a].w, slot, ar[a].z, 0);
    }
    // the longest epsilon path OUT of every state: the epsilon arcs form a DAG (the set was validated), so a state is settled once
    // all its epsilon targets are -- Kahn's order over the reversed arcs
    std::vector<int32_t> left((size_t)S), blevel((size_t)S, 0), order, rev_off((size_t)S + 1, 0), rev;
    for (int32_t s = 0; s < S; ++s) {
      left[(size_t)s] = oo[s].y - oo[s].x;
      for (int32_t a = oo[s].x; a < oo[s].y; ++a) ++rev_off[(size_t)ar[a].w + 1];
    }
    for (int32_t s = 0; s < S; ++s) rev_off[(size_t)s + 1] += rev_off[(size_t)s];
    rev.resize((size_t)rev_off[(size_t)S]);
    {
      std::vector<int32_t> at(rev_off.begin(), rev_off.end() - 1);
      for (int32_t s = 0; s < S; ++s)
        for (int32_t a = oo[s].x; a < oo[s].y; ++a) rev[(size_t)at[(size_t)ar[a].w]++] = s;
    }
    for (int32_t s = 0; s < S; ++s)
      if (!left[(size_t)s]) order.push_back(s);
    for (size_t k = 0; k < order.size(); ++k) {
      const int32_t t = order[k];
      for (int32_t i = rev_off[(size_t)t]; i < rev_off[(size_t)t + 1]; ++i) {
        const int32_t s = rev[(size_t)i];
        blevel[(size_t)s] = std::max(blevel[(size_t)s], blevel[(size_t)t] + 1);
        if (--left[(size_t)s] == 0) order.push_back(s);
      }
    }
    if ((int32_t)order.size() != S) return capi_fail(WFST_E_FORMAT, "align graph " + std::to_string(g) + ": its epsilon arcs form a cycle");
    int32_t bdepth = 0;
    for (int32_t s = 0; s < S; ++s) bdepth = std::max(bdepth, blevel[(size_t)s]);
    int32_t *B = bhdr.data() + (size_t)g * kGpostHdr;
    B[0] = H[6]; B[1] = H[11]; B[2] = (int32_t)blvl_state.size(); B[3] = (int32_t)blvl_off.size(); B[4] = bdepth;
    for (int32_t L = 0; L <= bdepth; ++L) {
      blvl_off.push_back((int32_t)blvl_state.size() - B[2]);
      for (int32_t s = 0; s < S; ++s)
        if (blevel[(size_t)s] == L) blvl_state.push_back(s);
    }
    blvl_off.push_back((int32_t)blvl_state.size() - B[2]);
  }
  std::unique_ptr<GpostTables> t(new GpostTables);
  int rc = upload(t->d_bhdr, bhdr);
  if (rc == WFST_OK) rc = upload(t->d_out_off, gs->h_out_off);
  if (rc == WFST_OK) rc = upload(t->d_orec, orec);
  if (rc == WFST_OK) rc = upload(t->d_blvl_state, blvl_state);
  if (rc == WFST_OK) rc = upload(t->d_blvl_off, blvl_off);
  if (rc != WFST_OK) return rc;
  *out = gs->gpost = t.release();
  return WFST_OK;
}

}  // namespace

extern "C" {

int wfst_decoder_graph_posteriors(wfst_decoder *d, const int32_t *channels, int32_t n, const wfst_align_graphs *graphs,
                                  const int32_t *graph_of, const int32_t *n_frames_in, const int32_t *label_map, int32_t n_tid,
                                  double graph_scale, double acoustic_scale, double min_post, int64_t max_cells, int32_t cap_frames,
                                  int32_t cap_entries, int32_t cap_arcs, void *const *grad, const int64_t *grad_pitch,
                                  const int32_t *grad_frames, int32_t n_cols, double grad_scale, void *consumer_stream, int32_t *status,
                                  int32_t *found, int32_t *n_frames, double *log_like, int32_t *n_entries, int32_t *n_arcs,
                                  int32_t *frame_off, int32_t *n_distinct, double *frame_mass, int32_t *entry_class, double *entry_post,
                                  double *arc_occ) {
  if (!d || !channels) return capi_fail(WFST_E_ARG, "NULL decoder / channel list");
  if (!graphs || !graph_of) return capi_fail(WFST_E_ARG, "NULL align graphs / graph_of");
  if (!std::isfinite(graph_scale) || !std::isfinite(acoustic_scale) || graph_scale < 0.0 || acoustic_scale < 0.0)
    return capi_fail(WFST_E_ARG, "graph_scale / acoustic_scale must be finite and >= 0");
  if (!(min_post >= 0.0 && min_post <= 1.0)) return capi_fail(WFST_E_ARG, "min_post outside 0 .. 1");
  const bool lists = cap_frames != 0 || cap_entries != 0;   // (0, 0: no lists, the dense rows and the channels' numbers only)
  if (lists && (cap_frames < 1 || cap_entries < 1)) return capi_fail(WFST_E_ARG, "cap_frames / cap_entries < 1 (both 0: no lists)");
  if (cap_arcs < 0) return capi_fail(WFST_E_ARG, "cap_arcs < 0");
  if (max_cells < 0) return capi_fail(WFST_E_ARG, "max_cells < 0");
  if (label_map) {
    if (n_tid < 1) return capi_fail(WFST_E_ARG, "label_map with n_tid < 1");
    for (int32_t t = 1; t <= n_tid; ++t)
      if (label_map[t] < 0) return capi_fail(WFST_E_ARG, "a negative class in label_map");
  }
  if (!std::isfinite(grad_scale)) return capi_fail(WFST_E_ARG, "grad_scale is not finite");
  if (grad) {
    if (!grad_frames || n_cols < 1) return capi_fail(WFST_E_ARG, "grad without grad_frames, or n_cols < 1");
    for (int32_t i = 0; i < n; ++i) {
      if (!grad[i]) continue;
      if (reinterpret_cast<uintptr_t>(grad[i]) % 4) return capi_fail(WFST_E_ARG, "a grad pointer is not aligned to 4 bytes");
      if (grad_frames[i] < 0) return capi_fail(WFST_E_ARG, "grad_frames < 0");
      if (grad_pitch && grad_pitch[i] < n_cols) return capi_fail(WFST_E_ARG, "a grad_pitch below n_cols");
    }
    if (label_map)
      for (int32_t t = 1; t <= n_tid; ++t)
        if (label_map[t] >= n_cols) return capi_fail(WFST_E_ARG, "a label_map class >= n_cols");
  }
  const ForcedView V = forced_view(d);
  if (n <= 0 || n > V.n_channels) return capi_fail(WFST_E_ARG, "bad channel count");
  {
    std::vector<char> seen((size_t)V.n_channels, 0);
    for (int32_t i = 0; i < n; ++i) {
      const int32_t c = channels[i];
      if (c < 0 || c >= V.n_channels) return capi_fail(WFST_E_ARG, "channel index out of range");
      if (seen[(size_t)c]) return capi_fail(WFST_E_ARG, "duplicate channel in list");
      seen[(size_t)c] = 1;
    }
    for (int32_t i = 0; i < n; ++i)
      if (V.state[channels[i]] == 0) return capi_fail(WFST_E_STATE, "GraphPosteriors before InitDecoding");
  }
  if (graphs->device != V.device) return capi_fail(WFST_E_ARG, "the align graphs live on another device than the decoder");
  const size_t N = (size_t)n;
  const std::vector<int32_t> &t2p = *V.tid2pdf;
  struct Src { const float *ll; int32_t stride, T; };
  std::vector<Src> src(N);
  for (size_t i = 0; i < N; ++i) {
    const int32_t c = channels[i], g = graph_of[i];
    if (g < 0 || g >= graphs->n_graphs) return capi_fail(WFST_E_ARG, "graph_of out of range");
    const int32_t *H = graphs->hdr.data() + (size_t)g * kFalignHdr;
    // the frames the channel's scores cover: the library's history, or what the search has decoded of the caller's own matrix
    Src s = {nullptr, 0, 0};
    if (V.hist_rows[c] > 0) s = Src{V.hist_dev[c], V.hist_stride, V.hist_rows[c]};
    else if (V.ll_base[c]) s = Src{V.ll_base[c], V.ll_stride, V.decoded[c]};
    const int32_t want = n_frames_in ? n_frames_in[i] : -1;
    if (want < -1 || want > s.T)
      return capi_fail(WFST_E_ARG, "channel " + std::to_string(c) + ": n_frames_in " + std::to_string(want) + " outside the " + std::to_string(s.T) + " frames held");
    if (want >= 0) s.T = want;
    src[i] = s;
    if (!t2p.empty() && H[12] >= (int32_t)t2p.size())
      return capi_fail(WFST_E_ARG, "align graph " + std::to_string(g) + ": ilabel " + std::to_string(H[12]) + " outside the decoder graph's tid2pdf range");
    if (label_map && H[12] > n_tid) return capi_fail(WFST_E_ARG, "align graph " + std::to_string(g) + ": arc ilabel outside label_map range");
    if (grad && !label_map && H[12] >= n_cols)
      return capi_fail(WFST_E_ARG, "align graph " + std::to_string(g) + ": n_cols does not exceed its largest transition-id");
    if (s.T > 0) {   // every column the kernel may read lies inside a row
      for (int32_t j = 0; j < H[5]; ++j) {
        const int32_t il = graphs->labels[(size_t)H[10] + (size_t)j], col = t2p.empty() ? il : t2p[(size_t)il];
        if (col < 0 || col >= s.stride)
          return capi_fail(WFST_E_ARG, "align graph " + std::to_string(g) + ": transition-id " + std::to_string(il) + " reads column " + std::to_string(col) +
                                           " beyond the score stride " + std::to_string(s.stride) + " of channel " + std::to_string(c));
      }
    }
  }
  // ---- the outputs zeroed, the channels' own failures -----------------------------------------------------------------------------
  const size_t capf = (size_t)cap_frames, cape = (size_t)cap_entries, capa = (size_t)cap_arcs;
  align_zero(status, N); align_zero(found, N); align_zero(n_frames, N); align_zero(log_like, N); align_zero(n_entries, N);
  align_zero(n_arcs, N); align_zero(frame_off, N * (capf + 1)); align_zero(n_distinct, N * capf); align_zero(frame_mass, N * capf);
  align_zero(entry_class, N * cape); align_zero(entry_post, N * cape); align_zero(arc_occ, N * capa);
  const int64_t bound = max_cells ? max_cells : kFalignDefaultCells;
  std::vector<int64_t> need(N);
  std::vector<char> run(N, 1);
  bool any = false;
  for (size_t i = 0; i < N; ++i) {
    const int32_t *H = graphs->hdr.data() + (size_t)graph_of[i] * kFalignHdr;
    need[i] = ((int64_t)src[i].T + 1) * H[2];
    if (need[i] > bound) {
      run[i] = 0;
      const int code = capi_fail(WFST_E_CAPACITY, "channel " + std::to_string(channels[i]) + ": graph posteriors: a table of " + std::to_string(src[i].T + 1) +
                                                      " x " + std::to_string(H[2]) + " cells, max_cells is " + std::to_string(bound));
      if (status) status[i] = code;
      if (n_frames) n_frames[i] = src[i].T;
    }
    any |= run[i] != 0;
  }
  if (!any) return WFST_OK;
  hipStream_t stream;
  int rc = forced_stream(d, &stream);
  if (rc != WFST_OK) return rc;
  const GpostTables *tables;
  rc = gpost_tables(graphs, &tables);
  if (rc != WFST_OK) return rc;
  GraphPostState &F = *graphpost_state(d);
  // ---- per distinct graph of the list its class CSR: the classes ascending, per class its emitting arcs by arc index ------------------
  struct Cls { int64_t off; int32_t n_slots; };
  std::map<int32_t, Cls> cls_of;
  const size_t n_col = t2p.size();
  std::vector<int32_t> maps(t2p.begin(), t2p.end());
  for (size_t i = 0; i < N; ++i) {
    const int32_t g = graph_of[i];
    if (!run[i] || cls_of.count(g)) continue;
    const int32_t *H = graphs->hdr.data() + (size_t)g * kFalignHdr;
    const int4 *ar = graphs->h_arcs.data() + H[11];
    std::vector<int32_t> classes;
    for (int32_t j = 0; j < H[5]; ++j) {
      const int32_t il = graphs->labels[(size_t)H[10] + (size_t)j];
      classes.push_back(label_map ? label_map[il] : il);
    }
    std::sort(classes.begin(), classes.end());
    classes.erase(std::unique(classes.begin(), classes.end()), classes.end());
    const size_t ns = classes.size();
    std::vector<int32_t> slot_off(ns + 1, 0), slot_arc;
    auto slot_of = [&](int32_t il) { return (size_t)(std::lower_bound(classes.begin(), classes.end(), label_map ? label_map[il] : il) - classes.begin()); };
    for (int32_t a = 0; a < H[3]; ++a)
      if (ar[a].x) ++slot_off[slot_of(ar[a].x) + 1];
    for (size_t j = 0; j < ns; ++j) slot_off[j + 1] += slot_off[j];
    slot_arc.resize((size_t)slot_off[ns]);
    std::vector<int32_t> at(slot_off.begin(), slot_off.end() - 1);
    for (int32_t a = 0; a < H[3]; ++a)
      if (ar[a].x) slot_arc[(size_t)at[slot_of(ar[a].x)]++] = a;
    cls_of[g] = Cls{(int64_t)(maps.size() - n_col), (int32_t)ns};
    maps.insert(maps.end(), classes.begin(), classes.end());
    maps.insert(maps.end(), slot_off.begin(), slot_off.end());
    maps.insert(maps.end(), slot_arc.begin(), slot_arc.end());
  }
  ALIGN_TRY(align_grow(F.maps, maps.size()));
  if (!maps.empty()) ALIGN_TRY(hipMemcpyAsync(F.maps.p, maps.data(), maps.size() * 4, hipMemcpyHostToDevice, stream));
  const size_t out_ints = (size_t)gpost_out_ints(cap_frames, cap_entries), out_dbl = (size_t)gpost_out_doubles(cap_frames, cap_entries, cap_arcs);
  std::vector<GpostChan> entries;
  std::vector<int32_t> landed;
  std::vector<double> landed_d;
  // ---- round by round: lists whose tables pass kFalignRoundCells together; an explicit max_cells bounds a round as well -------------
  const int64_t round_cells = max_cells ? std::min(max_cells, kFalignRoundCells / 2) : kFalignRoundCells / 2;   // 8-byte cells: 256 MiB
  for (size_t first = 0; first < N;) {
    const RoundCut cut = cut_round(need, run, first, round_cells);
    first = cut.next;
    if (cut.members.empty()) break;
    const size_t cnt = cut.members.size();
    entries.assign(cnt, GpostChan{});
    int64_t tab_cells = 0, row_cells = 0, gam_cells = 0, post_cells = 0, cnt_ints = 0;
    int32_t max_T = 0;
    bool dense = false;
    for (size_t j = 0; j < cnt; ++j) {
      const size_t i = cut.members[j];
      const int32_t *H = graphs->hdr.data() + (size_t)graph_of[i] * kFalignHdr;
      const Cls &K = cls_of[graph_of[i]];
      GpostChan &E = entries[j];
      E.ll = src[i].ll; E.stride = src[i].stride; E.T = src[i].T; E.graph = graph_of[i];
      E.tab_off = tab_cells; E.row_off = row_cells; E.gam_off = gam_cells; E.post_off = post_cells; E.cnt_off = cnt_ints;
      E.cls_off = (int64_t)n_col + K.off;
      E.n_slots = K.n_slots;
      E.want_occ = arc_occ != nullptr;
      if (grad && grad[i]) {
        E.grad = static_cast<float *>(grad[i]);
        E.grad_pitch = grad_pitch ? grad_pitch[i] : (int64_t)n_cols;
        E.grad_rows = grad_frames[i];
        dense = dense || (E.grad_rows > 0 && E.T > 0);
      }
      tab_cells += need[i];
      if (H[2] > kGpostLdsStates) row_cells += 2ll * H[2];
      gam_cells += 3ll * H[3];
      post_cells += (int64_t)E.T * K.n_slots;
      cnt_ints += E.T;
      max_T = std::max(max_T, E.T);
    }
    if (align_grow(F.tab, (size_t)tab_cells) != hipSuccess || align_grow(F.rows, (size_t)row_cells) != hipSuccess ||
        align_grow(F.gam, (size_t)gam_cells) != hipSuccess || align_grow(F.post, (size_t)post_cells) != hipSuccess ||
        align_grow(F.cnt, (size_t)cnt_ints) != hipSuccess || align_grow(F.chan, cnt) != hipSuccess ||
        align_grow(F.out, cnt * out_ints) != hipSuccess || align_grow(F.dout, cnt * out_dbl) != hipSuccess) {
      (void)hipGetLastError();
      return capi_fail(WFST_E_CAPACITY, "graph posteriors: no device memory for the workspace of " + std::to_string(cnt) + " channel(s): " +
                                            std::to_string(tab_cells) + " table cells of 8 bytes; lower max_cells or list fewer channels");
    }
    ALIGN_TRY(hipMemcpyAsync(F.chan.p, entries.data(), cnt * sizeof(GpostChan), hipMemcpyHostToDevice, stream));
    ALIGN_TRY(hipMemsetAsync(F.out.p, 0, cnt * out_ints * 4, stream));
    ALIGN_TRY(hipMemsetAsync(F.dout.p, 0, cnt * out_dbl * 8, stream));
    GpostDev Q = {};
    Q.G = graphs->view();
    Q.B = tables->view();
    Q.chan = F.chan.p;
    Q.col_map = n_col ? F.maps.p : nullptr;
    Q.cls = F.maps.p;
    Q.graph_scale = graph_scale; Q.acoustic_scale = acoustic_scale; Q.min_post = min_post; Q.grad_scale = grad_scale;
    Q.tab = F.tab.p; Q.rows = F.rows.p; Q.gam = F.gam.p; Q.post = F.post.p; Q.cnt = F.cnt.p;
    Q.cap_frames = cap_frames; Q.cap_entries = cap_entries; Q.cap_arcs = cap_arcs; Q.n_cols = n_cols;
    Q.out = F.out.p; Q.dout = F.dout.p;
    // the dense rows against the caller's stream, both ways, as wfst_decoder_sequence_stats orders them
    const bool linked = dense && consumer_stream != WFST_STREAM_NONE;
    const hipStream_t cons = linked ? static_cast<hipStream_t>(consumer_stream) : nullptr;
    if (linked) {
      if (!F.free_ev.h) ALIGN_TRY(F.free_ev.create());
      if (!F.rows_ev.h) ALIGN_TRY(F.rows_ev.create());
      ALIGN_TRY(hipEventRecord(F.free_ev.h, cons));
      ALIGN_TRY(hipStreamWaitEvent(stream, F.free_ev.h, 0));
    }
    launch_graph_post(Q, (int)cnt, max_T, dense, stream);
    ALIGN_TRY(hipGetLastError());
    if (linked) {
      ALIGN_TRY(hipEventRecord(F.rows_ev.h, stream));
      ALIGN_TRY(hipStreamWaitEvent(cons, F.rows_ev.h, 0));
    }
    landed.resize(cnt * out_ints);
    landed_d.resize(cnt * out_dbl);
    ALIGN_TRY(hipMemcpyAsync(landed.data(), F.out.p, cnt * out_ints * 4, hipMemcpyDeviceToHost, stream));
    ALIGN_TRY(hipMemcpyAsync(landed_d.data(), F.dout.p, cnt * out_dbl * 8, hipMemcpyDeviceToHost, stream));
    ALIGN_TRY(hipStreamSynchronize(stream));
    for (size_t j = 0; j < cnt; ++j) {
      const size_t i = cut.members[j];
      const int32_t *r = landed.data() + j * out_ints, c = channels[i];
      const double *dd = landed_d.data() + j * out_dbl;
      if (!r[0]) continue;   // not found: every output of the channel stays zero
      const int32_t T = r[1], ne = r[2], A = graphs->hdr[(size_t)graph_of[i] * kFalignHdr + 3];
      if (found) found[i] = 1;
      if (n_frames) n_frames[i] = T;
      if (log_like) log_like[i] = dd[0];
      if (n_entries) n_entries[i] = ne;
      if (n_arcs) n_arcs[i] = A;
      if (arc_occ && A <= cap_arcs) memcpy(arc_occ + i * capa, dd + 1 + capf + cape, (size_t)A * 8);
      if (lists && !r[3]) {
        const int32_t *r_off = r + kGpostHead, *r_nd = r_off + capf + 1, *r_class = r_nd + capf;
        if (frame_off) memcpy(frame_off + i * (capf + 1), r_off, ((size_t)T + 1) * 4);
        if (n_distinct) memcpy(n_distinct + i * capf, r_nd, (size_t)T * 4);
        if (frame_mass) memcpy(frame_mass + i * capf, dd + 1, (size_t)T * 8);
        if (entry_class) memcpy(entry_class + i * cape, r_class, (size_t)ne * 4);
        if (entry_post) memcpy(entry_post + i * cape, dd + 1 + capf, (size_t)ne * 8);
      }
      // the rows do not hold the lists or the occupancies: the counts are the room they take, log_like and the dense rows stand
      if (r[3] || (arc_occ && A > cap_arcs)) {
        const int code = capi_fail(WFST_E_CAPACITY, "channel " + std::to_string(c) + ": graph posteriors: " + std::to_string(T) + " frames, " + std::to_string(ne) +
                                                        " entries and " + std::to_string(A) + " arcs; cap_frames is " + std::to_string(cap_frames) +
                                                        ", cap_entries " + std::to_string(cap_entries) + " and cap_arcs " + std::to_string(cap_arcs));
        if (status) status[i] = code;
      }
    }
  }
  return WFST_OK;
}

int wfst_decoder_graph_posteriors_workspace(wfst_decoder *d, int64_t *bytes) {
  if (!d || !bytes) return capi_fail(WFST_E_ARG, "NULL decoder / bytes");
  *bytes = graphpost_state(d)->bytes();
  return WFST_OK;
}

}  // extern "C"
