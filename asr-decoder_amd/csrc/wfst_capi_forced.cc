// wfst_align_graphs_create / _info / _free and wfst_decoder_force_align: batched forced alignment of the listed channels' scores against
// per-utterance graphs, one launch per round (forced_align_kernel, wfst_forced.hip).  A translation unit of its own -- see
// wfst_capi_forced.h.
#include "wfst_capi_forced.h"

#include <algorithm>
#include <cstring>
#include <memory>

#include "wfst_capi_align.h"   // capi_fail, ALIGN_TRY, align_grow, align_zero, cut_round
#include "wfst_openfst.h"

using namespace wfst;

namespace {
template <class T>
int upload(DevBuf<T> &buf, const std::vector<T> &v) {
  ALIGN_TRY(buf.alloc(v.size()));
  if (!v.empty()) ALIGN_TRY(hipMemcpy(buf.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return WFST_OK;
}
}  // namespace

extern "C" {

int wfst_align_graphs_create(int32_t n_graphs, const int32_t *start, const int32_t *final_state, const int32_t *n_states,
                             const int32_t *n_arcs, const wfst_state_info *states, const wfst_arc *arcs, int device,
                             wfst_align_graphs **out) {
  if (!out) return capi_fail(WFST_E_ARG, "out is NULL");
  *out = nullptr;
  if (n_graphs <= 0 || !start || !final_state || !n_states || !n_arcs || !states) return capi_fail(WFST_E_ARG, "empty graph set or NULL arrays");
  // ---- validation and the kernel's tables, on the host: no device is touched before every graph stands ---------------------------
  std::unique_ptr<wfst_align_graphs> gs(new wfst_align_graphs);
  gs->n_graphs = n_graphs;
  gs->hdr.assign((size_t)n_graphs * kFalignHdr, 0);
  std::vector<int2> in_off;
  std::vector<int4> rec, arcs_dev;
  std::vector<int32_t> lvl_state, lvl_off;
  int64_t s0 = 0, a0 = 0;
  for (int32_t g = 0; g < n_graphs; ++g) {
    const std::string who = "align graph " + std::to_string(g) + ": ";
    const int32_t S = n_states[g], A = n_arcs[g];
    if (S <= 0 || A < 0 || (A > 0 && !arcs)) return capi_fail(WFST_E_ARG, who + "empty graph or NULL arrays");
    if (start[g] < 0 || start[g] >= S) return capi_fail(WFST_E_ARG, who + "start state out of range");
    if (final_state[g] < 0 || final_state[g] >= S) return capi_fail(WFST_E_ARG, who + "final state out of range");
    const wfst_state_info *st = states + s0;
    const wfst_arc *ar = arcs + a0;
    // everything wfst_graph_from_arrays checks of the reference format, labels and targets
    std::vector<int32_t> src((size_t)A);
    int64_t off = 0;
    int32_t max_il = 0;
    for (int32_t s = 0; s < S; ++s) {
      const uint32_t na = st[s].num_arcs, ne = st[s].niepsilons;
      if (ne > na || off + na > A) return capi_fail(WFST_E_FORMAT, who + "state arc counts inconsistent with total_arcs");
      for (uint32_t i = 0; i < na; ++i) {
        const wfst_arc &a = ar[off + i];
        if (a.ilabel < 0 || a.olabel < 0) return capi_fail(WFST_E_FORMAT, who + "negative label");
        if ((i < ne) != (a.ilabel == 0))
          return capi_fail(WFST_E_FORMAT, who + "input-epsilon arcs must precede a state's other arcs (reference flat format)");
        if (a.nextstate < 0 || a.nextstate >= S) return capi_fail(WFST_E_FORMAT, who + "arc nextstate out of range");
        src[(size_t)(off + i)] = s;
        max_il = std::max(max_il, a.ilabel);
      }
      off += na;
    }
    if (off != A) return capi_fail(WFST_E_FORMAT, who + "sum of num_arcs != total_arcs");
    // the level of every state in the epsilon DAG: 0 without an epsilon in-arc, else 1 + the highest level of such an arc's source
    std::vector<int32_t> n_eps_in((size_t)S, 0), level((size_t)S, 0), order;
    for (int32_t a = 0; a < A; ++a)
      if (ar[a].ilabel == 0) ++n_eps_in[(size_t)ar[a].nextstate];
    std::vector<int32_t> left = n_eps_in;
    for (int32_t s = 0; s < S; ++s)
      if (!left[(size_t)s]) order.push_back(s);
    {
      std::vector<int64_t> first((size_t)S + 1, 0);
      for (int32_t s = 0; s < S; ++s) first[(size_t)s + 1] = first[(size_t)s] + st[s].num_arcs;
      for (size_t k = 0; k < order.size(); ++k) {
        const int32_t s = order[k];
        for (uint32_t i = 0; i < st[s].niepsilons; ++i) {
          const int32_t t = ar[first[(size_t)s] + i].nextstate;
          level[(size_t)t] = std::max(level[(size_t)t], level[(size_t)s] + 1);
          if (--left[(size_t)t] == 0) order.push_back(t);
        }
      }
    }
    if ((int32_t)order.size() != S) {
      // a state that never became free has an epsilon in-arc from another such state: S steps backwards end inside a cycle
      int32_t u = 0;
      while (left[(size_t)u] == 0) ++u;
      for (int32_t step = 0; step < S; ++step)
        for (int32_t a = 0; a < A; ++a)
          if (ar[a].ilabel == 0 && ar[a].nextstate == u && left[(size_t)src[(size_t)a]] > 0) { u = src[(size_t)a]; break; }
      return capi_fail(WFST_E_FORMAT, who + "its epsilon arcs form a cycle through state " + std::to_string(u));
    }
    int32_t depth = 0;
    for (int32_t s = 0; s < S; ++s) depth = std::max(depth, level[(size_t)s]);
    // the distinct ilabels
    std::vector<int32_t> labs;
    for (int32_t a = 0; a < A; ++a)
      if (ar[a].ilabel != 0) labs.push_back(ar[a].ilabel);
    std::sort(labs.begin(), labs.end());
    labs.erase(std::unique(labs.begin(), labs.end()), labs.end());
    // the in-arc index by destination: emitting records first, each kind by arc index ascending (a counting sort over two keys)
    int32_t *H = gs->hdr.data() + (size_t)g * kFalignHdr;
    if ((int64_t)in_off.size() + S + 1 > INT32_MAX || (int64_t)rec.size() + A > INT32_MAX)
      return capi_fail(WFST_E_FORMAT, "align graphs: 2^31 states or arcs in one set");
    H[0] = start[g]; H[1] = final_state[g]; H[2] = S; H[3] = A; H[4] = depth; H[5] = (int32_t)labs.size();
    H[6] = (int32_t)in_off.size(); H[7] = (int32_t)rec.size(); H[8] = (int32_t)lvl_state.size(); H[9] = (int32_t)lvl_off.size();
    H[10] = (int32_t)gs->labels.size(); H[11] = (int32_t)arcs_dev.size(); H[12] = max_il;
    std::vector<int32_t> n_emit((size_t)S, 0), n_eps((size_t)S, 0);
    for (int32_t a = 0; a < A; ++a) ++(ar[a].ilabel ? n_emit : n_eps)[(size_t)ar[a].nextstate];
    std::vector<int32_t> at_emit((size_t)S), at_eps((size_t)S);
    int32_t at = 0;
    int32_t first_arc = 0;
    for (int32_t s = 0; s < S; ++s) {
      at_emit[(size_t)s] = at;
      at_eps[(size_t)s] = at + n_emit[(size_t)s];
      in_off.push_back(make_int2(at, at + n_emit[(size_t)s]));
      at += n_emit[(size_t)s] + n_eps[(size_t)s];
      gs->h_out_off.push_back(make_int2(first_arc, first_arc + (int32_t)st[s].niepsilons));
      first_arc += (int32_t)st[s].num_arcs;
    }
    in_off.push_back(make_int2(at, at));
    gs->h_out_off.push_back(make_int2(first_arc, first_arc));
    const size_t r0 = rec.size();
    rec.resize(r0 + (size_t)A);
    for (int32_t a = 0; a < A; ++a) {
      const wfst_arc &x = ar[a];
      int32_t wbits, slot = -1;
      memcpy(&wbits, &x.weight, 4);
      if (x.ilabel) slot = (int32_t)(std::lower_bound(labs.begin(), labs.end(), x.ilabel) - labs.begin());
      int32_t &pos = (x.ilabel ? at_emit : at_eps)[(size_t)x.nextstate];
      rec[r0 + (size_t)pos++] = make_int4(src[(size_t)a], slot, wbits, a);
      arcs_dev.push_back(make_int4(x.ilabel, x.olabel, wbits, x.nextstate));
    }
    // the states with epsilon in-arcs, by level
    for (int32_t L = 1; L <= depth; ++L) {
      lvl_off.push_back((int32_t)lvl_state.size() - H[8]);
      for (int32_t s = 0; s < S; ++s)
        if (level[(size_t)s] == L) lvl_state.push_back(s);
    }
    lvl_off.push_back((int32_t)lvl_state.size() - H[8]);
    gs->labels.insert(gs->labels.end(), labs.begin(), labs.end());
    s0 += S;
    a0 += A;
  }
  gs->total_states = s0;
  gs->total_arcs = a0;
  // ---- the device ---------------------------------------------------------------------------------------------------------------
  const int ndev = wfst_device_count();
  if (ndev <= 0) return capi_fail(WFST_E_DEVICE, "no HIP device available (this library has no CPU path)");
  if (device < 0 || device >= ndev) return capi_fail(WFST_E_ARG, "device index out of range");
  ALIGN_TRY(hipSetDevice(device));
  gs->device = device;
  int rc = upload(gs->d_hdr, gs->hdr);
  if (rc == WFST_OK) rc = upload(gs->d_in_off, in_off);
  if (rc == WFST_OK) rc = upload(gs->d_rec, rec);
  if (rc == WFST_OK) rc = upload(gs->d_lvl_state, lvl_state);
  if (rc == WFST_OK) rc = upload(gs->d_lvl_off, lvl_off);
  if (rc == WFST_OK) rc = upload(gs->d_labels, gs->labels);
  if (rc == WFST_OK) rc = upload(gs->d_arcs, arcs_dev);
  if (rc != WFST_OK) return rc;
  gs->h_arcs = std::move(arcs_dev);
  *out = gs.release();
  return WFST_OK;
}

int wfst_align_graphs_load(int32_t n_graphs, const char *const *paths, int device, wfst_align_graphs **out) {
  if (!out) return capi_fail(WFST_E_ARG, "out is NULL");
  *out = nullptr;
  if (n_graphs <= 0 || !paths) return capi_fail(WFST_E_ARG, "empty graph set or NULL paths");
  std::vector<int32_t> start, fin, ns, na;
  std::vector<wfst_state_info> states;
  std::vector<wfst_arc> arcs;
  for (int32_t g = 0; g < n_graphs; ++g) {
    if (!paths[g]) return capi_fail(WFST_E_ARG, "NULL path");
    HostGraph hg;
    std::string err;
    const int rc = read_graph_file(paths[g], &hg, &err);
    if (rc != WFST_OK) return capi_fail(rc, std::string(paths[g]) + ": " + err);
    start.push_back(hg.start); fin.push_back(hg.final_state);
    ns.push_back((int32_t)hg.states.size()); na.push_back((int32_t)hg.arcs.size());
    states.insert(states.end(), hg.states.begin(), hg.states.end());
    arcs.insert(arcs.end(), hg.arcs.begin(), hg.arcs.end());
  }
  return wfst_align_graphs_create(n_graphs, start.data(), fin.data(), ns.data(), na.data(), states.data(), arcs.data(), device, out);
}

int wfst_align_graphs_info(const wfst_align_graphs *g, int32_t *n_graphs, int64_t *total_states, int64_t *total_arcs,
                           int32_t *n_states, int32_t *n_arcs, int32_t *max_ilabel, int32_t *eps_depth, int32_t *n_labels,
                           int64_t *device_bytes) {
  if (!g) return capi_fail(WFST_E_ARG, "NULL align graphs");
  if (n_graphs) *n_graphs = g->n_graphs;
  if (total_states) *total_states = g->total_states;
  if (total_arcs) *total_arcs = g->total_arcs;
  for (int32_t i = 0; i < g->n_graphs; ++i) {
    const int32_t *H = g->hdr.data() + (size_t)i * kFalignHdr;
    if (n_states) n_states[i] = H[2];
    if (n_arcs) n_arcs[i] = H[3];
    if (max_ilabel) max_ilabel[i] = H[12];
    if (eps_depth) eps_depth[i] = H[4];
    if (n_labels) n_labels[i] = H[5];
  }
  if (device_bytes) *device_bytes = g->device_bytes();
  return WFST_OK;
}

void wfst_align_graphs_free(wfst_align_graphs *g) {
  if (!g) return;
  (void)hipSetDevice(g->device);
  gpost_tables_free(g->gpost);
  delete g;
}

int wfst_decoder_force_align(wfst_decoder *d, const int32_t *channels, int32_t n, const wfst_align_graphs *graphs,
                             const int32_t *graph_of, const int32_t *n_frames_in, const int32_t *label_map, int32_t n_tid,
                             int64_t max_cells, int32_t cap_frames, int32_t cap_hops, int32_t cap_words, int32_t *status,
                             int32_t *found, int32_t *n_frames, float *path_cost, float *tot_score, float *lm_score, int32_t *n_hops,
                             int32_t *hop_arc, int32_t *alignment, int32_t *n_words, int32_t *words, int32_t *word_frame) {
  if (!d || !channels) return capi_fail(WFST_E_ARG, "NULL decoder / channel list");
  if (!graphs || !graph_of) return capi_fail(WFST_E_ARG, "NULL align graphs / graph_of");
  if (cap_frames < 0 || cap_hops < 0 || cap_words < 0) return capi_fail(WFST_E_ARG, "cap_frames / cap_hops / cap_words < 0");
  if (max_cells < 0) return capi_fail(WFST_E_ARG, "max_cells < 0");
  if (label_map) {
    if (n_tid < 1) return capi_fail(WFST_E_ARG, "label_map with n_tid < 1");
    for (int32_t t = 1; t <= n_tid; ++t)
      if (label_map[t] < 0) return capi_fail(WFST_E_ARG, "a negative class in label_map");
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
      if (V.state[channels[i]] == 0) return capi_fail(WFST_E_STATE, "ForceAlign before InitDecoding");
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
  const size_t capf = (size_t)cap_frames, caph = (size_t)cap_hops, capw = (size_t)cap_words;
  align_zero(status, N); align_zero(found, N); align_zero(n_frames, N); align_zero(path_cost, N); align_zero(tot_score, N);
  align_zero(lm_score, N); align_zero(n_hops, N); align_zero(hop_arc, N * caph); align_zero(alignment, N * capf); align_zero(n_words, N);
  align_zero(words, N * capw); align_zero(word_frame, N * capw);
  const int64_t bound = max_cells ? max_cells : kFalignDefaultCells;
  std::vector<int64_t> need(N);
  std::vector<char> run(N, 1);
  bool any = false;
  for (size_t i = 0; i < N; ++i) {
    const int32_t *H = graphs->hdr.data() + (size_t)graph_of[i] * kFalignHdr;
    need[i] = ((int64_t)src[i].T + 1) * H[2];
    if (need[i] > bound) {
      run[i] = 0;
      const int code = capi_fail(WFST_E_CAPACITY, "channel " + std::to_string(channels[i]) + ": force align: a table of " + std::to_string(src[i].T + 1) +
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
  ForcedState &F = *V.fs;
  // the maps: the decoder graph's tid2pdf, then the caller's classes
  const size_t n_col = t2p.size(), n_lab = label_map ? (size_t)n_tid + 1 : 0;
  ALIGN_TRY(align_grow(F.maps, n_col + n_lab));
  if (n_col) ALIGN_TRY(hipMemcpyAsync(F.maps.p, t2p.data(), n_col * 4, hipMemcpyHostToDevice, stream));
  if (n_lab) ALIGN_TRY(hipMemcpyAsync(F.maps.p + n_col, label_map, n_lab * 4, hipMemcpyHostToDevice, stream));
  const size_t out_ints = (size_t)falign_out_ints(cap_frames, cap_hops, cap_words);
  std::vector<ForcedChan> entries;
  std::vector<int32_t> landed;
  // ---- round by round: lists whose backpointers pass kFalignRoundCells together; an explicit max_cells bounds a round as well ------
  const int64_t round_cells = max_cells ? std::min(max_cells, kFalignRoundCells) : kFalignRoundCells;
  for (size_t first = 0; first < N;) {
    const RoundCut cut = cut_round(need, run, first, round_cells);
    first = cut.next;
    if (cut.members.empty()) break;
    const size_t cnt = cut.members.size();
    entries.assign(cnt, ForcedChan{});
    int64_t bp_cells = 0, row_floats = 0, path_ints = 0;
    for (size_t j = 0; j < cnt; ++j) {
      const size_t i = cut.members[j];
      const int32_t *H = graphs->hdr.data() + (size_t)graph_of[i] * kFalignHdr;
      ForcedChan &E = entries[j];
      E.ll = src[i].ll; E.stride = src[i].stride; E.T = src[i].T; E.graph = graph_of[i];
      E.bp_off = bp_cells; E.row_off = row_floats; E.path_off = path_ints;
      // a path has T emitting hops and at most `depth` epsilon hops inside each of its T + 1 frames
      const int64_t pc = std::min<int64_t>((int64_t)E.T + ((int64_t)E.T + 1) * H[4], INT32_MAX);
      E.path_cap = (int32_t)pc;
      bp_cells += need[i];
      if (H[2] > kFalignLdsStates) row_floats += 2ll * H[2];
      path_ints += pc;
    }
    if (align_grow(F.bp, (size_t)bp_cells) != hipSuccess || align_grow(F.rows, (size_t)row_floats) != hipSuccess ||
        align_grow(F.path, (size_t)path_ints) != hipSuccess || align_grow(F.chan, cnt) != hipSuccess ||
        align_grow(F.out, cnt * out_ints) != hipSuccess) {
      (void)hipGetLastError();
      return capi_fail(WFST_E_CAPACITY, "force align: no device memory for the workspace of " + std::to_string(cnt) + " channel(s): " +
                                            std::to_string(bp_cells) + " backpointer cells of 4 bytes; lower max_cells or list fewer channels");
    }
    ALIGN_TRY(hipMemcpyAsync(F.chan.p, entries.data(), cnt * sizeof(ForcedChan), hipMemcpyHostToDevice, stream));
    ALIGN_TRY(hipMemsetAsync(F.out.p, 0, cnt * out_ints * 4, stream));
    ForcedDev Q = {};
    Q.G = graphs->view();
    Q.chan = F.chan.p;
    Q.col_map = n_col ? F.maps.p : nullptr;
    Q.label_map = n_lab ? F.maps.p + n_col : nullptr;
    Q.bp = F.bp.p; Q.path = F.path.p; Q.rows = F.rows.p;
    Q.cap_frames = cap_frames; Q.cap_hops = cap_hops; Q.cap_words = cap_words;
    Q.out = F.out.p;
    launch_forced_align(Q, (int)cnt, stream);
    ALIGN_TRY(hipGetLastError());
    landed.resize(cnt * out_ints);
    ALIGN_TRY(hipMemcpyAsync(landed.data(), F.out.p, cnt * out_ints * 4, hipMemcpyDeviceToHost, stream));
    ALIGN_TRY(hipStreamSynchronize(stream));
    for (size_t j = 0; j < cnt; ++j) {
      const size_t i = cut.members[j];
      const int32_t *r = landed.data() + j * out_ints, c = channels[i];
      if (r[7]) {
        const int code = capi_fail(WFST_E_DEVICE, "channel " + std::to_string(c) + ": force align: a traced path that does not end in the seed");
        if (status) status[i] = code;
        continue;
      }
      if (!r[0]) continue;   // not found: every output of the channel stays zero
      const int32_t T = r[1], nh = r[5], nw = r[6];
      if (found) found[i] = 1;
      if (n_frames) n_frames[i] = T;
      if (path_cost) memcpy(&path_cost[i], &r[2], 4);
      if (tot_score) memcpy(&tot_score[i], &r[3], 4);
      if (lm_score) memcpy(&lm_score[i], &r[4], 4);
      if (n_hops) n_hops[i] = nh;
      if (n_words) n_words[i] = nw;
      const int32_t *r_hops = r + kFalignHead, *r_ali = r_hops + caph, *r_words = r_ali + capf, *r_wf = r_words + capw;
      if (hop_arc) memcpy(hop_arc + i * caph, r_hops, std::min((size_t)nh, caph) * 4);
      if (alignment) memcpy(alignment + i * capf, r_ali, std::min((size_t)T, capf) * 4);
      if (words) memcpy(words + i * capw, r_words, std::min((size_t)nw, capw) * 4);
      if (word_frame) memcpy(word_frame + i * capw, r_wf, std::min((size_t)nw, capw) * 4);
      // the rows do not hold the path: the counts are the room it takes, what fits is written, the scores stand
      if ((alignment && T > cap_frames) || (hop_arc && nh > cap_hops) || ((words || word_frame) && nw > cap_words)) {
        const int code = capi_fail(WFST_E_CAPACITY, "channel " + std::to_string(c) + ": force align: " + std::to_string(T) + " frames, " + std::to_string(nh) +
                                                        " hops and " + std::to_string(nw) + " words; cap_frames is " + std::to_string(cap_frames) +
                                                        ", cap_hops " + std::to_string(cap_hops) + " and cap_words " + std::to_string(cap_words));
        if (status) status[i] = code;
      }
    }
  }
  return WFST_OK;
}

int wfst_decoder_force_align_workspace(wfst_decoder *d, int64_t *bytes) {
  if (!d || !bytes) return capi_fail(WFST_E_ARG, "NULL decoder / bytes");
  *bytes = forced_view(d).fs->bytes();
  return WFST_OK;
}

}  // extern "C"
