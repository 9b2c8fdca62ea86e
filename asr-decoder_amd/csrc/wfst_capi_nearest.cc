// wfst_decoder_nearest_words: the path of a channel's raw lattice nearest a reference word sequence -- least word edit distance, then
// least cost -- with the edit counts, the path's words, their times and scores, for a channel list (live and finalized channels mixed)
// and several references per channel, one launch per stage (lattice_emit_kernel for the live channels, align_index_kernel,
// nearest_kernel: wfst_nearest.hip).  A translation unit of its own -- see wfst_capi_nearest.h.
#include "wfst_capi_nearest.h"

#include <algorithm>
#include <cstring>
#include <string>

#include "wfst_capi_words.h"   // capi_fail, capi_fail_ctl

using namespace wfst;

#define N_TRY(expr)                                                                                   \
  do {                                                                                                \
    hipError_t e_ = (expr);                                                                           \
    if (e_ != hipSuccess) return capi_fail(WFST_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

namespace {
template <class B>
hipError_t grow(B &buf, size_t need) { return buf.n >= need ? hipSuccess : buf.alloc(need); }
template <class T>
void zero(T *p, size_t n) { if (p) std::fill(p, p + n, (T)0); }
}  // namespace

int wfst_decoder_nearest_words(wfst_decoder *d, const int32_t *channels, int32_t n, int32_t use_final_probs, int32_t n_refs, int32_t cap_words,
                               const int32_t *ref_words, const int32_t *ref_len, int32_t cap_hyp, int64_t max_cells, int32_t *status,
                               int32_t *found, int32_t *n_err, int32_t *n_cor, int32_t *n_sub, int32_t *n_ins, int32_t *n_del, int32_t *n_arcs,
                               int32_t *n_hyp, int32_t *hyp_words, int32_t *begin_frame, int32_t *end_frame, int32_t *ref_hyp, float *tot_score,
                               float *lm_score) {
  if (!d || !channels) return capi_fail(WFST_E_ARG, "NULL decoder / channel list");
  if (n_refs < 1 || n_refs > 64) return capi_fail(WFST_E_ARG, "1 <= n_refs <= 64 references per channel");
  if (cap_words <= 0 || cap_hyp <= 0) return capi_fail(WFST_E_ARG, "cap_words / cap_hyp <= 0");
  if (!ref_words || !ref_len) return capi_fail(WFST_E_ARG, "NULL references");
  if (max_cells < 0) return capi_fail(WFST_E_ARG, "max_cells < 0");
  AlignView V;
  int rc = align_begin(d, channels, n, &V);
  if (rc != WFST_OK) return rc;
  const size_t ns = (size_t)n_refs, cap = (size_t)cap_words, hcap = (size_t)cap_hyp, np = (size_t)n * ns;
  for (size_t p = 0; p < np; ++p) {
    if (ref_len[p] > cap_words) return capi_fail(WFST_E_ARG, "a ref_len above cap_words");
    for (int k = 0; k < ref_len[p]; ++k)
      if (ref_words[p * cap + (size_t)k] <= 0) return capi_fail(WFST_E_ARG, "a word id <= 0 inside a reference");
  }
  if (status) std::fill(status, status + n, (int32_t)WFST_OK);
  zero(found, np); zero(n_err, np); zero(n_cor, np); zero(n_sub, np); zero(n_ins, np); zero(n_del, np); zero(n_arcs, np); zero(n_hyp, np);
  zero(hyp_words, np * hcap); zero(begin_frame, np * hcap); zero(end_frame, np * hcap); zero(ref_hyp, np * cap);
  zero(tot_score, np); zero(lm_score, np);
  // the channels with a lattice to look at (a finalized channel without final-probs has none: GetRawLattice, base-inl.h:879-884),
  // by their position in the caller's list
  std::vector<int32_t> pos, list;
  for (int i = 0; i < n; ++i)
    if (align_channel_state(d, channels[i]) == 1 || use_final_probs) { pos.push_back(i); list.push_back(channels[i]); }
  if (pos.empty()) return WFST_OK;
  std::vector<int32_t> sizes;
  rc = align_emit(d, list, use_final_probs, &sizes);
  if (rc != WFST_OK) return rc;
  hipStream_t st = V.stream;
  AlignState &S = *V.as;
  const int64_t limit = max_cells > 0 ? max_cells : kNearestDefaultCells;
  // per listed channel: its own failure (reported in status[], the call goes on) or the cells its references' tables take
  std::vector<int64_t> need(pos.size(), 0);
  std::vector<char> run(pos.size(), 0);
  for (size_t i = 0; i < pos.size(); ++i) {
    const int32_t *z = &sizes[4 * i];
    const size_t o = (size_t)pos[i];
    if (z[3]) {   // a device error of THIS channel's utterance
      const int code = capi_fail_ctl(list[i], z[3]);
      if (status) status[o] = code;
      continue;
    }
    bool over = z[1] >= (1 << 30);   // (a traceback step names its in-arc record in 30 bits)
    for (size_t q = 0; q < ns; ++q) {
      const int32_t len = ref_len[o * ns + q];
      if (len < 0) continue;
      const int64_t cells = (int64_t)std::max(z[0], 0) * (len + 1);
      if (cells > limit) over = true;
      need[i] += cells;
    }
    if (over) {
      const int code = capi_fail(WFST_E_CAPACITY, "channel " + std::to_string(list[i]) + ": nearest: a table of " + std::to_string(z[0]) +
                                                      " lattice states x (words + 1) is beyond max_cells (" + std::to_string(limit) + ")");
      if (status) status[o] = code;
      continue;
    }
    run[i] = 1;
  }
  const size_t per = (size_t)nearest_out_ints(cap_words, cap_hyp);
  for (size_t first = 0; first < pos.size();) {
    // a round: the next channels whose tables fit the round's budget together (at least one)
    std::vector<size_t> rnd;
    int64_t cells = 0;
    size_t next = first;
    for (; next < pos.size(); ++next) {
      if (!run[next]) continue;
      if (!rnd.empty() && cells + need[next] > kNearestRoundCells) break;
      rnd.push_back(next);
      cells += need[next];
    }
    first = next;
    if (rnd.empty()) break;
    const size_t cnt = rnd.size(), pairs = cnt * ns;
    AlignDev A = {};
    A.ns_cap = 1; A.na_cap = 1; A.fr_cap = 2;
    for (size_t i : rnd) {
      A.ns_cap = std::max(A.ns_cap, sizes[4 * i]);
      A.na_cap = std::max(A.na_cap, sizes[4 * i + 1]);
      A.fr_cap = std::max(A.fr_cap, sizes[4 * i + 2] + 2);
    }
    A.idx_ints = align_idx_ints(A.ns_cap, A.na_cap, A.fr_cap);
    NearestDev N = {};
    N.lat_toks = V.D->lat_toks;
    N.lat_tok_cap = V.D->lat_tok_cap;
    N.n_refs = n_refs;
    N.cap_words = cap_words;
    N.cap_hyp = cap_hyp;
    N.path_cap = A.ns_cap + cap_words;   // a path has fewer arcs than the lattice has states, and at most one deletion per reference word
    N.sil_bits = V.sil_bits;
    N.n_tid = V.sil_ntid;
    // staged inputs: the pairs' table offsets (64-bit, first: aligned), the round's channels, the lengths, the words
    const size_t in_ints = 2 * pairs + cnt + pairs + pairs * cap, out_ints = pairs * per;
    const size_t idx_need = (size_t)A.idx_ints * cnt, path_need = pairs * (size_t)N.path_cap;
    const size_t cell_words = 2 * (size_t)std::max<int64_t>(cells, 1);   // (AlignState::cells counts 32-bit words)
    if (S.idx.n < idx_need || S.path.n < path_need || S.in.n < in_ints || S.out.n < out_ints || S.cells.n < cell_words) {
      N_TRY(hipStreamSynchronize(st));
      if (grow(S.idx, idx_need) != hipSuccess || grow(S.path, path_need) != hipSuccess || grow(S.in, in_ints) != hipSuccess ||
          grow(S.out, out_ints) != hipSuccess || grow(S.cells, cell_words) != hipSuccess) {
        (void)hipGetLastError();
        return capi_fail(WFST_E_CAPACITY, "nearest: no device memory for the workspace of " + std::to_string(cnt) + " lattice(s), " +
                                              std::to_string(n_refs) + " references each (" + std::to_string(cells) + " cells of 8 bytes): lower max_cells or ask for fewer channels at a time");
      }
    }
    N_TRY(S.pin.reserve(std::max(in_ints, out_ints)));
    int64_t *h_off = reinterpret_cast<int64_t *>(S.pin.p);
    int32_t *h_chan = S.pin.p + 2 * pairs, *h_len = h_chan + cnt, *h_words = h_len + pairs;
    int64_t at = 0;
    for (size_t j = 0; j < cnt; ++j) {
      const size_t i = rnd[j], o = (size_t)pos[i];
      h_chan[j] = list[i];
      memcpy(h_len + j * ns, ref_len + o * ns, ns * 4);
      memcpy(h_words + j * ns * cap, ref_words + o * ns * cap, ns * cap * 4);
      for (size_t q = 0; q < ns; ++q) {
        const int32_t len = ref_len[o * ns + q];
        h_off[j * ns + q] = len < 0 ? -1 : at;
        if (len >= 0) at += (int64_t)std::max(sizes[4 * i], 0) * (len + 1);
      }
    }
    N_TRY(hipMemcpyAsync(S.in.p, S.pin.p, in_ints * 4, hipMemcpyHostToDevice, st));
    A.idx = S.idx.p;
    N.cell_off = reinterpret_cast<const int64_t *>(S.in.p);
    const int32_t *dev_chan = S.in.p + 2 * pairs;
    N.ref_len = dev_chan + cnt;
    N.ref_words = N.ref_len + pairs;
    N.cells = reinterpret_cast<unsigned long long *>(S.cells.p);
    N.path = S.path.p;
    N.out = S.out.p;
    launch_align_index(*V.D, A, dev_chan, (int)cnt, st);
    N_TRY(hipGetLastError());
    launch_nearest(A, N, dev_chan, (int)cnt, st);
    N_TRY(hipGetLastError());
    // (the staged inputs share the landing place of the results: in stream order the upload has read it before the kernels run)
    N_TRY(hipMemcpyAsync(S.pin.p, S.out.p, out_ints * 4, hipMemcpyDeviceToHost, st));
    N_TRY(hipStreamSynchronize(st));
    for (size_t j = 0; j < cnt; ++j) {
      const size_t i = rnd[j], o = (size_t)pos[i];
      int code = WFST_OK;
      for (size_t q = 0; q < ns && code == WFST_OK; ++q) {
        const int32_t e = S.pin.p[(j * ns + q) * per + 4];
        if (e == kAlnCycle) code = capi_fail(WFST_E_DEVICE, "channel " + std::to_string(list[i]) + ": nearest: the lattice has an epsilon cycle");
        else if (e == kAlnTooLarge) code = capi_fail(WFST_E_CAPACITY, "channel " + std::to_string(list[i]) + ": nearest: the lattice outgrew the round's index");
        else if (e) code = capi_fail(WFST_E_DEVICE, "channel " + std::to_string(list[i]) + ": nearest: internal invariant violated on the device (a traced path that does not reproduce its cell)");
      }
      if (code != WFST_OK) {
        if (status) status[o] = code;
        continue;
      }
      for (size_t q = 0; q < ns; ++q) {
        const int32_t *r = S.pin.p + (j * ns + q) * per;
        if (!r[0]) continue;
        const size_t p = o * ns + q;
        const size_t len = (size_t)std::max(ref_len[p], 0), nh = std::min((size_t)r[10], hcap);
        if (found) found[p] = 1;
        if (n_arcs) n_arcs[p] = r[1];
        if (tot_score) memcpy(&tot_score[p], &r[2], 4);
        if (lm_score) memcpy(&lm_score[p], &r[3], 4);
        if (n_err) n_err[p] = r[5];
        if (n_cor) n_cor[p] = r[6];
        if (n_sub) n_sub[p] = r[7];
        if (n_ins) n_ins[p] = r[8];
        if (n_del) n_del[p] = r[9];
        if (n_hyp) n_hyp[p] = r[10];
        if (hyp_words) memcpy(hyp_words + p * hcap, r + kNearestHead, nh * 4);
        if (begin_frame) memcpy(begin_frame + p * hcap, r + kNearestHead + hcap, nh * 4);
        if (end_frame) memcpy(end_frame + p * hcap, r + kNearestHead + 2 * hcap, nh * 4);
        if (ref_hyp) memcpy(ref_hyp + p * cap, r + kNearestHead + 3 * hcap, len * 4);
        // the path has more words than the caller made room for: everything else of the answer stands, n_hyp is the room it takes
        if ((size_t)r[10] > hcap && code == WFST_OK)
          code = capi_fail(WFST_E_CAPACITY, "channel " + std::to_string(list[i]) + ": nearest: a path of " + std::to_string(r[10]) +
                                                " words, cap_hyp is " + std::to_string(cap_hyp));
      }
      if (status) status[o] = code;
    }
  }
  return WFST_OK;
}
