// wfst_decoder_get_nbest_words: the n-best TEXT of a channel list, live and finalized channels mixed, one launch per stage
// (nbest_words_kernel, wfst_nbest.hip).  A translation unit of its own -- see wfst_capi_nbwords.h.
#include "wfst_capi_nbwords.h"

#include <algorithm>
#include <cstring>
#include <string>

#include "wfst_capi_words.h"   // capi_fail

using namespace wfst;

#define N_TRY(expr)                                                                                   \
  do {                                                                                                \
    hipError_t e_ = (expr);                                                                           \
    if (e_ != hipSuccess) return capi_fail(WFST_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

int wfst_decoder_get_nbest_words(wfst_decoder *d, const int32_t *channels, int32_t n, int32_t n_paths, int32_t use_final_probs,
                                 const wfst_lm *old_lm, const wfst_lm *new_lm, int32_t cap_words, int32_t *status, int32_t *got_paths,
                                 int32_t *n_words, int32_t *words, float *tot_score, float *lm_score, float *path_tot) {
  int32_t slots = 0;
  NbWordsState *S = nullptr;
  hipStream_t st = nullptr;
  int rc = nbw_begin(d, channels, n, n_paths, old_lm, new_lm, cap_words, &slots, &S, &st);
  if (rc != WFST_OK) return rc;
  const size_t np = (size_t)n_paths, cap = (size_t)cap_words, per = (size_t)kNbWordsHead + cap;
  if (status) std::fill(status, status + n, (int32_t)WFST_OK);
  if (got_paths) std::fill(got_paths, got_paths + n, 0);
  if (n_words) std::fill(n_words, n_words + (size_t)n * np, 0);
  if (words) std::fill(words, words + (size_t)n * np * cap, 0);
  if (tot_score) std::fill(tot_score, tot_score + (size_t)n * np, 0.0f);
  if (lm_score) std::fill(lm_score, lm_score + (size_t)n * np, 0.0f);
  if (path_tot) std::fill(path_tot, path_tot + (size_t)n * np, 0.0f);
  // the channels with a lattice to look at (a finalized channel without final-probs has none: GetRawLattice, base-inl.h:879-884),
  // by their position in the caller's list
  std::vector<int32_t> pos;
  for (int i = 0; i < n; ++i)
    if (nbw_channel_state(d, channels[i]) == 1 || use_final_probs) pos.push_back(i);
  std::vector<int32_t> list, st_round;
  for (size_t first = 0; first < pos.size(); first += (size_t)slots) {
    const int32_t cnt = (int32_t)std::min(pos.size() - first, (size_t)slots);
    list.resize((size_t)cnt);
    for (int i = 0; i < cnt; ++i) list[(size_t)i] = channels[pos[first + (size_t)i]];
    NbPathsDev P = {};
    rc = nbw_round(d, list, use_final_probs, old_lm, new_lm, n_paths, &st_round, &P);
    if (rc != WFST_OK) return rc;
    const size_t ints = (size_t)cnt * 4 + (size_t)cnt * np * per;
    if (S->out.n < ints) {
      N_TRY(hipStreamSynchronize(st));
      N_TRY(S->out.alloc(ints));
    }
    N_TRY(S->pin.reserve(ints));
    launch_nbest_words(P, cnt, cap_words, S->out.p, st);
    N_TRY(hipGetLastError());
    N_TRY(hipMemcpyAsync(S->pin.p, S->out.p, ints * 4, hipMemcpyDeviceToHost, st));   // only text crosses the link, in one copy
    N_TRY(hipStreamSynchronize(st));
    const int32_t *head = S->pin.p, *recs = S->pin.p + (size_t)cnt * 4;
    for (int i = 0; i < cnt; ++i) {
      const size_t o = (size_t)pos[first + (size_t)i];
      const std::string who = "channel " + std::to_string(list[(size_t)i]) + ": ";
      int32_t code = st_round[(size_t)i];
      const int32_t *h = head + (size_t)4 * i;
      if (code == WFST_OK && h[2] == 3) code = capi_fail(WFST_E_DEVICE, who + "n-best: the lattice has a cycle");
      if (code == WFST_OK && h[2] == 1)
        code = capi_fail(WFST_E_CAPACITY, who + "n-best: " + std::to_string(n_paths) + " paths outgrew the batch's path workspace (ask channel by channel: wfst_decoder_get_nbest_paths)");
      int32_t found = (code == WFST_OK && h[2] == 0) ? std::min(std::max(h[0], 0), n_paths) : 0;
      for (int k = 0; k < found && code == WFST_OK; ++k)
        if (recs[((size_t)i * np + (size_t)k) * per] < 0) code = capi_fail(WFST_E_DEVICE, who + "n-best: a path through an arc outside the lattice");
      if (code != WFST_OK) found = 0;
      bool too_long = false;
      for (int k = 0; k < found; ++k) {
        const int32_t *r = recs + ((size_t)i * np + (size_t)k) * per;
        const size_t q = o * np + (size_t)k;
        if (n_words) n_words[q] = r[0];
        if (tot_score) memcpy(&tot_score[q], &r[1], 4);
        if (lm_score) memcpy(&lm_score[q], &r[2], 4);
        if (path_tot) memcpy(&path_tot[q], &r[3], 4);
        if (words) memcpy(words + q * cap, r + kNbWordsHead, (size_t)std::min<int32_t>(r[0], cap_words) * 4);
        if (r[0] > cap_words) too_long = true;
      }
      if (too_long) code = capi_fail(WFST_E_CAPACITY, who + "more words than cap_words; n_words holds the needed size");
      if (status) status[o] = code;
      if (got_paths) got_paths[o] = found;
    }
  }
  return WFST_OK;
}

int wfst_decoder_get_determinizer_slots(wfst_decoder *d, int32_t *slots, int64_t *bytes_per_slot) { return nbw_det_slots(d, slots, bytes_per_slot); }
