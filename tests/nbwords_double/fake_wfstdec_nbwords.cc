// A TEST DOUBLE of the C ABI for GpuChannelPool's kNbestWords request under ThreadSanitizer: the pool's double (a channel counts and
// checksums its rows; overlapping calls on one decoder abort) plus wfst_decoder_get_nbest_words -- per listed channel min(n_paths, 2)
// paths whose words name the channel, the frames it holds and what was asked, so that a driver can tell that every thread got ITS
// channel's answer to ITS question.  It counts its calls and the channels they listed.
#include "../pool_double/fake_wfstdec.cc"

static long long g_nbw_calls = 0, g_nbw_channels = 0;

extern "C" {
int wfst_decoder_get_nbest_words(wfst_decoder *d, const int32_t *ch, int32_t n, int32_t n_paths, int32_t use_final, const wfst_lm *old_lm,
                                 const wfst_lm *new_lm, int32_t cap_words, int32_t *status, int32_t *got, int32_t *n_words, int32_t *words,
                                 float *tot, float *lm, float *path_tot) {
  Guard g(d);
  if (n_paths < 1 || n_paths > 64 || cap_words <= 0 || (old_lm == nullptr) != (new_lm == nullptr)) return fail(WFST_E_ARG, "bad argument");
  for (int i = 0; i < n; ++i)
    if (ch[i] < 0 || ch[i] >= d->n || d->state[ch[i]] == 0) return fail(WFST_E_STATE, "GetNbestTxt before InitDecoding");
  g_nbw_calls++;
  g_nbw_channels += n;
  std::this_thread::sleep_for(std::chrono::microseconds(50));   // (synchronous: the batcher stands here while requests queue up)
  for (int i = 0; i < n; ++i) {
    const int c = ch[i];
    const int k = (d->state[c] == 2 && !use_final) ? 0 : std::min(n_paths, 2);
    status[i] = WFST_OK;
    got[i] = k;
    for (int p = 0; p < k; ++p) {
      const size_t q = (size_t)i * n_paths + p;
      n_words[q] = 4;
      const int32_t w[4] = {c + 1, d->rows[c], n_paths * 2 + (use_final ? 1 : 0), old_lm ? 7 : 5};
      for (int x = 0; x < 4 && x < cap_words; ++x) words[q * cap_words + x] = w[x];
      tot[q] = (float)d->sum[c] + p;
      lm[q] = (float)p;
      if (path_tot) path_tot[q] = tot[q];
    }
  }
  return WFST_OK;
}
long long fake_nbw_calls(int what) { return what ? g_nbw_channels : g_nbw_calls; }
}
