// The C-ABI test double of tests/pool_double (a channel counts and checksums its rows; overlapping calls on one decoder abort) plus
// the partial-words halves, for GpuChannelPool's partial request kind under ThreadSanitizer.  A channel's partial words derive from
// the channel and its frame count alone -- {channel + 1, 8 rows + 1, 8 rows + 2, ...}, 1 + rows / 3 of them, rows / 6 stable -- so
// that a driver can tell whether every request was answered with its own channel's words at its own frame count.  The double
// polices the halves' contract: a second _enqueue while one is outstanding is counted (and refused, as the library refuses it).
#include "../pool_double/fake_wfstdec.cc"

namespace {
struct Partial {
  std::vector<int32_t> list;
  int cap = 0;
  long long ready_ns = 0;
  std::atomic<long long> enqueues{0}, overlapping{0}, requests{0};
} g_pt;   // (the driver has one decoder)
}  // namespace

extern "C" {
int wfst_decoder_partial_enqueue(wfst_decoder *d, const int32_t *ch, int32_t n, int32_t cap_words) {
  Guard gd(d);
  if (!g_pt.list.empty()) { g_pt.overlapping++; return fail(WFST_E_STATE, "a partial request is outstanding"); }
  if (n <= 0 || cap_words <= 0) return fail(WFST_E_ARG, "bad argument");
  for (int i = 0; i < n; ++i) {
    if (ch[i] < 0 || ch[i] >= d->n) return fail(WFST_E_ARG, "channel out of range");
    if (d->state[ch[i]] == 0) return fail(WFST_E_STATE, "partial words before InitDecoding");
    if (d->state[ch[i]] == 2) return fail(WFST_E_STATE, "partial words after FinalizeDecoding");
  }
  g_pt.enqueues++;
  g_pt.requests += n;
  g_pt.list.assign(ch, ch + n);
  g_pt.cap = cap_words;
  g_pt.ready_ns = now_ns() + 90000;   // "on the device" for 90 us
  return WFST_OK;
}
int wfst_decoder_partial_ready(wfst_decoder *d) {
  Guard gd(d);
  if (g_pt.list.empty()) return fail(WFST_E_STATE, "nothing outstanding");
  return now_ns() >= g_pt.ready_ns ? 1 : 0;
}
int wfst_decoder_partial_fetch(wfst_decoder *d, int32_t *words, int32_t *n_words, int32_t *n_stable, int32_t *stable_frame) {
  while (now_ns() < g_pt.ready_ns) std::this_thread::sleep_for(std::chrono::microseconds(10));
  Guard gd(d);
  if (g_pt.list.empty()) return fail(WFST_E_STATE, "nothing outstanding");
  std::vector<int32_t> list;
  list.swap(g_pt.list);
  int rc = WFST_OK;
  for (size_t i = 0; i < list.size(); ++i) {
    const int c = list[i], rows = d->rows[c], nw = rows > 0 ? 1 + rows / 3 : 0;
    if (n_words) n_words[i] = nw;
    if (n_stable) n_stable[i] = rows / 6;
    if (stable_frame) stable_frame[i] = rows / 2;
    if (nw > g_pt.cap) rc = fail(WFST_E_CAPACITY, "cap_words");
    for (int k = 0; k < std::min(nw, g_pt.cap) && words; ++k) words[i * (size_t)g_pt.cap + k] = k == 0 ? c + 1 : 8 * rows + k;
  }
  return rc;
}
int wfst_decoder_get_partial(wfst_decoder *d, const int32_t *ch, int32_t n, int32_t cap_words, int32_t *words, int32_t *n_words, int32_t *n_stable,
                             int32_t *stable_frame) {
  const int rc = wfst_decoder_partial_enqueue(d, ch, n, cap_words);
  if (rc != WFST_OK) return rc;
  return wfst_decoder_partial_fetch(d, words, n_words, n_stable, stable_frame);
}
long long fake_partial_count(int k) { return k == 0 ? g_pt.enqueues.load() : k == 1 ? g_pt.overlapping.load() : g_pt.requests.load(); }
}
