// The round cutter of the word queries (cut_round, asr-decoder_amd/csrc/wfst_capi_align.h) against a restatement of its rule and as
// properties, on hand-made cases and on random ones; run under AddressSanitizer + UBSan by tests/test_host_rounds.py.  Calls nothing
// of HIP: the header is only included.  Prints "rounds ok <vectors> <rounds>" and returns 0, or says what broke and returns 1.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "wfst_capi_align.h"

namespace {
typedef std::vector<std::vector<size_t> > Rounds;

// the rule, restated: skip what does not run; close a round before the first entry that would take a NON-EMPTY round over the budget
Rounds restated(const std::vector<int64_t> &need, const std::vector<char> &run, int64_t budget) {
  Rounds out;
  int64_t sum = 0;
  for (size_t i = 0; i < need.size(); ++i) {
    if (!run[i]) continue;
    if (out.empty() || sum + need[i] > budget) { out.push_back(std::vector<size_t>()); sum = 0; }
    out.back().push_back(i);
    sum += need[i];
  }
  return out;
}

long n_vectors = 0, n_rounds = 0;

bool check(const char *what, const std::vector<int64_t> &need, const std::vector<char> &run, int64_t budget) {
  ++n_vectors;
  // the driver's loop (word_query_run), with a bound on its turns: every turn but the last takes an entry
  Rounds got;
  size_t turns = 0;
  for (size_t first = 0; first < need.size();) {
    if (++turns > need.size() + 1) { printf("%s: does not terminate\n", what); return false; }
    const wfst::RoundCut c = wfst::cut_round(need, run, first, budget);
    if (c.next < first || c.next > need.size()) { printf("%s: next %zu from %zu of %zu\n", what, c.next, first, need.size()); return false; }
    first = c.next;
    if (c.members.empty()) {
      if (c.cells != 0) { printf("%s: an empty round of %lld cells\n", what, (long long)c.cells); return false; }
      for (size_t i = first; i < need.size(); ++i)
        if (run[i]) { printf("%s: stopped before runnable entry %zu\n", what, i); return false; }
      break;
    }
    int64_t sum = 0;
    for (size_t i : c.members) sum += need[i];
    if (sum != c.cells) { printf("%s: a round says %lld cells, its members need %lld\n", what, (long long)c.cells, (long long)sum); return false; }
    if (sum > budget && c.members.size() != 1) { printf("%s: %zu members over the budget\n", what, c.members.size()); return false; }
    got.push_back(c.members);
  }
  n_rounds += (long)got.size();
  // every runnable index in exactly one round, in order; the others in none; no round empty
  size_t at = 0;
  for (const auto &r : got) {
    if (r.empty()) { printf("%s: an empty round\n", what); return false; }
    for (size_t i : r) {
      while (at < need.size() && !run[at]) ++at;
      if (i != at) { printf("%s: entry %zu where %zu was due\n", what, i, at); return false; }
      ++at;
    }
  }
  while (at < need.size() && !run[at]) ++at;
  if (at != need.size()) { printf("%s: runnable entry %zu in no round\n", what, at); return false; }
  if (got != restated(need, run, budget)) { printf("%s: not the restated rule's rounds\n", what); return false; }
  return true;
}

bool check_rounds(const char *what, const std::vector<int64_t> &need, const std::vector<char> &run, int64_t budget, const Rounds &want) {
  if (!check(what, need, run, budget)) return false;
  if (restated(need, run, budget) != want) { printf("%s: not the rounds written down for it\n", what); return false; }
  return true;
}

uint32_t rng_state = 12345;
uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
}  // namespace

int main() {
  bool ok = true;
  const std::vector<char> all3(3, 1), all5(5, 1);
  ok &= check_rounds("empty input", {}, {}, 10, {});
  ok &= check_rounds("nothing runnable", {4, 5, 6}, {0, 0, 0}, 10, {});
  ok &= check_rounds("one entry over budget alone", {25}, {1}, 10, {{0}});
  ok &= check_rounds("an over-budget entry between small ones", {3, 4, 25, 2, 1}, all5, 10, {{0, 1}, {2}, {3, 4}});
  ok &= check_rounds("an over-budget entry first", {25, 2, 1}, all3, 10, {{0}, {1, 2}});
  ok &= check_rounds("exactly the budget", {3, 3, 4, 5, 5}, all5, 10, {{0, 1, 2}, {3, 4}});
  ok &= check_rounds("one cell over", {3, 3, 5, 5, 5}, all5, 10, {{0, 1}, {2, 3}, {4}});
  ok &= check_rounds("zero-cell entries", {0, 0, 0}, all3, 10, {{0, 1, 2}});
  ok &= check_rounds("zero-cell entries, no budget to speak of", {0, 0, 0}, all3, 0, {{0, 1, 2}});
  ok &= check_rounds("zero-cell entries behind a full round", {10, 0, 0, 1}, {1, 1, 1, 1}, 10, {{0, 1, 2}, {3}});
  ok &= check_rounds("skipped entries inside and between rounds", {6, 9, 4, 9, 6, 9}, {1, 0, 1, 0, 1, 0}, 10, {{0, 2}, {4}});
  ok &= check_rounds("an all-skipped tail", {6, 6, 9, 9, 9}, {1, 1, 0, 0, 0}, 10, {{0}, {1}});
  ok &= check_rounds("an all-skipped head", {9, 9, 6, 3}, {0, 0, 1, 1}, 10, {{2, 3}});
  // random vectors: sizes 0..24, needs of 0..40 cells (a fifth of them 0), a quarter not runnable, budgets from 1 to the total
  for (int t = 0; t < 400 && ok; ++t) {
    const size_t n = rnd() % 25;
    std::vector<int64_t> need(n);
    std::vector<char> run(n);
    int64_t total = 0;
    for (size_t i = 0; i < n; ++i) {
      need[i] = rnd() % 5 ? (int64_t)(rnd() % 40 + 1) : 0;
      run[i] = rnd() % 4 ? 1 : 0;
      total += need[i];
    }
    const int64_t budgets[] = {1, total / 7 + 1, total / 3 + 1, total > 1 ? total - 1 : 1, total > 0 ? total : 1,
                               1 + (int64_t)(rnd() % (uint32_t)(total > 0 ? total : 1))};
    for (int64_t b : budgets) ok &= check("random", need, run, b);
  }
  if (!ok) return 1;
  printf("rounds ok %ld %ld\n", n_vectors, n_rounds);
  return 0;
}
