// The seam between the library and wfst_capi_altern.cc (wfst_decoder_word_alternatives): the entry point that launches
// slot_mass_kernel and slot_none_kernel (wfst_altern.hip) behind wfst_decoder_word_confidence's own launches is a translation unit of
// its own, as wfst_capi_posterior.cc and wfst_capi_seqpost.cc are.  It sees a decoder through wfst_capi_align.h's view; what comes back
// lies in the posterior workspace wfst_capi_posterior.h lays out, what stays on the device in AlignState::alt.  Host only.
#ifndef WFST_CAPI_ALTERN_H_
#define WFST_CAPI_ALTERN_H_

#include "wfst_capi_posterior.h"

namespace wfst {

// the slots of a pair's (cell, word) table in the workspace: a power of two above the arcs of the round's largest lattice.  The distinct
// keys of a sequence are at most the lattice's word-carrying arcs; the host knows the arcs (align_emit's sizes), their word-carrying
// share only after one more readback, so the arcs bound it.
inline int64_t altern_tab_slots(int64_t na_cap) {
  int64_t t = 2;
  while (t <= na_cap) t <<= 1;
  return t;
}
// doubles of AlignState::alt a round takes: acost [pairs][ns_cap], early [pairs][cap_words], tab_key and tab_mass [pairs][tab_slots]
inline size_t altern_stay_doubles(size_t pairs, size_t ns_cap, size_t cap_words, size_t tab_slots) {
  return pairs * (ns_cap + cap_words + 2 * tab_slots);
}

}  // namespace wfst
#endif
