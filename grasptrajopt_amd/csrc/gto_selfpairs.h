// gto_selfpairs.h — the link-pair mask of the self-clearance check (gto_set_self_pairs, gto_self_clearance:
// include/gto_solver.h), judged on the host.
//
// Host only: no kernel, no HIP call, nothing of the handle.  tests/self_pairs_main.cpp builds this header into a stand-alone
// program under AddressSanitizer and UBSan.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/gto_solver.h"

namespace gto_selfpairs {

// "every pair of distinct links": what a handle uses until gto_set_self_pairs gives it a mask.  rows [GTO_MAX_LINKS].
inline void all_distinct_pairs(int n_links, uint32_t* rows) {
  const uint32_t all = n_links >= 32 ? 0xffffffffu : ((1u << n_links) - 1u);
  for (int a = 0; a < GTO_MAX_LINKS; ++a) rows[a] = a < n_links ? (all & ~(1u << a)) : 0u;
}

// Every refusal of gto_set_self_pairs, in the order bits at or above n_links, diagonal, symmetry.  rows [n_links]; bit b of
// rows[a] enables the pair (a, b).  Reads the rows only.
inline int check_self_pairs(int n_links, const int32_t* rows, std::string& why) {
  auto refuse = [&](const char* msg) {
    why = msg;
    return GTO_ERR_INVALID_ARG;
  };
  const uint32_t all = n_links >= 32 ? 0xffffffffu : ((1u << n_links) - 1u);
  for (int a = 0; a < n_links; ++a)
    if ((uint32_t)rows[a] & ~all) return refuse("gto_set_self_pairs: a bit at or above n_links is set");
  for (int a = 0; a < n_links; ++a)
    if (((uint32_t)rows[a] >> a) & 1u) return refuse("gto_set_self_pairs: a link is paired with itself");
  for (int a = 0; a < n_links; ++a)
    for (int b = a + 1; b < n_links; ++b)
      if ((((uint32_t)rows[a] >> b) & 1u) != (((uint32_t)rows[b] >> a) & 1u)) return refuse("gto_set_self_pairs: the mask is not symmetric");
  return GTO_OK;
}

// What gto_self_clearance and its device variant check before any device work, the handle aside.
inline int check_self_clearance_args(int32_t B, int32_t Tp, double cutoff, std::string& why) {
  if (B < 0 || Tp < 1) {
    why = "gto_self_clearance: B >= 0 and Tp >= 1 are required";
    return GTO_ERR_INVALID_ARG;
  }
  if (!(cutoff > 0.0)) {  // (a NaN lands here)
    why = "gto_self_clearance: the cutoff must be > 0 (+inf: none)";
    return GTO_ERR_INVALID_ARG;
  }
  return GTO_OK;
}

}  // namespace gto_selfpairs
