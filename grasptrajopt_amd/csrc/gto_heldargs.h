// gto_heldargs.h — what gto_held_clearance and its device variant refuse before any device work (include/gto_solver.h),
// judged on the host.
//
// Host only: no kernel, no HIP call, nothing of the handle but its number of collision links.
// tests/held_args_main.cpp builds this header into a stand-alone program under AddressSanitizer and UBSan.
#pragma once
#include <cstdint>
#include <string>

#include "../../include/gto_solver.h"

namespace gto_heldargs {

// Every refusal of gto_held_clearance[_device], in the order shapes, attach_col, cutoff, link_mask, limits, null arrays.
// n_links: the handle's collision links (GTO_MAX_LINKS where there is no handle to ask).  Reads no array.  *empty: B = 0,
// which is GTO_OK without a launch whatever the arrays are.
inline int check_held_clearance_args(int n_links, int32_t B, int32_t Tp, const void* paths, const void* attach, int32_t attach_ld,
                                     int32_t attach_col, const void* held_points, int32_t P_max, const void* n_held,
                                     const void* base_pos, int32_t link_mask, double cutoff, const void* d2_out, std::string& why,
                                     bool* empty) {
  auto refuse = [&](int rc, const char* msg) {
    why = std::string("gto_held_clearance: ") + msg;
    return rc;
  };
  *empty = B == 0;
  if (!base_pos) return refuse(GTO_ERR_INVALID_ARG, "null base position");
  if (B < 0 || Tp < 1 || P_max < 1) return refuse(GTO_ERR_INVALID_ARG, "B >= 0, Tp >= 1 and P_max >= 1 are required");
  if (attach && (attach_col < 0 || attach_col >= attach_ld)) return refuse(GTO_ERR_INVALID_ARG, "attach_col must be in [0, attach_ld)");
  if (!(cutoff > 0.0)) return refuse(GTO_ERR_INVALID_ARG, "the cutoff must be > 0 (+inf: none)");  // (a NaN lands here)
  const uint32_t all = n_links >= 32 ? 0xffffffffu : ((1u << (n_links < 0 ? 0 : n_links)) - 1u);
  if ((uint32_t)link_mask & ~all) return refuse(GTO_ERR_INVALID_ARG, "a link_mask bit at or above n_links is set");
  if (B == 0) return GTO_OK;
  if (B > 65535 || P_max > 65535) return refuse(GTO_ERR_UNSUPPORTED, "at most 65535 plans of at most 65535 held points in one call");
  if (!paths || !held_points || !n_held || !d2_out) return refuse(GTO_ERR_INVALID_ARG, "null paths, held_points, n_held or d2_out");
  return GTO_OK;
}

}  // namespace gto_heldargs
