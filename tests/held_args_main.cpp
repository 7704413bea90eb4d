// The host-side judgements of gto_held_clearance (grasptrajopt_amd/csrc/gto_heldargs.h) as a stand-alone host program, for a
// build under AddressSanitizer and UBSan: no HIP, no device.
//   held_args_main <n_links> <B> <Tp> <P_max> <attach 0|1> <attach_ld> <attach_col> <link_mask> <cutoff> <arrays 0|1>
// link_mask as an unsigned 32-bit word; arrays 0: paths, held_points, n_held and d2_out are null.
// prints "rc=<code> empty=<0|1> why=<message>".
#include <cstdio>
#include <cstdlib>
#include <string>

#include "gto_heldargs.h"

int main(int argc, char** argv) {
  if (argc != 11) return 2;
  std::string why;
  bool empty = false;
  double x[3] = {0.0, 0.0, 0.0};
  const void* arr = std::atoi(argv[10]) ? x : nullptr;
  const int rc = gto_heldargs::check_held_clearance_args(
      std::atoi(argv[1]), std::atoi(argv[2]), std::atoi(argv[3]), arr, std::atoi(argv[5]) ? x : nullptr, std::atoi(argv[6]),
      std::atoi(argv[7]), arr, std::atoi(argv[4]), arr, x, (int32_t)(uint32_t)std::strtoul(argv[8], nullptr, 10), std::atof(argv[9]),
      arr, why, &empty);
  std::printf("rc=%d empty=%d why=%s\n", rc, empty ? 1 : 0, why.c_str());
  return 0;
}
