// The inertial passes of gto_robot.h (check_inertials, fill_inertials) as a stand-alone host program, for a build under
// AddressSanitizer and UBSan (tests/test_dynamics_cpu.py).  Reads records from stdin: "n_frames has_gravity" and then
// n_frames masses, 3 n_frames centre-of-mass entries, 6 n_frames inertia entries and, if has_gravity, 3 more numbers;
// the arrays are heap blocks of exactly those lengths.  Prints per record the return code, the message, and on success the
// table's mass sum, the inertia entries' sum and gravity.
#include <cstdio>
#include <string>
#include <vector>

#include "gto_robot.h"

int main() {
  int F, has_g;
  while (std::scanf("%d %d", &F, &has_g) == 2) {
    std::vector<double> mass(F), com(3 * F), inertia(6 * F), g(3);
    for (double& v : mass) if (std::scanf("%lf", &v) != 1) return 2;
    for (double& v : com) if (std::scanf("%lf", &v) != 1) return 2;
    for (double& v : inertia) if (std::scanf("%lf", &v) != 1) return 2;
    if (has_g)
      for (double& v : g) if (std::scanf("%lf", &v) != 1) return 2;
    std::string why;
    const int rc = gto_robot::check_inertials(F, mass.data(), com.data(), inertia.data(), has_g ? g.data() : nullptr, why);
    if (rc) {
      std::printf("rc=%d why=%s\n", rc, why.c_str());
      continue;
    }
    DynDev dyn;
    gto_robot::fill_inertials(F, mass.data(), com.data(), inertia.data(), has_g ? g.data() : nullptr, dyn);
    double sm = 0, si = 0, sc = 0;
    for (int f = 0; f < GTO_MAX_FRAMES; ++f) {
      sm += dyn.mass[f];
      for (int k = 0; k < 3; ++k) sc += dyn.com[f][k];
      for (int k = 0; k < 6; ++k) si += dyn.inertia[f][k];
    }
    std::printf("rc=0 mass=%.17g com=%.17g inertia=%.17g gravity=%.17g %.17g %.17g\n", sm, sc, si, dyn.gravity[0], dyn.gravity[1],
                dyn.gravity[2]);
  }
  return 0;
}
