// tests/host/direct_main.cpp — TEST INFRASTRUCTURE ONLY.
// mjpc_hip::DirectCost::AssembleHost (csrc/planner.cc) in a stand-alone program that the test builds with the address and undefined-behaviour
// sanitizers: every input array is a vector of exactly the documented size, so a read or write past a block shows up.  Windows of
// T = 3, 4, 6 on 5 dofs, sensors from residual row 2 of 12 (a dense L2 norm among them), a masked pair, the end settings both ways.
#include <cmath>
#include <cstdio>
#include <vector>
#include "../../include/mjpc_hip_planner.h"

static unsigned long long g_state = 12345;
static double rnd() { g_state = g_state * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(g_state >> 11) / 9007199254740992.0 - 0.5; }
static std::vector<double> fill(size_t n) { std::vector<double> v(n); for (double& x : v) x = rnd(); return v; }

int main() {
  const int nv = 5, nr = 12;
  const int dim[3] = {2, 4, 3}, stage[3] = {0, 1, 2}, norm[3] = {0, 2, 6};
  const double prm[6] = {0, 0, 0.1, 0, 0.2, 0}, noise[3] = {1.0, 2.0, 0.5};
  for (int T : {3, 4, 6})
    for (int last = 0; last < 2; last++) {
      mjpc_hip::DirectCost dc;
      dc.Allocate(nv, nr, T);
      dc.SetSensors(2, 3, dim, stage, norm, prm, noise);
      dc.timestep = 0.01;
      dc.settings.last_step_position_sensors = last; dc.settings.last_step_velocity_sensors = last;
      std::vector<int> mask((size_t)T * 3, 1); mask[4] = 0;
      dc.SetMask(mask.data(), T);
      const size_t n = nv, ns = 9, Tz = T;
      const std::vector<double> rs = fill(Tz * ns), rf = fill(Tz * n), Dfq = fill(Tz * n * n), Dfv = fill(Tz * n * n), Dfa = fill(Tz * n * n);
      const std::vector<double> Dsq = fill(Tz * nr * n), Dsv = fill(Tz * nr * n), Dsa = fill(Tz * nr * n), V0 = fill(Tz * n * n), V1 = fill(Tz * n * n);
      if (!dc.AssembleHost(T, rs.data(), rf.data(), Dfq.data(), Dfv.data(), Dfa.data(), Dsq.data(), Dsv.data(), Dsa.data(), V0.data(), V1.data())) return 1;
      if (dc.gradient.size() != Tz * n || dc.hessian_band.size() != Tz * n * 3 * n) return 2;
      for (double v : dc.hessian_band) if (!std::isfinite(v)) return 3;
      for (double v : dc.gradient) if (!std::isfinite(v)) return 4;
      if (!(dc.cost[0] > 0) || dc.cost[0] != dc.cost[1] + dc.cost[2]) return 5;
      // the diagonal of a Gauss-Newton Hessian with positive weights is not negative
      for (size_t R = 0; R < Tz * n; R++) if (dc.hessian_band[R * 3 * n + 3 * n - 1] < 0) return 6;
    }
  std::printf("direct ok\n");
  return 0;
}
