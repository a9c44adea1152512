// tests/emu/emu_riccati.cpp — TEST INFRASTRUCTURE ONLY.
// The iLQG backward-pass kernel (mujoco_mpc_amd/csrc/riccati.h) in the 1-lane emulation mode: emu_riccati plays rc_backward_kernel
// (engine.hip) as one thread that owns every entry of every phase, in the kernel's phase order, through a NaN-poisoned work image onto
// the caller's (NaN-poisoned) outputs, so that an entry read before it was computed, or never stored, shows up.  emu_boxqp plays
// rc_boxqp alone.  Never loaded by the product.
#define MJPC_EMU 1
#include <vector>
#include "../../mujoco_mpc_amd/csrc/riccati.h"

extern "C" int emu_riccati(int T, int nd, int nu, const double *A, const double *B, const double *cx, const double *cu, const double *cxx, const double *cxu,
                           const double *cuu, const double *actions, const double *limits, int reg_type, int action_limits, int max_iter, double reg_min,
                           double reg_max, double reg_factor, double *reg, double *k, double *K, double *Vx, double *Vxx, double *Qx, double *Qu, double *Qxx,
                           double *Qxu, double *Quu, double *dV, int *status) {
  if (T < 2 || nd < 1 || nu < 1) return -1;
  RcArgs a;
  a.A = A; a.B = B; a.cx = cx; a.cu = cu; a.cxx = cxx; a.cxu = cxu; a.cuu = cuu; a.actions = actions; a.limits = limits;
  a.T = T; a.nd = nd; a.nu = nu; a.reg_type = reg_type; a.action_limits = action_limits; a.max_iter = max_iter;
  a.reg_min = reg_min; a.reg_max = reg_max; a.reg_factor = reg_factor; a.reg = reg;
  a.k = k; a.K = K; a.Vx = Vx; a.Vxx = Vxx; a.Qx = Qx; a.Qu = Qu; a.Qxx = Qxx; a.Qxu = Qxu; a.Quu = Quu; a.dV = dV; a.status = status;
  const double nan = 0.0 / 0.0;
  std::vector<double> image(RC_WORK_DOUBLES(nd, nu), nan);
  a.scratch = image.data();
  rc_backward(a, rc_work(nd, nu, image.data()), 0, 1);
  return rc_fits(nd, nu);
}

extern "C" int emu_boxqp(int n, const double *H, const double *g, const double *lower, const double *upper, double *res, double *R, int *index) {
  const double nan = 0.0 / 0.0;
  std::vector<double> scr(4 * (size_t)n, nan);
  std::vector<int> mask(n, 0);
  return rc_boxqp(res, R, index, mask.data(), H, g, n, lower, upper, scr.data());
}
