// tests/emu/emu_gradient.cpp — TEST INFRASTRUCTURE ONLY.
// The Sample-Gradient device functions (mujoco_mpc_amd/csrc/gradient.h) in the 1-lane emulation mode: the batch assembly element by
// element, and the gradient reduction with the launch structure of sg_gradient_kernel (engine.hip) played back in one thread -
// every producer group of a tile, then the consumer lanes of the tile before it, two staging tiles.  The tiles are poisoned with
// NaN before every k-block, so a product the consumer adds without a producer having staged it shows up.  Never loaded by the
// product.
#define MJPC_EMU 1
#include <vector>
#include "../../mujoco_mpc_amd/csrc/gradient.h"

extern "C" void emu_sg_assemble(const double *nominal, const double *noise_std, const double *eps, const double *ctrlrange, double *cand,
                                double *hist, long long hist_stride, int offset, int nlocal, int PN, int nu, int nominal_index,
                                int first_explicit) {
  SgAssembleArgs a{nominal, noise_std, eps, ctrlrange, cand, hist, hist_stride, offset, nlocal, PN, nu, nominal_index, first_explicit};
  for (size_t idx = 0; idx < (size_t)nlocal * PN; idx++) sg_assemble(a, idx);
}

extern "C" void emu_sg_gradient(const double *hist, long long hist_stride, const int *slot, const double *scale, int n, int PN,
                                double *gradient) {
  SgGradArgs a{hist, hist_stride, slot, scale, n, PN, gradient};
  const int ntile = (n + SG_T - 1) / SG_T;
  std::vector<double> buf[2] = {std::vector<double>(SG_T * SG_KT), std::vector<double>(SG_T * SG_KT)};
  for (int kb = 0; kb * SG_KT < PN; kb++) {
    for (auto &b : buf) for (auto &v : b) v = 0.0 / 0.0;
    double acc[SG_KT];
    for (int kl = 0; kl < SG_KT; kl++) acc[kl] = 0.0;
    for (int t = 0; t <= ntile; t++) {
      if (t < ntile)
        for (int g = 0; g < SG_PROD; g++)
          for (int kl = 0; kl < SG_KT; kl++) sg_produce(a, kb, t, g, kl, buf[t & 1].data());
      if (t > 0)
        for (int kl = 0; kl < SG_KT; kl++) acc[kl] = sg_consume(a, t - 1, kl, buf[(t - 1) & 1].data(), acc[kl]);
    }
    for (int kl = 0; kl < SG_KT; kl++)
      if (kb * SG_KT + kl < PN) gradient[kb * SG_KT + kl] = acc[kl];
  }
}

extern "C" void emu_sg_shape(int *out) { out[0] = SG_KT; out[1] = SG_U; out[2] = SG_PROD; out[3] = SG_T; }
