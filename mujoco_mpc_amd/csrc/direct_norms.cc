// direct_norms.cc — the device's norm functions (cost_derivatives.h: norm_grad_hess, norm_hess_entry, norm_dense) compiled for the host, for
// the host mirror of the direct optimiser's window cost (DirectCost::AssembleHost, planner.cc).  The device headers are compiled in their
// 1-lane MJPC_EMU mode, as the test emulations compile them, in this translation unit alone: their macros and helpers stay out of the
// host planner.  Built without contraction, like planner.cc.
#define MJPC_EMU 1
#include "cost_derivatives.h"

namespace mjpc_hip {
namespace device_norms {
double norm_grad_hess(double* g, double* hd, double* hs, const double* x, const double* prm, int n, int type) { return ::norm_grad_hess(g, hd, hs, x, prm, n, type); }
double norm_hess_entry(int type, const double* x, const double* g, const double* hs, int i, int j) { return ::norm_hess_entry(type, x, g, hs, i, j); }
int norm_dense(int type) { return ::norm_dense(type); }
}  // namespace device_norms
}  // namespace mjpc_hip
