// inv_tu.h — body of an inverse-kernel translation unit (rollout_inv_*.hip): the inverse-dynamics kernel of inverse.h in the flavour
// whose macros the including file sets, exactly as step_tu.h does for the one-step kernel of that flavour (same MJPC_TU_NVT_LIST, same
// flavour switches: the pre-solve window is that flavour's own).  Full capacity only: no dense tier.
#include <hip/hip_runtime.h>
#include "inverse.h"

#define MJPC_CAT2(a, b) a##b
#define MJPC_CAT(a, b) MJPC_CAT2(a, b)

template <int NVT>
__global__ void __launch_bounds__(64 * MJPC_WAVES, 1) MJPC_CAT(inv_kernel_, MJPC_TU)(const InvParams I) {
  if ((int)blockIdx.x >= I.S.K.nlocal) return;
  inverse<NVT>((IP)__builtin_amdgcn_kernarg_segment_ptr());
}

typedef void (*InvFn)(const InvParams);
// the inverse kernel of this flavour for a model with nv dofs: the instantiation mjpc_pick_step_<flavour> picks for the step.
// engine.hip does not see InvParams (that needs core.h): it holds the kernel as an opaque pointer and launches it through
// mjpc_launch_inv_<flavour>
extern "C" const void *MJPC_CAT(mjpc_pick_inv_, MJPC_TU)(int nv) {
#define MJPC_PICK(N) if (nv == N) return (const void *)MJPC_CAT(inv_kernel_, MJPC_TU)<N>;
  MJPC_TU_NVT_LIST(MJPC_PICK)
#undef MJPC_PICK
  return (const void *)MJPC_CAT(inv_kernel_, MJPC_TU)<0>;
}
extern "C" void MJPC_CAT(mjpc_launch_inv_, MJPC_TU)(const void *fn, int n, size_t lds_bytes, hipStream_t stream, const KParams *K, const double *state_tab,
                                                    const double *ctrl_tab, const double *time_tab, const double *qacc_tab, int discrete,
                                                    double *qfrc_inverse_out, double *qfrc_constraint_out, double *residual_out, int *failure_out,
                                                    const int *late_tab) {
  InvParams I;
  I.S.K = *K; I.S.K.nlocal = n;
  I.S.state_tab = state_tab; I.S.ctrl_tab = ctrl_tab; I.S.time_tab = time_tab; I.S.next_state = nullptr; I.S.residual_out = residual_out;
  I.S.failure_out = failure_out; I.S.late_tab = late_tab;
  I.qacc_tab = qacc_tab; I.qfrc_inverse_out = qfrc_inverse_out; I.qfrc_constraint_out = qfrc_constraint_out; I.discrete = discrete;
  hipLaunchKernelGGL((InvFn)fn, dim3(n), dim3(64 * MJPC_WAVES), lds_bytes, stream, I);
}
