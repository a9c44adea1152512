// step_tu.h — body of a step-kernel translation unit (rollout_step_*.hip): the one-step kernel of transition.h in the flavour whose
// macros the including file sets, exactly as rollout_tu.inc does for the rollout kernel of that flavour (same MJPC_TU_NVT_LIST, same
// flavour switches: a step is then bit for bit the first step of that flavour's rollout).  Full capacity only: no dense tier.
#include <hip/hip_runtime.h>
#include "transition.h"

#define MJPC_CAT2(a, b) a##b
#define MJPC_CAT(a, b) MJPC_CAT2(a, b)

template <int NVT>
__global__ void __launch_bounds__(64 * MJPC_WAVES, 1) MJPC_CAT(step_kernel_, MJPC_TU)(const StepParams S) {
  if ((int)blockIdx.x >= S.K.nlocal) return;
  transition<NVT>((SP)__builtin_amdgcn_kernarg_segment_ptr());
}

typedef void (*StepFn)(const StepParams);
// the step kernel of this flavour for a model with nv dofs: the instantiation mjpc_pick_rollout_<flavour> picks for the rollout.
// engine.hip does not see StepParams (that needs core.h): it holds the kernel as an opaque pointer and launches it through
// mjpc_launch_step_<flavour>
extern "C" const void *MJPC_CAT(mjpc_pick_step_, MJPC_TU)(int nv) {
#define MJPC_PICK(N) if (nv == N) return (const void *)MJPC_CAT(step_kernel_, MJPC_TU)<N>;
  MJPC_TU_NVT_LIST(MJPC_PICK)
#undef MJPC_PICK
  return (const void *)MJPC_CAT(step_kernel_, MJPC_TU)<0>;
}
extern "C" void MJPC_CAT(mjpc_launch_step_, MJPC_TU)(const void *fn, int n, size_t lds_bytes, hipStream_t stream, const KParams *K, const double *state_tab,
                                                     const double *ctrl_tab, const double *time_tab, double *next_state, double *residual_out, int *failure_out,
                                                     const int *late_tab) {
  StepParams S;
  S.K = *K; S.K.nlocal = n;
  S.state_tab = state_tab; S.ctrl_tab = ctrl_tab; S.time_tab = time_tab; S.next_state = next_state; S.residual_out = residual_out; S.failure_out = failure_out; S.late_tab = late_tab;
  hipLaunchKernelGGL((StepFn)fn, dim3(n), dim3(64 * MJPC_WAVES), lds_bytes, stream, S);
}
