// feedback_tu.h — body of a feedback-rollout translation unit (rollout_fb_*.hip): the rollout kernel of feedback.h in the flavour whose
// macros the including file sets, exactly as rollout_tu.inc does for the open-loop kernel of that flavour (same MJPC_TU_NVT_LIST, same
// flavour switches).  Full capacity only: no dense tier, no retry launch.
#include <hip/hip_runtime.h>
#include "feedback.h"

#define MJPC_CAT2(a, b) a##b
#define MJPC_CAT(a, b) MJPC_CAT2(a, b)

template <int NVT>
__global__ void __launch_bounds__(64 * MJPC_WAVES, 1) MJPC_CAT(fb_kernel_, MJPC_TU)(const FeedbackParams F) {
  if ((int)blockIdx.x >= F.K.nlocal) return;
  rollout_feedback<NVT>((FP)__builtin_amdgcn_kernarg_segment_ptr());
}

typedef void (*FbFn)(const FeedbackParams);
// the feedback kernel of this flavour for a model with nv dofs: the instantiation mjpc_pick_rollout_<flavour> picks for the open-loop
// rollout.  engine.hip does not see FeedbackParams (that needs core.h): it holds the kernel as an opaque pointer and launches it
// through mjpc_launch_fb_<flavour>
extern "C" const void *MJPC_CAT(mjpc_pick_fb_, MJPC_TU)(int nv) {
#define MJPC_PICK(N) if (nv == N) return (const void *)MJPC_CAT(fb_kernel_, MJPC_TU)<N>;
  MJPC_TU_NVT_LIST(MJPC_PICK)
#undef MJPC_PICK
  return (const void *)MJPC_CAT(fb_kernel_, MJPC_TU)<0>;
}
extern "C" void MJPC_CAT(mjpc_launch_fb_, MJPC_TU)(const void *fn, int n, size_t lds_bytes, hipStream_t stream, const KParams *K, const double *xbar,
                                                   const double *ubar, const double *kbar, const double *Kbar, const double *alpha, const double *scale) {
  FeedbackParams F;
  F.K = *K; F.K.nlocal = n;
  F.xbar = xbar; F.ubar = ubar; F.kbar = kbar; F.Kbar = Kbar; F.alpha = alpha; F.scale = scale;
  hipLaunchKernelGGL((FbFn)fn, dim3(n), dim3(64 * MJPC_WAVES), lds_bytes, stream, F);
}
