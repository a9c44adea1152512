// rollout_inv_cached.hip — inverse-dynamics kernels (inverse.h) in the flavour of rollout_cached.hip: model tables from the LDS copy.
#define MJPC_TU cached
#define MJPC_TU_NVT_LIST(X) X(2) X(18) X(27)
#include "inv_tu.h"
