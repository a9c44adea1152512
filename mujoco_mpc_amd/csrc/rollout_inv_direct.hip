// rollout_inv_direct.hip — inverse-dynamics kernels (inverse.h) in the flavour of rollout_direct.hip: tables from HBM / L2, hot prefix in LDS.
#define MJPC_TU direct
#define MJPC_NO_MODEL_CACHE 1
#define MJPC_HOT_CACHE 1
#define MJPC_TU_NVT_LIST(X) X(33)
#include "inv_tu.h"
