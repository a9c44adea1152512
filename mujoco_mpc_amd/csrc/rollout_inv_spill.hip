// rollout_inv_spill.hip — inverse-dynamics kernels (inverse.h) in the flavour of rollout_spill.hip: row- and contact-sized blocks in the
// per-candidate HBM slab.
#define MJPC_TU spill
#define MJPC_NO_MODEL_CACHE 1
#define MJPC_HOT_CACHE 1
#define MJPC_SPILL 1
#define MJPC_TU_NVT_LIST(X) X(27) X(33)
#include "inv_tu.h"
