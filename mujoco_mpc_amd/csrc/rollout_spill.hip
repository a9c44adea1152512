// rollout_spill.hip — rollout kernels for models whose per-candidate state does not fit 160 KiB of LDS: the blocks sized by
// nefcmax / nconmax (constraint rows, the efc_* vectors, contacts, the noslip table) live in a per-candidate slab in HBM
// (KParams::slab, host.h make_layout), the tree- and body-sized state stays in LDS.  Tables as in rollout_direct.hip.  The
// engine picks it only where every other flavour is refused (engine.hip); 27 and 33 have a dense tier whose overflow retries
// resume here with the same compile-time nv.
#define MJPC_TU spill
#define MJPC_NO_MODEL_CACHE 1
#define MJPC_HOT_CACHE 1
#define MJPC_SPILL 1
#define MJPC_MIN_BLOCKS 1
#define MJPC_TU_NVT_LIST(X) X(27) X(33)
#include "rollout_tu.inc"
