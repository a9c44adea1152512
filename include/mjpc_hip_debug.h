/* mjpc_hip_debug.h — diagnostics knobs of libmjpc_hip.so.  NOT part of the drop-in ABI (include/mjpc_hip.h): used by this
 * repository's tests and measurement scripts to force code paths that the engine otherwise picks by itself.  Nothing here is read
 * from the environment; a knob only exists after an explicit call, is process-wide, and is looked at while an engine is created
 * (mjpc_hip_create / mjpc_hip_multi_create).
 *
 *   name              value            effect
 *   "tier"            "A" | "B"        never / always launch the dense capacity tier (two candidates per CU) first
 *   "dense_tier_cap"  "rows,contacts"  capacity of the dense tier (a tiny one makes most candidates take the checkpointed retry)
 *   "no_model_cache"  any              read the model tables from HBM / L2 instead of the per-workgroup LDS copy
 *   "dense_factor"    any              dense elimination order for every factorisation (ignore the elimination tree)
 *   "fault_inject"    "sync"           one helper wave of candidate 1 stays silent in step 2 (exercises the hand-shake timeout)
 *   "spill"           "all"            full-capacity launch on the spill flavour (rollout_spill.hip) with every eligible block - rows,
 *                                      efc_* vectors, contacts, noslip table - in the per-candidate HBM slab, even for a model that fits
 *
 * value == NULL removes the knob. */
#ifndef MJPC_HIP_DEBUG_H_
#define MJPC_HIP_DEBUG_H_
#ifdef __cplusplus
extern "C" {
#endif
void mjpc_hip_debug_set(const char *name, const char *value);
/* Capacity of the engine's dense tier (rows, contacts; 0, 0 without one); *hot = 1 when it is the variant with the hot tables in
   LDS (rollout_dense2h.hip).  Diagnostics / tests only. */
void mjpc_hip_debug_dense_capacity(struct MjpcHipEngine *e, int *nefc, int *ncon, int *hot);
/* 1 when the engine's full-capacity launch runs the spill flavour (per-candidate state partly in an HBM slab, rollout_spill.hip);
   *slab_bytes = the slab per candidate (a multiple of 256; 0 when the flavour's compile-time-nv layout fits LDS as it is). */
int mjpc_hip_debug_spill(struct MjpcHipEngine *e, int *slab_bytes);
/* Host only, no GPU needed: the (LDS bytes, slab bytes per candidate) of the full-capacity flavour mjpc_hip_create would pick for
   this model under the knobs set now.  1 when that is the spill flavour, 0 when not, < 0 when the model is refused
   (mjpc_hip_last_error tells why). */
struct MjpcHipModel; struct MjpcHipTask;
int mjpc_hip_debug_spill_layout(const struct MjpcHipModel *model, const struct MjpcHipTask *task, int *lds_bytes, int *slab_bytes);
#ifdef __cplusplus
}
#endif
#endif /* MJPC_HIP_DEBUG_H_ */
