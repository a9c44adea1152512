/* tests/emu/oracle_loop_shim.c — TEST INFRASTRUCTURE ONLY.
 * Field access to the oracle's OData for a closed loop driven from Python (tests/oracle_loop_lib.py): the test steps the oracle with
 * oracle_step / oracle_forward itself and reads and writes the state through these accessors, compiled against oracle/oracle.h so
 * that no struct layout is restated by hand. */
#include <string.h>
#include "../../oracle/oracle.h"

/* the start of a rollout as oracle_rollout has it: state, mocap, userdata and time in; warm start zeroed once; no force noise */
void shim_begin(const OModel *om, OData *d, const double *state, const double *mocap, const double *userdata, double time) {
  const MjpcHipModel *m = &om->m;
  for (int i = 0; i < m->nmocap; i++) {
    memcpy(d->mocap_pos + 3 * i, mocap + 7 * i, 3 * sizeof(double));
    memcpy(d->mocap_quat + 4 * i, mocap + 7 * i + 3, 4 * sizeof(double));
  }
  if (m->nuserdata && userdata) memcpy(d->userdata, userdata, sizeof(double) * m->nuserdata);
  memcpy(d->qpos, state, sizeof(double) * m->nq);
  memcpy(d->qvel, state + m->nq, sizeof(double) * m->nv);
  if (m->na > 0) memcpy(d->act, state + m->nq + m->nv, sizeof(double) * m->na);
  d->time = time;
  d->warning = 0;
  memset(d->qacc_warmstart, 0, sizeof(double) * m->nv);
  d->xfrc_on = 0;
  memset(d->xfrc_applied, 0, sizeof(double) * 6 * m->nbody);
}
void shim_set_ctrl(const OModel *om, OData *d, const double *ctrl) { memcpy(d->ctrl, ctrl, sizeof(double) * om->m.nu); }
void shim_get_state(const OModel *om, const OData *d, double *state) {
  const MjpcHipModel *m = &om->m;
  memcpy(state, d->qpos, sizeof(double) * m->nq);
  memcpy(state + m->nq, d->qvel, sizeof(double) * m->nv);
  if (m->na > 0) memcpy(state + m->nq + m->nv, d->act, sizeof(double) * m->na);
}
double shim_get_time(const OData *d) { return d->time; }
int shim_get_warning(const OData *d) { return d->warning; }
void shim_get_residual(const OModel *om, const OData *d, double *residual) { memcpy(residual, d->sensordata, sizeof(double) * om->t.num_residual); }
