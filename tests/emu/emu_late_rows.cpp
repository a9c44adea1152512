// tests/emu/emu_late_rows.cpp — TEST INFRASTRUCTURE ONLY.
// The one-step kernel (mujoco_mpc_amd/csrc/transition.h) with its late-row phase (late_rows.h) in the 1-lane emulation mode:
// emu_transition.cpp's player with the task's late table (host.h late_table, as mjpc_hip_create packs it behind the model buffers)
// handed to the kernel through StepParams.  Never loaded by the product.
#define MJPC_EMU 1
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../mujoco_mpc_amd/csrc/transition.h"
#include "../../mujoco_mpc_amd/csrc/host.h"

namespace {
struct Emu {
  PackedModel pm;
  StepParams S;
  int ds, nu, nr, ntr;
  std::vector<double> states, actions, times, residual, costs, trace, knots, returns, lds;
  std::vector<int> failure, diag;
  bool init(const MjpcHipModel *m, const MjpcHipTask *t, const double *mocap) {
    if (!mjpc_host::build(pm, m, t, 1)) return false;
    memset(&S, 0, sizeof(S));
    KParams &K = S.K;
    K.M = mjpc_host::relocate(pm, pm.ib.data(), pm.db.data());
    K.L = pm.L;
    K.ibase = pm.ib.data(); K.dbase = pm.db.data(); K.cache_i = (int)pm.cache_i; K.cache_d = (int)pm.cache_d;
    ds = m->nq + m->nv + m->na; nu = m->nu; nr = t->num_residual; ntr = 3 * t->num_trace;
    states.assign(2 * ds, 0); actions.assign(2 * nu + 1, 0); times.assign(2, 0); residual.assign(2 * nr + 1, 0); costs.assign(2, 0);
    trace.assign(2 * ntr + 1, 0); knots.assign(nu + 1, 0); returns.assign(1, 0); failure.assign(1, 0); diag.assign(4, 0);
    K.mocap = mocap; K.P = 1; K.interp = 0; K.H = 2; K.N = 1; K.nlocal = 1;
    K.states = states.data(); K.actions = actions.data(); K.times = times.data(); K.residual = residual.data(); K.costs = costs.data();
    K.trace = trace.data(); K.knots = knots.data(); K.returns = returns.data(); K.failure = failure.data(); K.diag = diag.data();
    lds.assign((size_t)pm.L.total_doubles + 16, 0);
    S.late_tab = pm.late_blocks ? pm.ib.data() + pm.late_i0 : nullptr;      // as step_rows (engine.hip) hands it over
    return true;
  }
  void step(size_t n, const double *st, const double *ct, const double *tt, double *ns, double *rs, int *fl) {
    for (size_t r = 0; r < n; r++) {
      for (auto &v : lds) v = 0.0 / 0.0;      // poison: catches reads of uninitialised LDS
      g_emu_lds = lds.data(); g_emu_r = 0;
      S.state_tab = st + r * ds; S.ctrl_tab = ct + r * nu; S.time_tab = tt + r;
      S.next_state = ns + r * ds; S.residual_out = rs + r * nr; S.failure_out = fl + r;
      transition<0>(&S);
    }
  }
};
thread_local std::string g_error;
}  // namespace

// -1: the model / task was refused (emu_late_error says why)
extern "C" int emu_late_step_batch(const MjpcHipModel *m, const MjpcHipTask *t, int n, const double *states, const double *ctrl, const double *time,
                                   const double *mocap, double *next_states, double *residual, int *failure) {
  Emu E;
  if (!E.init(m, t, mocap)) { g_error = E.pm.error; return -1; }
  E.step((size_t)n, states, ctrl, time, next_states, residual, failure);
  return 0;
}
// number of late blocks host.h finds in the task (0: the kernel gets a null table), -1: refused
extern "C" int emu_late_blocks(const MjpcHipModel *m, const MjpcHipTask *t) {
  PackedModel pm;
  if (!mjpc_host::build(pm, m, t, 1)) { g_error = pm.error; return -1; }
  return pm.late_blocks;
}
extern "C" const char *emu_late_error(void) { return g_error.c_str(); }
