// tests/emu/emu_transition.cpp — TEST INFRASTRUCTURE ONLY.
// The one-step kernel (mujoco_mpc_amd/csrc/transition.h) and the finite-difference kernels (transition_fd.h) in the 1-lane emulation
// mode: emu_step_batch plays the step kernel workgroup by workgroup, emu_transition_fd the launch sequence of mjpc_hip_transition_fd
// (engine.hip): assemble element by element, the step kernel over the table, the difference tile by tile through a NaN-poisoned
// staging tile, so that an entry stored without having been computed shows up.  Never loaded by the product.
#define MJPC_EMU 1
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../mujoco_mpc_amd/csrc/transition.h"
#include "../../mujoco_mpc_amd/csrc/transition_fd.h"
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
    return true;
  }
  // rows [0, n) of the tables, one "workgroup" after the other.  cand_index() stays 0 (the row buffers hold one candidate): the
  // table pointers are moved to the row instead
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
}  // namespace

extern "C" int emu_step_batch(const MjpcHipModel *m, const MjpcHipTask *t, int n, const double *states, const double *ctrl, const double *time,
                              const double *mocap, double *next_states, double *residual, int *failure) {
  Emu E;
  if (!E.init(m, t, mocap)) return -1;
  E.step((size_t)n, states, ctrl, time, next_states, residual, failure);
  return 0;
}

extern "C" int emu_transition_fd(const MjpcHipModel *m, const MjpcHipTask *t, int T, const double *x, const double *u, const double *time,
                                 const double *mocap, double eps, int centered, int last_is_terminal, double *A, double *B, double *C, double *D,
                                 int *failure) {
  Emu E;
  if (!E.init(m, t, mocap)) return -1;
  const int nq = m->nq, nv = m->nv, na = m->na, nu = m->nu, nr = t->num_residual, ds = nq + nv + na, nd = 2 * nv + na;
  std::vector<int> dofmap(2 * nv + 2, -1);
  for (int j = 0; j < m->njnt; j++) {
    const int type = m->jnt_type[j], qa = m->jnt_qposadr[j], da = m->jnt_dofadr[j];
    if (type == 0) { for (int k = 0; k < 3; k++) { dofmap[2 * (da + k)] = qa + k; dofmap[2 * (da + k) + 1] = -1; dofmap[2 * (da + 3 + k)] = qa + 3; dofmap[2 * (da + 3 + k) + 1] = k; } }
    else if (type == 1) { for (int k = 0; k < 3; k++) { dofmap[2 * (da + k)] = qa; dofmap[2 * (da + k) + 1] = k; } }
    else { dofmap[2 * da] = qa; dofmap[2 * da + 1] = -1; }
  }
  FdArgs a;
  a.x = x; a.u = u; a.time = time; a.dofmap = dofmap.data(); a.ctrllimited = E.S.K.M.actuator_ctrllimited; a.ctrlrange = E.S.K.M.actuator_ctrlrange;
  a.T = T; a.nq = nq; a.nv = nv; a.na = na; a.nu = nu; a.nr = nr; a.centered = centered ? 1 : 0; a.last_is_terminal = last_is_terminal ? 1 : 0;
  a.eps = eps; a.cs = cos(0.5 * eps); a.sn = sin(0.5 * eps);
  const size_t R = (size_t)T * fd_slots(a);
  const double nan = 0.0 / 0.0;
  std::vector<double> st(R * ds, nan), ct(R * nu + 1, nan), tt(R, nan), ns(R * ds, nan), rs(R * nr + 1, nan);
  std::vector<int> fl(R, -1);
  a.state_tab = st.data(); a.ctrl_tab = ct.data(); a.time_tab = tt.data(); a.next_state = ns.data(); a.residual = rs.data(); a.fail = fl.data();
  a.A = A; a.B = B; a.C = C; a.D = D; a.failure = failure;
  for (size_t g = 0; g < R; g++) for (int i = 0; i < ds + nu + 1; i++) fd_assemble(a, g, i);
  E.step(R, st.data(), ct.data(), tt.data(), ns.data(), rs.data(), fl.data());
  const int TILE = 16, no = nd + nr, nc = nd + nu;
  for (int tk = 0; tk < T; tk++) {
    for (int o0 = 0; o0 < no; o0 += TILE)
      for (int c0 = 0; c0 < nc; c0 += TILE) {
        double tile[16][17];
        for (auto &row : tile) for (auto &v : row) v = nan;
        for (int th = 0; th < TILE * TILE; th++) {
          int oi = th % TILE, ci = th / TILE, o = o0 + oi, c = c0 + ci;
          if (o < no && c < nc && fd_dest(a, tk, o, c)) tile[oi][ci] = fd_entry(a, tk, o, c);
        }
        for (int th = 0; th < TILE * TILE; th++) {
          int ci = th % TILE, oi = th / TILE, o = o0 + oi, c = c0 + ci;
          if (o < no && c < nc) { double *d = fd_dest(a, tk, o, c); if (d) *d = tile[oi][ci]; }
        }
      }
    failure[tk] = fd_failure(a, tk, 0, 1);
  }
  return 0;
}
