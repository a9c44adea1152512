// tests/emu/emu_inverse.cpp — TEST INFRASTRUCTURE ONLY.
// The inverse-dynamics kernel (mujoco_mpc_amd/csrc/inverse.h) and its finite-difference kernels (inverse_fd.h) in the 1-lane emulation
// mode: emu_inverse_batch plays the inverse kernel workgroup by workgroup, emu_inverse_fd the launch sequence of mjpc_hip_inverse_fd
// (engine.hip): assemble element by element, the inverse kernel over the table, the difference tile by tile through a NaN-poisoned
// staging tile.  emu_inv_step_batch and emu_inv_transition_fd are the one-step kernel and its derivatives compiled in this same unit
// (inverse.h included): what they return must be what tests/emu/emu_transition.cpp's build returns.
// Never loaded by the product.
#define MJPC_EMU 1
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../mujoco_mpc_amd/csrc/inverse.h"
#include "../../mujoco_mpc_amd/csrc/inverse_fd.h"
#include "../../mujoco_mpc_amd/csrc/host.h"

namespace {
struct Emu {
  PackedModel pm;
  InvParams I;
  int ds, nu, nr, ntr, nv;
  std::vector<double> states, actions, times, residual, costs, trace, knots, returns, lds;
  std::vector<int> failure, diag;
  bool init(const MjpcHipModel *m, const MjpcHipTask *t, const double *mocap) {
    if (!mjpc_host::build(pm, m, t, 1)) return false;
    memset(&I, 0, sizeof(I));
    KParams &K = I.S.K;
    K.M = mjpc_host::relocate(pm, pm.ib.data(), pm.db.data());
    K.L = pm.L;
    K.ibase = pm.ib.data(); K.dbase = pm.db.data(); K.cache_i = (int)pm.cache_i; K.cache_d = (int)pm.cache_d;
    ds = m->nq + m->nv + m->na; nu = m->nu; nr = t->num_residual; ntr = 3 * t->num_trace; nv = m->nv;
    states.assign(2 * ds, 0); actions.assign(2 * nu + 1, 0); times.assign(2, 0); residual.assign(2 * nr + 1, 0); costs.assign(2, 0);
    trace.assign(2 * ntr + 1, 0); knots.assign(nu + 1, 0); returns.assign(1, 0); failure.assign(1, 0); diag.assign(4, 0);
    K.mocap = mocap; K.P = 1; K.interp = 0; K.H = 2; K.N = 1; K.nlocal = 1;
    K.states = states.data(); K.actions = actions.data(); K.times = times.data(); K.residual = residual.data(); K.costs = costs.data();
    K.trace = trace.data(); K.knots = knots.data(); K.returns = returns.data(); K.failure = failure.data(); K.diag = diag.data();
    lds.assign((size_t)pm.L.total_doubles + 16, 0);
    I.S.late_tab = pm.late_blocks ? pm.ib.data() + pm.late_i0 : nullptr;      // as the engine hands it over
    return true;
  }
  void poison() {
    for (auto &v : lds) v = 0.0 / 0.0;      // catches reads of uninitialised LDS
    g_emu_lds = lds.data(); g_emu_r = 0;
  }
  // rows [0, n) of the tables, one "workgroup" after the other; cand_index() stays 0: the table pointers are moved to the row instead
  void inv(size_t n, const double *st, const double *ct, const double *tt, const double *at, int discrete, double *fi, double *fc, double *rs, int *fl) {
    for (size_t r = 0; r < n; r++) {
      poison();
      I.S.state_tab = st + r * ds; I.S.ctrl_tab = ct + r * nu; I.S.time_tab = tt + r; I.S.next_state = nullptr;
      I.S.residual_out = rs + r * nr; I.S.failure_out = fl + r;
      I.qacc_tab = at + r * nv; I.qfrc_inverse_out = fi + r * nv; I.qfrc_constraint_out = fc + r * nv; I.discrete = discrete;
      inverse<0>(&I);
    }
  }
  void step(size_t n, const double *st, const double *ct, const double *tt, double *ns, double *rs, int *fl) {
    for (size_t r = 0; r < n; r++) {
      poison();
      I.S.state_tab = st + r * ds; I.S.ctrl_tab = ct + r * nu; I.S.time_tab = tt + r;
      I.S.next_state = ns + r * ds; I.S.residual_out = rs + r * nr; I.S.failure_out = fl + r;
      transition<0>(&I.S);
    }
  }
};
thread_local std::string g_error;

std::vector<int> make_dofmap(const MjpcHipModel *m) {
  const int nv = m->nv;
  std::vector<int> dofmap(2 * nv + 2, -1);
  for (int j = 0; j < m->njnt; j++) {
    const int type = m->jnt_type[j], qa = m->jnt_qposadr[j], da = m->jnt_dofadr[j];
    if (type == 0) { for (int k = 0; k < 3; k++) { dofmap[2 * (da + k)] = qa + k; dofmap[2 * (da + k) + 1] = -1; dofmap[2 * (da + 3 + k)] = qa + 3; dofmap[2 * (da + 3 + k) + 1] = k; } }
    else if (type == 1) { for (int k = 0; k < 3; k++) { dofmap[2 * (da + k)] = qa; dofmap[2 * (da + k) + 1] = k; } }
    else { dofmap[2 * da] = qa; dofmap[2 * da + 1] = -1; }
  }
  return dofmap;
}
}  // namespace

extern "C" const char *emu_inverse_error(void) { return g_error.c_str(); }

// -1: the model / task was refused, -3: discrete on a model with a dense implicit integrator (emu_inverse_error says why)
extern "C" int emu_inverse_batch(const MjpcHipModel *m, const MjpcHipTask *t, int n, const double *states, const double *ctrl, const double *qacc,
                                 const double *time, const double *mocap, int discrete, double *qfrc_inverse, double *qfrc_constraint,
                                 double *residual, int *failure) {
  Emu E;
  if (!E.init(m, t, mocap)) { g_error = E.pm.error; return -1; }
  if (discrete && E.I.S.K.M.int_dense) { g_error = "discrete inverse dynamics is not built for the dense implicit integrators"; return -3; }
  E.inv((size_t)n, states, ctrl, time, qacc, discrete ? 1 : 0, qfrc_inverse, qfrc_constraint, residual, failure);
  return 0;
}

extern "C" int emu_inverse_fd(const MjpcHipModel *m, const MjpcHipTask *t, int T, const double *x, const double *u, const double *qacc,
                              const double *time, const double *mocap, int discrete, double eps, int centered, double *DfDq, double *DfDv,
                              double *DfDa, double *DsDq, double *DsDv, double *DsDa, int *failure, double *table_out) {
  Emu E;
  if (!E.init(m, t, mocap)) { g_error = E.pm.error; return -1; }
  if (discrete && E.I.S.K.M.int_dense) { g_error = "discrete inverse dynamics is not built for the dense implicit integrators"; return -3; }
  const int nq = m->nq, nv = m->nv, na = m->na, nu = m->nu, nr = t->num_residual, ds = nq + nv + na;
  const std::vector<int> dofmap = make_dofmap(m);
  InvFdArgs a;
  a.x = x; a.u = u; a.a = qacc; a.time = time; a.dofmap = dofmap.data();
  a.T = T; a.nq = nq; a.nv = nv; a.na = na; a.nu = nu; a.nr = nr; a.centered = centered ? 1 : 0;
  a.eps = eps; a.cs = cos(0.5 * eps); a.sn = sin(0.5 * eps);
  const size_t R = (size_t)T * ifd_slots(a);
  const double nan = 0.0 / 0.0;
  std::vector<double> st(R * ds, nan), ct(R * nu + 1, nan), tt(R, nan), at(R * nv, nan), fi(R * nv, nan), fc(R * nv, nan), rs(R * nr + 1, nan);
  std::vector<int> fl(R, -1);
  a.state_tab = st.data(); a.ctrl_tab = ct.data(); a.time_tab = tt.data(); a.qacc_tab = at.data(); a.qfrc = fi.data(); a.residual = rs.data(); a.fail = fl.data();
  a.DfDq = DfDq; a.DfDv = DfDv; a.DfDa = DfDa; a.DsDq = DsDq; a.DsDv = DsDv; a.DsDa = DsDa; a.failure = failure;
  for (size_t g = 0; g < R; g++) for (int i = 0; i < ifd_row_elements(a); i++) ifd_assemble(a, g, i);
  if (table_out)          // the nudged table, rows [state | ctrl | time | qacc], for the tests' own differences
    for (size_t g = 0; g < R; g++) {
      double *o = table_out + g * (size_t)ifd_row_elements(a);
      memcpy(o, &st[g * ds], sizeof(double) * ds); if (nu) memcpy(o + ds, &ct[g * nu], sizeof(double) * nu);
      o[ds + nu] = tt[g]; memcpy(o + ds + nu + 1, &at[g * nv], sizeof(double) * nv);
    }
  E.inv(R, st.data(), ct.data(), tt.data(), at.data(), discrete ? 1 : 0, fi.data(), fc.data(), rs.data(), fl.data());
  const int TILE = 16, no = nv + nr, nc = 3 * nv;
  for (int tk = 0; tk < T; tk++) {
    for (int o0 = 0; o0 < no; o0 += TILE)
      for (int c0 = 0; c0 < nc; c0 += TILE) {
        double tile[16][17];
        for (auto &row : tile) for (auto &v : row) v = nan;
        for (int th = 0; th < TILE * TILE; th++) {
          int oi = th % TILE, ci = th / TILE, o = o0 + oi, c = c0 + ci;
          if (o < no && c < nc && ifd_dest(a, tk, o, c)) tile[oi][ci] = ifd_entry(a, tk, o, c);
        }
        for (int th = 0; th < TILE * TILE; th++) {
          int ci = th % TILE, oi = th / TILE, o = o0 + oi, c = c0 + ci;
          if (o < no && c < nc) { double *d = ifd_dest(a, tk, o, c); if (d) *d = tile[oi][ci]; }
        }
      }
    failure[tk] = ifd_failure(a, tk, 0, 1);
  }
  return 0;
}

// the one-step kernel in this translation unit (late table handed over as the engine does)
extern "C" int emu_inv_step_batch(const MjpcHipModel *m, const MjpcHipTask *t, int n, const double *states, const double *ctrl, const double *time,
                                  const double *mocap, double *next_states, double *residual, int *failure) {
  Emu E;
  if (!E.init(m, t, mocap)) { g_error = E.pm.error; return -1; }
  E.step((size_t)n, states, ctrl, time, next_states, residual, failure);
  return 0;
}
// mjpc_hip_transition_fd's launch sequence in this translation unit: tests/emu/emu_transition.cpp's emu_transition_fd over this unit's step
extern "C" int emu_inv_transition_fd(const MjpcHipModel *m, const MjpcHipTask *t, int T, const double *x, const double *u, const double *time,
                                     const double *mocap, double eps, int centered, int last_is_terminal, double *A, double *B, double *C, double *D,
                                     int *failure) {
  Emu E;
  if (!E.init(m, t, mocap)) { g_error = E.pm.error; return -1; }
  const int nq = m->nq, nv = m->nv, na = m->na, nu = m->nu, nr = t->num_residual, ds = nq + nv + na, nd = 2 * nv + na;
  const std::vector<int> dofmap = make_dofmap(m);
  FdArgs a;
  a.x = x; a.u = u; a.time = time; a.dofmap = dofmap.data(); a.ctrllimited = E.I.S.K.M.actuator_ctrllimited; a.ctrlrange = E.I.S.K.M.actuator_ctrlrange;
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
  const int no = nd + nr, nc = nd + nu;
  for (int tk = 0; tk < T; tk++) {
    for (int o = 0; o < no; o++)
      for (int c = 0; c < nc; c++) { double *d = fd_dest(a, tk, o, c); if (d) *d = fd_entry(a, tk, o, c); }
    failure[tk] = fd_failure(a, tk, 0, 1);
  }
  return 0;
}
// the forward step's qfrc_constraint and qacc of one row, read from the LDS image the step leaves (as the solver stored them)
extern "C" int emu_inv_step_forces(const MjpcHipModel *m, const MjpcHipTask *t, const double *state, const double *ctrl, double time,
                                   const double *mocap, double *qfrc_constraint, double *qacc) {
  Emu E;
  if (!E.init(m, t, mocap)) { g_error = E.pm.error; return -1; }
  std::vector<double> ns(E.ds), rs(E.nr + 1);
  int fl = 0;
  E.step(1, state, ctrl, &time, ns.data(), rs.data(), &fl);
  Ctx c; ctx_init(c, &E.I.S.K, E.lds.data());
  for (int i = 0; i < E.nv; i++) { qfrc_constraint[i] = c.qfrc_constraint[i]; qacc[i] = c.qacc[i]; }
  return fl;
}
