// transition.h — ONE step of the engine for a batch of different states: workgroup r advances row r of a state table by one
// mj_step under row r of a control table and reports the next state, the residual evaluated inside that step and the warning
// bits.  This is what a finite-difference transition derivative is made of (mjpc/planners/model_derivatives.cc:45-165: one
// mjd_transitionFD per knot = 1 + (2nv+na+nu) independent steps); a rollout starts every candidate from the same K->state.
//
// Included by the rollout_step_*.hip translation units only (never by rollout_tu.inc or core.h: the rollout kernels do not
// change).  The phases are core.h's own, on core.h's step skeleton for t = 0, last = 0; with H = 2 and
// P = 1 in the kernel parameters they record into candidate rows [r][2][...] of the engine's row buffers exactly as the first step
// of a two-step plan does, so a step is bit for bit the first step of mjpc_hip_plan(N = 1, H = 2, P = 1, candidate_knots = ctrl).
#pragma once
#include "core.h"

// kernel parameter block of the step kernels: KParams first, so that the kernarg segment pointer is the KP the phases take
struct StepParams {
  KParams K;                  // H = 2, P = 1, interp = 0; nlocal = rows of this launch
  const double *state_tab;    // [nlocal][nq+nv+na]
  const double *ctrl_tab;     // [nlocal][nu]      the single knot of row r's policy
  const double *time_tab;     // [nlocal]
  double *next_state;         // [nlocal][nq+nv+na]
  double *residual_out;       // [nlocal][num_residual]
  int *failure_out;           // [nlocal]           MJPC_WARN_* bits, 0 = the step succeeded
  const int *late_tab;        // the task's late table (model.h) in device memory, or null: no late rows, no late phase
};
#ifdef MJPC_EMU
typedef const StepParams *SP;
#else
typedef const __attribute__((address_space(4))) StepParams *SP;
#endif
DEV const StepParams *sp_generic(SP s) { return (const StepParams *)kp_generic((KP)s); }
#include "late_rows.h"

// state, time and the one-knot policy come from row r of the tables
DEV_NOINLINE void ph_init_step(SP Sc) {
  Ctx c;
  const StepParams *S = sp_generic(Sc);
  const KParams *K = &S->K;
  ctx_init(c, K, lds_base());
  init_model_cache(K);
  const DevModel &M = *c.M;
  Rows R = out_rows(K);
  int nu = M.nu, r = cand_index();
  const double *x = S->state_tab + (size_t)r * R.ds;
  if (LANE == 0) c.knot_times[0] = 0.0;          // P = 1: spline_sample returns the knot's value at any time
  PFOR(k, nu) {
    double v = S->ctrl_tab[(size_t)r * nu + k];   // unclipped, as an explicit candidate policy is; ph_head clips
    c.knot_values[k] = v;
    K->knots[(size_t)r * nu + k] = v;
  }
  init_arrays(c, K, R, x);
  // a step that stops before its residual (bad state) reports NaN there, not what an earlier launch left
  PFOR(i, R.nr) S->residual_out[(size_t)r * R.nr + i] = __builtin_nan("");
  init_world(c, R, S->time_tab[r]);
  ctx_close(c);
}

// what ends a one-row evaluation (ph_finish_step here, ph_finish_inverse in inverse.h): the residual row, the warning bits to the
// caller's table and the engine's own, and the diagnostics (an evaluation without a solve reports 0 iterations)
DEV void finish_row(Ctx &c, const StepParams *S, int failure, int have_residual, bool solved) {
  const KParams *K = c.K;
  const int r = cand_index(), nr = c.M->task.num_residual;
  if (have_residual) PFOR(i, nr) S->residual_out[(size_t)r * nr + i] = c.residual[i];
  if (LANE == 0) {
    int w = failure ? (c.warning ? c.warning : 1) : 0;
    S->failure_out[r] = w;
    K->failure[r] = w;
    if (K->diag) { K->diag[4 * r] = solved ? c.misc[MISC_SUM_ITER] : 0; K->diag[4 * r + 1] = c.misc[MISC_MAX_NCON]; K->diag[4 * r + 2] = c.misc[MISC_MAX_NEFC]; K->diag[4 * r + 3] = c.warning; }
  }
}

// side wave, after the last barrier: the state in LDS (the integrated one, or the input when the step stopped before integration),
// then the row's tail
DEV_NOINLINE void ph_finish_step(SP Sc, int failure, int have_residual) {
  Ctx c; ctx_open(c, (KP)Sc, 1);
  const StepParams *S = sp_generic(Sc);
  const DevModel &M = *c.M;
  int r = cand_index(), nq = M.nq, nv = M.nv, ds = nq + nv + M.na;
  double *y = S->next_state + (size_t)r * ds;
  PFOR(i, nq) y[i] = c.qpos[i];
  PFOR(i, nv) y[nq + i] = c.qvel[i];
  if (M.na) PFOR(i, M.na) y[nq + nv + i] = C_ACT(c)[i];
  finish_row(c, S, failure, have_residual, true);
}

// the body of rollout<NVT> for t = 0, last = 0, once: no terminal forward, no checkpoint / retry, no return
template <int NVT>
DEV void transition(SP Sc) {
  KP Kc = (KP)Sc;
  const bool r0 = ROLE0, r1 = ROLE1;
  if (r0) ph_init_step(Sc);
  XBAR();
  const int *misc = (const int *)(lds_base() + Kc->L.ints) + Kc->L.i_misc;
  int failure = 0, have_residual = 0;
  const int t = 0, last = 0;
  do {
    if (r0) ph_head<NVT>(Kc, t, last);
    XBAR();
    if (uniform_i(misc[MISC_BAD_STATE])) { failure = 1; break; }
    presolve_window<NVT>(Kc, t, r0, r1);
    XBAR();
    solve_window<NVT>(Kc, t, last, r0);
    if (r1) {
      ph_residual_cost(Kc, t, last);
      ph_prefactor<NVT>(Kc);
    }
    XBAR();
    have_residual = 1;
    // late rows (accelerations, touch): the side wave, idle here, between the solve and the integration; uniform from the kernel arguments
    if (Sc->late_tab) {
      if (r1) ph_late_rows(Sc);
      XBAR();
    }
    if (uniform_i(misc[MISC_WARNING]) | uniform_i(misc[MISC_WARN_OTHERS])) { failure = 1; break; }
    if (r0) ph_integrate<NVT>(Kc, t);
  } while (0);
  XBAR();
  if (r1) ph_finish_step(Sc, failure, have_residual);
}
