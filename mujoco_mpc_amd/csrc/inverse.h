// inverse.h — ONE inverse-dynamics evaluation of the engine for a batch of different configurations: workgroup r takes row r of a
// state, control, time and ACCELERATION table and reports the generalized force that produces that acceleration, the constraint
// force, the residual and the warning bits.  This is what the reference's direct trajectory optimiser is made of
// (mjpc/direct/direct.cc:1545-1576: mj_inverse at every configuration of a window; :1717-1756: mjd_inverseFD = 1 + 3 nv of them).
//
// Included by the rollout_inv_*.hip translation units only.  A sibling of transition.h: the same init, head and pre-solve window
// (core.h's step skeleton), and then NO solver: behind the window the owner wave evaluates the force law of the step's
// constraint rows at jar = J a - aref once (ph_inverse), the side wave the residual; the late rows then read the given
// acceleration and the inverse efc_force.  No ph_solve, ph_noslip, ph_prefactor or ph_integrate, and the helper waves never enter ph_solve_helper: its loops wait for job words only solve_constraints posts.
//
//   qfrc_constraint = J^T f(J a - aref)                                  constraint_update<DIMT, true>(c, 0, jar), solver.h
//   qfrc_inverse    = M a + qfrc_bias - qfrc_passive - qfrc_constraint   (MuJoCo's meaning: actuator forces are not subtracted)
// evaluated as (M a - qfrc_smooth) + qfrc_actuator - qfrc_constraint: ph_smooth keeps one sum qfrc_smooth = passive - bias +
// actuator, and the actuator part is rebuilt here from c.actuator_force and the moments.
//
// discrete != 0 (mjENBL_INVDISCRETE, what direct/ uses): the given acceleration is (v' - v) / h of the integrator, which solves
// A a_d = qfrc_smooth + qfrc_constraint = M a_c, so a_c = M^-1 (A a_d) first, with A = M + h diag(damping) (+ the idrv entries of
// implicitfast, prefactor_body's rule for clamped actuator forces), built as a product (M a from mat_rows_times) and solved with M's own
// factor, which is intact here because nothing prefactors.  Models with int_dense are refused by the host for discrete != 0.
#pragma once
#include "transition.h"

// kernel parameter block of the inverse kernels: StepParams first (next_state stays null), so that ph_head .. ph_late_rows take it
struct InvParams {
  StepParams S;
  const double *qacc_tab;       // [nlocal][nv]
  double *qfrc_inverse_out;     // [nlocal][nv]
  double *qfrc_constraint_out;  // [nlocal][nv]
  int discrete;
};
#ifdef MJPC_EMU
typedef const InvParams *IP;
#else
typedef const __attribute__((address_space(4))) InvParams *IP;
#endif
DEV const InvParams *ip_generic(IP s) { return (const InvParams *)kp_generic((KP)s); }

// sibling of ph_init_step that also loads the row's acceleration (into qacc_ws: nothing warm-starts here) and poisons the row's outputs
DEV_NOINLINE void ph_init_inverse(IP Ic) {
  ph_init_step((SP)Ic);
  const InvParams *I = ip_generic(Ic);
  Ctx c; ctx_open(c, (KP)Ic);
  const int nv = c.M->nv, r = cand_index();
  PFOR(i, nv) {
    c.qacc_ws[i] = I->qacc_tab[(size_t)r * nv + i];
    // a row that stops before its forces (bad state) reports NaN there, not what an earlier launch left
    I->qfrc_inverse_out[(size_t)r * nv + i] = __builtin_nan("");
    I->qfrc_constraint_out[(size_t)r * nv + i] = __builtin_nan("");
  }
  ctx_close(c);
}

// moment^T actuator_force of dof d's joint and tendon transmissions (velocity_stage's gather)
DEV double inv_act_gather(Ctx &c, int d) {
  double act = 0;
  for (int q = MI(dact_adr)[d]; q < MI(dact_adr)[d + 1]; q++) { int e = MI(dact_e)[q]; act += MD(act_coef)[e] * c.actuator_force[MI(act_of)[e]]; }
  return act;
}

// qfrc_actuator into out[nv]: the actuator terms of qfrc_smooth in the order velocity_stage / ph_smooth_extras add them (gather, the
// joint-level clamp, site transmissions, site transmissions against a reference site)
DEV void inv_qfrc_actuator(Ctx &c, double *out) {
  const DevModel &M = *c.M;
  const int nv = M.nv;
  PFOR(d, nv) out[d] = inv_act_gather(c, d);
  SYNC();
  if (M.nactfrc > 0) {
    PFOR(k, M.nactfrc) { int dd = MI(actfrc_dof)[k]; out[dd] = d_clip(out[dd], MD(actfrc_range)[2 * k], MD(actfrc_range)[2 * k + 1]); }
    SYNC();
  }
  if (M.nsiteact > 0) {
    PFOR(d, nv) {
      double acc = out[d];
      const double *cd = c.cdof + 6 * d;
      for (int k = 0; k < M.nsiteact; k++) {
        int a = MI(sact_i)[3 * k], s = MI(sact_i)[3 * k + 1], b = MI(sact_i)[3 * k + 2];
        if (!((MDM()[b] >> d) & 1ull)) continue;
        double f[3], tq[3], off[3], t[3];
        d_mulmatvec3(f, c.xmat + 9 * b, MD(sact_g) + 6 * k); d_mulmatvec3(tq, c.xmat + 9 * b, MD(sact_g) + 6 * k + 3);
        d_sub3(off, c.site_xpos + 3 * s, c.subtree_com + 3 * MIH(body_rootid)[b]);
        d_cross(t, cd, off);
        acc += c.actuator_force[a] * ((cd[3] + t[0]) * f[0] + (cd[4] + t[1]) * f[1] + (cd[5] + t[2]) * f[2] + cd[0] * tq[0] + cd[1] * tq[1] + cd[2] * tq[2]);
      }
      out[d] = acc;
    }
    SYNC();
  }
  if (M.nrsact > 0) {
    PFOR(d, nv) {
      double acc = out[d];
      for (int k = 0; k < M.nrsact; k++) {
        const int *ri = MI(rsact_i) + 7 * k;
        double w[3];
        d_mulmatvec3(w, c.xmat + 9 * ri[4], MD(rsact_g) + 3 * k);
        acc += rs_moment(c, ri, w, d) * c.actuator_force[ri[0]];
      }
      out[d] = acc;
    }
    SYNC();
  }
}

// owner wave, behind the pre-solve window: the continuous acceleration (c.qacc), the force law at it (efc_force, efc_state: where
// ph_late_rows reads them), qfrc_constraint and qfrc_inverse.  Scratch: Ma, Mgrad, grad, efc_jar, sgl - the solver's own, which
// nothing else touches between the two barriers
template <int NVT>
DEV_NOINLINE void ph_inverse(IP Ic) {
  LATE_FP_STRICT        // the sums written here are rounded one by one, in the emulation and on the device alike
  Ctx c; ctx_open(c, (KP)Ic);
  const InvParams *I = ip_generic(Ic);
  const DevModel &M = *c.M;
  const int nv = M.nv, nvp = M.nvp, r = cand_index();
  c.solver_iter = 0;
  {
    int b = 0;
    PFOR(i, nv) { double v = c.qacc_ws[i]; if (!(v - v == 0)) b = 1; }       // NaN or infinite
    if (wave_or_i(b)) c.warning |= WARN_BADQACC;
  }
  if (I->discrete && M.any_damping) {
    // a_c = M^-1 (A a_d), A the matrix ph_integrate solves with (prefactor_body)
    const double h = M.timestep;
    mat_rows_times<NVT>(c, c.qacc_ws, c.Ma, c.efc_jar);
    SYNC();
    PFOR(i, nv) c.Mgrad[i] = c.Ma[i] + (h * MD(dof_damping)[i]) * c.qacc_ws[i];
    if (M.nidrv) {
      SYNC();
      if (LANE == 0)
        for (int k = 0; k < M.nidrv; k++) {
          int i = MI(idrv_e)[3 * k], j = MI(idrv_e)[3 * k + 1], a = MI(idrv_e)[3 * k + 2];
          if (a >= 0 && MI(actuator_forcelimited)[a]) {
            double f = c.actuator_force[a];
            if (f <= MD(actuator_forcerange)[2 * a] || f >= MD(actuator_forcerange)[2 * a + 1]) continue;
          }
          double v = h * MD(idrv_c)[k];
          c.Mgrad[i] += v * c.qacc_ws[j];
          if (i != j) c.Mgrad[j] += v * c.qacc_ws[i];
        }
    }
    SYNC();
    chol_solve<NVT>(c.qL, c.Linv, c.Mgrad, nv, nvp, M.tree_ok);       // M's own factor (crb_and_factor)
    SYNC();
    PFOR(i, nv) c.qacc[i] = c.Mgrad[i];
  } else {
    PFOR(i, nv) c.qacc[i] = c.qacc_ws[i];
  }
  SYNC();
  mat_rows_times<NVT>(c, c.qacc, c.Ma, c.efc_jar);
  PFOR(q, c.nefc) c.efc_jar[q] -= c.efc_aref[q];
  SYNC();
  if (c.nefc > 0) {
    if (M.maxdim <= 3) constraint_update<3, true>(c, 0, c.efc_jar); else constraint_update<6, true>(c, 0, c.efc_jar);
    SYNC();
  }
  inv_qfrc_actuator(c, c.grad);
  // J^T f, rows ascending: a friction-loss row is the unit vector of its dof, a limit row holds its one entry
  PFOR(i, nv) {
    double s = 0;
    const int nfr = M.nfric;
    for (int q = 0; q < c.nefc; q++) {
      const double f = c.efc_force[q];
      if (q < nfr) { if (c.efc_dof[q] == i) s += f; }
      else if (q < c.nsingle) { if (c.efc_dof[q] == i) s += c.efc_J[q * nvp + i] * f; }
      else s += c.efc_J[q * nvp + i] * f;
    }
    c.qfrc_constraint[i] = s;
    const double inv = ((c.Ma[i] - c.qfrc_smooth[i]) + c.grad[i]) - s;
    I->qfrc_constraint_out[(size_t)r * nv + i] = s;
    I->qfrc_inverse_out[(size_t)r * nv + i] = inv;
  }
  if (LANE == 0) { if (c.ncon > c.misc[MISC_MAX_NCON]) c.misc[MISC_MAX_NCON] = c.ncon; if (c.nefc > c.misc[MISC_MAX_NEFC]) c.misc[MISC_MAX_NEFC] = c.nefc; }
  ctx_close(c);
}

// side wave, after the last barrier: the row's tail alone (the forces went out in ph_inverse)
DEV_NOINLINE void ph_finish_inverse(IP Ic, int failure, int have_residual) {
  Ctx c; ctx_open(c, (KP)Ic, 1);
  finish_row(c, sp_generic((SP)Ic), failure, have_residual, false);
}

// transition<NVT> without its solve, prefactor and integration
template <int NVT>
DEV void inverse(IP Ic) {
  KP Kc = (KP)Ic;
  SP Sc = (SP)Ic;
  const bool r0 = ROLE0, r1 = ROLE1;
  if (r0) ph_init_inverse(Ic);
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
    // (the helper waves go straight to the next barrier: no job loop)
    if (r0) ph_inverse<NVT>(Ic);
    if (r1) ph_residual_cost(Kc, t, last);
    XBAR();
    have_residual = 1;
    if (Sc->late_tab) {
      if (r1) ph_late_rows(Sc);
      XBAR();
    }
    if (uniform_i(misc[MISC_WARNING]) | uniform_i(misc[MISC_WARN_OTHERS])) failure = 1;
  } while (0);
  XBAR();
  if (r1) ph_finish_inverse(Ic, failure, have_residual);
}
