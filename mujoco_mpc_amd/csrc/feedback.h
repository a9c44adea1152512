// feedback.h — rollouts under a FEEDBACK policy: candidate i applies at step t < H-1
//   u = clamp( (ubar[t] + alpha_i * kbar[t]) + s_i * ( Kbar[t] * StateDiff(xbar[t], x_t) ), ctrlrange )
// where x_t is the candidate's own state at that step.  Both rollouts of iLQG are this form (mjpc/planners/ilqg/planner.cc:618-712):
// ActionRollouts has s_i = 1 and alpha_i = the line-search step, FeedbackRollouts alpha_i = 0 and s_i = the step.  The per-step tables
// ubar / kbar / xbar / Kbar [H] are shared by the whole batch (read-only, the same lines for every workgroup: served from L2); a
// time-interpolated policy is resampled into them once per call (feedback_resample.h), never inside the rollout.
//
// Included by the rollout_fb_*.hip translation units only (never by rollout_tu.inc or core.h: the open-loop kernels do not change).
// ph_init_feedback is ph_init without a spline policy, ph_head_feedback<NVT> is ph_head with the policy block replaced; every other
// phase is core.h's own, on core.h's step skeleton.  Full capacity only: no dense tier, no checkpoint.
//
// Bit rule: the arithmetic is that of the host's iLQGPolicy::Action / StateDiff (planner.cc) - each row of Kbar * dx starts
// at 0.0 and takes ascending index with one rounded product and one rounded add, alpha * kbar is one product and one add (mju_addScl),
// the scaled add likewise (mju_addToScl), the clamp comes last and only there.
#pragma once
#include "core.h"
#include "atan2_cr.h"
#include "feedback_resample.h"      // FB_DX_CAPACITY, shared with the host side

// kernel parameter block of the feedback rollout kernels: KParams first, so that the kernarg segment pointer is the KP the phases take
struct FeedbackParams {
  KParams K;                  // P = 0 (no knots), cand_knots / noise unused
  const double *xbar;         // [H][nq+nv+na]   null: the feedback term is skipped (not multiplied by zero)
  const double *ubar;         // [H][nu]
  const double *kbar;         // [H][nu]         null: the alpha term is skipped
  const double *Kbar;         // [H][nu][2nv+na]
  const double *alpha;        // [nlocal]        action step of candidate r
  const double *scale;        // [nlocal]        feedback scale of candidate r
};
#ifdef MJPC_EMU
typedef const FeedbackParams *FP;
#else
typedef const __attribute__((address_space(4))) FeedbackParams *FP;
#endif
DEV const FeedbackParams *fp_generic(FP f) { return (const FeedbackParams *)kp_generic((KP)f); }

// body-frame rotation vector of qa^-1 qb (mju_subQuat), spelled as the host's StateDiff spells it: separately rounded products in the
// host's association, IEEE sqrt and divide (dmath.h's d_subquat normalises with a reciprocal multiply: not the same bits), and the
// angle from atan2_cr (atan2_cr.h), which host and device share: a library atan2 is not the same function on both
DEV void fb_quat_diff(double *res, const double *qa, const double *qb) {
  const double d0 = add_rn(add_rn(add_rn(mul_rn(qa[0], qb[0]), mul_rn(qa[1], qb[1])), mul_rn(qa[2], qb[2])), mul_rn(qa[3], qb[3]));
  const double d1 = add_rn(add_rn(add_rn(mul_rn(qa[0], qb[1]), -mul_rn(qa[1], qb[0])), -mul_rn(qa[2], qb[3])), mul_rn(qa[3], qb[2]));
  const double d2 = add_rn(add_rn(add_rn(mul_rn(qa[0], qb[2]), mul_rn(qa[1], qb[3])), -mul_rn(qa[2], qb[0])), -mul_rn(qa[3], qb[1]));
  const double d3 = add_rn(add_rn(add_rn(mul_rn(qa[0], qb[3]), -mul_rn(qa[1], qb[2])), mul_rn(qa[2], qb[1])), -mul_rn(qa[3], qb[0]));
  double ax[3] = {d1, d2, d3};
  const double sn = sqrt(add_rn(add_rn(mul_rn(d1, d1), mul_rn(d2, d2)), mul_rn(d3, d3)));
  if (sn < D_MINVAL) { ax[0] = 1.0; ax[1] = 0.0; ax[2] = 0.0; }
  else { ax[0] = ax[0] / sn; ax[1] = ax[1] / sn; ax[2] = ax[2] / sn; }
  double speed = mul_rn(2.0, atan2_cr(sn, d0));          // not the library's atan2: atan2_cr.h
  if (speed > D_PI) speed = add_rn(speed, -mul_rn(2.0, D_PI));
  for (int k = 0; k < 3; k++) res[k] = mul_rn(ax[k], speed);
}

// the engine's state and time; no knots are read and no knot rows written
DEV_NOINLINE void ph_init_feedback(FP Fc) {
  Ctx c;
  const KParams *K = &fp_generic(Fc)->K;
  ctx_init(c, K, lds_base());
  init_model_cache(K);
  Rows R = out_rows(K);
  init_arrays(c, K, R, K->state);
  init_world(c, R, K->time);
  ctx_close(c);
}

// where the head keeps dx = StateDiff(xbar[t], x_t): the solver's vectors Mgrad | search | Mv | vtmp, one contiguous block of
// 4 (nv + 1) doubles (host.h make_layout) that nothing reads between the integration of one step and the solve of the next.  The
// host refuses a model whose 2 nv + na does not fit (FB_DX_CAPACITY, feedback_resample.h)

// role 0, head of a step: ph_head with the feedback policy in place of the spline
template <int NVT>
DEV_NOINLINE void ph_head_feedback(FP Fc, int t, int last) {
  Ctx c; ctx_open(c, (KP)Fc);
  const FeedbackParams *F = fp_generic(Fc);
  const KParams *K = c.K;
  const DevModel &M = *c.M;
  Rows R = out_rows(K);
  int nu = M.nu;
  if (!last) {
    const int nq = M.nq, nv = M.nv, na = M.na, nd = 2 * nv + na, r = cand_index();
    double *dx = c.Mgrad;
    if (F->xbar) {
      // StateDiff(xbar[t], x_t), h = 1 (mj_differentiatePos per joint, then the plain differences of qvel and act)
      const double *xb = F->xbar + (size_t)t * R.ds;
      PFOR(j, M.njnt) {
        int qa = MIH(jnt_qposadr)[j], da = MIH(jnt_dofadr)[j], type = MIH(jnt_type)[j];
        if (type == 0) {
          for (int k = 0; k < 3; k++) dx[da + k] = add_rn(c.qpos[qa + k], -xb[qa + k]);
          fb_quat_diff(dx + da + 3, xb + qa + 3, c.qpos + qa + 3);
        } else if (type == 1) fb_quat_diff(dx + da, xb + qa, c.qpos + qa);
        else dx[da] = add_rn(c.qpos[qa], -xb[qa]);
      }
      PFOR(i, nv) dx[nv + i] = add_rn(c.qvel[i], -xb[nq + i]);
      if (na) PFOR(i, na) dx[2 * nv + i] = add_rn(C_ACT(c)[i], -xb[nq + nv + i]);
      SYNC();
    }
    const double alpha = F->alpha[r], scale = F->scale[r];
    // one lane per row of Kbar[t]
    PFOR(k, nu) {
      double a = F->ubar[(size_t)t * nu + k];
      if (F->kbar) a = add_rn(a, mul_rn(F->kbar[(size_t)t * nu + k], alpha));
      if (F->xbar) {
        const double *row = F->Kbar + ((size_t)t * nu + k) * nd;
        // a plain loop over the run-time nd: the compiler unrolls it by eight with the chunk's loads in flight together and finishes with
        // a scalar remainder loop.  An explicit chunked preload with the tail's index held inside the row measured slower
        double s = 0.0;
        for (int j = 0; j < nd; j++) s = add_rn(s, mul_rn(row[j], dx[j]));
        a = add_rn(a, mul_rn(s, scale));
      }
      a = d_clip(a, MD(actuator_ctrlrange)[2 * k], MD(actuator_ctrlrange)[2 * k + 1]);
      c.ctrl[k] = a; R.actions[t * nu + k] = a;
    }
    SYNC();
    if (bad_values(c.qpos, M.nq)) c.warning |= WARN_BADQPOS;
    if (bad_values(c.qvel, M.nv)) c.warning |= WARN_BADQVEL;
    if (c.warning) { if (LANE == 0) c.misc[MISC_BAD_STATE] = 1; ctx_close(c); return; }
  }
  PROF(c, 0);
  kinematics(c); PROF(c, 1);
#if !MJPC_SIDE_COM
  com_pos(c);
#endif
  PROF(c, 2);
  ctx_close(c);
}

// rollout<NVT> with the two feedback phases; no retry launch (full capacity only)
template <int NVT>
DEV void rollout_feedback(FP Fc) {
  KP Kc = (KP)Fc;
  int H = Kc->H;
  const bool r0 = ROLE0, r1 = ROLE1;
  if (r0) ph_init_feedback(Fc);
  XBAR();
  const int *misc = (const int *)(lds_base() + Kc->L.ints) + Kc->L.i_misc;
  double total = 0, total_before = 0;
  int failure = 0, t_fail = 0;
  for (int t = 0; t < H; t++) {
    int last = (t == H - 1);
    t_fail = t; total_before = total;
    if (r0) ph_head_feedback<NVT>(Fc, t, last);
    XBAR();
    if (uniform_i(misc[MISC_BAD_STATE])) { failure = 1; break; }
    presolve_window<NVT>(Kc, t, r0, r1);
    XBAR();
    solve_window<NVT>(Kc, t, last, r0);
    if (r1) {
      CostOut o = ph_residual_cost(Kc, t, last); total += o.cost;
      if (!last) ph_prefactor<NVT>(Kc);
    }
    XBAR();
    if (uniform_i(misc[MISC_WARNING]) | uniform_i(misc[MISC_WARN_OTHERS])) { failure = 1; break; }
    if (r0 && !last) ph_integrate<NVT>(Kc, t);
  }
  XBAR();
  if (r1) ph_finish(Kc, total, failure, t_fail, total_before);
}
