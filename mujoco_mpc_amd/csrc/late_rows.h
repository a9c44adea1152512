// late_rows.h — residual rows that need the converged solve: accelerations (qacc, frame accelerations, accelerometer), the site-frame
// velocity sensors (gyro, velocimeter) and touch.  One phase of the one-step kernels, included by transition.h only: the rollout
// kernels never see it, and what residuals.h reads of the table shows a late block as a term-less SUM block (host.h pack_task), so in
// a rollout those rows are 0.0.
//
// The phase runs on the side wave between the barrier behind ph_solve / ph_residual_cost and ph_integrate: qacc, efc_force and the
// contact list are final, qpos / qvel are still the step's own, and the velocity stage's cvel, cdof and bias cacc (dynamics.h: the
// full-capacity layouts give them LDS of their own, nothing writes them until the next step's sweep) are still there.  It reads only
// that state and writes the late rows of c.residual, which ph_finish_step copies out.
//
// Order of every sum, so that a sequential loop reproduces the bits: dofs ascending, contacts ascending, the terms of a block in table
// order, the components of a NORM ascending.  The additions and multiplications written here are rounded one by one (no contraction),
// in the emulation and on the device alike; a sum over lanes adds the included lanes one after the other in lane order.
#pragma once

#ifdef MJPC_EMU
#define LATE_FP_STRICT
#else
#define LATE_FP_STRICT _Pragma("clang fp contract(off)")
#endif

// s + the values f of the lanes whose `inc` is set, added in ascending lane order; uniform control flow, the result in every lane
DEV double late_ordered_add(double s, double f, int inc) {
  LATE_FP_STRICT
#ifdef MJPC_EMU
  return inc ? s + f : s;
#else
  unsigned long long m = __builtin_amdgcn_ballot_w64(inc != 0);
  while (m) {
    const int l = __builtin_ctzll(m);
    m &= m - 1;
    s = s + lane_value(f, l);
  }
  return s;
#endif
}

DEV void late_cross(double *r, const double *a, const double *b) {
  LATE_FP_STRICT
  r[0] = a[1] * b[2] - a[2] * b[1]; r[1] = a[2] * b[0] - a[0] * b[2]; r[2] = a[0] * b[1] - a[1] * b[0];
}
DEV double late_pick3(const double *x, int e) { return e == 0 ? x[0] : (e == 1 ? x[1] : x[2]); }

// spatial acceleration of a body after the solve, about the com of its tree like cvel: the velocity stage's bias cacc (-gravity
// at the world, + cdof_dot qvel along the path) + cdof[d] qacc[d] over the dofs d of the path root .. body, ascending
DEV void late_cacc(Ctx &c, int body, double *a) {
  LATE_FP_STRICT
  for (int k = 0; k < 6; k++) a[k] = c.cacc[6 * body + k];
  unsigned long long m = MDM()[body];
  while (m) {
    const int d = __builtin_ctzll(m);
    m &= m - 1;
    const double qa = c.qacc[d];
    for (int k = 0; k < 6; k++) a[k] = a[k] + c.cdof[6 * d + k] * qa;
  }
}

// component e of a kinematic late source: the object's frame origin p, dif = p - com of the tree;
//   omega = cvel[0:3], v = cvel[3:6] + omega x dif;  alpha = cacc[0:3], a = cacc[3:6] + alpha x dif + omega x v   (mj_objectAcceleration)
// LINACC / ANGACC in the world frame; ACCELEROMETER / GYRO / VELOCIMETER = R^T (a / omega / v), R the site's frame
DEV double late_frame(Ctx &c, int kind, int ty, int id, int e) {
  LATE_FP_STRICT
  const int body = tbl_body(c, ty, id);
  const double *p = tbl_pos(c, ty, id), *com = c.subtree_com + 3 * MIH(body_rootid)[body], *cv = c.cvel + 6 * body;
  double dif[3], v[3], x[3], t[3];
  for (int k = 0; k < 3; k++) dif[k] = p[k] - com[k];
  late_cross(t, cv, dif);
  for (int k = 0; k < 3; k++) v[k] = cv[3 + k] + t[k];
  if (kind == TBL_GYRO) { for (int k = 0; k < 3; k++) x[k] = cv[k]; }
  else if (kind == TBL_VELOCIMETER) { for (int k = 0; k < 3; k++) x[k] = v[k]; }
  else {
    double A[6];
    late_cacc(c, body, A);
    if (kind == TBL_ANGACC) { for (int k = 0; k < 3; k++) x[k] = A[k]; }
    else {
      double u[3];
      late_cross(t, A, dif);
      late_cross(u, cv, v);
      for (int k = 0; k < 3; k++) x[k] = (A[3 + k] + t[k]) + u[k];
    }
  }
  if (kind == TBL_LINACC || kind == TBL_ANGACC) return late_pick3(x, e);
  double q[4], R[9];
  tbl_quat(c, ty, id, q);
  d_quat2mat(R, q);
  // column e of R against x
  const double r0 = e == 0 ? R[0] : (e == 1 ? R[1] : R[2]), r1 = e == 0 ? R[3] : (e == 1 ? R[4] : R[5]), r2 = e == 0 ? R[6] : (e == 1 ? R[7] : R[8]);
  return (r0 * x[0] + r1 * x[1]) + r2 * x[2];
}

// p (site coordinates) inside the zone; size in MuJoCo's conventions
DEV int late_in_zone(int shape, const double *p, const double *size) {
  LATE_FP_STRICT
  const double x = p[0], y = p[1], z = p[2], s0 = size[0];
  if (shape == ZONE_SPHERE) return (x * x + y * y) + z * z <= s0 * s0;
  if (shape == ZONE_BOX) return fabs(x) <= s0 && fabs(y) <= size[1] && fabs(z) <= size[2];
  if (shape == ZONE_ELLIPSOID) { const double a = x / s0, b = y / size[1], g = z / size[2]; return (a * a + b * b) + g * g <= 1.0; }
  if (shape == ZONE_CYLINDER) return x * x + y * y <= s0 * s0 && fabs(z) <= size[1];
  // capsule: distance to the segment +-h z
  const double h = size[1], zc = z > h ? h : (z < -h ? -h : z), dz = z - zc;
  return (x * x + y * y) + dz * dz <= s0 * s0;
}

// touch: lanes over the contacts of the solve; a contact counts when one of its geoms sits on the site's body, its normal force is
// positive and its position lies in the zone.  Normal force: the first row's (frictionless / elliptic), the sum of the edge forces
// in row order (pyramidal).  Uniform control flow; the sum (ascending contact index) in every lane
DEV double late_touch(Ctx &c, int shape, int site, const double *size) {
  LATE_FP_STRICT
  const DevModel &M = *c.M;
  const int sbody = MI(site_bodyid)[site];
  const double *sp = c.site_xpos + 3 * site;
  double q[4], R[9], s = 0;
  tbl_quat(c, 6, site, q);
  d_quat2mat(R, q);
  for (int base = 0; base < c.ncon; base += NLANE) {
    const int ci = base + LANE;
    double f = 0;
    int inc = 0;
    if (ci < c.ncon) {
      const int *cin = c.con_i + ci * CONI_STRIDE;
      const int dim = cin[0], r0 = cin[3];
      if (MI(geom_bodyid)[cin[1]] == sbody || MI(geom_bodyid)[cin[2]] == sbody) {
        if (dim > 1 && M.cone != 1) { for (int k = 0; k < 2 * (dim - 1); k++) f = f + c.efc_force[r0 + k]; }
        else f = c.efc_force[r0];
        if (f > 0) {
          const double *cp = c.contact + ci * M.con_stride + CON_POS;
          const double d0 = cp[0] - sp[0], d1 = cp[1] - sp[1], d2 = cp[2] - sp[2];
          double p[3];
          for (int k = 0; k < 3; k++) p[k] = (R[k] * d0 + R[3 + k] * d1) + R[6 + k] * d2;
          inc = late_in_zone(shape, p, size);
        }
      }
    }
    s = late_ordered_add(s, f, inc);
  }
  return s;
}

// side wave, behind the solve: every late block of the table at S->late_tab (model.h; host.h late_table).  Blocks one after the
// other, lanes over a block's components; a touch term is summed by the whole wave
DEV_NOINLINE void ph_late_rows(SP Sc) {
  LATE_FP_STRICT
  Ctx c; ctx_open(c, (KP)Sc, 1);
  const int *tab = sp_generic(Sc)->late_tab;
  const double *D = MD(task.dbl_data);
  const int nblock = uniform_i(tab[0]);
  const int *B = tab + LATE_HEADER, *T = B + LATE_BLOCK_INTS * nblock;
  for (int b = 0; b < nblock; b++, B += LATE_BLOCK_INTS) {
    const int op = uniform_i(B[0]), row = uniform_i(B[1]), ncomp = uniform_i(B[3]), t0 = uniform_i(B[4]), nt = uniform_i(B[5]);
    double ssq = 0;
    for (int k0 = 0; k0 < ncomp; k0 += NLANE) {
      const int k = k0 + LANE, active = k < ncomp;
      double v = 0;
      for (int j = t0; j < t0 + nt; j++) {
        const int *Tj = T + LATE_TERM_INTS * j;
        const int kind = uniform_i(Tj[0]), ty = uniform_i(Tj[1]), id = uniform_i(Tj[2]), off = uniform_i(Tj[3]);
        const double coef = D[uniform_i(Tj[4])];
        double x = 0;
        if (kind == TBL_TOUCH) x = late_touch(c, ty, id, D + off);
        else if (active) {
          const int e = off + k;
          if (kind == TBL_CONST) x = D[id + e];
          else if (kind == TBL_PARAM) x = MD(task.parameters)[e];
          else if (kind == TBL_QACC) x = c.qacc[e];
          else x = late_frame(c, kind, ty, id, e);
        }
        v = v + coef * x;
      }
      if (op == TBL_OP_NORM) ssq = late_ordered_add(ssq, v * v, active);
      else if (active) c.residual[row + k] = v;
    }
    if (op == TBL_OP_NORM && LANE == 0) c.residual[row] = sqrt(ssq);
  }
  ctx_close(c);
}
