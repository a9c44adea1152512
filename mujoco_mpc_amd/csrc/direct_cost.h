// direct_cost.h — device side of the direct optimiser's window cost (mjpc/direct/direct.cc: BlockSensor, BlockForce, ResidualSensor,
// ResidualForce, CostSensor, CostForce, TotalGradient, TotalHessian; SetBlockInBand of mjpc/utilities.cc), restated in this project's order:
//   dc_norms        per configuration: the residuals with the zeroing rules of the window's ends, the sensors' weights, norm values,
//                   gradients and Hessian parts (norm_grad_hess of cost_derivatives.h), the force term's weighted residual and value
//   dc_cost         the three totals
//   dc_block_*      the chain rule: a configuration's Jacobian block J_t [ns + nv][3 nv] from the six inverse blocks and the velocity
//                   blocks, with the end rules of InverseDerivatives::Compute applied while the blocks are read
//   dc_nj           N_t J_t: the norm Hessian times the block (the reference's tmp0)
//   dc_gradient, dc_band   one entry of the gradient / of the band Hessian
// The __global__ wrappers are in engine.hip; the 1-lane MJPC_EMU build (tests/emu/emu_direct.cpp) plays the same functions in a single
// thread.
//
// Window.  T >= 3 configurations of nv dofs; ntotal = nv T, nband = 3 nv.  Column c of configuration t's block stands for global column
// nv (t - 1) + c: group 0 (c < nv) is configuration t - 1, group 1 configuration t, group 2 configuration t + 1.  Configuration 0 has
// group 1 alone (the reference keeps its block as [ns][nv] at column 0: the same entries), configuration T - 1 groups 0 and 1; the
// groups a configuration does not have are stored as zeros and never read.
//   interior t    J = [ Dv V0 + Da A0 | Dq + Dv V1 + Da A1 | Da A2 ],  V0 = dv_t/dq_{t-1}, V1 = dv_t/dq_t,
//                 A0 = -V0 / h, A1 = (dv_{t+1}/dq_t - V1) / h, A2 = (dv_{t+1}/dq_{t+1}) / h
//   t = T - 1     sensor rows [ Dv V0 | Dq + Dv V1 ] without the acceleration-stage rows; no force rows
//   t = 0         sensor rows [ 0 | Dq ] of the position-stage rows alone; no force rows
// D* are the six blocks of mjpc_hip_inverse_fd as ifd_difference_kernel leaves them ([nv][nv] and [nr][nv] per configuration, entry
// [i][j] = d out_i / d in_j; the sensors are rows row0 .. row0 + ns of the nr residual rows).
//
// Band Hessian [ntotal][nband], MuJoCo's lower band: row R holds columns R - nband + 1 .. R, the diagonal at column nband - 1.
//
// Summation rule: cost_derivatives.h's.  Every contraction starts at 0.0 and runs over the ascending contraction index, one rounded
// product and one rounded add per step, never fused; `/` and sqrt() are the compiler's correctly rounded ones.  An entry of J is
// (base + P1) + P2 with base = Dq's entry (group 1) or 0.0, P1 = the contraction with V over all nv (0.0 where the configuration has
// none: group 2, t = 0), P2 the one with A (0.0 outside the interior).  A gradient or band entry is (sensor part) + (force part); the
// sensor part runs over ascending t and within t over ascending sensor, each sensor's contraction over its rows scaled by its weight;
// the force part over ascending t.  A masked (t, sensor) pair is skipped.  Every entry has one owner, so the overlapping blocks of
// neighbouring configurations need no atomics, two calls give the same bits, and a host restatement gives the device's.
#pragma once
#include "cost_derivatives.h"

#define DC_TILE 16
#define DC_THREADS 256
enum { DC_STAGE_POS = 0, DC_STAGE_VEL = 1, DC_STAGE_ACC = 2 };

struct DcArgs {
  int T, nv, nr, ns, row0, num_sensor;
  // the sensors: [num_sensor] dimension, first row (within the ns rows), stage, norm type, {p, q}, noise; row_sensor [ns] = a row's sensor
  const int *dim, *first, *stage, *norm, *row_sensor;
  const double *prm, *noise_sensor, *noise_process;
  const int *mask;                      // [T][num_sensor], null: every sensor on
  int sensor_flag, force_flag, time_scaling_sensor, time_scaling_force, first_pos, last_pos, last_vel;
  double h;
  // inputs
  const double *rs, *rf;                // [T][ns] prediction - measurement, [T][nv] (rows 0 and T - 1 are not read)
  const double *Df[3], *Ds[3];          // by q, v, a: [T][nv][nv], [T][nr][nv]
  const double *V0, *V1;                // [T][nv][nv] dv_t/dq_{t-1}, dv_t/dq_t (index 0 is not read)
  // per configuration, written by dc_norms
  double *res_s, *ng_s, *hd_s;          // [T][ns] residual behind the end rules, norm gradient, Hessian diagonal
  double *hs_s, *w_s, *wy_s;            // [T][num_sensor][2] dense scalars, [T][num_sensor] weight, weight * norm
  double *res_f, *ng_f, *y_f;           // [T][nv] force residual, weighted residual, [T] the term's value
  // blocks
  double *Js, *Jf, *NJs, *NJf;          // [T][ns][nband], [T][nv][nband]
  double *gradient, *band, *cost;       // [ntotal], [ntotal][nband], [3] = cost, cost_sensor, cost_force
};

DEV int dc_nband(const DcArgs &a) { return 3 * a.nv; }
DEV int dc_interior(const DcArgs &a, int t) { return t >= 1 && t <= a.T - 2; }
DEV int dc_masked(const DcArgs &a, int t, int i) { return a.mask && !a.mask[(size_t)t * a.num_sensor + i]; }

// ------------------------------------------------------------------------------ residuals, weights, norms
// does the residual of a sensor of stage st count at configuration t (ResidualSensor's zeroing of the two ends)
DEV int dc_keep_residual(const DcArgs &a, int t, int st) {
  if (t == 0) return st == DC_STAGE_POS;
  if (t == a.T - 1) return (st == DC_STAGE_POS && a.last_pos) || (st == DC_STAGE_VEL && a.last_vel);
  return 1;
}
// time_weight / noise / dim / T, times the end settings; time_weight = 1, h^2, h^4 by stage under time_scaling_sensor
DEV double dc_sensor_weight(const DcArgs &a, int t, int i) {
  const double h2 = mul_rn(a.h, a.h);
  double tw = 1.0;
  if (a.time_scaling_sensor) tw = a.stage[i] == DC_STAGE_VEL ? h2 : (a.stage[i] == DC_STAGE_ACC ? mul_rn(h2, h2) : 1.0);
  double w = tw / a.noise_sensor[i] / (double)a.dim[i] / (double)a.T;
  if (t == 0) w = mul_rn(w, a.first_pos ? 1.0 : 0.0);
  if (t == a.T - 1) w = mul_rn(w, (a.last_pos || a.last_vel) ? 1.0 : 0.0);
  return w;
}
// h^4 / noise / nv / (T - 2) (1 in place of h^4 without time_scaling_force)
DEV double dc_force_weight(const DcArgs &a, int i) {
  const double h2 = mul_rn(a.h, a.h);
  return (a.time_scaling_force ? mul_rn(h2, h2) : 1.0) / a.noise_process[i] / (double)a.nv / (double)(a.T - 2);
}
// The value of a norm by the summation rule, so that the costs are the host's bits too: the types whose value needs no more than
// sqrt are written out here; every other type's value is the one norm_grad_hess returns (libm's pow / cosh / exp / log, as their
// gradients).
DEV double dc_norm_value(const double *x, const double *prm, int n, int type, double y) {
  const double p = prm[0];
  double c = 0;
  switch (type) {
    case -1: return x[0];
    case 0:
      for (int i = 0; i < n; i++) c = add_rn(c, mul_rn(x[i], x[i]));
      return mul_rn(0.5, c);
    case 2:
      for (int i = 0; i < n; i++) c = add_rn(c, mul_rn(x[i], x[i]));
      return add_rn(sqrt(add_rn(c, mul_rn(p, p))), -p);
    case 6:
      for (int i = 0; i < n; i++) c = add_rn(c, add_rn(sqrt(add_rn(mul_rn(x[i], x[i]), mul_rn(p, p))), -p));
      return c;
    default: return y;
  }
}
// sensor i of configuration t
DEV void dc_norm_sensor(const DcArgs &a, int t, int i) {
  const int f = a.first[i], n = a.dim[i], keep = dc_keep_residual(a, t, a.stage[i]);
  const size_t o = (size_t)t * a.ns + f, k = (size_t)t * a.num_sensor + i;
  for (int r = 0; r < n; r++) a.res_s[o + r] = keep ? a.rs[o + r] : 0.0;
  const double y = norm_grad_hess(a.ng_s + o, a.hd_s + o, a.hs_s + 2 * k, a.res_s + o, a.prm + 2 * i, n, a.norm[i]);
  const double w = dc_sensor_weight(a, t, i);
  a.w_s[k] = w;
  a.wy_s[k] = dc_masked(a, t, i) ? 0.0 : mul_rn(w, dc_norm_value(a.res_s + o, a.prm + 2 * i, n, a.norm[i], y));
}
// dof i of configuration t's force term
DEV void dc_norm_force(const DcArgs &a, int t, int i) {
  const size_t o = (size_t)t * a.nv + i;
  const int in = dc_interior(a, t);
  a.res_f[o] = in ? a.rf[o] : 0.0;
  a.ng_f[o] = in ? mul_rn(dc_force_weight(a, i), a.rf[o]) : 0.0;
}
// 0.5 r . (w r) of configuration t
DEV double dc_force_value(const DcArgs &a, int t) {
  if (!dc_interior(a, t)) return 0.0;
  double c = 0;
  for (int i = 0; i < a.nv; i++) { const double r = a.rf[(size_t)t * a.nv + i]; c = add_rn(c, mul_rn(r, mul_rn(dc_force_weight(a, i), r))); }
  return mul_rn(0.5, c);
}
// which = 0: cost_sensor, 1: cost_force
DEV double dc_cost_part(const DcArgs &a, int which) {
  double c = 0;
  if (which == 0) { if (a.sensor_flag) for (size_t k = 0; k < (size_t)a.T * a.num_sensor; k++) c = add_rn(c, a.wy_s[k]); }
  else if (a.force_flag) for (int t = 1; t <= a.T - 2; t++) c = add_rn(c, a.y_f[t]);
  return c;
}

// ------------------------------------------------------------------------------ chain rule
// row o of a configuration's block: a sensor row (o < ns) or dof o - ns of the force.  Entry [o][k] of the inverse block `which`
// (0 q, 1 v, 2 a) behind the end rules: what the ends drop reads as 0.0 and is not loaded
DEV double dc_D(const DcArgs &a, int t, int which, int o, int k) {
  if (o < a.ns) {
    const int st = a.stage[a.row_sensor[o]];
    const int keep = t == 0 ? (which == 0 && st == DC_STAGE_POS) : (t == a.T - 1 ? (which < 2 && st < DC_STAGE_ACC) : 1);
    return keep ? a.Ds[which][((size_t)t * a.nr + a.row0 + o) * a.nv + k] : 0.0;
  }
  return dc_interior(a, t) ? a.Df[which][((size_t)t * a.nv + (o - a.ns)) * a.nv + k] : 0.0;
}
DEV int dc_has_V(const DcArgs &a, int t, int g) { return t >= 1 && g < 2; }
DEV int dc_has_A(const DcArgs &a, int t) { return dc_interior(a, t); }
// entry [k][j] of the velocity block of group g
DEV double dc_V(const DcArgs &a, int t, int g, int k, int j) {
  if (!dc_has_V(a, t, g)) return 0.0;
  return (g == 0 ? a.V0 : a.V1)[((size_t)t * a.nv + k) * a.nv + j];
}
// entry [k][j] of the acceleration block of group g
DEV double dc_A(const DcArgs &a, int t, int g, int k, int j) {
  if (!dc_has_A(a, t)) return 0.0;
  const double ih = 1.0 / a.h;
  const size_t e = ((size_t)t * a.nv + k) * a.nv + j, e1 = e + (size_t)a.nv * a.nv;
  if (g == 0) return mul_rn(a.V0[e], -ih);
  if (g == 1) return mul_rn(add_rn(a.V0[e1], -a.V1[e]), ih);
  return mul_rn(a.V1[e1], ih);
}
// A workgroup owns the DC_TILE x DC_TILE tile of configuration t's block at rows o0, columns c0, and walks the contraction index in
// chunks of DC_TILE through LDS: thread tid stages entry [tid / DC_TILE][tid % DC_TILE] of the four operand tiles (Dv, Da by k along
// a row of the inverse blocks; V, A by column along a row of the velocity blocks: both sides read whole segments), then adds its
// entry's products of the chunk in ascending k.  Odd row stride: no bank conflicts either way.
#define DC_LD (DC_TILE + 1)
struct DcTiles { double *dv, *da, *bv, *ba; };        // [DC_TILE][DC_LD] each
#define DC_TILE_DOUBLES (4 * DC_TILE * DC_LD)
DEV DcTiles dc_tiles(double *sm) { DcTiles L; L.dv = sm; L.da = L.dv + DC_TILE * DC_LD; L.bv = L.da + DC_TILE * DC_LD; L.ba = L.bv + DC_TILE * DC_LD; return L; }
DEV void dc_block_stage(const DcArgs &a, int t, int o0, int c0, int k0, int tid, const DcTiles &L) {
  const int hi = tid / DC_TILE, lo = tid % DC_TILE, no = a.ns + a.nv;
  {
    const int o = o0 + hi, k = k0 + lo, in = o < no && k < a.nv;
    L.dv[hi * DC_LD + lo] = in ? dc_D(a, t, 1, o, k) : 0.0;
    L.da[hi * DC_LD + lo] = in ? dc_D(a, t, 2, o, k) : 0.0;
  }
  {
    const int k = k0 + hi, c = c0 + lo, in = k < a.nv && c < dc_nband(a), g = c / a.nv, j = c - g * a.nv;
    L.bv[hi * DC_LD + lo] = in ? dc_V(a, t, g, k, j) : 0.0;
    L.ba[hi * DC_LD + lo] = in ? dc_A(a, t, g, k, j) : 0.0;
  }
}
DEV void dc_block_accum(const DcArgs &a, int k0, int tid, const DcTiles &L, double &p1, double &p2) {
  const int oi = tid / DC_TILE, ci = tid % DC_TILE, n = a.nv - k0 < DC_TILE ? a.nv - k0 : DC_TILE;
  for (int kk = 0; kk < n; kk++) {
    p1 = add_rn(p1, mul_rn(L.dv[oi * DC_LD + kk], L.bv[kk * DC_LD + ci]));
    p2 = add_rn(p2, mul_rn(L.da[oi * DC_LD + kk], L.ba[kk * DC_LD + ci]));
  }
}
DEV void dc_block_store(const DcArgs &a, int t, int o0, int c0, int tid, double p1, double p2) {
  const int o = o0 + tid / DC_TILE, c = c0 + tid % DC_TILE, nb = dc_nband(a);
  if (o >= a.ns + a.nv || c >= nb) return;
  const int g = c / a.nv, j = c - g * a.nv;
  const double base = g == 1 ? dc_D(a, t, 0, o, j) : 0.0;
  const double v = add_rn(add_rn(base, dc_has_V(a, t, g) ? p1 : 0.0), dc_has_A(a, t) ? p2 : 0.0);
  if (o < a.ns) a.Js[((size_t)t * a.ns + o) * nb + c] = v;
  else a.Jf[((size_t)t * a.nv + (o - a.ns)) * nb + c] = v;
}

// entry e of [T][ns + nv][nband]: the norm Hessian times the block
DEV void dc_nj(const DcArgs &a, size_t e) {
  const int nb = dc_nband(a), no = a.ns + a.nv;
  const int c = (int)(e % nb), o = (int)(e / nb % no), t = (int)(e / nb / no);
  if (o >= a.ns) {
    const size_t at = ((size_t)t * a.nv + (o - a.ns)) * nb + c;
    a.NJf[at] = dc_interior(a, t) ? mul_rn(dc_force_weight(a, o - a.ns), a.Jf[at]) : 0.0;
    return;
  }
  const int i = a.row_sensor[o], f = a.first[i], n = a.dim[i];
  const size_t row = (size_t)t * a.ns, at = (row + o) * nb + c;
  if (!norm_dense(a.norm[i])) { a.NJs[at] = mul_rn(a.hd_s[row + o], a.Js[at]); return; }
  double s = 0;
  for (int q = 0; q < n; q++)
    s = add_rn(s, mul_rn(norm_hess_entry(a.norm[i], a.res_s + row + f, a.ng_s + row + f, a.hs_s + 2 * ((size_t)t * a.num_sensor + i), o - f, q),
                         a.Js[(row + f + q) * nb + c]));
  a.NJs[at] = s;
}

// ------------------------------------------------------------------------------ gradient, band Hessian
// column of configuration t's block that stands for global column G; -1: the block has none
DEV int dc_col(const DcArgs &a, int t, int G) {
  const int c = G - a.nv * (t - 1);
  if (c < 0 || c >= dc_nband(a)) return -1;
  const int g = c / a.nv;
  if (t == 0 && g != 1) return -1;
  if (t == a.T - 1 && g == 2) return -1;
  return c;
}
// the configurations whose block can hold global column G: t_lo .. t_hi
DEV void dc_trange(const DcArgs &a, int G, int &lo, int &hi) {
  const int b = G / a.nv;
  lo = b - 1 < 0 ? 0 : b - 1; hi = b + 1 > a.T - 1 ? a.T - 1 : b + 1;
}
// sum over the sensors of configuration t of w (J_i[.][ca])' X_i[.][cb]; X = null: the norm gradient (a vector), else NJs
DEV double dc_sensor_sum(const DcArgs &a, int t, int ca, const double *X, int cb, double acc) {
  const int nb = dc_nband(a);
  for (int i = 0; i < a.num_sensor; i++) {
    if (dc_masked(a, t, i)) continue;
    const size_t row = (size_t)t * a.ns + a.first[i];
    double s = 0;
    for (int r = 0; r < a.dim[i]; r++) s = add_rn(s, mul_rn(a.Js[(row + r) * nb + ca], X ? X[(row + r) * nb + cb] : a.ng_s[row + r]));
    acc = add_rn(acc, mul_rn(a.w_s[(size_t)t * a.num_sensor + i], s));
  }
  return acc;
}
DEV double dc_force_sum(const DcArgs &a, int t, int ca, const double *X, int cb, double acc) {
  const int nb = dc_nband(a);
  const size_t row = (size_t)t * a.nv;
  double s = 0;
  for (int r = 0; r < a.nv; r++) s = add_rn(s, mul_rn(a.Jf[(row + r) * nb + ca], X ? X[(row + r) * nb + cb] : a.ng_f[row + r]));
  return add_rn(acc, s);
}
DEV double dc_gradient(const DcArgs &a, int G) {
  int lo, hi; dc_trange(a, G, lo, hi);
  double gs = 0, gf = 0;
  for (int t = lo; t <= hi; t++) {
    const int c = dc_col(a, t, G);
    if (c < 0) continue;
    if (a.sensor_flag) gs = dc_sensor_sum(a, t, c, nullptr, 0, gs);
    if (a.force_flag && dc_interior(a, t)) gf = dc_force_sum(a, t, c, nullptr, 0, gf);
  }
  return add_rn(gs, gf);
}
// entry [R][C] of the band: global column R - (nband - 1 - C); in front of the first column it is a leading zero
DEV double dc_band(const DcArgs &a, int R, int C) {
  const int G = R - (dc_nband(a) - 1 - C);
  if (G < 0) return 0.0;
  int lo, hi; dc_trange(a, R, lo, hi);
  double hs = 0, hf = 0;
  for (int t = lo; t <= hi; t++) {
    const int ca = dc_col(a, t, R), cb = dc_col(a, t, G);
    if (ca < 0 || cb < 0) continue;
    if (a.sensor_flag) hs = dc_sensor_sum(a, t, ca, a.NJs, cb, hs);
    if (a.force_flag && dc_interior(a, t)) hf = dc_force_sum(a, t, ca, a.NJf, cb, hf);
  }
  return add_rn(hs, hf);
}
// entry e of [ntotal][nband + 1]: a row's nband band entries, then its gradient entry
DEV void dc_entry(const DcArgs &a, size_t e) {
  const int nb = dc_nband(a), R = (int)(e / (nb + 1)), C = (int)(e % (nb + 1));
  if (C == nb) a.gradient[R] = dc_gradient(a, R);
  else a.band[(size_t)R * nb + C] = dc_band(a, R, C);
}

// ------------------------------------------------------------------------------ the window: velocities, accelerations, velocity blocks
// (ConfigurationToVelocityAcceleration, VelocityAccelerationDerivatives of direct.cc; DifferentiateDifferentiatePos and
// DifferentiateSubQuat of mjpc/utilities.cc.)  nwin windows of T configurations; row g = w T + t.
//   v_t = differentiatePos(q_{t-1}, q_t) / h for t >= 1, a_t = (v_{t+1} - v_t) / h for 1 <= t <= T - 2; v_0 = a_0 = a_{T-1} = 0
// A quaternion dof's velocity is the body-frame rotation vector of q_{t-1}^-1 q_t in feedback.h's spelling (fb_quat_diff: separately rounded
// products, IEEE sqrt and divide, the angle from atan2_cr.h, which host and device share).  The rows are written where the inverse
// kernel (value call: its table itself) or ifd_assemble (derivative call: the nominal rows) reads them.
#include "atan2_cr.h"

struct DcWinArgs {
  const double *q, *act, *ctrl, *time;      // [nwin][T][nq], [nwin][T][na], [nwin][T][nu], [T]
  const int *dofmap;                        // [nv][2], as FdArgs::dofmap: (qpos address, axis) of a dof, axis < 0: a plain coordinate
  int nwin, T, nq, nv, na, nu;
  double h;
  double *x, *u, *a, *tm;                   // rows [nwin T]: state [nq + nv + na], control, acceleration, time
  double *V0, *V1;                          // [T][nv][nv] of window 0 (derivative call), or null
};

// unit axis ax[3], half angle th2 (signed: the wrapped angle keeps its sign on th2, not on the axis) and cot = cos / sin of the half
// angle of q0^-1 q1; returns 0 below the small-angle threshold of the normalisation (axis = x, angle 0)
DEV int dc_quat_axis(const double *qa, const double *qb, double *ax, double &th2, double &cot) {
  const double d0 = add_rn(add_rn(add_rn(mul_rn(qa[0], qb[0]), mul_rn(qa[1], qb[1])), mul_rn(qa[2], qb[2])), mul_rn(qa[3], qb[3]));
  const double d1 = add_rn(add_rn(add_rn(mul_rn(qa[0], qb[1]), -mul_rn(qa[1], qb[0])), -mul_rn(qa[2], qb[3])), mul_rn(qa[3], qb[2]));
  const double d2 = add_rn(add_rn(add_rn(mul_rn(qa[0], qb[2]), mul_rn(qa[1], qb[3])), -mul_rn(qa[2], qb[0])), -mul_rn(qa[3], qb[1]));
  const double d3 = add_rn(add_rn(add_rn(mul_rn(qa[0], qb[3]), -mul_rn(qa[1], qb[2])), mul_rn(qa[2], qb[1])), -mul_rn(qa[3], qb[0]));
  const double sn = sqrt(add_rn(add_rn(mul_rn(d1, d1), mul_rn(d2, d2)), mul_rn(d3, d3)));
  if (sn < D_MINVAL) { ax[0] = 1.0; ax[1] = 0.0; ax[2] = 0.0; th2 = 0.0; cot = 0.0; return 0; }
  ax[0] = d1 / sn; ax[1] = d2 / sn; ax[2] = d3 / sn;
  double speed = mul_rn(2.0, atan2_cr(sn, d0));
  if (speed > D_PI) speed = add_rn(speed, -mul_rn(2.0, D_PI));
  th2 = mul_rn(0.5, speed); cot = d0 / sn;
  return 1;
}
// component k of v_t of window w (t >= 1)
DEV double dc_velocity(const DcWinArgs &a, int w, int t, int k) {
  const double *q0 = a.q + ((size_t)w * a.T + t - 1) * a.nq, *q1 = q0 + a.nq;
  const int qa = a.dofmap[2 * k], axk = a.dofmap[2 * k + 1];
  if (axk < 0) return add_rn(q1[qa], -q0[qa]) / a.h;
  double ax[3], th2, cot;
  dc_quat_axis(q0 + qa, q1 + qa, ax, th2, cot);
  return mul_rn(ax[axk], mul_rn(2.0, th2)) / a.h;
}
// element i of row g: i < ds the state, ds <= i < ds + nu the control, i == ds + nu the time, then the nv accelerations
DEV void dc_window_row(const DcWinArgs &a, size_t g, int i) {
  const int nq = a.nq, nv = a.nv, ds = nq + nv + a.na, nu = a.nu, w = (int)(g / (size_t)a.T), t = (int)(g - (size_t)w * a.T);
  if (i == ds + nu) { a.tm[g] = a.time[t]; return; }
  if (i >= ds && i < ds + nu) { a.u[g * nu + (i - ds)] = a.ctrl[g * nu + (i - ds)]; return; }
  if (i > ds + nu) {
    const int k = i - (ds + nu + 1);
    a.a[g * nv + k] = (t >= 1 && t <= a.T - 2) ? add_rn(dc_velocity(a, w, t + 1, k), -dc_velocity(a, w, t, k)) / a.h : 0.0;
    return;
  }
  if (i < nq) a.x[g * ds + i] = a.q[g * nq + i];
  else if (i < nq + nv) a.x[g * ds + i] = t >= 1 ? dc_velocity(a, w, t, i - nq) : 0.0;
  else a.x[g * ds + i] = a.act[g * a.na + (i - nq - nv)];
}
// entry e of [T][nv][nv]: dv_t/dq_{t-1} and dv_t/dq_t of window 0, row k, column j.  A plain coordinate: -1/h and 1/h on the diagonal.
// A quaternion dof: with the rotation q_{t-1}^-1 q_t = (axis, angle), th2 = angle / 2, c1 = 1 - th2 / tan(th2) (0 below |th2| = 6e-8),
//   Jm = I + c1 (axis axis' - I) + th2 [axis]x-like terms (the reference's nine entries, kept as it writes them),
// dv_t/dq_t = Jm / h and dv_t/dq_{t-1} = -Jm' / h: the reference differentiates subQuat(q_t, q_{t-1}) and swaps the arguments' roles.
// th2 / tan(th2) is th2 times the quaternion's own cos / sin of the half angle: no library tangent, the same bits on host and device.
DEV void dc_velocity_block(const DcWinArgs &a, size_t e) {
  const int nv = a.nv, j = (int)(e % nv), k = (int)(e / nv % nv), t = (int)(e / nv / nv);
  double v0 = 0.0, v1 = 0.0;
  const int qa = a.dofmap[2 * k], axk = a.dofmap[2 * k + 1];
  if (t >= 1) {
    const double ih = 1.0 / a.h;
    if (axk < 0) { if (j == k) { v0 = -ih; v1 = ih; } }
    else if (a.dofmap[2 * j] == qa && a.dofmap[2 * j + 1] >= 0) {
      const int axj = a.dofmap[2 * j + 1];
      const double *q0 = a.q + ((size_t)t - 1) * a.nq + qa, *q1 = q0 + a.nq;
      double x[3], th2, cot;
      dc_quat_axis(q0, q1, x, th2, cot);
      const double c0 = th2, c1 = add_rn(1.0, -(fabs(th2) < 6e-8 ? 1.0 : mul_rn(th2, cot)));
      double J[9];
      J[0] = add_rn(1.0, mul_rn(c1, add_rn(-mul_rn(x[1], x[1]), -mul_rn(x[2], x[2]))));
      J[1] = add_rn(mul_rn(mul_rn(c1, x[0]), x[1]), -mul_rn(c0, x[2]));
      J[2] = add_rn(mul_rn(c0, x[1]), mul_rn(mul_rn(c1, x[0]), x[2]));
      J[3] = add_rn(mul_rn(c0, x[2]), mul_rn(mul_rn(c1, x[0]), x[1]));
      J[4] = add_rn(1.0, mul_rn(c1, add_rn(-mul_rn(x[0], x[0]), -mul_rn(x[2], x[2]))));
      J[5] = add_rn(mul_rn(mul_rn(c1, x[1]), x[2]), -mul_rn(c0, x[0]));
      J[6] = add_rn(mul_rn(mul_rn(c1, x[0]), x[2]), -mul_rn(c0, x[1]));
      J[7] = add_rn(mul_rn(c0, x[0]), mul_rn(mul_rn(c1, x[1]), x[2]));
      J[8] = add_rn(1.0, mul_rn(c1, add_rn(-mul_rn(x[0], x[0]), -mul_rn(x[1], x[1]))));
      v1 = mul_rn(J[3 * axk + axj], ih); v0 = mul_rn(-J[3 * axj + axk], ih);
    }
  }
  a.V0[e] = v0; a.V1[e] = v1;
}

// the residuals of the window's evaluations: entry e of [nwin T][ns + nv]; the evaluation of row g is table row g * E (E slots per
// configuration, slot 0 the base), prediction - measurement (the measurements are shared by the windows)
struct DcResArgs { const double *residual, *qfrc, *y_s, *y_f; int T, nv, nr, ns, row0, E; double *rs, *rf; };
DEV void dc_residual(const DcResArgs &a, size_t e) {
  const int no = a.ns + a.nv, o = (int)(e % no); const size_t g = e / no, t = g % a.T, row = g * a.E;
  if (o < a.ns) a.rs[g * a.ns + o] = add_rn(a.residual[row * a.nr + a.row0 + o], -a.y_s[t * a.ns + o]);
  else a.rf[g * a.nv + (o - a.ns)] = add_rn(a.qfrc[row * a.nv + (o - a.ns)], -a.y_f[t * a.nv + (o - a.ns)]);
}
// window w of a value call: the per-configuration arrays and the costs of that window
DEV DcArgs dc_window(DcArgs a, int w) {
  const size_t T = a.T, m = a.num_sensor;
  a.rs += w * T * a.ns; a.res_s += w * T * a.ns; a.ng_s += w * T * a.ns; a.hd_s += w * T * a.ns;
  a.hs_s += 2 * w * T * m; a.w_s += w * T * m; a.wy_s += w * T * m;
  a.rf += w * T * a.nv; a.res_f += w * T * a.nv; a.ng_f += w * T * a.nv; a.y_f += w * T;
  a.cost += 3 * w;
  return a;
}
