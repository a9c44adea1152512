// feedback_resample.h — a time-interpolated iLQG policy resampled at the step times of a rollout, once per call: the [H] tables
// xbar / ubar / kbar / Kbar the feedback rollout kernels read (feedback.h).  Every candidate of a batch starts at the same time and
// steps by the same timestep, so the tables do not depend on the candidate and the rollout never interpolates a gain matrix.
//
// Contract: the host's iLQGPolicy::Action (planner.cc; mjpc/planners/ilqg/policy.cc:68-140, utilities.cc:286-404) up to and without
// its StateDiff: FindInterval over the T knot times decides zero / linear / cubic, the actions and gains interpolate over the first
// T - 1 knots and the states over all T, and the quaternions of an interpolated state are renormalised.  Same bits as the host: the
// host's association, one rounded product / add per operation, IEEE sqrt and divide.  The step times are formed exactly as the
// rollout accumulates them (ph_integrate: time += timestep, once per step), so both see the same bits.
// The __global__ wrapper is in engine.hip; the 1-lane MJPC_EMU build (tests/emu/emu_feedback.cpp) runs the same functions.
#pragma once
#include <stddef.h>
#include "spmd.h"
#include "dmath.h"

// doubles of the feedback head's state-difference scratch (feedback.h: the solver vectors Mgrad | search | Mv | vtmp of the layout)
#define FB_DX_CAPACITY(nv) (4 * ((nv) + 1))

struct FbResampleArgs {
  const double *times, *states, *actions, *gains, *improvement;     // the policy: [T], [T][ds], [T][nu], [T][nu][nd], [T][nu] or null
  const int *jnt_type, *jnt_qposadr;                                // [njnt]
  int T, H, ds, nu, nd, njnt, representation;
  double time0, timestep;
  double *xbar, *ubar, *kbar, *Kbar;                                // [H] tables (kbar null with improvement)
};

DEV double fb_step_time(const FbResampleArgs &a, int t) {
  double time = a.time0;
  for (int s = 0; s < t; s++) time += a.timestep;
  return time;
}
// FindInterval (utilities.h:122-141) over the first n knot times
DEV void fb_find_interval(int *b, const double *xs, double v, int n) {
  int ub = 0;
  while (ub < n && !(v < xs[ub])) ub++;
  const int lo = ub - 1;
  if (lo < 0) { b[0] = 0; b[1] = 0; }
  else if (lo > n - 1) { b[0] = n - 1; b[1] = n - 1; }
  else { b[0] = lo; b[1] = ub < n - 1 ? ub : n - 1; }
}
// FiniteDifferenceSlope at the knot time x, component i
DEV double fb_slope(double x, const double *xs, const double *ys, int dim, int n, int i) {
  int b[2];
  fb_find_interval(b, xs, x, n);
  if (b[0] == 0 && b[1] == 0) return n > 2 ? add_rn(ys[dim * (b[1] + 1) + i], -ys[dim * b[1] + i]) / add_rn(xs[b[1] + 1], -xs[b[1]]) : 0.0;
  if (b[0] == n - 1 && b[1] == n - 1) return n > 2 ? add_rn(ys[dim * b[0] + i], -ys[dim * (b[0] - 1) + i]) / add_rn(xs[b[0]], -xs[b[0] - 1]) : 0.0;
  if (b[0] == 0) return add_rn(ys[dim * b[1] + i], -ys[dim * b[0] + i]) / add_rn(xs[b[1]], -xs[b[0]]);
  return add_rn(mul_rn(0.5, add_rn(ys[dim * b[1] + i], -ys[dim * b[0] + i])) / add_rn(xs[b[1]], -xs[b[0]]),
                mul_rn(0.5, add_rn(ys[dim * b[0] + i], -ys[dim * (b[0] - 1) + i])) / add_rn(xs[b[0]], -xs[b[0] - 1]));
}
// component i of Zero / Linear / CubicInterpolation of the first n knots at x
DEV double fb_interp(int rep, double x, const double *xs, const double *ys, int dim, int n, int i) {
  int b[2];
  fb_find_interval(b, xs, x, n);
  if (rep == 0 || b[0] == b[1]) return ys[dim * b[0] + i];
  const double dxs = add_rn(xs[b[1]], -xs[b[0]]), t = add_rn(x, -xs[b[0]]) / dxs;
  if (rep == 1) return add_rn(mul_rn(ys[dim * b[0] + i], add_rn(1.0, -t)), mul_rn(ys[dim * b[1] + i], t));
  const double t2 = mul_rn(t, t), t3 = mul_rn(t2, t);             // t * t * t = (t * t) * t
  const double c0 = add_rn(add_rn(mul_rn(mul_rn(mul_rn(2.0, t), t), t), -mul_rn(mul_rn(3.0, t), t)), 1.0);
  const double c1 = mul_rn(add_rn(add_rn(t3, -mul_rn(mul_rn(2.0, t), t)), t), dxs);
  const double c2 = add_rn(mul_rn(mul_rn(mul_rn(-2.0, t), t), t), mul_rn(mul_rn(3.0, t), t));
  const double c3 = mul_rn(add_rn(t3, -t2), dxs);
  const double p0 = ys[dim * b[0] + i], p1 = ys[dim * b[1] + i];
  const double m0 = fb_slope(xs[b[0]], xs, ys, dim, n, i), m1 = fb_slope(xs[b[1]], xs, ys, dim, n, i);
  return add_rn(add_rn(add_rn(mul_rn(c0, p0), mul_rn(c1, m0)), mul_rn(c2, p1)), mul_rn(c3, m1));
}

// the representation iLQGPolicy::Action uses at step t's time (zero when the time falls outside the knots)
DEV int fb_rep(const FbResampleArgs &a, double time) {
  int b[2];
  fb_find_interval(b, a.times, time, a.T);
  return b[0] == b[1] ? 0 : a.representation;
}
// element e of step t's row: e < ds the state, then nu actions, nu improvements, nu * nd gains
DEV void fb_resample(const FbResampleArgs &a, int t, int e) {
  const double time = fb_step_time(a, t);
  const int rep = fb_rep(a, time), ds = a.ds, nu = a.nu, nd = a.nd, T = a.T;
  if (e < ds) { a.xbar[(size_t)t * ds + e] = fb_interp(rep, time, a.times, a.states, ds, T, e); return; }
  e -= ds;
  if (e < nu) { a.ubar[(size_t)t * nu + e] = fb_interp(rep, time, a.times, a.actions, nu, T - 1, e); return; }
  e -= nu;
  if (e < nu) { if (a.improvement) a.kbar[(size_t)t * nu + e] = fb_interp(rep, time, a.times, a.improvement, nu, T - 1, e); return; }
  e -= nu;
  a.Kbar[(size_t)t * nu * nd + e] = fb_interp(rep, time, a.times, a.gains, nu * nd, T - 1, e);
}
DEV int fb_resample_elements(const FbResampleArgs &a) { return a.ds + 2 * a.nu + a.nu * a.nd; }
// mj_normalizeQuat of joint j's quaternion in step t's interpolated state (after every element of the row is written)
DEV void fb_resample_normalize(const FbResampleArgs &a, int t, int j) {
  if (a.jnt_type[j] > 1 || fb_rep(a, fb_step_time(a, t)) == 0) return;
  double *q = a.xbar + (size_t)t * a.ds + a.jnt_qposadr[j] + (a.jnt_type[j] == 0 ? 3 : 0);
  const double nrm = sqrt(add_rn(add_rn(add_rn(mul_rn(q[0], q[0]), mul_rn(q[1], q[1])), mul_rn(q[2], q[2])), mul_rn(q[3], q[3])));
  if (nrm < D_MINVAL) { q[0] = 1.0; q[1] = 0.0; q[2] = 0.0; q[3] = 0.0; }
  else for (int k = 0; k < 4; k++) q[k] = q[k] / nrm;
}
