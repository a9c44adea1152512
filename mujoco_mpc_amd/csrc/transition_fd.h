// transition_fd.h — finite-difference transition derivatives around the one-step kernel (transition.h):
//   fd_assemble   the perturbed (state, ctrl, time) table of a group of knots from the nominal rows (x_t, u_t, time_t)
//   fd_entry      one entry of A / B / C / D from the next states and residuals of those evaluations
// Contract: MuJoCo's mjd_transitionFD (tangent order [dq(nv), dv(nv), dact(na)], entry [i][j] = d out_i / d in_j), with the
// control-nudge rule and the residual alignment spelled out in include/mjpc_hip.h (mjpc_hip_transition_fd).
// The __global__ wrappers are in engine.hip; the 1-lane MJPC_EMU build (tests/emu/emu_transition.cpp) runs the same functions in a
// single thread.
//
// Evaluation slots of knot t (E per knot, table row t * E + s):
//   one-sided  E = 1 + nd + nu        s = 0 base; s = 1 + c: column c nudged (+eps; a control backwards when it cannot go forwards)
//   centred    E = 1 + 2 (nd + nu)    s = 0 base; s = 1 + 2c: column c at +eps; s = 2 + 2c: at -eps
// A control slot whose nudge the rule forbids, and every control slot of a terminal knot, holds the base row: the evaluation is
// redundant, the difference never reads it.
#pragma once
#include <stddef.h>
#include "spmd.h"
#include "dmath.h"

struct FdArgs {
  const double *x, *u, *time;        // nominal rows of the group: [T][ds], [T][nu], [T]
  const int *dofmap;                 // [nv][2]: qpos address of dof d's coordinate (of w for a quaternion), axis 0..2 of a quaternion dof or -1
  const int *ctrllimited;            // [nu]
  const double *ctrlrange;           // [nu][2]
  int T, nq, nv, na, nu, nr, centered, last_is_terminal;
  double eps, cs, sn;                // cs / sn = cos / sin of eps / 2, from the host's libm: the same bits on every flavour
  double *state_tab, *ctrl_tab, *time_tab;             // [T * E] rows the step kernel reads
  const double *next_state, *residual; const int *fail;   // [T * E] rows the step kernel wrote
  double *A, *B, *C, *D;             // [T] blocks, row-major
  int *failure;                      // [T]: OR of the warning bits of every evaluation at t
};

DEV int fd_slots(const FdArgs &a) { int nc = 2 * a.nv + a.na + a.nu; return a.centered ? 1 + 2 * nc : 1 + nc; }
// bit 0: the forward nudge of a control is used, bit 1: the backward one
DEV int fd_nudge(int limited, double u, double eps, double lo, double hi, int centered) {
  int fwd = !limited || u + eps <= hi;
  int bwd = (centered || !fwd) && (!limited || u - eps >= lo);
  return fwd | (bwd << 1);
}

// q <- normalise(normalise(q) * [cs, sn * e_ax]): ph_integrate's position update of a rotational dof for a unit velocity along body
// axis ax over the "time" eps (d_quatintegrate), spelled with separately rounded products and IEEE sqrt / divide so that every
// flavour, the emulation and a host restatement produce the same bits (the step function amplifies an input ulp by 1 / eps)
DEV void fd_normalize4(double *q) {
  double n2 = add_rn(add_rn(add_rn(mul_rn(q[0], q[0]), mul_rn(q[1], q[1])), mul_rn(q[2], q[2])), mul_rn(q[3], q[3]));
  double n = sqrt(n2);
  if (n < D_MINVAL) { q[0] = 1; q[1] = 0; q[2] = 0; q[3] = 0; }
  else if (fabs(n - 1) > D_MINVAL) { q[0] = q[0] / n; q[1] = q[1] / n; q[2] = q[2] / n; q[3] = q[3] / n; }
}
DEV void fd_quat_nudge(double *q, int ax, double cs, double sn) {
  fd_normalize4(q);
  // q * [cs, sn e_ax]: the two non-zero products of every component of d_mulquat
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  double r[4];
  if (ax == 0)      { r[0] = add_rn(mul_rn(w, cs), -mul_rn(x, sn)); r[1] = add_rn(mul_rn(w, sn), mul_rn(x, cs)); r[2] = add_rn(mul_rn(y, cs), mul_rn(z, sn)); r[3] = add_rn(mul_rn(z, cs), -mul_rn(y, sn)); }
  else if (ax == 1) { r[0] = add_rn(mul_rn(w, cs), -mul_rn(y, sn)); r[1] = add_rn(mul_rn(x, cs), -mul_rn(z, sn)); r[2] = add_rn(mul_rn(w, sn), mul_rn(y, cs)); r[3] = add_rn(mul_rn(z, cs), mul_rn(x, sn)); }
  else              { r[0] = add_rn(mul_rn(w, cs), -mul_rn(z, sn)); r[1] = add_rn(mul_rn(x, cs), mul_rn(y, sn)); r[2] = add_rn(mul_rn(y, cs), -mul_rn(x, sn)); r[3] = add_rn(mul_rn(w, sn), mul_rn(z, cs)); }
  fd_normalize4(r);
  q[0] = r[0]; q[1] = r[1]; q[2] = r[2]; q[3] = r[3];
}

// element i of table row g: i < ds the state, ds <= i < ds + nu the control, i == ds + nu the time
DEV void fd_assemble(const FdArgs &a, size_t g, int i) {
  const int nq = a.nq, nv = a.nv, nd = 2 * nv + a.na, ds = nq + nv + a.na, nu = a.nu, E = fd_slots(a);
  const int t = (int)(g / (size_t)E), s = (int)(g - (size_t)t * E);
  const double *x = a.x + (size_t)t * ds, *u = a.u + (size_t)t * nu;
  if (i == ds + nu) { a.time_tab[g] = a.time[t]; return; }
  int c = -1; double sgn = 0;          // nudged column and its sign; -1: the base row
  if (s > 0) {
    if (a.centered) { c = (s - 1) >> 1; sgn = ((s - 1) & 1) ? -1.0 : 1.0; }
    else { c = s - 1; sgn = 1.0; }
    if (c >= nd) {
      const int k = c - nd;
      const int f = (a.last_is_terminal && t == a.T - 1) ? 0 : fd_nudge(a.ctrllimited[k], u[k], a.eps, a.ctrlrange[2 * k], a.ctrlrange[2 * k + 1], a.centered);
      if (a.centered) { if (!(f & (sgn > 0 ? 1 : 2))) c = -1; }
      else { if (f & 1) sgn = 1.0; else if (f & 2) sgn = -1.0; else c = -1; }
    }
  }
  if (i >= ds) {
    const int k = i - ds;
    double v = u[k];
    if (c == nd + k) v = v + sgn * a.eps;
    a.ctrl_tab[g * nu + k] = v;
    return;
  }
  double v = x[i];
  if (c >= 0 && c < nv) {
    const int qa = a.dofmap[2 * c], ax = a.dofmap[2 * c + 1];
    if (ax < 0) { if (i == qa) v = v + sgn * a.eps; }
    else if (i >= qa && i < qa + 4) {
      double q[4] = {x[qa], x[qa + 1], x[qa + 2], x[qa + 3]};
      fd_quat_nudge(q, ax, a.cs, sgn * a.sn);
      v = q[i - qa];
    }
  } else if (c >= nv && c < nd) {
    if (i == nq + (c - nv)) v = v + sgn * a.eps;        // qvel and act follow qpos in the state row in tangent order
  }
  a.state_tab[g * ds + i] = v;
}

// entry [o][c] of knot t's combined matrix: rows o < nd are A | B's (next-state tangent), rows nd <= o < nd + nr are C | D's (residual);
// columns c < nd are the state's, nd <= c < nd + nu the controls'
DEV double fd_entry(const FdArgs &a, int t, int o, int c) {
  const int nq = a.nq, nv = a.nv, nd = 2 * nv + a.na, ds = nq + nv + a.na, E = fd_slots(a);
  int sa, sb; double den = a.eps;      // (y(sb) - y(sa)) / den
  if (c < nd) {
    if (a.centered) { sb = 1 + 2 * c; sa = 2 + 2 * c; den = 2 * a.eps; }
    else { sb = 1 + c; sa = 0; }
  } else {
    const int k = c - nd;
    const int f = fd_nudge(a.ctrllimited[k], a.u[(size_t)t * a.nu + k], a.eps, a.ctrlrange[2 * k], a.ctrlrange[2 * k + 1], a.centered);
    if (!f) return 0.0;
    if (a.centered) {
      sb = (f & 1) ? 1 + 2 * c : 0; sa = (f & 2) ? 2 + 2 * c : 0;
      if (f == 3) den = 2 * a.eps;
    } else { sb = (f & 1) ? 1 + c : 0; sa = (f & 1) ? 0 : 1 + c; }
  }
  const size_t ga = (size_t)t * E + sa, gb = (size_t)t * E + sb;
  double num;
  if (o < nv) {
    const double *ya = a.next_state + ga * ds, *yb = a.next_state + gb * ds;
    const int qa = a.dofmap[2 * o], ax = a.dofmap[2 * o + 1];
    if (ax < 0) num = yb[qa] - ya[qa];
    else { double r[3]; d_subquat(r, yb + qa, ya + qa); num = r[ax]; }      // body-frame rotation vector of ya^-1 * yb
  } else if (o < nd) {
    num = a.next_state[gb * ds + nq + (o - nv)] - a.next_state[ga * ds + nq + (o - nv)];
  } else {
    num = a.residual[gb * a.nr + (o - nd)] - a.residual[ga * a.nr + (o - nd)];
  }
  return num / den;                     // an IEEE division: no reciprocal
}

// where entry [o][c] of knot t goes; null: not written (A / B / D of a terminal knot)
DEV double *fd_dest(const FdArgs &a, int t, int o, int c) {
  const int nd = 2 * a.nv + a.na, nu = a.nu, nr = a.nr;
  const bool term = a.last_is_terminal && t == a.T - 1;
  if (o < nd) {
    if (term) return nullptr;
    return c < nd ? a.A + ((size_t)t * nd + o) * nd + c : a.B + ((size_t)t * nd + o) * nu + (c - nd);
  }
  if (c < nd) return a.C + ((size_t)t * nr + (o - nd)) * nd + c;
  return term ? nullptr : a.D + ((size_t)t * nr + (o - nd)) * nu + (c - nd);
}

// OR of the warning bits of knot t's evaluations s = first, first + stride, ...
DEV int fd_failure(const FdArgs &a, int t, int first, int stride) {
  const int E = fd_slots(a);
  int w = 0;
  for (int s = first; s < E; s += stride) w |= a.fail[(size_t)t * E + s];
  return w;
}
