// inverse_fd.h — finite-difference derivatives of the inverse dynamics around the inverse kernel (inverse.h):
//   ifd_assemble   the perturbed (state, ctrl, time, qacc) table of a group of configurations from the nominal rows
//   ifd_entry      one entry of the six blocks df/dq, df/dv, df/da, ds/dq, ds/dv, ds/da (f = qfrc_inverse, s = the residual)
// Contract: MuJoCo's mjd_inverseFD as mjpc/direct/direct.cc:1717-1756 calls it, with entry [i][j] = d out_i / d in_j (transition_fd.h's
// convention; mjd_inverseFD stores the transpose).  Positions are nudged along tangent c by transition_fd.h's own rule
// (fd_quat_nudge for a quaternion dof), so a state row here has the bits of the same nudge there.  Activations and controls are not
// differentiated.  The __global__ wrappers are in engine.hip; the 1-lane MJPC_EMU build (tests/emu/emu_inverse.cpp) runs the same
// functions in a single thread.
//
// Evaluation slots of configuration t (E per configuration, table row t * E + s), columns c < nv: q, nv <= c < 2 nv: v, 2 nv <= c < 3 nv: a
//   one-sided  E = 1 + 3 nv    s = 0 base; s = 1 + c: column c at +eps
//   centred    E = 1 + 6 nv    s = 0 base; s = 1 + 2c: column c at +eps; s = 2 + 2c: at -eps
#pragma once
#include "transition_fd.h"

struct InvFdArgs {
  const double *x, *u, *a, *time;    // nominal rows of the group: [T][ds], [T][nu], [T][nv], [T]
  const int *dofmap;                 // [nv][2], as FdArgs::dofmap
  int T, nq, nv, na, nu, nr, centered;
  double eps, cs, sn;                // cs / sn = cos / sin of eps / 2, from the host's libm
  double *state_tab, *ctrl_tab, *time_tab, *qacc_tab;            // [T * E] rows the inverse kernel reads
  const double *qfrc, *residual; const int *fail;                 // [T * E] rows the inverse kernel wrote
  double *DfDq, *DfDv, *DfDa, *DsDq, *DsDv, *DsDa;                // [T] blocks, row-major [nv][nv] / [nr][nv]; null: not wanted
  int *failure;                      // [T]: OR of the warning bits of every evaluation at t
};

DEV int ifd_slots(const InvFdArgs &a) { return a.centered ? 1 + 6 * a.nv : 1 + 3 * a.nv; }
// elements of a table row: the state, the control, the time, the acceleration
DEV int ifd_row_elements(const InvFdArgs &a) { return a.nq + a.nv + a.na + a.nu + 1 + a.nv; }

// element i of table row g: i < ds the state, ds <= i < ds + nu the control, i == ds + nu the time, then the nv accelerations
DEV void ifd_assemble(const InvFdArgs &a, size_t g, int i) {
  const int nq = a.nq, nv = a.nv, ds = nq + nv + a.na, nu = a.nu, E = ifd_slots(a);
  const int t = (int)(g / (size_t)E), s = (int)(g - (size_t)t * E);
  const double *x = a.x + (size_t)t * ds;
  if (i == ds + nu) { a.time_tab[g] = a.time[t]; return; }
  if (i >= ds && i < ds + nu) { a.ctrl_tab[g * nu + (i - ds)] = a.u[(size_t)t * nu + (i - ds)]; return; }
  int c = -1; double sgn = 0;          // nudged column and its sign; -1: the base row
  if (s > 0) {
    if (a.centered) { c = (s - 1) >> 1; sgn = ((s - 1) & 1) ? -1.0 : 1.0; }
    else { c = s - 1; sgn = 1.0; }
  }
  if (i > ds + nu) {
    const int k = i - (ds + nu + 1);
    double v = a.a[(size_t)t * nv + k];
    if (c == 2 * nv + k) v = v + sgn * a.eps;
    a.qacc_tab[g * nv + k] = v;
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
  } else if (c >= nv && c < 2 * nv) {
    if (i == nq + (c - nv)) v = v + sgn * a.eps;
  }
  a.state_tab[g * ds + i] = v;
}

// where entry [o][c] of configuration t goes: rows o < nv are f's, rows nv <= o < nv + nr the residual's; columns as the slots.
// null: that block is not wanted
DEV double *ifd_dest(const InvFdArgs &a, int t, int o, int c) {
  const int nv = a.nv, nr = a.nr, blk = c / nv, j = c - blk * nv;
  if (o < nv) {
    double *B = blk == 0 ? a.DfDq : (blk == 1 ? a.DfDv : a.DfDa);
    return B ? B + ((size_t)t * nv + o) * nv + j : nullptr;
  }
  double *B = blk == 0 ? a.DsDq : (blk == 1 ? a.DsDv : a.DsDa);
  return B ? B + ((size_t)t * nr + (o - nv)) * nv + j : nullptr;
}

DEV double ifd_entry(const InvFdArgs &a, int t, int o, int c) {
  const int nv = a.nv, E = ifd_slots(a);
  int sa, sb; double den = a.eps;      // (y(sb) - y(sa)) / den
  if (a.centered) { sb = 1 + 2 * c; sa = 2 + 2 * c; den = 2 * a.eps; }
  else { sb = 1 + c; sa = 0; }
  const size_t ga = (size_t)t * E + sa, gb = (size_t)t * E + sb;
  double num;
  if (o < nv) num = a.qfrc[gb * nv + o] - a.qfrc[ga * nv + o];
  else num = a.residual[gb * a.nr + (o - nv)] - a.residual[ga * a.nr + (o - nv)];
  return num / den;                     // an IEEE division: no reciprocal
}

// OR of the warning bits of configuration t's evaluations s = first, first + stride, ...
DEV int ifd_failure(const InvFdArgs &a, int t, int first, int stride) {
  const int E = ifd_slots(a);
  int w = 0;
  for (int s = first; s < E; s += stride) w |= a.fail[(size_t)t * E + s];
  return w;
}
