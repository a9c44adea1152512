// cost_derivatives.h — device side of the derivative-based planners besides the transition derivatives (transition_fd.h):
//   norm_grad_hess   Norm(g, H, x, params, n, type) of mjpc/norm.cc:50-210: value, gradient and Hessian of one cost term's norm
//   cd_*             CostDerivatives (mjpc/planners/cost_derivatives.cc:77-224): cr, cx, cu, cxx, cxu, cuu of every knot from the
//                    residual and its Jacobian J = [C | D], Gauss-Newton, with the risk transform
//   gd_*             Gradient::Compute / GradientStep (mjpc/planners/gradient/gradient.cc:43-108): the backward recursion
// The __global__ wrappers are in engine.hip; the 1-lane MJPC_EMU build (tests/emu/emu_cost_derivatives.cpp) plays the same functions
// in a single thread.
//
// Summation rule (MuJoCo's BLAS is not part of this project, so the order is defined here): every contraction starts at 0.0 and
// runs over the ascending contraction index, one rounded product and one rounded add per step, never fused; an accumulation
// `+= w * v` is one rounded product and one rounded add.  A host restatement with contraction off gives the same bits.
// Divisions and roots of the derivative formulas are the compiler's correctly rounded `/` and sqrt(), as in transition_fd.h:
// dmath.h's d_div / d_sqrt are ~1 ulp sequences on the device and exact only in the emulation, which would break that equality.
#pragma once
#include <stddef.h>
#include "spmd.h"
#include "dmath.h"

#define CD_TILE 16
#define CD_RISK_NEUTRAL 1.0e-6        // kRiskNeutralTolerance (mjpc/utilities.h)

// Hessian of types 1 (L22) and 2 (L2) is dense inside the term's block; every other type's is diagonal
DEV int norm_dense(int type) { return type == 1 || type == 2; }

// Value y (returned, spelled as residuals.h's norm_value spells it: the derivatives belong to the cost the rollouts report),
// gradient g[n], and of the Hessian: hd[n] its diagonal for a diagonal type, hs[2] the two scalars norm_hess_entry builds a dense
// type's entries from.  prm = {p, q}.
DEV double norm_grad_hess(double *g, double *hd, double *hs, const double *x, const double *prm, int n, int type) {
  const double p = prm[0], q = prm[1];
  double y = 0;
  hs[0] = 0; hs[1] = 0;
  switch (type) {
    case -1:      // kNull: g[0] = 1, H = 0
      y = x[0];
      for (int i = 0; i < n; i++) { g[i] = i == 0 ? 1.0 : 0.0; hd[i] = 0.0; }
      break;
    case 0:       // kQuadratic
      for (int i = 0; i < n; i++) { y += x[i] * x[i]; g[i] = x[i]; hd[i] = 1.0; }
      y *= 0.5;
      break;
    case 1: {     // kL22: dense, H[i][j] = b (delta_ij + x_i x_j c)
      double cq = 0, c = 0;
      for (int i = 0; i < n; i++) { cq += x[i] * x[i]; c = add_rn(c, mul_rn(x[i], x[i])); }
      { double a = pow(cq, q / 2) + pow(p, q); y = pow(a, 1 / q) - p; }
      const double a = add_rn(pow(c, q / 2), pow(p, q)), s = pow(a, 1 / q), d = pow(c, q / 2 - 1);
      const double b = mul_rn(s / a, d);
      for (int i = 0; i < n; i++) { g[i] = mul_rn(b, x[i]); hd[i] = 0.0; }
      hs[0] = b;
      hs[1] = add_rn(mul_rn(1 - q, d) / a, (q - 2) / (c > D_MINVAL ? c : D_MINVAL));      // max(c, mjMINVAL)
      break;
    }
    case 2: {     // kL2: dense, H = (I - g g') / s; s == 0 gives zeros
      double sq = 0, c = 0;
      for (int i = 0; i < n; i++) { sq += x[i] * x[i]; c = add_rn(c, mul_rn(x[i], x[i])); }
      y = sqrt(sq + p * p) - p;
      const double s = sqrt(add_rn(c, mul_rn(p, p)));
      const double inv = s ? 1.0 / s : 0.0;
      for (int i = 0; i < n; i++) { g[i] = s ? mul_rn(x[i], inv) : 0.0; hd[i] = 0.0; }
      hs[0] = s;
      break;
    }
    case 3:       // kCosh
      for (int i = 0; i < n; i++) {
        y += p * p * (cosh(x[i] / p) - 1.0);
        g[i] = mul_rn(p, sinh(x[i] / p)); hd[i] = cosh(x[i] / p);
      }
      break;
    case 5:       // kPowerLoss
      for (int i = 0; i < n; i++) {
        const double s = fabs(x[i]), sg = x[i] > 0 ? 1.0 : (x[i] < 0 ? -1.0 : 0.0);
        y += pow(s, p);
        g[i] = mul_rn(mul_rn(sg, p), pow(s, p - 1));
        hd[i] = mul_rn(mul_rn(p - 1, p), pow(s, p - 2));
      }
      break;
    case 6:       // kSmoothAbsLoss
      for (int i = 0; i < n; i++) {
        { double s = sqrt(x[i] * x[i] + p * p); y += s - p; }
        const double s = sqrt(add_rn(mul_rn(x[i], x[i]), mul_rn(p, p)));
        g[i] = s ? x[i] / s : 0.0;
        hd[i] = s ? add_rn(1.0, -mul_rn(g[i], g[i])) / s : 0.0;
      }
      break;
    case 7:       // kSmoothAbs2Loss
      for (int i = 0; i < n; i++) {
        const double a = fabs(x[i]), d = pow(a, q), e = d + pow(p, q), s = pow(e, 1 / q);
        y += s - p;
        const double c = mul_rn(s, pow(a, q - 2)) / e;
        g[i] = mul_rn(c, x[i]);
        hd[i] = mul_rn(mul_rn(c, q - 1), add_rn(1.0, -(d / e)));
      }
      break;
    case 8:       // kRectifyLoss: the p <= 0 branch is the plain rectifier
      for (int i = 0; i < n; i++) {
        if (p > 0) {
          const double s = exp(x[i] / p);
          y += p * log(1 + s);
          g[i] = s / add_rn(1.0, s);
          hd[i] = s / mul_rn(mul_rn(p, add_rn(1.0, s)), add_rn(1.0, s));
        } else {
          y += x[i] > 0 ? x[i] : 0;
          g[i] = x[i] > 0 ? 1.0 : 0.0; hd[i] = 0.0;
        }
      }
      break;
    default:
      for (int i = 0; i < n; i++) { g[i] = 0.0; hd[i] = 0.0; }
      break;
  }
  return y;
}

// entry [i][j] of a dense type's Hessian from the term's residual x, gradient g and the scalars hs of norm_grad_hess
DEV double norm_hess_entry(int type, const double *x, const double *g, const double *hs, int i, int j) {
  const double dl = i == j ? 1.0 : 0.0;
  if (type == 1) return mul_rn(hs[0], add_rn(dl, mul_rn(mul_rn(x[i], x[j]), hs[1])));
  return hs[0] ? add_rn(dl, -mul_rn(g[i], g[j])) / hs[0] : 0.0;
}

// ------------------------------------------------------------------------------ per-knot cost derivatives
struct CdArgs {
  const double *residual, *C, *D;        // [T][nr], [T][nr][nd], [T][nr][nu] (a terminal knot's D is never read)
  const int *dim_norm_residual, *norm, *num_norm_parameter;      // the engine's cost table (DevTask)
  const double *weight, *norm_parameter;
  int num_term;
  double risk;
  int T, nd, nu, nr, last_is_terminal, hessians;
  double *cr, *cx, *cu, *cxx, *cuu, *cxu;        // [T][nr], [T][nd], [T][nu], [T][nd][nd], [T][nu][nu], [T][nd][nu]; any may be null
};

// a workgroup's LDS (doubles): the knot's norm derivatives, computed once and read by every entry of the tile
struct CdLds {
  double *cr, *hd;       // [nr] norm gradient, Hessian diagonal
  double *hs;            // [num_term][2] scalars of the dense terms
  double *wy;            // [num_term] w_k * Norm_k
  double *gv;            // [2 * CD_TILE] the scaled gradient at the tile's columns, then at its rows
  double *S;             // [nr][CD_TILE] crr J of the dense term at hand, the tile's columns
};
#define CD_LDS_DOUBLES(nr, num_term) ((size_t)(2 + CD_TILE) * (size_t)(nr) + 3 * (size_t)(num_term) + 2 * CD_TILE)      // (a macro: the host sizes the launch with it)
DEV CdLds cd_lds(const CdArgs &a, double *sm) {
  CdLds L;
  L.cr = sm; L.hd = L.cr + a.nr; L.hs = L.hd + a.nr; L.wy = L.hs + 2 * a.num_term; L.gv = L.wy + a.num_term; L.S = L.gv + 2 * CD_TILE;
  return L;
}
DEV int cd_terminal(const CdArgs &a, int t) { return a.last_is_terminal && t == a.T - 1; }
DEV double cd_weight(const CdArgs &a, int k) { return a.weight[k] / (double)a.T; }        // weights[i] / T
// J[r][j] of knot t: row r of [C_t | D_t]
DEV double cd_J(const CdArgs &a, int t, int r, int j) {
  return j < a.nd ? a.C[((size_t)t * a.nr + r) * a.nd + j] : a.D[((size_t)t * a.nr + r) * a.nu + (j - a.nd)];
}
// first residual row of term k
DEV int cd_row0(const CdArgs &a, int k) { int fs = 0; for (int j = 0; j < k; j++) fs += a.dim_norm_residual[j]; return fs; }

// term k of knot t: its rows of cr / hd, its scalars, its weighted value
DEV void cd_term(const CdArgs &a, int t, int k, const CdLds &L) {
  int fs = 0, ps = 0;
  for (int j = 0; j < k; j++) { fs += a.dim_norm_residual[j]; ps += a.num_norm_parameter[j]; }
  double prm[2] = {0, 0};
  for (int j = 0; j < a.num_norm_parameter[k] && j < 2; j++) prm[j] = a.norm_parameter[ps + j];
  const double y = norm_grad_hess(L.cr + fs, L.hd + fs, L.hs + 2 * k, a.residual + (size_t)t * a.nr + fs, prm, a.dim_norm_residual[k], a.norm[k]);
  L.wy[k] = mul_rn(cd_weight(a, k), y);
}
// exp(risk * c), c the sum of the weighted norms in ascending term order; 1 below the risk-neutral tolerance (no transform)
DEV double cd_risk_scale(const CdArgs &a, const CdLds &L) {
  if (fabs(a.risk) < CD_RISK_NEUTRAL) return 1.0;
  double c = 0;
  for (int k = 0; k < a.num_term; k++) c = add_rn(c, L.wy[k]);
  return exp(mul_rn(a.risk, c));
}
// element j of [cx | cu] of knot t, risk-scaled: sum over the terms of w_k (J_k' cr_k)[j]
DEV double cd_gradient(const CdArgs &a, int t, int j, const CdLds &L, double s) {
  if (j >= a.nd && cd_terminal(a, t)) return 0.0;
  double acc = 0;
  int fs = 0;
  for (int k = 0; k < a.num_term; k++) {
    const int ni = a.dim_norm_residual[k];
    double g = 0;
    for (int r = fs; r < fs + ni; r++) g = add_rn(g, mul_rn(cd_J(a, t, r, j), L.cr[r]));
    acc = add_rn(acc, mul_rn(cd_weight(a, k), g));
    fs += ni;
  }
  return fabs(a.risk) < CD_RISK_NEUTRAL ? acc : mul_rn(acc, s);
}
// S[r][j] = (crr_k J_k)[r][j] of dense term k (rows fs .. fs + ni), r relative to fs
DEV double cd_S_dense(const CdArgs &a, int t, int k, int fs, int ni, int r, int j, const CdLds &L) {
  const double *x = a.residual + (size_t)t * a.nr + fs;
  double s = 0;
  for (int q = 0; q < ni; q++) s = add_rn(s, mul_rn(norm_hess_entry(a.norm[k], x, L.cr + fs, L.hs + 2 * k, r, q), cd_J(a, t, fs + q, j)));
  return s;
}
// (J_k' S)[i][j]; jj = j's place in the tile (the staged S of a dense term)
DEV double cd_G(const CdArgs &a, int t, int fs, int ni, int dense, int i, int j, int jj, const CdLds &L) {
  double G = 0;
  if (dense) for (int r = 0; r < ni; r++) G = add_rn(G, mul_rn(cd_J(a, t, fs + r, i), L.S[r * CD_TILE + jj]));
  else for (int r = fs; r < fs + ni; r++) G = add_rn(G, mul_rn(cd_J(a, t, r, i), mul_rn(L.hd[r], cd_J(a, t, r, j))));
  return G;
}
// entry [i][j] of knot t's (nd + nu)^2 matrix: cxx top-left, cxu top-right, cuu bottom-right; null: not stored (the bottom-left block, a
// null output, and everything outside cxx of a terminal knot, which is zeroed by cd_zero_terminal)
DEV double *cd_dest(const CdArgs &a, int t, int i, int j) {
  const int nd = a.nd, nu = a.nu, n = nd + nu;
  if (i >= n || j >= n) return nullptr;
  if ((i >= nd || j >= nd) && cd_terminal(a, t)) return nullptr;
  if (i < nd) {
    if (j < nd) return a.cxx ? a.cxx + ((size_t)t * nd + i) * nd + j : nullptr;
    return a.cxu ? a.cxu + ((size_t)t * nd + i) * nu + (j - nd) : nullptr;
  }
  if (j < nd) return nullptr;
  return a.cuu ? a.cuu + ((size_t)t * nu + (i - nd)) * nu + (j - nd) : nullptr;
}
// the risk transform of a Hessian entry (cost_derivatives.cc:160-224).  gi, gj are the gradient elements ALREADY scaled by s: the
// reference scales cx and cu first and forms the outer products from the scaled vectors, so the second term carries s^3 where the
// derivative of exp(risk c) has s.  That is the reference's order (a quirk); it is kept.
DEV double cd_risk_entry(const CdArgs &a, double H, double gi, double gj, double s) {
  if (fabs(a.risk) < CD_RISK_NEUTRAL) return H;
  return add_rn(mul_rn(H, s), mul_rn(mul_rn(gi, gj), mul_rn(a.risk, s)));
}
// the blocks of a terminal knot that have no D: entry e of cuu (which = 0) / cxu (which = 1)
DEV void cd_zero_terminal(const CdArgs &a, int which, size_t e) {
  const int t = a.T - 1;
  if (which == 0) { if (a.cuu && e < (size_t)a.nu * a.nu) a.cuu[(size_t)t * a.nu * a.nu + e] = 0.0; }
  else if (a.cxu && e < (size_t)a.nd * a.nu) a.cxu[(size_t)t * a.nd * a.nu + e] = 0.0;
}

// ------------------------------------------------------------------------------ backward recursion
struct GdArgs {
  const double *A, *B;       // [T - 1][nd][nd], [T - 1][nd][nu] (blocks of a longer array: stride per knot is the block's own size)
  const double *cx, *cu;     // [T][nd], [T][nu]
  int T, nd, nu;
  double *k, *Vx, *Qx, *Qu, *dV;        // [T][nu], [T][nd], [T - 1][nd], [T - 1][nu], [2]
};
// The block [A_{t-1} | B_{t-1}] (nd rows of nd + nu) is what a step reads, and none of it depends on the chain.  The workgroup keeps the
// block of the step at hand in LDS and fetches the NEXT step's block into registers (GD_R elements per thread, whole segments) before
// the chain starts; the registers go to LDS behind the chain.  So the loads of A_{t-2} / B_{t-2} are in flight while step t - 1 adds.
#define GD_THREADS 256
#define GD_R 32                       // block elements a thread stages: blocks up to GD_THREADS * GD_R doubles (64 KB) take the LDS path
#define GD_U 8
DEV int gd_staged(const GdArgs &a) { return (size_t)a.nd * (a.nd + a.nu) <= (size_t)GD_THREADS * GD_R; }
// element idx = r * (nd + nu) + c of the block of step t (t >= 1): A_{t-1}[r][c] or B_{t-1}[r][c - nd]
DEV double gd_block(const GdArgs &a, int t, int idx) {
  const int nd = a.nd, nu = a.nu, n = nd + nu, r = idx / n, c = idx - r * n;
  return c < nd ? a.A[((size_t)(t - 1) * nd + r) * nd + c] : a.B[((size_t)(t - 1) * nd + r) * nu + (c - nd)];
}
// column c of [A_{t-1} | B_{t-1}]' Vx_t, then + cx_{t-1} / cu_{t-1}: Qx (c < nd) or Qu.  vx: Vx_t (LDS).  blk: the block in LDS (lanes
// read consecutive doubles of a row: no bank conflicts), or null: straight from memory, GD_U rows' loads issued together
DEV double gd_column(const GdArgs &a, int t, int c, const double *vx, const double *blk) {
  const int nd = a.nd, nu = a.nu, n = nd + nu;
  double q = 0;
  if (blk) {
#pragma unroll 8
    for (int r = 0; r < nd; r++) q = add_rn(q, mul_rn(blk[r * n + c], vx[r]));
  } else {
    const double *M = c < nd ? a.A + (size_t)(t - 1) * nd * nd + c : a.B + (size_t)(t - 1) * nd * nu + (c - nd);
    const int ld = c < nd ? nd : nu;
    int r = 0;
    for (; r + GD_U <= nd; r += GD_U) {
      double m[GD_U];
#pragma unroll
      for (int u = 0; u < GD_U; u++) m[u] = M[(size_t)(r + u) * ld];
#pragma unroll
      for (int u = 0; u < GD_U; u++) q = add_rn(q, mul_rn(m[u], vx[r + u]));
    }
    for (; r < nd; r++) q = add_rn(q, mul_rn(M[(size_t)r * ld], vx[r]));
  }
  return add_rn(q, c < nd ? a.cx[(size_t)(t - 1) * nd + c] : a.cu[(size_t)(t - 1) * nu + (c - nd)]);
}
// dV[0] += k . Qu of step t - 1 in ascending element order (qu: Qu_{t-1}, k = -Qu)
DEV double gd_dv(const GdArgs &a, const double *qu, double dv) {
  double d = 0;
  for (int i = 0; i < a.nu; i++) d = add_rn(d, mul_rn(-qu[i], qu[i]));
  return add_rn(dv, d);
}
