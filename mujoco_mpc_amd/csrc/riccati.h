// riccati.h — device side of the iLQG backward pass (mjpc/planners/ilqg/backward_pass.cc, boxqp.h, planner.cc:429-520):
//   rc_chol / rc_cholsolve   dense Cholesky of a principal submatrix and the two triangular solves
//   rc_boxqp                 box-constrained QP by projected Newton steps (this project's definition, below)
//   rc_step                  RiccatiStep (backward_pass.cc:65-250): Q blocks, regularisation, gains, cost-to-go of one knot
//   rc_backward              the sweep t = T-2 .. 0 inside the regularisation loop of planner.cc:429-520 / ScaleRegularization
// The __global__ wrapper (rc_backward_kernel) is in engine.hip: ONE workgroup, the chain in t is serial, so the threads share the
// entries of each matrix phase: `for (e = tid; e < entries; e += nth)` between workgroup barriers.  The 1-lane MJPC_EMU build
// (tests/emu/emu_riccati.cpp) plays rc_backward with tid = 0, nth = 1: the same phases in the same order, in one thread.
//
// Summation rule: that of cost_derivatives.h.  Every contraction starts at 0.0 and runs over the ascending contraction index, one
// rounded product and one rounded add per step, never fused; `/` and sqrt() are the compiler's correctly rounded ones.  The host
// restatement (csrc/planner.cc, compiled without contraction) gives the same bits.
//
// Kept from the reference: K is solved from the UNREGULARISED Qxu in both branches (with limits, on the free set, with the factor of
// the regularised H_free; clamped controls get zero rows); the `if (mu)` guard around control / state-control regularisation;
// value regularisation is formed even when mu == 0.  The reference also forms Qxu_reg and never reads it; it is not formed here.
//
// Cholesky (mju_cholFactor's place): left-looking, L[j][j] = sqrt(H[j][j] - sum_k L[j][k]^2), L[i][j] = (H[i][j] - sum_k L[i][k] L[j][k])
// / L[j][j]; a pivot that is not > 0 (NaN included) is a failure ("rank below m").
//
// Box-QP (mju_boxQP's place; MuJoCo is not part of this project, so this is the project's own definition of the documented
// projected-Newton method, Tassa, Mansard, Todorov 2014; the four constants are as recalled from MuJoCo, not checked against it):
//   minimise 0.5 x'Hx + g'x over lower <= x <= upper, from the warm start clamped into the box.  Per iteration: gradient g + Hx; the
//   clamped set is {x_i = lower_i and grad_i > 0} or {x_i = upper_i and grad_i < 0}; H_free is refactored only when the set changed
//   (not positive definite: -1); stop when the squared norm of the free gradient < 1e-16; Newton direction -H_free^-1 grad_free on the
//   free set; Armijo backtracking on the clamped candidate: accept when value(candidate) - value <= 0.1 * step * (direction . grad),
//   else step *= 0.5, giving up below 1e-22; at most 100 iterations.  Returns the number of free dimensions, index[] lists them
//   ascending and R [nfree][nfree] (row-major, lower triangle, zeros above) is the factor of H_free.
#pragma once
#include <stddef.h>
#include "spmd.h"

#define RC_THREADS 256
#define RC_QP_MAXITER 100
#define RC_QP_MINGRAD 1.0e-16
#define RC_QP_BACKTRACK 0.5
#define RC_QP_ARMIJO 0.1
#define RC_QP_MINSTEP 1.0e-22

#ifdef MJPC_EMU
#define RC_BAR() ((void)0)
#else
#define RC_BAR() __syncthreads()
#endif

// factor of H[index][index] (H has leading dimension ldh) into R [nf][nf]; 0: a pivot is not > 0
DEV int rc_chol(double *R, const double *H, int ldh, const int *index, int nf) {
  for (int j = 0; j < nf; j++) {
    double s = 0;
    for (int k = 0; k < j; k++) s = add_rn(s, mul_rn(R[j * nf + k], R[j * nf + k]));
    const double d = add_rn(H[index[j] * ldh + index[j]], -s);
    if (!(d > 0)) return 0;
    const double l = sqrt(d);
    R[j * nf + j] = l;
    for (int i = j + 1; i < nf; i++) {
      double q = 0;
      for (int k = 0; k < j; k++) q = add_rn(q, mul_rn(R[i * nf + k], R[j * nf + k]));
      R[i * nf + j] = add_rn(H[index[i] * ldh + index[j]], -q) / l;
      R[j * nf + i] = 0.0;
    }
  }
  return 1;
}
// x = (L L')^-1 b, L the lower triangle of R [nf][nf]; x may be b
DEV void rc_cholsolve(double *x, const double *R, int nf, const double *b) {
  for (int i = 0; i < nf; i++) {
    double s = 0;
    for (int k = 0; k < i; k++) s = add_rn(s, mul_rn(R[i * nf + k], x[k]));
    x[i] = add_rn(b[i], -s) / R[i * nf + i];
  }
  for (int i = nf - 1; i >= 0; i--) {
    double s = 0;
    for (int k = i + 1; k < nf; k++) s = add_rn(s, mul_rn(R[k * nf + i], x[k]));
    x[i] = add_rn(x[i], -s) / R[i * nf + i];
  }
}
DEV double rc_clamp(double v, double lo, double hi) { v = v < hi ? v : hi; return v > lo ? v : lo; }
// 0.5 x'Hx + g'x
DEV double rc_qp_value(const double *H, const double *g, int n, const double *x) {
  double q = 0, l = 0;
  for (int i = 0; i < n; i++) {
    double s = 0;
    for (int j = 0; j < n; j++) s = add_rn(s, mul_rn(H[i * n + j], x[j]));
    q = add_rn(q, mul_rn(x[i], s));
    l = add_rn(l, mul_rn(x[i], g[i]));
  }
  return add_rn(mul_rn(0.5, q), l);
}
// res [n]: warm start in, solution out.  mask [n] ints and scr [4 n] doubles are scratch.
DEV int rc_boxqp(double *res, double *R, int *index, int *mask, const double *H, const double *g, int n, const double *lower, const double *upper, double *scr) {
  double *grad = scr, *search = scr + n, *cand = scr + 2 * n, *y = scr + 3 * n;
  for (int i = 0; i < n; i++) { res[i] = rc_clamp(res[i], lower[i], upper[i]); mask[i] = -1; }
  double value = rc_qp_value(H, g, n, res);
  int nf = 0;
  for (int iter = 0; iter < RC_QP_MAXITER; iter++) {
    int changed = 0;
    nf = 0;
    for (int i = 0; i < n; i++) {
      double s = 0;
      for (int j = 0; j < n; j++) s = add_rn(s, mul_rn(H[i * n + j], res[j]));
      grad[i] = add_rn(g[i], s);
      const int c = (res[i] == lower[i] && grad[i] > 0) || (res[i] == upper[i] && grad[i] < 0);
      if (mask[i] != c) changed = 1;
      mask[i] = c;
      if (!c) index[nf++] = i;
    }
    if (nf == 0) break;
    if (changed && !rc_chol(R, H, n, index, nf)) return -1;
    double gn = 0;
    for (int i = 0; i < nf; i++) gn = add_rn(gn, mul_rn(grad[index[i]], grad[index[i]]));
    if (gn < RC_QP_MINGRAD) break;
    for (int i = 0; i < nf; i++) y[i] = grad[index[i]];
    rc_cholsolve(y, R, nf, y);
    for (int i = 0; i < n; i++) search[i] = 0.0;
    double sdotg = 0;
    for (int i = 0; i < nf; i++) { search[index[i]] = -y[i]; sdotg = add_rn(sdotg, mul_rn(-y[i], grad[index[i]])); }
    if (!(sdotg < 0)) break;
    double step = 1.0, nv = value;
    int accepted = 0;
    while (step >= RC_QP_MINSTEP) {
      for (int i = 0; i < n; i++) cand[i] = rc_clamp(add_rn(res[i], mul_rn(step, search[i])), lower[i], upper[i]);
      nv = rc_qp_value(H, g, n, cand);
      if (add_rn(nv, -value) <= mul_rn(RC_QP_ARMIJO, mul_rn(step, sdotg))) { accepted = 1; break; }
      step = mul_rn(step, RC_QP_BACKTRACK);
    }
    if (!accepted) break;
    for (int i = 0; i < n; i++) res[i] = cand[i];
    value = nv;
  }
  return nf;
}

// ScaleRegularization (backward_pass.cc:327-338) on r = {regularization, regularization_rate}
DEV void rc_scale_regularization(double *r, double factor, double reg_min, double reg_max) {
  const double s = mul_rn(r[1], factor);
  if (factor > 1) r[1] = s > factor ? s : factor;
  else r[1] = s < factor ? s : factor;
  double v = mul_rn(r[0], r[1]);
  v = v > reg_min ? v : reg_min;
  r[0] = v < reg_max ? v : reg_max;
}

// ------------------------------------------------------------------------------ the backward pass
struct RcArgs {
  const double *A, *B;                     // [T-1][nd][nd], [T-1][nd][nu]
  const double *cx, *cu, *cxx, *cxu, *cuu; // [T][nd], [T][nu], [T][nd][nd], [T][nd][nu], [T][nu][nu] (of index T-1 only cx, cxx are read)
  const double *actions, *limits;          // [T-1][nu], [nu][2] (read only when action_limits == 1)
  int T, nd, nu, reg_type, action_limits, max_iter;
  double reg_min, reg_max, reg_factor;
  double *reg;                             // [2] in / out: regularization, regularization_rate
  double *k, *K, *Vx, *Vxx;                // [T][nu], [T][nu][nd], [T][nd], [T][nd][nd]
  double *Qx, *Qu, *Qxx, *Qxu, *Quu;       // [T-1][..]
  double *dV;                              // [2]
  int *status;                             // [3]: complete, failing time index (-1 when complete), regularisation increases
  double *scratch;                         // the work image in global memory when it does not fit the workgroup's LDS (rc_fits), else unused
};
// The work image (doubles), in LDS when it fits and else in a global scratch of the same layout: three nd x nd matrices (Vxx_{t+1};
// A'Vxx, later Qxu K; Qxx, later the unsymmetrised Vxx), four nd x nu ones, three nu x nu ones, the vectors of the serial part.
struct RcWork {
  double *W, *tmp, *P;            // [nd][nd]
  double *tmp2, *Qxu, *K, *QK;    // [nu][nd] (B'Vxx, later a column scratch of the gain solves), [nd][nu], [nu][nd], [nu][nd]
  double *Quu, *H, *R;            // [nu][nu]
  double *wx, *qx;                // [nd] Vx_{t+1} (then Vx_t), Qx
  double *qu, *kk, *t2, *res, *lower, *upper, *qp;   // [nu] each, qp [4 nu]
  double *dv, *ctl;               // [2], [2]: step ok, free dimensions
  int *index, *mask;              // [nu] each
};
#define RC_WORK_DOUBLES(nd, nu) (3 * (size_t)(nd) * (nd) + 4 * (size_t)(nd) * (nu) + 3 * (size_t)(nu) * (nu) + 2 * (size_t)(nd) + 11 * (size_t)(nu) + 4)
#define RC_LDS_LIMIT (160 * 1024)
DEV int rc_fits(int nd, int nu) { return RC_WORK_DOUBLES(nd, nu) * sizeof(double) <= RC_LDS_LIMIT; }
DEV RcWork rc_work(int nd, int nu, double *p) {
  const size_t nn = (size_t)nd * nd, nm = (size_t)nd * nu, mm = (size_t)nu * nu;
  RcWork w;
  w.W = p; w.tmp = w.W + nn; w.P = w.tmp + nn;
  w.tmp2 = w.P + nn; w.Qxu = w.tmp2 + nm; w.K = w.Qxu + nm; w.QK = w.K + nm;
  w.Quu = w.QK + nm; w.H = w.Quu + mm; w.R = w.H + mm;
  w.wx = w.R + mm; w.qx = w.wx + nd;
  w.qu = w.qx + nd; w.kk = w.qu + nu; w.t2 = w.kk + nu; w.res = w.t2 + nu; w.lower = w.res + nu; w.upper = w.lower + nu; w.qp = w.upper + nu;
  w.dv = w.qp + 4 * nu; w.ctl = w.dv + 2;
  w.index = (int *)(w.ctl + 2); w.mask = w.index + nu;      // 2 nu ints in nu doubles
  return w;
}

// Vxx_{t+1}[k][j], with mu on the diagonal for value regularisation
DEV double rc_wreg(const RcWork &w, int n, int k, int j, double mu) { const double v = w.W[k * n + j]; return k == j ? add_rn(v, mu) : v; }

// one knot.  Returns 1, or 0 when the control solve failed (uniform over the threads); barriers inside.
DEV int rc_step(const RcArgs &a, const RcWork &w, int t, double mu, int tid, int nth) {
  const int n = a.nd, m = a.nu, nn = n * n, nm = n * m, mm = m * m;
  const double *A = a.A + (size_t)t * nn, *B = a.B + (size_t)t * nm;
  // phase 1: A'Vxx, B'Vxx, Qx, Qu
  for (int e = tid; e < nn + nm + n + m; e += nth) {
    if (e < nn) {
      const int i = e / n, j = e - i * n;
      double s = 0;
      for (int k = 0; k < n; k++) s = add_rn(s, mul_rn(A[k * n + i], w.W[k * n + j]));
      w.tmp[e] = s;
    } else if (e < nn + nm) {
      const int f = e - nn, i = f / n, j = f - i * n;
      double s = 0;
      for (int k = 0; k < n; k++) s = add_rn(s, mul_rn(B[k * m + i], w.W[k * n + j]));
      w.tmp2[f] = s;
    } else if (e < nn + nm + n) {
      const int i = e - nn - nm;
      double s = 0;
      for (int k = 0; k < n; k++) s = add_rn(s, mul_rn(A[k * n + i], w.wx[k]));
      s = add_rn(s, a.cx[(size_t)t * n + i]);
      w.qx[i] = s; a.Qx[(size_t)t * n + i] = s;
    } else {
      const int i = e - nn - nm - n;
      double s = 0;
      for (int k = 0; k < n; k++) s = add_rn(s, mul_rn(B[k * m + i], w.wx[k]));
      s = add_rn(s, a.cu[(size_t)t * m + i]);
      w.qu[i] = s; a.Qu[(size_t)t * m + i] = s;
    }
  }
  RC_BAR();
  // phase 2: Qxx, Qxu, Quu; the gain starts as zeros
  for (int e = tid; e < nn + nm + mm; e += nth) {
    if (e < nn) {
      const int i = e / n, j = e - i * n;
      double s = 0;
      for (int k = 0; k < n; k++) s = add_rn(s, mul_rn(w.tmp[i * n + k], A[k * n + j]));
      s = add_rn(s, a.cxx[(size_t)t * nn + e]);
      w.P[e] = s; a.Qxx[(size_t)t * nn + e] = s;
    } else if (e < nn + nm) {
      const int f = e - nn, i = f / m, j = f - i * m;
      double s = 0;
      for (int k = 0; k < n; k++) s = add_rn(s, mul_rn(w.tmp[i * n + k], B[k * m + j]));
      s = add_rn(s, a.cxu[(size_t)t * nm + f]);
      w.Qxu[f] = s; a.Qxu[(size_t)t * nm + f] = s;
      w.K[f] = 0.0;
    } else {
      const int f = e - nn - nm, i = f / m, j = f - i * m;
      double s = 0;
      for (int k = 0; k < n; k++) s = add_rn(s, mul_rn(w.tmp2[i * n + k], B[k * m + j]));
      s = add_rn(s, a.cuu[(size_t)t * mm + f]);
      w.Quu[f] = s; a.Quu[(size_t)t * mm + f] = s;
    }
  }
  RC_BAR();
  // phase 3: Quu_reg into H
  if (a.reg_type == 2) {
    for (int f = tid; f < nm; f += nth) {
      const int i = f / n, j = f - i * n;
      double s = 0;
      for (int k = 0; k < n; k++) s = add_rn(s, mul_rn(B[k * m + i], rc_wreg(w, n, k, j, mu)));
      w.tmp2[f] = s;
    }
    RC_BAR();
  }
  for (int f = tid; f < mm; f += nth) {
    const int i = f / m, j = f - i * m;
    double h = w.Quu[f];
    if (a.reg_type == 2) {
      double s = 0;
      for (int k = 0; k < n; k++) s = add_rn(s, mul_rn(w.tmp2[i * n + k], B[k * m + j]));
      h = add_rn(s, a.cuu[(size_t)t * mm + f]);
    } else if (mu) {
      if (a.reg_type == 0) { if (i == j) h = add_rn(h, mu); }
      else if (a.reg_type == 1) {
        double s = 0;
        for (int k = 0; k < n; k++) s = add_rn(s, mul_rn(B[k * m + i], B[k * m + j]));
        h = add_rn(h, mul_rn(s, mu));
      }
    }
    w.H[f] = h;
  }
  RC_BAR();
  // phase 4 (one thread): the control solve, k, dV
  if (tid == 0) {
    int nf = m, ok = 1;
    if (a.action_limits == 1) {
      for (int i = 0; i < m; i++) {
        w.lower[i] = add_rn(a.limits[2 * i], -a.actions[(size_t)t * m + i]);
        w.upper[i] = add_rn(a.limits[2 * i + 1], -a.actions[(size_t)t * m + i]);
      }
      nf = rc_boxqp(w.res, w.R, w.index, w.mask, w.H, w.qu, m, w.lower, w.upper, w.qp);
      if (nf < 0) ok = 0;
      else for (int i = 0; i < m; i++) w.kk[i] = w.res[i];
    } else {
      for (int i = 0; i < m; i++) w.index[i] = i;
      ok = rc_chol(w.R, w.H, m, w.index, m);
      if (ok) { rc_cholsolve(w.kk, w.R, m, w.qu); for (int i = 0; i < m; i++) w.kk[i] = -w.kk[i]; }
    }
    if (ok) {
      double d0 = 0, d1 = 0;
      for (int i = 0; i < m; i++) {
        a.k[(size_t)t * m + i] = w.kk[i];
        d0 = add_rn(d0, mul_rn(w.kk[i], w.qu[i]));
        double s = 0;
        for (int j = 0; j < m; j++) s = add_rn(s, mul_rn(w.Quu[i * m + j], w.kk[j]));
        d1 = add_rn(d1, mul_rn(w.kk[i], s));
        w.t2[i] = add_rn(s, w.qu[i]);
      }
      w.dv[0] = add_rn(w.dv[0], d0);
      w.dv[1] = add_rn(w.dv[1], mul_rn(0.5, d1));
    }
    w.ctl[0] = ok; w.ctl[1] = nf;
  }
  RC_BAR();
  const int ok = (int)w.ctl[0], nf = (int)w.ctl[1];
  if (!ok) {           // the reference has zeroed this knot's gain before it fails
    for (int f = tid; f < nm; f += nth) a.K[(size_t)t * nm + f] = 0.0;
    RC_BAR();
    return 0;
  }
  // phase 5: the gain's columns on the free set, one solve per state column (the scratch column lives in tmp2's place)
  for (int j = tid; j < n; j += nth) {
    double *y = w.tmp2 + j * m;
    for (int i = 0; i < nf; i++) y[i] = w.Qxu[j * m + w.index[i]];
    rc_cholsolve(y, w.R, nf, y);
    for (int i = 0; i < nf; i++) w.K[w.index[i] * n + j] = -y[i];
  }
  RC_BAR();
  // phase 6: Quu K, Qxu K, Vx; the gain goes out
  for (int e = tid; e < nm + nn + n; e += nth) {
    if (e < nm) {
      const int r = e / n, j = e - r * n;
      double s = 0;
      for (int q = 0; q < m; q++) s = add_rn(s, mul_rn(w.Quu[r * m + q], w.K[q * n + j]));
      w.QK[e] = s;
      a.K[(size_t)t * nm + e] = w.K[e];
    } else if (e < nm + nn) {
      const int f = e - nm, i = f / n, j = f - i * n;
      double s = 0;
      for (int r = 0; r < m; r++) s = add_rn(s, mul_rn(w.Qxu[i * m + r], w.K[r * n + j]));
      w.tmp[f] = s;
    } else {
      const int i = e - nm - nn;
      double s = 0, q = 0;
      for (int r = 0; r < m; r++) s = add_rn(s, mul_rn(w.K[r * n + i], w.t2[r]));
      for (int j = 0; j < m; j++) q = add_rn(q, mul_rn(w.Qxu[i * m + j], w.kk[j]));
      const double v = add_rn(add_rn(w.qx[i], s), q);
      w.wx[i] = v; a.Vx[(size_t)t * n + i] = v;
    }
  }
  RC_BAR();
  // phase 7: (Qxx + K'QuuK) + (QxuK + (QxuK)')
  for (int e = tid; e < nn; e += nth) {
    const int i = e / n, j = e - i * n;
    double s = 0;
    for (int r = 0; r < m; r++) s = add_rn(s, mul_rn(w.K[r * n + i], w.QK[r * n + j]));
    w.P[e] = add_rn(add_rn(w.P[e], s), add_rn(w.tmp[i * n + j], w.tmp[j * n + i]));
  }
  RC_BAR();
  // phase 8: symmetrised into Vxx_t
  for (int e = tid; e < nn; e += nth) {
    const int i = e / n, j = e - i * n;
    const double v = mul_rn(0.5, add_rn(w.P[i * n + j], w.P[j * n + i]));
    w.W[e] = v; a.Vxx[(size_t)t * nn + e] = v;
  }
  RC_BAR();
  return 1;
}

// the whole call.  Every thread of the workgroup runs it (tid of nth); the emulation runs it once with tid = 0, nth = 1.
DEV void rc_backward(const RcArgs &a, const RcWork &w, int tid, int nth) {
  const int n = a.nd, m = a.nu, nn = n * n, nm = n * m, T = a.T;
  double reg[2] = {a.reg[0], a.reg[1]};
  int iter = 0, done = 0, failed = -1;
  for (int e = tid; e < n; e += nth) a.Vx[(size_t)(T - 1) * n + e] = a.cx[(size_t)(T - 1) * n + e];
  for (int e = tid; e < nn; e += nth) a.Vxx[(size_t)(T - 1) * nn + e] = a.cxx[(size_t)(T - 1) * nn + e];
  for (int e = tid; e < m; e += nth) w.res[e] = 0.0;             // the box-QP's warm start: zero at the start of a call
  if (tid == 0) { w.dv[0] = 0.0; w.dv[1] = 0.0; }
  RC_BAR();            // (the inputs' a.reg has been read by everybody before thread 0 stores the result below: it stores after later barriers)
  while (iter < a.max_iter && !done) {
    if (tid == 0) { w.dv[0] = 0.0; w.dv[1] = 0.0; }
    for (int e = tid; e < n; e += nth) w.wx[e] = a.cx[(size_t)(T - 1) * n + e];
    for (int e = tid; e < nn; e += nth) w.W[e] = a.cxx[(size_t)(T - 1) * nn + e];
    RC_BAR();
    failed = -1;
    for (int t = T - 2; t >= 0; t--)
      if (!rc_step(a, w, t, reg[0], tid, nth)) { failed = t; break; }
    if (failed < 0) {
      done = 1;
      for (int e = tid; e < m; e += nth) a.k[(size_t)(T - 1) * m + e] = a.k[(size_t)(T - 2) * m + e];
      for (int e = tid; e < nm; e += nth) a.K[(size_t)(T - 1) * nm + e] = a.K[(size_t)(T - 2) * nm + e];    // (stored by this same thread in phase 6)
    } else if (reg[0] <= a.reg_max) {
      rc_scale_regularization(reg, a.reg_factor, a.reg_min, a.reg_max);
      iter++;
    } else break;      // (the reference would spin here: its loop neither scales nor counts once the regularisation exceeds the maximum)
  }
  if (tid == 0) {
    a.reg[0] = reg[0]; a.reg[1] = reg[1];
    a.dV[0] = w.dv[0]; a.dV[1] = w.dv[1];
    a.status[0] = done; a.status[1] = done ? -1 : failed; a.status[2] = iter;
  }
}
