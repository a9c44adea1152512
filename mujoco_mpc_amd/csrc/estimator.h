// estimator.h — the unscented filter's moments around the one-step kernel (transition.h):
//   ukf_sigma            the sigma-point table (state, ctrl, time rows the step kernel reads) from the mean state and a Cholesky factor
//   ukf_mean_component   weighted mean of one next-state / sensor component over the stepped rows
//   ukf_quat_mean        the mean of one quaternion joint (principal eigenvector of the weighted outer-product matrix)
//   ukf_diff             one entry of the difference table d[2nd+1][nd+ns] (tangent-space state part, sensor part)
//   ukf_cov_*            the three covariance blocks, a 16 x 16 tile of the combined matrix [[ss, sy], [sy', yy]] per workgroup
// Contract: mjpc/estimators/unscented.cc (SigmaPoints :293, EvaluateSigmaPoints :353, SigmaPointDifferences :397, SigmaCovariances
// :425, QuaternionMeans :578).  Rows i < nd are x (+) c_i, rows nd + i are x (-) c_i with c_i = sigma_step * L[:, i], row 2nd is x: the
// reference's order, the nominal point last.  The __global__ wrappers are in engine.hip; the 1-lane MJPC_EMU build
// (tests/emu/emu_estimator.cpp) runs the same functions in a single thread.  (+) on a quaternion is ukf_quatintegrate below: the engine's
// d_quatintegrate in a spelling whose bits do not depend on who computes it.
//
// Summation rule: every sum over sigma points runs over the ASCENDING row index with one separately rounded product and one
// separately rounded add per step (mul_rn / add_rn), so a host loop in the same order gives the same bits.  That is why the
// covariance is not an f64 MFMA: its internal summation order is not this one.
//
// Two additions to the reference in ukf_quat_mean, both about what PrincipalEigenVector4 (utilities.cc:1459) leaves open:
//   sign    an eigenvector is defined up to sign and the reference takes what the formula gives; here the sign is chosen so that the
//           dot product with the NOMINAL row's next quaternion is >= 0 (q and -q are the same rotation, but the difference table is
//           taken against the stored numbers and the next update starts from them).
//   order   the formula divides by the eigenvector's LAST component, which is 0 / 0 when that component vanishes (for the [w x y z]
//           order: every rotation about an axis in the x-y plane, the identity included).  The matrix is therefore permuted cyclically
//           so that the last slot is the nominal quaternion's largest component; the result is permuted back.  The method is unchanged.
#pragma once
#include <stddef.h>
#include "spmd.h"
#include "dmath.h"

struct UkfArgs {
  const double *x, *L, *u;           // mean state [ds], lower Cholesky factor [nd][nd] row-major (entries above the diagonal not read), ctrl [nu]
  const int *dofmap;                 // [nv][2]: qpos address of dof d's coordinate (of w for a quaternion), axis 0..2 of a quaternion dof or -1
  const int *qmap;                   // [nq][2]: dof of position coordinate i (first rotational dof for a quaternion), component 0..3 of a quaternion or -1
  int nq, nv, na, nu, nr, ns, first; // nr: the engine's residual rows; the measurement is rows [first, first + ns)
  double sigma_step, time, w_mean0, w_cov0, w_sigma;
  double *state_tab, *ctrl_tab, *time_tab;                // [2nd+1] rows the step kernel reads
  const double *next_state, *residual; const int *fail;   // [2nd+1] rows the step kernel wrote
  const double *noise_process, *noise_sensor;             // [nd], [ns]: the diagonals of the ss and yy blocks
  double *state_mean, *sensor_mean, *diff;                // [ds], [ns], [2nd+1][nd+ns]
  double *cov_ss, *cov_sy, *cov_yy;                       // [nd][nd], [nd][ns], [ns][ns]
  int *failure;                                           // OR of the rows' warning bits
};

// ---- the position integration of a quaternion, q <- normalise(normalise(q) * exp(scale * vel)): d_quatintegrate (dmath.h) restated with
// separately rounded operations, IEEE sqrt / divide and its own sin / cos (d_sincos's reduction and polynomials, uncontracted), so that
// the device, the emulation and a host restatement (planner.cc, tests/estimator_mirror.py) produce the SAME BITS, as fd_quat_nudge does
// for the finite differences.  The step function can amplify an ulp of a sigma point by 1e6 and more (the A1's contacts): a table that
// differs in the last place between two implementations makes everything behind the step incomparable.
DEV void ukf_sincos(double x, double *sn, double *cs) {
  if (!(fabs(x) < 64.0)) { *sn = sin(x); *cs = cos(x); return; }       // (no sigma point turns that far)
  const double k = rint(mul_rn(x, 0.63661977236758134308));
  const double r = add_rn(add_rn(x, -mul_rn(k, 1.57079632673412561417e+00)), -mul_rn(k, 6.07710050650619224932e-11));
  const double z = mul_rn(r, r);
  double ps = 1.58969099521155010221e-10, pc = -1.13596475577881948265e-11;
  const double S[5] = {-2.50507602534068634195e-08, 2.75573137070700676789e-06, -1.98412698298579493134e-04, 8.33333333332248946124e-03, -1.66666666666666324348e-01};
  const double C[5] = {2.08757232129817482790e-09, -2.75573143513906633035e-07, 2.48015872894767294178e-05, -1.38888888888741095749e-03, 4.16666666666666019037e-02};
  for (int i = 0; i < 5; i++) { ps = add_rn(S[i], mul_rn(z, ps)); pc = add_rn(C[i], mul_rn(z, pc)); }
  const double s = add_rn(r, mul_rn(mul_rn(r, z), ps));
  const double c = add_rn(add_rn(1.0, -mul_rn(0.5, z)), mul_rn(mul_rn(z, z), pc));
  const int q = ((int)k) & 3;
  const double s1 = (q & 1) ? c : s, c1 = (q & 1) ? s : c;
  *sn = (q & 2) ? -s1 : s1;
  *cs = ((q + 1) & 2) ? -c1 : c1;
}
DEV void ukf_normalize4(double *q) {
  double n2 = add_rn(add_rn(add_rn(mul_rn(q[0], q[0]), mul_rn(q[1], q[1])), mul_rn(q[2], q[2])), mul_rn(q[3], q[3]));
  double n = sqrt(n2);
  if (n < D_MINVAL) { q[0] = 1; q[1] = 0; q[2] = 0; q[3] = 0; }
  else if (fabs(n - 1) > D_MINVAL) { q[0] = q[0] / n; q[1] = q[1] / n; q[2] = q[2] / n; q[3] = q[3] / n; }
}
DEV void ukf_quatintegrate(double *q, const double *vel, double scale) {
  double ax[3] = {vel[0], vel[1], vel[2]};
  const double n = sqrt(add_rn(add_rn(mul_rn(ax[0], ax[0]), mul_rn(ax[1], ax[1])), mul_rn(ax[2], ax[2])));
  if (n < D_MINVAL) { ax[0] = 1; ax[1] = 0; ax[2] = 0; }
  else { ax[0] = ax[0] / n; ax[1] = ax[1] / n; ax[2] = ax[2] / n; }
  const double angle = mul_rn(scale, n);
  double b[4] = {1, 0, 0, 0};
  if (angle != 0) {
    double sn, cs;
    ukf_sincos(mul_rn(angle, 0.5), &sn, &cs);
    b[0] = cs; b[1] = mul_rn(ax[0], sn); b[2] = mul_rn(ax[1], sn); b[3] = mul_rn(ax[2], sn);
  }
  ukf_normalize4(q);
  const double a[4] = {q[0], q[1], q[2], q[3]};
  // d_mulquat's terms, left to right
  q[0] = add_rn(add_rn(add_rn(mul_rn(a[0], b[0]), -mul_rn(a[1], b[1])), -mul_rn(a[2], b[2])), -mul_rn(a[3], b[3]));
  q[1] = add_rn(add_rn(add_rn(mul_rn(a[0], b[1]), mul_rn(a[1], b[0])), mul_rn(a[2], b[3])), -mul_rn(a[3], b[2]));
  q[2] = add_rn(add_rn(add_rn(mul_rn(a[0], b[2]), -mul_rn(a[1], b[3])), mul_rn(a[2], b[0])), mul_rn(a[3], b[1]));
  q[3] = add_rn(add_rn(add_rn(mul_rn(a[0], b[3]), mul_rn(a[1], b[2])), -mul_rn(a[2], b[1])), mul_rn(a[3], b[0]));
  ukf_normalize4(q);
}

DEV int ukf_nd(const UkfArgs &a) { return 2 * a.nv + a.na; }
DEV int ukf_rows(const UkfArgs &a) { return 2 * ukf_nd(a) + 1; }
// element k of c_col = sigma_step * L[:, col]
DEV double ukf_col(const UkfArgs &a, int col, int k) { return k >= col ? mul_rn(a.sigma_step, a.L[(size_t)k * ukf_nd(a) + col]) : 0.0; }

// element i of table row g: i < ds the state, ds <= i < ds + nu the control, i == ds + nu the time
DEV void ukf_sigma(const UkfArgs &a, int g, int i) {
  const int nq = a.nq, nv = a.nv, nd = ukf_nd(a), ds = nq + nv + a.na, nu = a.nu;
  if (i == ds + nu) { a.time_tab[g] = a.time; return; }
  if (i >= ds) { a.ctrl_tab[(size_t)g * nu + (i - ds)] = a.u[i - ds]; return; }
  double v = a.x[i];
  if (g < 2 * nd) {
    const int col = g < nd ? g : g - nd;
    const double sgn = g < nd ? 1.0 : -1.0;          // the position integration's "time"
    if (i < nq) {
      const int d = a.qmap[2 * i], k = a.qmap[2 * i + 1];
      if (k < 0) v = add_rn(v, sgn * ukf_col(a, col, d));
      else {
        // each lane of a quaternion recomputes its four numbers
        double q[4] = {a.x[i - k], a.x[i - k + 1], a.x[i - k + 2], a.x[i - k + 3]};
        const double w[3] = {ukf_col(a, col, d), ukf_col(a, col, d + 1), ukf_col(a, col, d + 2)};
        ukf_quatintegrate(q, w, sgn);
        v = q[k];
      }
    } else v = add_rn(v, sgn * ukf_col(a, col, nv + (i - nq)));       // qvel and act follow qpos in tangent order
  }
  a.state_tab[(size_t)g * ds + i] = v;
}

DEV double ukf_weight_cov(const UkfArgs &a, int j) { return j < 2 * ukf_nd(a) ? a.w_sigma : a.w_cov0; }

// component i < ds of the state mean, ds <= i < ds + ns of the sensor mean (a quaternion's components are replaced by ukf_quat_mean).
// A lane's sum is serial, its loads are not: UKF_LOADS rows are fetched before they are added, in the same order
#define UKF_LOADS 8
DEV double ukf_mean_component(const UkfArgs &a, int i) {
  const int ds = a.nq + a.nv + a.na, nd = ukf_nd(a), R = 2 * nd + 1;
  const double *p = i < ds ? a.next_state + i : a.residual + a.first + (i - ds);
  const size_t stride = i < ds ? (size_t)ds : (size_t)a.nr;
  double acc = 0.0;
  for (int j0 = 0; j0 < R; j0 += UKF_LOADS) {
    double y[UKF_LOADS];
#ifndef MJPC_EMU
#pragma unroll
#endif
    for (int k = 0; k < UKF_LOADS; k++) y[k] = j0 + k < R ? p[(size_t)(j0 + k) * stride] : 0.0;
#ifndef MJPC_EMU
#pragma unroll
#endif
    for (int k = 0; k < UKF_LOADS; k++)
      if (j0 + k < R) acc = add_rn(acc, mul_rn(y[k], j0 + k < 2 * nd ? a.w_sigma : a.w_mean0));
  }
  return acc;
}

// principal eigenvector of the symmetric traceless 4 x 4 matrix m (row-major) by the method of PrincipalEigenVector4: Newton on the
// characteristic quartic from x0, then the QUEST eigenvector [X, gamma], normalised
DEV void ukf_eigenvector4(double *res, const double *m, double x0) {
  const double Z[3] = {m[3], m[7], m[11]};
  const double S[9] = {m[0] + m[15], m[1], m[2], m[4], m[5] + m[15], m[6], m[8], m[9], m[10] + m[15]};
  const double A = S[0], B = S[1], Cc = S[2], D = S[3], E = S[4], F = S[5], G = S[6], H = S[7], I = S[8];
  const double delta = A * (E * I - F * H) - B * (D * I - F * G) + Cc * (D * H - E * G);
  // kappa = trace(adj S) = trace(delta * S^-1)
  const double kappa = (E * I - F * H) + (A * I - Cc * G) + (A * E - B * D);
  const double sigma = 0.5 * (S[0] + S[4] + S[8]), sigma2 = sigma * sigma;
  double SZ[3]; d_mulmatvec3(SZ, S, Z);
  const double d = d_dot3(SZ, SZ), c = delta + d_dot3(Z, SZ), b = sigma2 + d_dot3(Z, Z), a_ = sigma2 - kappa;
  double x = x0;
  const double ab = a_ + b, bias = a_ * b + c * sigma - d;
  for (int it = 0; it < 10; it++) {
    const double x2 = x * x, x3 = x2 * x, x4 = x3 * x;
    const double num = x4 - ab * x2 - c * x + bias, den = 4.0 * x3 - 2.0 * ab * x - c;
    x -= num / den;
  }
  const double alpha = x * x - sigma2 + kappa, beta = x - sigma, gamma = (x + sigma) * alpha - delta;
  double X[3]; d_mulmatvec3(X, S, SZ);
  d_addtoscl3(X, SZ, beta); d_addtoscl3(X, Z, alpha);
  const double scl = 1.0 / sqrt(gamma * gamma + d_dot3(X, X));
  res[0] = scl * X[0]; res[1] = scl * X[1]; res[2] = scl * X[2]; res[3] = scl * gamma;
}

// the mean of the quaternion at qpos address qa: K = sum_j 4 w_j q_j q_j' - (sum_j w_j) I with the covariance weights, ascending j
DEV void ukf_quat_mean(const UkfArgs &a, int qa, double *out) {
  const int ds = a.nq + a.nv + a.na, nd = ukf_nd(a), R = 2 * nd + 1;
  double K[16];
  for (int e = 0; e < 16; e++) K[e] = 0.0;
  for (int j0 = 0; j0 < R; j0 += 4) {          // four rows' loads in flight, added in row order
    double q[4][4];
#ifndef MJPC_EMU
#pragma unroll
#endif
    for (int k = 0; k < 4; k++) {
      const double *src = a.next_state + (size_t)(j0 + k < R ? j0 + k : R - 1) * ds + qa;
      q[k][0] = src[0]; q[k][1] = src[1]; q[k][2] = src[2]; q[k][3] = src[3];
    }
#ifndef MJPC_EMU
#pragma unroll
#endif
    for (int k = 0; k < 4; k++) {
      if (j0 + k >= R) break;
      const double w4 = 4.0 * ukf_weight_cov(a, j0 + k);
      for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) K[4 * r + c] = add_rn(K[4 * r + c], mul_rn(mul_rn(q[k][r], q[k][c]), w4));
    }
  }
  const double total = a.w_cov0 + (R - 1) * a.w_sigma;
  K[0] -= total; K[5] -= total; K[10] -= total; K[15] -= total;
  const double *qn = a.next_state + (size_t)(R - 1) * ds + qa;      // the nominal row's next quaternion
  int p = 0;
  for (int k = 1; k < 4; k++) if (fabs(qn[k]) > fabs(qn[p])) p = k;
  const int idx[4] = {(p + 1) & 3, (p + 2) & 3, (p + 3) & 3, p};
  double m[16], v[4];
  for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) m[4 * r + c] = K[4 * idx[r] + idx[c]];
  ukf_eigenvector4(v, m, 12.0);
  double dot = 0.0;
  for (int r = 0; r < 4; r++) { out[idx[r]] = v[r]; dot += v[r] * qn[idx[r]]; }
  if (dot < 0) { out[0] = -out[0]; out[1] = -out[1]; out[2] = -out[2]; out[3] = -out[3]; }
}

// entry [j][k] of the difference table: k < nd the state's tangent (d_subquat on quaternion coordinates), nd <= k the sensors'
DEV double ukf_diff(const UkfArgs &a, int j, int k) {
  const int nq = a.nq, nv = a.nv, nd = ukf_nd(a), ds = nq + nv + a.na;
  const double *y = a.next_state + (size_t)j * ds;
  if (k < nv) {
    const int qa = a.dofmap[2 * k], ax = a.dofmap[2 * k + 1];
    if (ax < 0) return y[qa] - a.state_mean[qa];
    double r[3]; d_subquat(r, y + qa, a.state_mean + qa);      // body-frame rotation vector of mean^-1 * y
    return r[ax];
  }
  if (k < nd) return y[nq + (k - nv)] - a.state_mean[nq + (k - nv)];
  return a.residual[(size_t)j * a.nr + a.first + (k - nd)] - a.sensor_mean[k - nd];
}

// OR of the warning bits of rows first, first + stride, ...
DEV int ukf_failure(const UkfArgs &a, int first, int stride) {
  int w = 0;
  for (int j = first; j < ukf_rows(a); j += stride) w |= a.fail[j];
  return w;
}

// ---- covariance tiles.  Thread th of a 256-thread workgroup stages element th % 16 of difference row j0 + th / 16 for the tile's
// rows (ta) and columns (tb): 16 consecutive doubles of a row each, so the global reads run along rows.  Then thread (ri, ci) =
// (th / 16, th % 16) adds the chunk's 16 sigma points to entry (r0 + ri, c0 + ci).
#define UKF_TILE 16
DEV double *ukf_cov_dest(const UkfArgs &a, int r, int c) {
  const int nd = ukf_nd(a), ns = a.ns;
  if (r >= nd + ns || c >= nd + ns) return nullptr;
  if (r < nd) return c < nd ? a.cov_ss + (size_t)r * nd + c : a.cov_sy + (size_t)r * ns + (c - nd);
  return c >= nd ? a.cov_yy + (size_t)(r - nd) * ns + (c - nd) : nullptr;      // the lower-left block is sy', not stored
}
DEV double ukf_cov_init(const UkfArgs &a, int r, int c) {
  const int nd = ukf_nd(a);
  if (r != c || r >= nd + a.ns) return 0.0;
  return r < nd ? a.noise_process[r] : a.noise_sensor[r - nd];
}
DEV void ukf_cov_stage(const UkfArgs &a, int j0, int r0, int c0, int th, double *ta, double *tb) {
  const int n = ukf_nd(a) + a.ns, j = j0 + th / UKF_TILE, e = th % UKF_TILE;
  const bool row = j < ukf_rows(a);
  ta[th] = (row && r0 + e < n) ? a.diff[(size_t)j * n + r0 + e] : 0.0;
  tb[th] = (row && c0 + e < n) ? a.diff[(size_t)j * n + c0 + e] : 0.0;
}
DEV double ukf_cov_accum(const UkfArgs &a, int j0, int ri, int ci, const double *ta, const double *tb, double acc) {
  const int R = ukf_rows(a);
  for (int jj = 0; jj < UKF_TILE && j0 + jj < R; jj++)
    acc = add_rn(acc, mul_rn(mul_rn(ta[jj * UKF_TILE + ri], tb[jj * UKF_TILE + ci]), ukf_weight_cov(a, j0 + jj)));
  return acc;
}
