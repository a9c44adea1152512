// tests/emu/emu_estimator.cpp — TEST INFRASTRUCTURE ONLY.
// The unscented-moments kernels (mujoco_mpc_amd/csrc/estimator.h) in the 1-lane emulation mode, in the launch sequence of
// mjpc_hip_unscented_moments (engine.hip): the sigma table element by element, the step kernel over the table (emu_transition.cpp's
// player, included below), ukf_mean_kernel's three phases in order, and ukf_cov_kernel tile by tile and chunk by chunk through
// NaN-poisoned staging tiles, so that an entry accumulated from a slot nobody staged shows up.  Never loaded by the product.
#include "emu_transition.cpp"
#include "../../mujoco_mpc_amd/csrc/estimator.h"

namespace {
struct Maps { std::vector<int> dofmap, qmap; };
Maps build_maps(const MjpcHipModel *m) {
  Maps M;
  M.dofmap.assign(2 * m->nv + 2, -1); M.qmap.assign(2 * m->nq + 2, -1);
  for (int j = 0; j < m->njnt; j++) {
    const int type = m->jnt_type[j], qa = m->jnt_qposadr[j], da = m->jnt_dofadr[j];
    if (type == 0) {
      for (int k = 0; k < 3; k++) { M.dofmap[2 * (da + k)] = qa + k; M.dofmap[2 * (da + k) + 1] = -1; M.dofmap[2 * (da + 3 + k)] = qa + 3; M.dofmap[2 * (da + 3 + k) + 1] = k; }
      for (int k = 0; k < 3; k++) { M.qmap[2 * (qa + k)] = da + k; M.qmap[2 * (qa + k) + 1] = -1; }
      for (int k = 0; k < 4; k++) { M.qmap[2 * (qa + 3 + k)] = da + 3; M.qmap[2 * (qa + 3 + k) + 1] = k; }
    } else if (type == 1) {
      for (int k = 0; k < 3; k++) { M.dofmap[2 * (da + k)] = qa; M.dofmap[2 * (da + k) + 1] = k; }
      for (int k = 0; k < 4; k++) { M.qmap[2 * (qa + k)] = da; M.qmap[2 * (qa + k) + 1] = k; }
    } else { M.dofmap[2 * da] = qa; M.dofmap[2 * da + 1] = -1; M.qmap[2 * qa] = da; M.qmap[2 * qa + 1] = -1; }
  }
  return M;
}
}  // namespace

// the sigma-point table alone: state_tab [2nd+1][ds], ctrl_tab [2nd+1][nu], time_tab [2nd+1]
extern "C" int emu_ukf_sigma(const MjpcHipModel *m, const double *x, const double *L, const double *u, double sigma_step, double time,
                             double *state_tab, double *ctrl_tab, double *time_tab) {
  Maps M = build_maps(m);
  UkfArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.L = L; a.u = u; a.dofmap = M.dofmap.data(); a.qmap = M.qmap.data();
  a.nq = m->nq; a.nv = m->nv; a.na = m->na; a.nu = m->nu; a.sigma_step = sigma_step; a.time = time;
  a.state_tab = state_tab; a.ctrl_tab = ctrl_tab; a.time_tab = time_tab;
  const int R = ukf_rows(a), n = m->nq + m->nv + m->na + m->nu + 1;
  for (int g = 0; g < R; g++) for (int i = 0; i < n; i++) ukf_sigma(a, g, i);
  return 0;
}

extern "C" int emu_unscented_moments(const MjpcHipModel *m, const MjpcHipTask *t, const double *x, const double *L, double sigma_step,
                                     const double *weights, const double *u, double time, const double *mocap, const double *noise_process,
                                     const double *noise_sensor, int first, int ns, double *state_mean, double *sensor_mean, double *cov_ss,
                                     double *cov_sy, double *cov_yy, double *sigma_next, double *diff, int *failure) {
  Emu E;
  if (!E.init(m, t, mocap)) return -1;
  Maps M = build_maps(m);
  const int nq = m->nq, nv = m->nv, na = m->na, nu = m->nu, nr = t->num_residual, ds = nq + nv + na, nd = 2 * nv + na, R = 2 * nd + 1, n = nd + ns;
  const double nan = 0.0 / 0.0;
  std::vector<double> st((size_t)R * ds, nan), ct((size_t)R * nu + 1, nan), tt(R, nan), rs((size_t)R * nr + 1, nan);
  std::vector<int> fl(R, -1);
  UkfArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.L = L; a.u = u; a.dofmap = M.dofmap.data(); a.qmap = M.qmap.data();
  a.nq = nq; a.nv = nv; a.na = na; a.nu = nu; a.nr = nr; a.ns = ns; a.first = first;
  a.sigma_step = sigma_step; a.time = time; a.w_mean0 = weights[0]; a.w_cov0 = weights[1]; a.w_sigma = weights[2];
  a.state_tab = st.data(); a.ctrl_tab = ct.data(); a.time_tab = tt.data(); a.next_state = sigma_next; a.residual = rs.data(); a.fail = fl.data();
  a.noise_process = noise_process; a.noise_sensor = noise_sensor;
  a.state_mean = state_mean; a.sensor_mean = sensor_mean; a.diff = diff; a.cov_ss = cov_ss; a.cov_sy = cov_sy; a.cov_yy = cov_yy; a.failure = failure;
  for (int g = 0; g < R; g++) for (int i = 0; i < ds + nu + 1; i++) ukf_sigma(a, g, i);
  E.step((size_t)R, st.data(), ct.data(), tt.data(), sigma_next, rs.data(), fl.data());
  // ukf_mean_kernel: components, then quaternions, then the difference table and the warning bits
  for (int i = 0; i < ds + ns; i++) { const double v = ukf_mean_component(a, i); if (i < ds) state_mean[i] = v; else sensor_mean[i - ds] = v; }
  for (int i = 0; i < nq; i++)
    if (a.qmap[2 * i + 1] == 0) { double q[4]; ukf_quat_mean(a, i, q); for (int k = 0; k < 4; k++) state_mean[i + k] = q[k]; }
  for (int e = 0; e < R * n; e++) diff[e] = ukf_diff(a, e / n, e % n);
  *failure = ukf_failure(a, 0, 1);
  // ukf_cov_kernel
  const int TH = UKF_TILE * UKF_TILE;
  for (int r0 = 0; r0 < n; r0 += UKF_TILE)
    for (int c0 = 0; c0 < n; c0 += UKF_TILE) {
      if (r0 >= nd && c0 + UKF_TILE <= nd) continue;
      double acc[UKF_TILE * UKF_TILE];
      for (int th = 0; th < TH; th++) acc[th] = ukf_cov_init(a, r0 + th / UKF_TILE, c0 + th % UKF_TILE);
      for (int j0 = 0; j0 < R; j0 += UKF_TILE) {
        double ta[UKF_TILE * UKF_TILE], tb[UKF_TILE * UKF_TILE];
        for (int th = 0; th < TH; th++) { ta[th] = nan; tb[th] = nan; }
        for (int th = 0; th < TH; th++) ukf_cov_stage(a, j0, r0, c0, th, ta, tb);
        for (int th = 0; th < TH; th++) acc[th] = ukf_cov_accum(a, j0, th / UKF_TILE, th % UKF_TILE, ta, tb, acc[th]);
      }
      for (int th = 0; th < TH; th++) { double *d = ukf_cov_dest(a, r0 + th / UKF_TILE, c0 + th % UKF_TILE); if (d) *d = acc[th]; }
    }
  return 0;
}

// ukf_quat_mean over given next-state rows [2nd+1][nq+nv+na] with the quaternion at qpos address qa
extern "C" void emu_ukf_quat_mean(int nq, int nv, int na, int qa, const double *next_state, double w_cov0, double w_sigma, double *out) {
  UkfArgs a;
  memset(&a, 0, sizeof(a));
  a.nq = nq; a.nv = nv; a.na = na; a.next_state = next_state; a.w_cov0 = w_cov0; a.w_sigma = w_sigma;
  ukf_quat_mean(a, qa, out);
}
