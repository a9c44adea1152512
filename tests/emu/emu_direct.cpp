// tests/emu/emu_direct.cpp — TEST INFRASTRUCTURE ONLY.
// The direct optimiser's window cost (mujoco_mpc_amd/csrc/direct_cost.h) in the 1-lane emulation mode: emu_direct_assemble plays the five
// dc_* kernels of engine.hip (norms, totals, chain rule, norm Hessian times block, gradient and band) workgroup by workgroup and thread by
// thread in the kernels' phase order, the chain rule through a NaN-poisoned LDS image, onto NaN-poisoned work arrays, so that an entry
// read before it was written, or never written, shows up.  Never loaded by the product.
#define MJPC_EMU 1
#include <vector>
#include "../../mujoco_mpc_amd/csrc/direct_cost.h"
#include "../../include/mjpc_hip.h"

static void give(double *dst, const std::vector<double> &src) { if (dst) for (size_t i = 0; i < src.size(); i++) dst[i] = src[i]; }

extern "C" int emu_direct_assemble(int T, int nv, int nr, const MjpcHipDirectSettings *s, const double *residual_sensor, const double *residual_force,
                                   const double *DfDq, const double *DfDv, const double *DfDa, const double *DsDq, const double *DsDv, const double *DsDa,
                                   const double *dvdq0, const double *dvdq1, double *cost, double *gradient, double *hessian_band, double *block_sensor,
                                   double *block_force, double *norm_gradient_sensor, double *norm_gradient_force, double *residual_sensor_out,
                                   double *residual_force_out) {
  if (!s || s->struct_size != (int)sizeof(MjpcHipDirectSettings) || T < 3 || nv < 1) return -1;
  const size_t Tz = T, n = nv, m = s->num_sensor, ns = s->num_sensor_rows, nb = 3 * n, no = ns + n;
  std::vector<int> first(m + 1), row_sensor(ns + 1);
  size_t rows = 0;
  for (size_t i = 0; i < m; i++) { first[i] = (int)rows; for (int r = 0; r < s->sensor_dim[i] && rows + r < ns; r++) row_sensor[rows + r] = (int)i; rows += s->sensor_dim[i]; }
  if (rows != ns || s->sensor_first_row < 0 || s->sensor_first_row + (int)ns > nr) return -1;
  const double nan = 0.0 / 0.0;
  std::vector<double> res_s(Tz * ns, nan), ng_s(Tz * ns, nan), hd_s(Tz * ns, nan), hs_s(2 * Tz * m, nan), w_s(Tz * m, nan), wy_s(Tz * m, nan);
  std::vector<double> res_f(Tz * n, nan), ng_f(Tz * n, nan), y_f(Tz, nan), Js(Tz * ns * nb, nan), Jf(Tz * n * nb, nan), NJs(Tz * ns * nb, nan), NJf(Tz * n * nb, nan);
  std::vector<double> band(Tz * n * nb, nan), grad(Tz * n, nan), cst(3, nan);
  DcArgs a;
  a.T = T; a.nv = nv; a.nr = nr; a.ns = (int)ns; a.row0 = s->sensor_first_row; a.num_sensor = (int)m;
  a.dim = s->sensor_dim; a.first = first.data(); a.stage = s->sensor_stage; a.norm = s->sensor_norm; a.row_sensor = row_sensor.data();
  a.prm = s->sensor_norm_parameter; a.noise_sensor = s->noise_sensor; a.noise_process = s->noise_process; a.mask = s->sensor_mask;
  a.sensor_flag = s->sensor_flag ? 1 : 0; a.force_flag = s->force_flag ? 1 : 0; a.time_scaling_sensor = s->time_scaling_sensor ? 1 : 0;
  a.time_scaling_force = s->time_scaling_force ? 1 : 0; a.first_pos = s->first_step_position_sensors ? 1 : 0;
  a.last_pos = s->last_step_position_sensors ? 1 : 0; a.last_vel = s->last_step_velocity_sensors ? 1 : 0; a.h = s->timestep;
  a.rs = residual_sensor; a.rf = residual_force; a.V0 = dvdq0; a.V1 = dvdq1;
  a.Df[0] = DfDq; a.Df[1] = DfDv; a.Df[2] = DfDa; a.Ds[0] = DsDq; a.Ds[1] = DsDv; a.Ds[2] = DsDa;
  a.res_s = res_s.data(); a.ng_s = ng_s.data(); a.hd_s = hd_s.data(); a.hs_s = hs_s.data(); a.w_s = w_s.data(); a.wy_s = wy_s.data();
  a.res_f = res_f.data(); a.ng_f = ng_f.data(); a.y_f = y_f.data(); a.Js = Js.data(); a.Jf = Jf.data(); a.NJs = NJs.data(); a.NJf = NJf.data();
  a.gradient = grad.data(); a.band = band.data(); a.cost = cst.data();
  // dc_norm_kernel
  for (int t = 0; t < T; t++) {
    for (int i = 0; i < a.num_sensor; i++) dc_norm_sensor(a, t, i);
    for (int i = 0; i < nv; i++) dc_norm_force(a, t, i);
    a.y_f[t] = dc_force_value(a, t);
  }
  // dc_cost_kernel
  { const double p0 = dc_cost_part(a, 0), p1 = dc_cost_part(a, 1); a.cost[0] = add_rn(p0, p1); a.cost[1] = p0; a.cost[2] = p1; }
  // dc_block_kernel
  const int NT = DC_TILE * DC_TILE;
  std::vector<double> sm(DC_TILE_DOUBLES), p1(NT), p2(NT);
  for (int t = 0; t < T; t++)
    for (int o0 = 0; o0 < (int)no; o0 += DC_TILE)
      for (int c0 = 0; c0 < (int)nb; c0 += DC_TILE) {
        for (auto &v : sm) v = nan;
        const DcTiles L = dc_tiles(sm.data());
        for (int tid = 0; tid < NT; tid++) { p1[tid] = 0; p2[tid] = 0; }
        for (int k0 = 0; k0 < nv; k0 += DC_TILE) {
          for (int tid = 0; tid < NT; tid++) dc_block_stage(a, t, o0, c0, k0, tid, L);
          for (int tid = 0; tid < NT; tid++) dc_block_accum(a, k0, tid, L, p1[tid], p2[tid]);
        }
        for (int tid = 0; tid < NT; tid++) dc_block_store(a, t, o0, c0, tid, p1[tid], p2[tid]);
      }
  // dc_nj_kernel, dc_entry_kernel
  for (size_t e = 0; e < Tz * no * nb; e++) dc_nj(a, e);
  for (size_t e = 0; e < Tz * n * (nb + 1); e++) dc_entry(a, e);
  give(cost, cst); give(gradient, grad); give(hessian_band, band); give(block_sensor, Js); give(block_force, Jf);
  give(norm_gradient_sensor, ng_s); give(norm_gradient_force, ng_f); give(residual_sensor_out, res_s); give(residual_force_out, res_f);
  return 0;
}

// dc_window_kernel and dc_vblock_kernel: the windows' rows (state, control, time, acceleration per row w T + t) and window 0's velocity
// blocks (V0, V1 may be null), onto the caller's NaN-poisoned arrays
extern "C" int emu_direct_window(int nwin, int T, int nq, int nv, int na, int nu, double h, const int *dofmap, const double *q, const double *act,
                                 const double *ctrl, const double *time, double *x, double *u, double *a, double *tm, double *V0, double *V1) {
  DcWinArgs w;
  w.q = q; w.act = act; w.ctrl = ctrl; w.time = time; w.dofmap = dofmap; w.nwin = nwin; w.T = T; w.nq = nq; w.nv = nv; w.na = na; w.nu = nu; w.h = h;
  w.x = x; w.u = u; w.a = a; w.tm = tm; w.V0 = V0; w.V1 = V1;
  const int n = nq + nv + na + nu + 1 + nv;
  for (size_t g = 0; g < (size_t)nwin * T; g++) for (int i = 0; i < n; i++) dc_window_row(w, g, i);
  if (V0 && V1) for (size_t e = 0; e < (size_t)T * nv * nv; e++) dc_velocity_block(w, e);
  return 0;
}

// dc_residual_kernel, then dc_norm_kernel and dc_cost_kernel over nwin windows (the value call's tail, the windows through dc_window()):
// residual [nwin T E][nr] and qfrc [nwin T E][nv] are the inverse evaluations' rows, slot 0 of every E the base.  rs [nwin T][ns],
// rf [nwin T][nv] and cost [nwin][3] come back; work arrays NaN-poisoned
extern "C" int emu_direct_value(int nwin, int T, int nv, int nr, int E, const MjpcHipDirectSettings *s, const double *residual, const double *qfrc,
                                const double *y_s, const double *y_f, double *rs, double *rf, double *cost) {
  if (!s || s->struct_size != (int)sizeof(MjpcHipDirectSettings) || T < 3 || nv < 1 || nwin < 1) return -1;
  const size_t R = (size_t)nwin * T, n = nv, m = s->num_sensor, ns = s->num_sensor_rows;
  std::vector<int> first(m + 1), row_sensor(ns + 1);
  size_t rows = 0;
  for (size_t i = 0; i < m; i++) { first[i] = (int)rows; for (int r = 0; r < s->sensor_dim[i] && rows + r < ns; r++) row_sensor[rows + r] = (int)i; rows += s->sensor_dim[i]; }
  if (rows != ns) return -1;
  DcResArgs r;
  r.residual = residual; r.qfrc = qfrc; r.y_s = y_s; r.y_f = y_f; r.T = T; r.nv = nv; r.nr = nr; r.ns = (int)ns; r.row0 = s->sensor_first_row; r.E = E; r.rs = rs; r.rf = rf;
  for (size_t e = 0; e < R * (ns + n); e++) dc_residual(r, e);
  const double nan = 0.0 / 0.0;
  std::vector<double> res_s(R * ns, nan), ng_s(R * ns, nan), hd_s(R * ns, nan), hs_s(2 * R * m, nan), w_s(R * m, nan), wy_s(R * m, nan), res_f(R * n, nan),
      ng_f(R * n, nan), y_f2(R, nan);
  DcArgs a;
  a.T = T; a.nv = nv; a.nr = nr; a.ns = (int)ns; a.row0 = s->sensor_first_row; a.num_sensor = (int)m;
  a.dim = s->sensor_dim; a.first = first.data(); a.stage = s->sensor_stage; a.norm = s->sensor_norm; a.row_sensor = row_sensor.data();
  a.prm = s->sensor_norm_parameter; a.noise_sensor = s->noise_sensor; a.noise_process = s->noise_process; a.mask = s->sensor_mask;
  a.sensor_flag = s->sensor_flag ? 1 : 0; a.force_flag = s->force_flag ? 1 : 0; a.time_scaling_sensor = s->time_scaling_sensor ? 1 : 0;
  a.time_scaling_force = s->time_scaling_force ? 1 : 0; a.first_pos = s->first_step_position_sensors ? 1 : 0;
  a.last_pos = s->last_step_position_sensors ? 1 : 0; a.last_vel = s->last_step_velocity_sensors ? 1 : 0; a.h = s->timestep;
  a.rs = rs; a.rf = rf; a.V0 = a.V1 = nullptr;
  for (int k = 0; k < 3; k++) { a.Df[k] = nullptr; a.Ds[k] = nullptr; }
  a.res_s = res_s.data(); a.ng_s = ng_s.data(); a.hd_s = hd_s.data(); a.hs_s = hs_s.data(); a.w_s = w_s.data(); a.wy_s = wy_s.data();
  a.res_f = res_f.data(); a.ng_f = ng_f.data(); a.y_f = y_f2.data(); a.Js = a.Jf = a.NJs = a.NJf = a.gradient = a.band = nullptr; a.cost = cost;
  for (int w = 0; w < nwin; w++) {          // dc_norm_kernel: grid (T, nwin)
    const DcArgs b = dc_window(a, w);
    for (int t = 0; t < T; t++) {
      for (int i = 0; i < b.num_sensor; i++) dc_norm_sensor(b, t, i);
      for (int i = 0; i < nv; i++) dc_norm_force(b, t, i);
      b.y_f[t] = dc_force_value(b, t);
    }
  }
  for (int w = 0; w < nwin; w++) {          // dc_cost_kernel: one workgroup per window
    const DcArgs b = dc_window(a, w);
    const double p0 = dc_cost_part(b, 0), p1 = dc_cost_part(b, 1);
    b.cost[0] = add_rn(p0, p1); b.cost[1] = p0; b.cost[2] = p1;
  }
  return 0;
}
