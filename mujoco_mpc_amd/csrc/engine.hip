// engine.hip — HIP kernels + C ABI (include/mjpc_hip.h) of the Predictive-Sampling rollout engine.
//
// Kernels (gfx950, wave64):
//   noise_kernel    Philox4x32-10 + Box-Muller standard normals  eps[nlocal, P, nu]
//   rollout_kernel  (rollout_cached / _dense2 / _dense2h / _direct / _spill.hip)  ONE WORKGROUP PER CANDIDATE (grid = nlocal blocks x 64*MJPC_WAVES threads: an owner wave on the
//                   critical path + helper / side waves on the CU's other SIMDs, see spmd.h); the candidate's
//                   whole mjData-equivalent lives in dynamic LDS for all H steps; HBM traffic is only
//                   the Trajectory record (coalesced row writes by the owning wave) + model reads
//                   that hit L2 / the scalar cache.  Replaces planner.cc:342-380 + trajectory.cc:100-210.
//   sg_assemble_kernel / sg_gradient_kernel  (gradient.h)  Sample-Gradient planner: the mixed candidate table + noise history of a
//                   mjpc_hip_plan_mixed step, and the weighted sum of history rows that is the planner's gradient
//   step_kernel    (rollout_step_cached / _direct / _spill.hip, transition.h)  one workgroup per ROW of a state table: one step of the
//                   rollout kernel's phases from that row's own state, control and time (mjpc_hip_step_batch)
//   fd_assemble_kernel / fd_difference_kernel  (transition_fd.h)  mjpc_hip_transition_fd: the perturbed table around the nominal
//                   knots, and the A / B / C / D entries from the stepped rows
//   inv_kernel     (rollout_inv_cached / _direct / _spill.hip, inverse.h)  one workgroup per ROW of a state / acceleration table: one inverse-
//                   dynamics evaluation behind the rollout kernel's pre-solve phases, no solver (mjpc_hip_inverse_batch)
//   ifd_assemble_kernel / ifd_difference_kernel  (inverse_fd.h)  mjpc_hip_inverse_fd: the perturbed table around the nominal
//                   configurations, and the six blocks df/d(q, v, a), ds/d(q, v, a) from the evaluated rows
//   ukf_sigma_kernel / ukf_mean_kernel / ukf_cov_kernel  (estimator.h)  mjpc_hip_unscented_moments: the sigma-point table around a mean
//                   state, and the weighted means, difference table and covariance blocks of the stepped rows
//   cd_kernel / gd_backward_kernel  (cost_derivatives.h)  mjpc_hip_cost_derivatives / mjpc_hip_trajectory_gradient: the cost derivatives of
//                   every knot from the residual and its Jacobian, and the gradient planner's backward recursion
//   rc_backward_kernel  (riccati.h)  mjpc_hip_ilqg_backward_pass / mjpc_hip_trajectory_ilqg: iLQG's backward pass, one workgroup: Riccati
//                   recursion, box-QP controls and the regularisation loop
//   fb_kernel / fb_resample_kernel  (rollout_fb_cached / _direct / _spill.hip, feedback.h; feedback_resample.h)  mjpc_hip_plan_feedback: the
//                   rollout kernel under a feedback policy read at the candidate's own state (iLQG's rollouts), and the policy resampled
//                   at the step times once per call
//   argmin_kernel   wavefront (value, index) min-reduction, lowest index wins ties
//                   (planner.cc:168-181 partial_sort -> trajectory_order[0]).
//   pack_kernel     the plan's result in one contiguous buffer for one D2H copy
// Host side (from the banner below): the engine's buffers (devbuf.h, enum Buf), flavour and dense-tier choice, the C ABI.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

#include "model.h"
#include "spmd.h"
#include "philox.h"
#include "gradient.h"
#include "transition_fd.h"
#include "inverse_fd.h"
#include "estimator.h"
#include "cost_derivatives.h"
#include "direct_cost.h"
#include "riccati.h"
#include "feedback_resample.h"
#include "host.h"
#include "devbuf.h"
#include "carve.h"
#include "../../include/mjpc_hip_debug.h"

// ------------------------------------------------------------------------------ kernels
// the rollout kernels live in their own translation units (rollout_*.hip, one per flavour; see rollout_tu.inc)
typedef void (*RolloutFn)(const KParams);
extern "C" RolloutFn mjpc_pick_rollout_cached(int nv, int *exact);
extern "C" RolloutFn mjpc_pick_rollout_direct(int nv, int *exact);
extern "C" RolloutFn mjpc_pick_rollout_dense2(int nv, int *exact);
extern "C" RolloutFn mjpc_pick_rollout_dense2h(int nv, int *exact);
extern "C" RolloutFn mjpc_pick_rollout_spill(int nv, int *exact);
extern "C" int mjpc_rollout_threads_cached(void);
// the one-step kernels (rollout_step_*.hip, step_tu.h): opaque here, their parameter block needs core.h
typedef void (*StepLaunchFn)(const void *fn, int n, size_t lds_bytes, hipStream_t stream, const KParams *K, const double *state_tab, const double *ctrl_tab,
                             const double *time_tab, double *next_state, double *residual_out, int *failure_out, const int *late_tab);
#define MJPC_STEP_DECL(tu) extern "C" const void *mjpc_pick_step_##tu(int nv); \
  extern "C" void mjpc_launch_step_##tu(const void *, int, size_t, hipStream_t, const KParams *, const double *, const double *, const double *, double *, double *, int *, const int *);
MJPC_STEP_DECL(cached) MJPC_STEP_DECL(direct) MJPC_STEP_DECL(spill)
#undef MJPC_STEP_DECL
// the inverse-dynamics kernels (rollout_inv_*.hip, inv_tu.h): opaque here as well
typedef void (*InvLaunchFn)(const void *fn, int n, size_t lds_bytes, hipStream_t stream, const KParams *K, const double *state_tab, const double *ctrl_tab,
                            const double *time_tab, const double *qacc_tab, int discrete, double *qfrc_inverse_out, double *qfrc_constraint_out,
                            double *residual_out, int *failure_out, const int *late_tab);
#define MJPC_INV_DECL(tu) extern "C" const void *mjpc_pick_inv_##tu(int nv); \
  extern "C" void mjpc_launch_inv_##tu(const void *, int, size_t, hipStream_t, const KParams *, const double *, const double *, const double *, const double *, int, double *, double *, double *, int *, const int *);
MJPC_INV_DECL(cached) MJPC_INV_DECL(direct) MJPC_INV_DECL(spill)
#undef MJPC_INV_DECL
// the feedback-policy rollout kernels (rollout_fb_*.hip, feedback_tu.h): opaque here as well
typedef void (*FbLaunchFn)(const void *fn, int n, size_t lds_bytes, hipStream_t stream, const KParams *K, const double *xbar, const double *ubar,
                           const double *kbar, const double *Kbar, const double *alpha, const double *scale);
#define MJPC_FB_DECL(tu) extern "C" const void *mjpc_pick_fb_##tu(int nv); \
  extern "C" void mjpc_launch_fb_##tu(const void *, int, size_t, hipStream_t, const KParams *, const double *, const double *, const double *, const double *, const double *, const double *);
MJPC_FB_DECL(cached) MJPC_FB_DECL(direct) MJPC_FB_DECL(spill)
#undef MJPC_FB_DECL

// Capacity tiers.  One candidate per CU leaves every SIMD with a single, mostly stalled wave; two resident workgroups per CU
// raise throughput ~1.6x once a shard has more candidates than CUs, but need <= 80 KiB of LDS each.  The dense tier gets
// there with a smaller contact / constraint-row capacity than the model asks for (and, to afford 100 rows / 28 contacts, reads the spline knots and the Hessian entry table from L2); a candidate that overflows it is flagged
// (MJPC_WARN_CONTACTFULL / CNSTRFULL) and the full-capacity kernel re-runs exactly those candidates right behind it on
// the stream (all other workgroups of that launch exit at once).  Rollouts are deterministic and independent, so the result
// is the same as running everything at full capacity: no candidate is lost to the smaller buffers.
#define TIERB_NEFCMAX 128    // first capacity tried for the dense tier (rows); contacts = rows / 4 + 2
#define TIERB_NEFCMIN 40
#define TIERB_LDS_LIMIT (80 * 1024)
#define TIERB_HOT_KEEP 75       // per cent of the plain dense tier's rows the hot-cached variant must still hold to be preferred

// eps[r, e] for global candidate (offset + r), element e = p*nu + k; sel[r] = second-std choice
extern "C" __global__ void noise_kernel(double *eps, int *sel, unsigned long long seed, unsigned long long stream,
                                        int offset, int nlocal, int PN, double sigma1) {
  size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t total = (size_t)nlocal * PN;
  if (idx < total) {
    int r = (int)(idx / PN), e = (int)(idx - (size_t)r * PN);
    eps[idx] = philox_normal(seed, stream, (unsigned)(offset + r), (unsigned)e);
  }
  if (idx < (size_t)nlocal) {
    unsigned o[4];
    philox4x32_10(seed, stream, (unsigned)(offset + (int)idx), 0xFFFFFFFFu, o);
    unsigned long long x = ((unsigned long long)o[0] << 32) | o[1];
    double u = (double)(x >> 11) * (1.0 / 9007199254740992.0);
    sel[idx] = (sigma1 > 0 && u < 0.2) ? 1 : 0;
  }
}

// mjpc_hip_plan_mixed: candidate table rows below first_explicit + noise history (gradient.h), one thread per table element
extern "C" __global__ void __launch_bounds__(256) sg_assemble_kernel(const SgAssembleArgs a) {
  size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx < (size_t)a.nlocal * a.PN) sg_assemble(a, idx);
}

// mjpc_hip_sample_gradient: block b owns parameters [b * SG_KT, (b + 1) * SG_KT); wave 0 (lanes < SG_KT) runs the add chains,
// waves 1 .. 3 are the SG_PROD producer groups; two tiles, one barrier per tile: the producers fill tile t while the consumer
// adds tile t - 1, and a tile is written again only after the barrier that follows its consumption
extern "C" __global__ void __launch_bounds__(256) sg_gradient_kernel(const SgGradArgs a) {
  __shared__ double buf[2][SG_T * SG_KT];
  const int kb = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ntile = (a.n + SG_T - 1) / SG_T;
  double acc = 0.0;
  for (int t = 0; t <= ntile; t++) {
    if (w > 0 && t < ntile) sg_produce(a, kb, t, (w - 1) * (64 / SG_KT) + lane / SG_KT, lane % SG_KT, buf[t & 1]);
    if (w == 0 && t > 0 && lane < SG_KT) acc = sg_consume(a, t - 1, lane, buf[(t - 1) & 1], acc);
    __syncthreads();
  }
  if (w == 0 && lane < SG_KT && kb * SG_KT + lane < a.PN) a.gradient[kb * SG_KT + lane] = acc;
}
static_assert(SG_PROD == 3 * (64 / SG_KT), "sg_gradient_kernel: three producer waves");

// mjpc_hip_transition_fd, table assembly: one wave per table row, its lanes walk the row's ds + nu + 1 elements (the nominal row is read
// and the table row stored in whole contiguous segments)
extern "C" __global__ void __launch_bounds__(256) fd_assemble_kernel(const FdArgs a, unsigned rows) {
  const size_t g = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= rows) return;
  const int n = a.nq + a.nv + a.na + a.nu + 1;
  for (int i = threadIdx.x & 63; i < n; i += 64) fd_assemble(a, g, i);
}

// mjpc_hip_transition_fd, differences: block (x, y, z) owns the FD_TILE x FD_TILE tile of knot z's combined matrix [A B; C D] at output
// rows y * FD_TILE, columns x * FD_TILE.  A column of the matrix is one evaluation pair, whose rows are contiguous in the step kernel's
// output; the matrices are row-major.  So a tile is read with the output row as the fast index (16 consecutive doubles of a next-state
// row per column), turned in LDS (odd row stride: no bank conflicts either way) and stored with the column as the fast index (16
// consecutive doubles of a matrix row): both sides move whole 128-byte segments instead of one double per segment.
#define FD_TILE 16
extern "C" __global__ void __launch_bounds__(FD_TILE * FD_TILE) fd_difference_kernel(const FdArgs a) {
  __shared__ double tile[FD_TILE][FD_TILE + 1];
  const int t = blockIdx.z, o0 = blockIdx.y * FD_TILE, c0 = blockIdx.x * FD_TILE;
  const int nd = 2 * a.nv + a.na, no = nd + a.nr, nc = nd + a.nu;
  {
    const int oi = threadIdx.x % FD_TILE, ci = threadIdx.x / FD_TILE, o = o0 + oi, c = c0 + ci;
    if (o < no && c < nc && fd_dest(a, t, o, c)) tile[oi][ci] = fd_entry(a, t, o, c);
  }
  __syncthreads();
  {
    const int ci = threadIdx.x % FD_TILE, oi = threadIdx.x / FD_TILE, o = o0 + oi, c = c0 + ci;
    if (o < no && c < nc) { double *d = fd_dest(a, t, o, c); if (d) *d = tile[oi][ci]; }
  }
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < 64) {
    int w = wave_or_i(fd_failure(a, t, (int)threadIdx.x, 64));
    if (threadIdx.x == 0) a.failure[t] = w;
  }
}

// mjpc_hip_inverse_fd, table assembly: one wave per table row, its lanes walk the row's ds + nu + 1 + nv elements
extern "C" __global__ void __launch_bounds__(256) ifd_assemble_kernel(const InvFdArgs a, unsigned rows) {
  const size_t g = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= rows) return;
  const int n = ifd_row_elements(a);
  for (int i = threadIdx.x & 63; i < n; i += 64) ifd_assemble(a, g, i);
}

// mjpc_hip_inverse_fd, differences: block (x, y, z) owns the FD_TILE x FD_TILE tile of configuration z's combined matrix
// [DfDq DfDv DfDa; DsDq DsDv DsDa] at output rows y * FD_TILE, columns x * FD_TILE, turned in LDS as in fd_difference_kernel
extern "C" __global__ void __launch_bounds__(FD_TILE * FD_TILE) ifd_difference_kernel(const InvFdArgs a) {
  __shared__ double tile[FD_TILE][FD_TILE + 1];
  const int t = blockIdx.z, o0 = blockIdx.y * FD_TILE, c0 = blockIdx.x * FD_TILE;
  const int no = a.nv + a.nr, nc = 3 * a.nv;
  {
    const int oi = threadIdx.x % FD_TILE, ci = threadIdx.x / FD_TILE, o = o0 + oi, c = c0 + ci;
    if (o < no && c < nc && ifd_dest(a, t, o, c)) tile[oi][ci] = ifd_entry(a, t, o, c);
  }
  __syncthreads();
  {
    const int ci = threadIdx.x % FD_TILE, oi = threadIdx.x / FD_TILE, o = o0 + oi, c = c0 + ci;
    if (o < no && c < nc) { double *d = ifd_dest(a, t, o, c); if (d) *d = tile[oi][ci]; }
  }
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < 64) {
    int w = wave_or_i(ifd_failure(a, t, (int)threadIdx.x, 64));
    if (threadIdx.x == 0) a.failure[t] = w;
  }
}

// mjpc_hip_unscented_moments, sigma-point table: one wave per table row, its lanes walk the row's ds + nu + 1 elements
extern "C" __global__ void __launch_bounds__(256) ukf_sigma_kernel(const UkfArgs a) {
  const int g = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  if (g >= ukf_rows(a)) return;
  const int n = a.nq + a.nv + a.na + a.nu + 1;
  for (int i = threadIdx.x & 63; i < n; i += 64) ukf_sigma(a, g, i);
}

// mjpc_hip_unscented_moments, means and differences: ONE workgroup.  One lane per mean component (a serial sum over the sigma rows);
// then the lane that owns a quaternion's w replaces its four numbers; then the difference table against the means just stored
// (the workgroup barrier orders the global stores before the loads) and the OR of the rows' warning bits
extern "C" __global__ void __launch_bounds__(256) ukf_mean_kernel(const UkfArgs a) {
  const int ds = a.nq + a.nv + a.na, nd = ukf_nd(a), n = nd + a.ns, R = ukf_rows(a);
  for (int i = threadIdx.x; i < ds + a.ns; i += 256) {
    const double v = ukf_mean_component(a, i);
    if (i < ds) a.state_mean[i] = v; else a.sensor_mean[i - ds] = v;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < a.nq; i += 256)
    if (a.qmap[2 * i + 1] == 0) {
      double q[4]; ukf_quat_mean(a, i, q);
      a.state_mean[i] = q[0]; a.state_mean[i + 1] = q[1]; a.state_mean[i + 2] = q[2]; a.state_mean[i + 3] = q[3];
    }
  __syncthreads();
  for (int e = threadIdx.x; e < R * n; e += 256) a.diff[e] = ukf_diff(a, e / n, e % n);
  if (threadIdx.x < 64) {
    int w = wave_or_i(ukf_failure(a, (int)threadIdx.x, 64));
    if (threadIdx.x == 0) *a.failure = w;
  }
}

// mjpc_hip_unscented_moments, covariances: block (x, y) owns the UKF_TILE x UKF_TILE tile of the combined matrix [[ss, sy], [sy', yy]]
// at rows y * UKF_TILE, columns x * UKF_TILE.  The difference rows go through LDS 16 sigma points at a time (estimator.h): the
// global reads run along the rows of the table, the LDS reads are a broadcast (ta) and 16 consecutive doubles (tb).  No f64 MFMA:
// the sum over sigma points is the serial, separately rounded one of the host restatement.
extern "C" __global__ void __launch_bounds__(UKF_TILE * UKF_TILE) ukf_cov_kernel(const UkfArgs a) {
  __shared__ double ta[UKF_TILE * UKF_TILE], tb[UKF_TILE * UKF_TILE];
  const int r0 = blockIdx.y * UKF_TILE, c0 = blockIdx.x * UKF_TILE, nd = ukf_nd(a), R = ukf_rows(a);
  if (r0 >= nd && c0 + UKF_TILE <= nd) return;          // a tile inside the lower-left block (sy'): nothing to store
  const int ri = threadIdx.x / UKF_TILE, ci = threadIdx.x % UKF_TILE;
  double acc = ukf_cov_init(a, r0 + ri, c0 + ci);
  for (int j0 = 0; j0 < R; j0 += UKF_TILE) {
    ukf_cov_stage(a, j0, r0, c0, (int)threadIdx.x, ta, tb);
    __syncthreads();
    acc = ukf_cov_accum(a, j0, ri, ci, ta, tb, acc);
    __syncthreads();
  }
  double *d = ukf_cov_dest(a, r0 + ri, c0 + ci);
  if (d) *d = acc;
}

// mjpc_hip_cost_derivatives: block (x, y, z) owns the CD_TILE x CD_TILE tile of knot z's (nd + nu)^2 Gauss-Newton matrix at rows
// y * CD_TILE, columns x * CD_TILE (hessians = 0: gridDim.y = 1 and the gradient alone).  The lanes of a wave run along the output
// column j: a row of J = [C | D] is contiguous in j, so J[r][j] is read in whole 128-byte segments and J[r][i] is a broadcast.  The
// knot's norm derivatives are computed once per workgroup into LDS; crr J of a dense term is staged there for the tile's columns
// (the tile's width is the column chunk), read back with one address per column: no bank conflicts.
extern "C" __global__ void __launch_bounds__(CD_TILE * CD_TILE) cd_kernel(const CdArgs a) {
  extern __shared__ double cd_sm[];
  const CdLds L = cd_lds(a, cd_sm);
  const int t = blockIdx.z, i0 = blockIdx.y * CD_TILE, j0 = blockIdx.x * CD_TILE, n = a.nd + a.nu, tid = threadIdx.x;
  for (int k = tid; k < a.num_term; k += CD_TILE * CD_TILE) cd_term(a, t, k, L);
  __syncthreads();
  const double s = cd_risk_scale(a, L);
  if (tid < (a.hessians ? 2 : 1) * CD_TILE) {
    const int j = tid < CD_TILE ? j0 + tid : i0 + (tid - CD_TILE);
    L.gv[tid] = j < n ? cd_gradient(a, t, j, L, s) : 0.0;
  }
  if (blockIdx.x == 0 && blockIdx.y == 0 && a.cr) for (int r = tid; r < a.nr; r += CD_TILE * CD_TILE) a.cr[(size_t)t * a.nr + r] = L.cr[r];
  __syncthreads();
  if (blockIdx.y == 0 && tid < CD_TILE && j0 + tid < n) {
    const int j = j0 + tid;
    if (j < a.nd) { if (a.cx) a.cx[(size_t)t * a.nd + j] = L.gv[tid]; }
    else if (a.cu) a.cu[(size_t)t * a.nu + (j - a.nd)] = L.gv[tid];
  }
  if (!a.hessians) return;
  const int term = cd_terminal(a, t);
  if (term && blockIdx.x == 0 && blockIdx.y == 0)
    for (size_t e = tid; e < (size_t)(a.nd > a.nu ? a.nd : a.nu) * a.nu; e += CD_TILE * CD_TILE) { cd_zero_terminal(a, 0, e); cd_zero_terminal(a, 1, e); }
  if (i0 >= a.nd && j0 + CD_TILE <= a.nd) return;             // the tile lies in the bottom-left block, which is not stored
  const int jj = tid % CD_TILE, ii = tid / CD_TILE, i = i0 + ii, j = j0 + jj;
  double *dst = cd_dest(a, t, i, j);
  double acc = 0;
  int fs = 0;
  for (int k = 0; k < a.num_term; k++) {
    const int ni = a.dim_norm_residual[k], dense = norm_dense(a.norm[k]);
    if (dense) {          // (uniform over the workgroup)
      __syncthreads();
      for (int idx = tid; idx < ni * CD_TILE; idx += CD_TILE * CD_TILE) {
        const int c = j0 + idx % CD_TILE;
        L.S[idx] = (c < n && !(term && c >= a.nd)) ? cd_S_dense(a, t, k, fs, ni, idx / CD_TILE, c, L) : 0.0;
      }
      __syncthreads();
    }
    if (dst) acc = add_rn(acc, mul_rn(cd_weight(a, k), cd_G(a, t, fs, ni, dense, i, j, jj, L)));
    fs += ni;
  }
  if (dst) *dst = cd_risk_entry(a, acc, L.gv[CD_TILE + ii], L.gv[jj], s);
}

// mjpc_hip_direct_cost / _derivatives, the window's rows: one wave per row (w, t), its lanes walk the row's ds + nu + 1 + nv elements
extern "C" __global__ void __launch_bounds__(256) dc_window_kernel(const DcWinArgs a, unsigned rows) {
  const size_t g = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= rows) return;
  const int n = a.nq + a.nv + a.na + a.nu + 1 + a.nv;
  for (int i = threadIdx.x & 63; i < n; i += 64) dc_window_row(a, g, i);
}

// mjpc_hip_direct_cost_derivatives, velocity blocks: one thread per entry of [T][nv][nv]
extern "C" __global__ void __launch_bounds__(DC_THREADS) dc_vblock_kernel(const DcWinArgs a, size_t n) {
  const size_t e = (size_t)blockIdx.x * DC_THREADS + threadIdx.x;
  if (e < n) dc_velocity_block(a, e);
}

// mjpc_hip_direct_cost / _derivatives, residuals: one thread per entry of [nwin T][ns + nv]
extern "C" __global__ void __launch_bounds__(DC_THREADS) dc_residual_kernel(const DcResArgs a, size_t n) {
  const size_t e = (size_t)blockIdx.x * DC_THREADS + threadIdx.x;
  if (e < n) dc_residual(a, e);
}

// mjpc_hip_direct_assemble, norms: block t owns configuration t; its threads walk the sensors, then the dofs of the force term
extern "C" __global__ void __launch_bounds__(64) dc_norm_kernel(const DcArgs a0) {
  const DcArgs a = dc_window(a0, (int)blockIdx.y);          // (a value call's windows in y; one window otherwise)
  const int t = blockIdx.x;
  for (int i = threadIdx.x; i < a.num_sensor; i += 64) dc_norm_sensor(a, t, i);
  for (int i = threadIdx.x; i < a.nv; i += 64) dc_norm_force(a, t, i);
  if (threadIdx.x == 0) a.y_f[t] = dc_force_value(a, t);
}

// mjpc_hip_direct_assemble, totals: one workgroup per window; thread 0 sums the sensors' weighted norms, thread 1 the force terms
extern "C" __global__ void __launch_bounds__(64) dc_cost_kernel(const DcArgs a0) {
  const DcArgs a = dc_window(a0, (int)blockIdx.x);          // one workgroup per window
  __shared__ double part[2];
  if (threadIdx.x < 2) part[threadIdx.x] = dc_cost_part(a, (int)threadIdx.x);
  __syncthreads();
  if (threadIdx.x == 0) { a.cost[0] = add_rn(part[0], part[1]); a.cost[1] = part[0]; a.cost[2] = part[1]; }
}

// mjpc_hip_direct_assemble, chain rule: block (x, y, z) owns the DC_TILE x DC_TILE tile of configuration x's block [ns + nv][3 nv] at
// rows y * DC_TILE, columns z * DC_TILE (the configuration in x: T is unbounded); the contraction over the dofs goes through LDS in
// chunks of DC_TILE (direct_cost.h)
extern "C" __global__ void __launch_bounds__(DC_TILE * DC_TILE) dc_block_kernel(const DcArgs a) {
  __shared__ double dc_sm[DC_TILE_DOUBLES];
  const DcTiles L = dc_tiles(dc_sm);
  const int t = blockIdx.x, o0 = blockIdx.y * DC_TILE, c0 = blockIdx.z * DC_TILE, tid = threadIdx.x;
  double p1 = 0, p2 = 0;
  for (int k0 = 0; k0 < a.nv; k0 += DC_TILE) {
    dc_block_stage(a, t, o0, c0, k0, tid, L);
    __syncthreads();
    dc_block_accum(a, k0, tid, L, p1, p2);
    __syncthreads();
  }
  dc_block_store(a, t, o0, c0, tid, p1, p2);
}

// mjpc_hip_direct_assemble, norm Hessian times block: one thread per entry of [T][ns + nv][3 nv], the lanes along a row
extern "C" __global__ void __launch_bounds__(DC_THREADS) dc_nj_kernel(const DcArgs a, size_t n) {
  const size_t e = (size_t)blockIdx.x * DC_THREADS + threadIdx.x;
  if (e < n) dc_nj(a, e);
}

// mjpc_hip_direct_assemble, gradient and band Hessian: one thread per entry of [ntotal][3 nv + 1], the lanes along a band row (the
// reads of N J run along its rows, the block's own entry is a broadcast)
extern "C" __global__ void __launch_bounds__(DC_THREADS) dc_entry_kernel(const DcArgs a, size_t n) {
  const size_t e = (size_t)blockIdx.x * DC_THREADS + threadIdx.x;
  if (e < n) dc_entry(a, e);
}

// mjpc_hip_trajectory_gradient, backward recursion: one workgroup, one lane per column of [A | B]; Vx_t and Qu_{t-1} pass through LDS
// (two buffers each).  Only Vx is on the serial chain: the block of step t - 1 is fetched into registers before step t's chain starts
// and stored to LDS behind it (cost_derivatives.h), so a step's memory latency runs under the previous step's adds.  LDS (doubles):
// vx[2][nd] | qu[2][nu] | block[nd][nd + nu] (the block only when it fits, gd_staged)
extern "C" __global__ void __launch_bounds__(GD_THREADS) gd_backward_kernel(const GdArgs a) {
  extern __shared__ double gd_sm[];
  const int nd = a.nd, nu = a.nu, n = nd + nu, T = a.T, tid = threadIdx.x, nb = nd * n;
  double *vx[2] = {gd_sm, gd_sm + nd}, *qu[2] = {gd_sm + 2 * nd, gd_sm + 2 * nd + nu};
  const bool staged = gd_staged(a);
  double *blk = staged ? gd_sm + 2 * n : nullptr;
  for (int c = tid; c < nd; c += GD_THREADS) { const double v = a.cx[(size_t)(T - 1) * nd + c]; vx[0][c] = v; a.Vx[(size_t)(T - 1) * nd + c] = v; }
  if (staged) for (int i = tid; i < nb; i += GD_THREADS) blk[i] = gd_block(a, T - 1, i);
  double dv = 0;
  __syncthreads();
  for (int t = T - 1; t > 0; t--) {
    const int b = (T - 1 - t) & 1;
    double next[GD_R];
    if (staged && t > 1) {
#pragma unroll
      for (int u = 0; u < GD_R; u++) { const int i = tid + u * GD_THREADS; next[u] = i < nb ? gd_block(a, t - 1, i) : 0.0; }
    }
    for (int c = tid; c < n; c += GD_THREADS) {
      const double q = gd_column(a, t, c, vx[b], blk);
      if (c < nd) { a.Qx[(size_t)(t - 1) * nd + c] = q; a.Vx[(size_t)(t - 1) * nd + c] = q; vx[b ^ 1][c] = q; }
      else {
        const int kk = c - nd;
        a.Qu[(size_t)(t - 1) * nu + kk] = q; a.k[(size_t)(t - 1) * nu + kk] = -q; qu[b][kk] = q;
        if (t == T - 1) a.k[(size_t)(T - 1) * nu + kk] = -q;         // k_{T-1} = k_{T-2}
      }
    }
    __syncthreads();
    if (tid == 0) dv = gd_dv(a, qu[b], dv);
    if (staged && t > 1) {
#pragma unroll
      for (int u = 0; u < GD_R; u++) { const int i = tid + u * GD_THREADS; if (i < nb) blk[i] = next[u]; }
      __syncthreads();
    }
  }
  if (tid == 0) { a.dV[0] = dv; a.dV[1] = 0.0; }
}

// mjpc_hip_ilqg_backward_pass / mjpc_hip_trajectory_ilqg: the whole regularised backward pass in ONE workgroup (riccati.h).  The work
// image lies in LDS when it fits (rc_fits) and in the call's global scratch otherwise; the two branches are the same function, so
// that the compiler sees which address space each copy works in.
extern "C" __global__ void __launch_bounds__(RC_THREADS) rc_backward_kernel(const RcArgs a) {
  extern __shared__ double rc_sm[];
  if (rc_fits(a.nd, a.nu)) rc_backward(a, rc_work(a.nd, a.nu, rc_sm), (int)threadIdx.x, RC_THREADS);
  else rc_backward(a, rc_work(a.nd, a.nu, a.scratch), (int)threadIdx.x, RC_THREADS);
}

// mjpc_hip_plan_feedback, time mode: workgroup t fills row t of the [H] tables (feedback_resample.h), then renormalises the row's quaternions
extern "C" __global__ void __launch_bounds__(256) fb_resample_kernel(const FbResampleArgs a) {
  const int t = (int)blockIdx.x, n = fb_resample_elements(a);
  for (int e = (int)threadIdx.x; e < n; e += (int)blockDim.x) fb_resample(a, t, e);
  __syncthreads();
  for (int j = (int)threadIdx.x; j < a.njnt; j += (int)blockDim.x) fb_resample_normalize(a, t, j);
}

// winner[0] = local index of the first minimum of returns[0..n), winner_val[0] = its value
extern "C" __global__ void __launch_bounds__(64) argmin_kernel(const double *returns, int n, int *winner, double *winner_val) {
  int lane = threadIdx.x;
  double best = 1.0e300; int bi = 0x7fffffff;
  for (int i = lane; i < n; i += 64) { double v = returns[i]; if (v < best) { best = v; bi = i; } }   // strict <: keeps the lowest index per lane
  for (int o = 32; o > 0; o >>= 1) {
    double ov = __shfl_xor(best, o, 64); int oi = __shfl_xor(bi, o, 64);
    if (ov < best || (ov == best && oi < bi)) { best = ov; bi = oi; }
  }
  if (lane == 0) { winner[0] = bi; winner_val[0] = best; }
}

// gathers everything the host wants after a plan step into ONE contiguous buffer (one D2H copy instead of eleven):
//   [winner index, winner return | returns[nl] | failure[nl] (as doubles) | winner knots | winner rows: states, actions, times,
//    residual, costs, trace]      (the rows only when a.rows: a shard of a multi-device plan sends the summary alone and the
//    owner of the global winner fetches its rows afterwards)
struct PackArgs {
  const int *winner; const double *winner_val, *returns; const int *failure;
  const double *states, *actions, *times, *residual, *costs, *trace, *knots;
  int nl, H, P, ds, nu, nr, ntr, rows;
  double *dst;
};
extern "C" __global__ void __launch_bounds__(256) pack_kernel(const PackArgs a) {
  int w = a.winner[0];
  int tid = blockIdx.x * blockDim.x + threadIdx.x, nth = gridDim.x * blockDim.x;
  double *d = a.dst;
  if (tid == 0) { d[0] = (double)w; d[1] = a.winner_val[0]; }
  d += 2;
  for (int i = tid; i < a.nl; i += nth) { d[i] = a.returns[i]; d[a.nl + i] = (double)a.failure[i]; }
  d += 2 * a.nl;
  if (w < 0 || w >= a.nl) return;
  size_t H = (size_t)a.H, r = (size_t)w;
  const double *src[7] = {a.knots + r * (size_t)a.P * a.nu, a.states + r * H * a.ds, a.actions + r * H * a.nu, a.times + r * H,
                          a.residual + r * H * a.nr, a.costs + r * H, a.trace + r * H * a.ntr};
  size_t cnt[7] = {(size_t)a.P * a.nu, H * a.ds, H * a.nu, H, H * a.nr, H, H * a.ntr};
  for (int k = 0; k < (a.rows ? 7 : 1); k++) {
    for (size_t i = tid; i < cnt[k]; i += nth) d[i] = src[k][i];
    d += cnt[k];
  }
}

// ------------------------------------------------------------------------------ host side
static thread_local std::string g_error;
static void set_error(const std::string &s) { g_error = s; }

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { set_error(std::string(#x) + ": " + hipGetErrorString(e_)); return -2; } } while (0)
// inside mjpc_hip_create only: `e` (when already allocated) and everything it owns are released on the error path
#define HIPCHKP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { set_error(std::string(#x) + ": " + hipGetErrorString(e_)); mjpc_hip_destroy(e); return nullptr; } } while (0)
// layout L (carve.h) in buffer b of engine `e`: lay() once on a null base for the bytes to reserve, once on the buffer for the pointers
#define PLACE(b, L, ...) do { Carve n_; lay(n_, L, __VA_ARGS__); HIPCHK(e->buf[b].reserve(n_.bytes())); Carve p_(e->buf[b].p); lay(p_, L, __VA_ARGS__); } while (0)

// Every device and pinned buffer of an engine is a DevBuf (devbuf.h) in MjpcHipEngine::buf, named by this enum: mjpc_hip_destroy walks
// the array, so a buffer added here cannot be forgotten there.  The seven per-candidate row arrays stand together, in the packed
// order of pack_kernel (row_doubles below); pinned host memory comes last (from H_PACK on).
enum Buf {
  B_IB, B_DB,                                                        // the packed model
  B_STATE, B_MOCAP, B_USERDATA, B_KT, B_KV, B_STD, B_SEL,            // plan inputs (userdata: mjData.userdata of the plan's state, State::CopyTo, states/state.cc:128-135: carried for residuals that read it)
  B_EPS, B_CAND,                                                     // noise / candidate table, grown on demand
  B_KNOTS, B_STATES, B_ACTIONS, B_TIMES, B_RESIDUAL, B_COSTS, B_TRACE,      // row arrays (knots grown on demand)
  B_RETURNS, B_FAILURE, B_DIAG, B_WINNER, B_WINNER_VAL, B_PROF, B_FRAME,
  B_CKPT,                                                            // dense-tier checkpoints for the retry launch
  B_SLAB,                                                            // spill flavour: per-candidate HBM slab
  B_HIST, B_SLOT, B_SCALE, B_GRAD,                                   // Sample-Gradient planner: noise history [max_local][P_max * nu], gradient inputs / output
  B_FBP,                                                             // feedback rollouts: the call's policy arrays, steps and [H] tables, grown on demand
  B_FD,                                                              // one-step calls: the call's tables (inputs, stepped rows, matrices), grown on demand
  B_PACK,                                                            // packed plan result, grown on demand
  H_PACK, H_SMALL, H_TASK0, H_TASK1,                                 // pinned: packed plan result | small plan inputs (Staging) | set_task staging
  B_COUNT
};
#define NROWS 7

// the dense tier (two workgroups per CU) of a model, see "Capacity tiers" above; k = nullptr: none
struct DenseTier { RolloutFn k = nullptr; Lay lay; int nefc = 0, ncon = 0, ci = 0, cd = 0; size_t lds = 0; };
// pinned staging block of the small inputs (H_SMALL), offsets in doubles: one layout for plans and one-step calls
struct Staging { size_t state, mocap, kt, kv, std, userdata, size; };

struct MjpcHipEngine {
  int device = 0;
  PackedModel pm;
  DevBuf buf[B_COUNT];
  template <class T = double> T *at(int b) const { return (T *)buf[b].p; }
  KParams K;
  int max_local = 0, max_horizon = 0, P_max = 0;
  int nq = 0, nv = 0, nu = 0, nmocap = 0, nr = 0, ntr = 0, ds = 0, nuserdata = 0;
  int na = 0, nd = 0;          // activations; tangent state 2 nv + na
  Dims dims() const { return Dims{(size_t)nq, (size_t)nv, (size_t)na, (size_t)nu, (size_t)nr, (size_t)ds, (size_t)nd}; }   // for the layouts of carve.h
  hipStream_t stream = nullptr;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  int nbody = 0, nsite = 0;
  int ckpt_stride = 0;
  Staging hs;
  hipEvent_t ev_task[2] = {nullptr, nullptr}; int task_slot = 0;   // set_task staging
  // last plan
  int last_H = 0, last_P = 0, last_nlocal = 0, last_offset = 0, pending = 0;
  // kernel timing accumulation
  double acc_rollout_us = 0, acc_total_us = 0; int acc_n = 0;
  size_t lds_bytes = 0;
  RolloutFn kernel = nullptr; bool cached = true;
  bool spill = false; int slab_bytes = 0;   // spill flavour: bytes of slab per candidate, whole 256-B blocks
  int fault = 0;               // diagnostics knob fault_inject (mjpc_hip_debug.h; test-suite only)
  int summary_only = 0, last_summary = 0;      // mjpc_hip_set_fetch_mode
  int last_dense = 0;
  int have_mixed = 0;          // a mjpc_hip_plan_mixed step has filled the noise history
  bool cost_rows_ok = false;   // cost_rows_tile of the current task
  // one-step kernel (mjpc_hip_step_batch / mjpc_hip_transition_fd): picked at the first call, in the full-capacity rollout's flavour
  const void *step_kernel = nullptr; StepLaunchFn step_launch = nullptr;
  // inverse-dynamics kernel (mjpc_hip_inverse_batch / mjpc_hip_inverse_fd): picked at the first call, same flavour
  const void *inv_kernel = nullptr; InvLaunchFn inv_launch = nullptr;
  // feedback rollout kernel (mjpc_hip_plan_feedback): picked at the first call, in the full-capacity rollout's flavour
  const void *fb_kernel = nullptr; FbLaunchFn fb_launch = nullptr;
  hipEvent_t ev_fb[2] = {nullptr, nullptr}; int fb_resampled = 0; double fb_resample_us = 0;
  DenseTier tierB; int num_cu = 256, force_tier = 0;
  MjpcHipEngine() { for (int b = H_PACK; b < B_COUNT; b++) buf[b].kind = DevBuf::PINNED; }
};

// doubles per candidate of row array k = 0 .. 6 (knots, states, actions, times, residual, costs, trace: buffer B_KNOTS + k, the order
// of the packed result) in a plan of H steps and P knots; pad: with the spare element per row the allocation of some of them carries
static size_t row_doubles(const MjpcHipEngine *e, int k, size_t H, size_t P, bool pad = false) {
  const int width[NROWS] = {e->nu, e->ds, e->nu, 1, e->nr, 1, e->ntr}, spare[NROWS] = {0, 0, 1, 0, 1, 0, 1};
  return (k == 0 ? P : H) * (size_t)(width[k] + (pad ? spare[k] : 0));
}
// where a plan output takes row array k (any may be null)
static double *out_row(const MjpcHipPlanOutput *out, int k) {
  double *dst[NROWS] = {out->winner_knots, out->states, out->actions, out->times, out->residual, out->costs, out->trace};
  return dst[k];
}

// the cost terms' rows tile the residual (the cost-derivative kernel indexes its LDS rows by them): checked when the task is packed
static bool cost_rows_tile(const MjpcHipEngine *e) {
  const DevTask ht = mjpc_host::relocate(e->pm, e->pm.ib.data(), e->pm.db.data()).task;
  long rows = 0;
  for (int k = 0; k < ht.num_term; k++) rows += ht.dim_norm_residual[k] > 0 ? ht.dim_norm_residual[k] : (long)e->nr + 1;
  return rows == e->nr;
}

static int upload_model(MjpcHipEngine *e) {
  int *d_ib = e->at<int>(B_IB); double *d_db = e->at(B_DB);
  HIPCHK(hipMemcpy(d_ib, e->pm.ib.data(), e->pm.ib.size() * sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d_db, e->pm.db.data(), e->pm.db.size() * sizeof(double), hipMemcpyHostToDevice));
  e->K.M = mjpc_host::relocate(e->pm, d_ib, d_db);
  e->K.L = e->pm.L;
  e->K.ibase = d_ib; e->K.dbase = d_db; e->K.cache_i = (int)e->pm.cache_i; e->K.cache_d = (int)e->pm.cache_d;
  return 0;
}

// everything in e->K that no call decides: the buffers allocated once by mjpc_hip_create and the engine's constants.  A plan sets the
// rest (plan_async_impl); a one-step call works on a copy and clears what it does not use (step_prepare)
static void bind_params(MjpcHipEngine *e) {
  KParams &K = e->K;
  K.state = e->at(B_STATE); K.mocap = e->at(B_MOCAP); K.userdata = e->at(B_USERDATA); K.nuserdata = e->nuserdata;
  K.knot_times = e->at(B_KT); K.knot_values = e->at(B_KV); K.noise_sel = e->at<int>(B_SEL);
  K.states = e->at(B_STATES); K.actions = e->at(B_ACTIONS); K.times = e->at(B_TIMES); K.residual = e->at(B_RESIDUAL); K.costs = e->at(B_COSTS);
  K.trace = e->at(B_TRACE); K.returns = e->at(B_RETURNS); K.failure = e->at<int>(B_FAILURE); K.diag = e->at<int>(B_DIAG);
  K.prof = e->at<long long>(B_PROF); K.frame = e->at(B_FRAME);
  K.retry = 0; K.tier = 0; K.ckpt = e->at(B_CKPT); K.ckpt_stride = e->ckpt_stride;
  K.fault = e->fault;
  K.slab = e->at(B_SLAB); K.slab_stride = e->slab_bytes / (long long)sizeof(double);
}

// the knots array holds max_local rows of P knots (grown on demand); K.knots follows a reallocation
static hipError_t reserve_knots(MjpcHipEngine *e, int P) {
  hipError_t rc = e->buf[B_KNOTS].reserve(sizeof(double) * ((size_t)e->max_local * P * e->nu + 1));
  e->K.knots = e->at(B_KNOTS);
  return rc;
}

// a copy of the engine's parameters for a launch that is no sampling plan: no spline policy, no noise, no candidate table, no force
// noise, full capacity.  The caller sets what is its own: P, H, N, offset, nlocal, time (and state / frame where it has none)
static KParams bare_params(const MjpcHipEngine *e) {
  KParams K = e->K;
  K.noise_eps = nullptr; K.noise_sel = nullptr; K.noise_std = nullptr; K.cand_knots = nullptr;
  K.sigma0 = 0; K.sigma1 = 0; K.seed = 0; K.stream = 0; K.interp = 0; K.use_device_noise = 0; K.nominal_index = 0;
  K.xfrc_std = 0; K.xfrc_rate = 0; K.retry = 0; K.tier = 0;
  return K;
}

// a kernel family's kernel of the engine's flavour (that of the full-capacity rollout kernel, pick_flavour; same compile-time dof
// count), looked up at the family's first call: its dynamic-LDS attribute is set, kernel and launcher are remembered
typedef const void *(*PickFn)(int nv);
template <class LaunchFn>
static int family_kernel(MjpcHipEngine *e, const void **kernel, LaunchFn *launch, const PickFn (&pick)[3], const LaunchFn (&launchers)[3]) {
  if (*kernel) return 0;
  const int f = e->spill ? 2 : e->cached ? 1 : 0;
  const void *k = pick[f](e->nv);
  HIPCHK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)e->lds_bytes));
  *kernel = k; *launch = launchers[f];
  return 0;
}
#define FAMILY_KERNEL(e, fam) family_kernel(e, &(e)->fam##_kernel, &(e)->fam##_launch, {mjpc_pick_##fam##_direct, mjpc_pick_##fam##_cached, mjpc_pick_##fam##_spill}, \
                                            {mjpc_launch_##fam##_direct, mjpc_launch_##fam##_cached, mjpc_launch_##fam##_spill})

// doubles of the packed result of nl candidates (pack_kernel): winner and its return, returns and failure words, then the winner's
// rows (the knot row alone for a summary-only engine; a plan without knots, P = 0, has an empty one)
static size_t pack_doubles(const MjpcHipEngine *e, int nl, int H, int P) {
  size_t n = 2 + 2 * (size_t)nl;
  for (int k = 0; k < (e->summary_only ? 1 : NROWS); k++) n += row_doubles(e, k, H, P);
  return n;
}

// what follows the rollouts of any plan (ev[2] recorded): the winner, its rows packed and on their way to pinned memory, and the
// plan marked in flight for mjpc_hip_plan_fetch
static int plan_tail(MjpcHipEngine *e, int nl, int H, int P, int offset, size_t need_pack) {
  hipLaunchKernelGGL(argmin_kernel, dim3(1), dim3(64), 0, e->stream, e->at(B_RETURNS), nl, e->at<int>(B_WINNER), e->at(B_WINNER_VAL));
  HIPCHK(hipEventRecord(e->ev[3], e->stream));
  PackArgs pa{e->at<int>(B_WINNER), e->at(B_WINNER_VAL), e->at(B_RETURNS), e->at<int>(B_FAILURE), e->at(B_KNOTS + 1), e->at(B_KNOTS + 2), e->at(B_KNOTS + 3),
              e->at(B_KNOTS + 4), e->at(B_KNOTS + 5), e->at(B_KNOTS + 6), e->at(B_KNOTS), nl, H, P, e->ds, e->nu, e->nr, e->ntr, e->summary_only ? 0 : 1, e->at(B_PACK)};
  e->last_summary = e->summary_only;
  hipLaunchKernelGGL(pack_kernel, dim3(8), dim3(256), 0, e->stream, pa);
  HIPCHK(hipMemcpyAsync(e->at(H_PACK), e->at(B_PACK), sizeof(double) * need_pack, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipGetLastError());
  e->last_H = H; e->last_P = P; e->last_nlocal = nl; e->last_offset = offset; e->pending = 1;
  return 0;
}

// n doubles of the caller's (zeros when src is null) through the pinned staging block at offset `at` into device buffer b, stream-ordered
static hipError_t stage(MjpcHipEngine *e, size_t at, const double *src, size_t n, int b) {
  double *h = e->at(H_SMALL) + at;
  if (src) memcpy(h, src, sizeof(double) * n); else memset(h, 0, sizeof(double) * n);
  return hipMemcpyAsync(e->at(b), h, sizeof(double) * n, hipMemcpyHostToDevice, e->stream);
}

// the struct_size test of the view structs (model = nullptr: the task alone); hint: appended to the message
static bool check_views(const MjpcHipModel *model, const MjpcHipTask *task, const char *who, const std::string &hint = "") {
  if ((!model || model->struct_size == (int)sizeof(MjpcHipModel)) && task->struct_size == (int)sizeof(MjpcHipTask)) return true;
  set_error(std::string(who) + (model ? ": MjpcHipModel / MjpcHipTask struct_size" : ": MjpcHipTask.struct_size") + " does not match this library" + hint);
  return false;
}

// Kernel flavour of the full-capacity launch: tables cached in LDS when that fits next to the candidate's state and a
// compile-time-nv kernel exists there; otherwise the flavour that reads them from HBM / L2; and when even that one's state exceeds
// 160 KiB, the spill flavour, which keeps the row- / contact-sized blocks in a per-candidate HBM slab (rollout_spill.hip).
// Host-only (no HIP call): mjpc_hip_create and mjpc_hip_debug_spill_layout share it.
static bool pick_flavour(const MjpcHipModel *model, const MjpcHipTask *task, int P_max, PackedModel &pm, RolloutFn *kernel, bool *cached, bool *spill, const char *who) {
  int exact_c = 0, exact_d = 0, exact_s = 0;
  RolloutFn kc = mjpc_pick_rollout_cached(model->nv, &exact_c), kd = mjpc_pick_rollout_direct(model->nv, &exact_d);
  RolloutFn ks = mjpc_pick_rollout_spill(model->nv, &exact_s);
  bool use_cache = !(exact_d && !exact_c);
  if (mjpc_host::debug_knob("no_model_cache")) use_cache = false;     // diagnostics knob (mjpc_hip_debug.h)
  std::string sp;
  const bool spill_all = mjpc_host::debug_knob("spill", &sp) && sp == "all";      // diagnostics knob: every eligible block in HBM
  *spill = false;
  // (the flavour without the whole copy still keeps the hot prefix - kinematic / tree tables - in LDS: hot_only)
  // (a compile-time-nv kernel solves with the Hessian in registers: its layout has no scaled-row table, host.h)
  if (spill_all) {
    use_cache = false; *spill = true;
    if (!mjpc_host::build(pm, model, task, P_max, false, false, true, exact_s != 0, SPILL_ALL)) { set_error(std::string(who) + ": " + pm.error); return false; }
  } else {
    if (!mjpc_host::build(pm, model, task, P_max, use_cache, false, !use_cache, use_cache ? exact_c != 0 : exact_d != 0)) { set_error(std::string(who) + ": " + pm.error); return false; }
    if (use_cache && (size_t)pm.L.total_doubles * sizeof(double) > 160 * 1024) {
      use_cache = false;
      if (!mjpc_host::build(pm, model, task, P_max, false, false, true, exact_d != 0)) { set_error(std::string(who) + ": " + pm.error); return false; }
    }
    if ((size_t)pm.L.total_doubles * sizeof(double) > 160 * 1024) {
      *spill = true;
      if (!mjpc_host::build(pm, model, task, P_max, false, false, true, exact_s != 0, SPILL_AUTO)) { set_error(std::string(who) + ": " + pm.error); return false; }
    }
  }
  if ((size_t)pm.L.total_doubles * sizeof(double) > 160 * 1024) {
    set_error(std::string(who) + ": per-candidate state exceeds 160 KiB of LDS even with the constraint-row and contact buffers in HBM; lower nconmax/nefcmax");
    return false;
  }
  *kernel = *spill ? ks : use_cache ? kc : kd;
  *cached = use_cache;
  return true;
}

// dense tier: needs a compile-time-nv kernel of that flavour, a model that asks for more capacity than the tier's and a
// layout of <= 80 KiB.  pm: the model as pick_flavour packed it (its own capacities)
static DenseTier pick_dense_tier(const MjpcHipModel *model, const MjpcHipTask *task, int P_max, const PackedModel &pm) {
  DenseTier plain, hot;
  int exact_b = 0;
  RolloutFn kb = mjpc_pick_rollout_dense2(model->nv, &exact_b);
  // (a model with a noslip pass runs at full capacity only: the pass recomputes qacc from efc_force, and the last commit's
  // force bits - unlike the iterate - are not pinned across kernel flavours, so the tiers would agree to rounding, not bit for bit)
  if (!(exact_b && model->noslip_iterations <= 0)) return plain;
  // capacity of the dense tier: the largest (rows, contacts = rows / 4 + 2) not above the model's own whose lean layout fits
  // 80 KiB; below 40 rows the retry pass would be the rule, not the exception
  int cap_e = 0, cap_c = 0;
  std::string cap;
  if (mjpc_host::debug_knob("dense_tier_cap", &cap)) {       // diagnostics knob "nefcmax,nconmax": a tiny dense tier forces the retry pass
    int a = 0, b = 0;
    if (sscanf(cap.c_str(), "%d,%d", &a, &b) == 2 && a > 0 && b > 0 && a <= pm.M.nefcmax && b <= pm.M.nconmax) { cap_e = a; cap_c = b; }
  }
  int first = pm.M.nefcmax < TIERB_NEFCMAX ? pm.M.nefcmax : TIERB_NEFCMAX;
  // two variants of the flavour: with the hot prefix of the tables in LDS (rollout_dense2h.hip; costs capacity) and without.
  // The hot-cached one is taken when it exists for this dof count and still holds TIERB_HOT_KEEP of the plain one's rows
  int exact_h = 0;
  RolloutFn kh = mjpc_pick_rollout_dense2h(model->nv, &exact_h);
  for (int variant = 0; variant < 2; variant++) {
    DenseTier &cd = variant ? hot : plain;
    if (variant && (!exact_h || cap_e)) break;          // (a forced tiny tier is the plain flavour's test case)
    for (int ne = cap_e ? cap_e : first; ne >= (cap_e ? cap_e : TIERB_NEFCMIN) && !cd.k; ne -= 4) {
      MjpcHipModel mb = *model;
      mb.nefcmax = ne; mb.nconmax = cap_e ? cap_c : ne / 4 + 2;
      if (mb.nconmax > pm.M.nconmax) mb.nconmax = pm.M.nconmax;
      PackedModel pmB;
      if (mjpc_host::build(pmB, &mb, task, P_max, false, true, variant == 1, true) && (size_t)pmB.L.total_doubles * sizeof(double) <= TIERB_LDS_LIMIT) {
        cd.k = variant ? kh : kb; cd.lay = pmB.L; cd.nefc = pmB.M.nefcmax; cd.ncon = pmB.M.nconmax;
        cd.ci = (int)pmB.cache_i; cd.cd = (int)pmB.cache_d;
        cd.lds = (size_t)pmB.L.total_doubles * sizeof(double);
      }
    }
  }
  return (hot.k && plain.k && hot.nefc * 100 >= plain.nefc * TIERB_HOT_KEEP) ? hot : plain;
}

extern "C" {
void mjpc_hip_destroy(MjpcHipEngine *e);

const char *mjpc_hip_last_error(void) { return g_error.c_str(); }
void mjpc_hip_debug_set(const char *name, const char *value) { if (name) mjpc_host::debug_set(name, value); }
int mjpc_hip_version(void) { return MJPC_HIP_ABI_VERSION; }
int mjpc_hip_sizeof_model(void) { return (int)sizeof(MjpcHipModel); }
int mjpc_hip_sizeof_task(void) { return (int)sizeof(MjpcHipTask); }
int mjpc_hip_sizeof_plan_input(void) { return (int)sizeof(MjpcHipPlanInput); }
int mjpc_hip_sizeof_plan_output(void) { return (int)sizeof(MjpcHipPlanOutput); }
int mjpc_hip_sizeof_feedback_policy(void) { return (int)sizeof(MjpcHipFeedbackPolicy); }

MjpcHipEngine *mjpc_hip_create(const MjpcHipModel *model, const MjpcHipTask *task, int max_local, int max_horizon, int device) {
  // arguments
  if (!model || !task || max_local < 1 || max_horizon < 1 || max_horizon > MJPC_MAX_HORIZON) { set_error("mjpc_hip_create: invalid argument"); return nullptr; }
  if (!check_views(model, task, "mjpc_hip_create", " (ABI revision " + std::to_string(MJPC_HIP_ABI_VERSION) + ": header and library out of step, or struct_size not set)")) return nullptr;
  int ndev = 0;
  MjpcHipEngine *e = nullptr;
  HIPCHKP(hipGetDeviceCount(&ndev));
  if (ndev < 1 || device < 0 || device >= ndev) { set_error("mjpc_hip_create: no such HIP device"); return nullptr; }
  HIPCHKP(hipSetDevice(device));
  e = new MjpcHipEngine();
  e->device = device;
  e->P_max = 36;     // MaxSamplingSplinePoints (mjpc/planners/sampling/planner.h:35-36)
  memset(&e->K, 0, sizeof(e->K));
  e->max_local = max_local; e->max_horizon = max_horizon;
  e->nq = model->nq; e->nv = model->nv; e->nu = model->nu; e->nmocap = model->nmocap; e->nuserdata = model->nuserdata;
  e->nr = task->num_residual; e->ntr = 3 * task->num_trace; e->ds = model->nq + model->nv + model->na;
  e->na = model->na; e->nd = 2 * model->nv + model->na;
  e->nbody = model->nbody; e->nsite = model->nsite;
  // flavour of the full-capacity launch, dense tier
  if (!pick_flavour(model, task, e->P_max, e->pm, &e->kernel, &e->cached, &e->spill, "mjpc_hip_create")) { mjpc_hip_destroy(e); return nullptr; }
  // (the compile-time-nv spill kernels' register-solver layout can fit without a slab where the generic direct one did not)
  if (e->spill) e->slab_bytes = (int)(((size_t)e->pm.slab_doubles * sizeof(double) + 255) / 256 * 256);
  e->lds_bytes = (size_t)e->pm.L.total_doubles * sizeof(double);
  e->tierB = pick_dense_tier(model, task, e->P_max, e->pm);
  if (e->tierB.k) e->ckpt_stride = 7 + e->nq + 2 * e->nv + model->na + 1;
  std::string tier, fi;                                 // diagnostics knobs: "A" = never the dense tier, "B" = always (when it exists)
  e->force_tier = mjpc_host::debug_knob("tier", &tier) ? (tier[0] == 'B' ? 2 : 1) : 0;
  e->fault = (mjpc_host::debug_knob("fault_inject", &fi) && fi == "sync") ? 1 : 0;
  // buffers of fixed size (the others grow with the calls), the model's image
  const size_t NL = (size_t)max_local, H = (size_t)max_horizon, D = sizeof(double), PN = (size_t)e->P_max * e->nu;
  Staging &s = e->hs;
  s.state = 0; s.mocap = s.state + e->ds; s.kt = s.mocap + 7 * e->nmocap; s.kv = s.kt + e->P_max; s.std = s.kv + PN; s.userdata = s.std + PN;
  s.size = s.userdata + e->nuserdata + 16;
  const struct { int b; size_t bytes; } fixed[] = {
    {B_IB, e->pm.ib.size() * sizeof(int)}, {B_DB, e->pm.db.size() * D},
    {B_SLAB, NL * e->slab_bytes},                // spill flavour: one slab per local candidate; holds no state across launches (like LDS)
    {B_STATE, D * (e->ds + 1)}, {B_MOCAP, D * (7 * e->nmocap + 7)}, {B_USERDATA, D * (e->nuserdata + 1)},
    {B_KT, D * e->P_max}, {B_KV, D * (PN + 1)}, {B_STD, D * (PN + 1)}, {B_SEL, sizeof(int) * NL},
    {B_RETURNS, D * NL}, {B_FAILURE, sizeof(int) * NL}, {B_DIAG, sizeof(int) * NL * 4}, {B_WINNER, sizeof(int) * 2}, {B_WINNER_VAL, D * 2},
    {B_FRAME, D * (18 * (size_t)e->nbody + 3 * (size_t)e->nsite + 1)}, {B_PROF, sizeof(long long) * NL * 24},
    {B_HIST, D * NL * e->P_max * (e->nu + 1)}, {B_SLOT, sizeof(int) * NL}, {B_SCALE, D * NL}, {B_GRAD, D * (PN + 1)},
    {B_CKPT, D * NL * e->ckpt_stride}, {H_SMALL, D * s.size}};
  for (const auto &f : fixed) HIPCHKP(e->buf[f.b].reserve(f.bytes));
  for (int k = 1; k < NROWS; k++) HIPCHKP(e->buf[B_KNOTS + k].reserve(D * NL * row_doubles(e, k, H, 0, true)));
  for (int b : {B_PROF, B_HIST, B_CKPT}) if (e->buf[b].p) HIPCHKP(hipMemset(e->buf[b].p, 0, e->buf[b].cap));
  if (upload_model(e) != 0) { mjpc_hip_destroy(e); return nullptr; }
  e->cost_rows_ok = cost_rows_tile(e);
  HIPCHKP(hipStreamCreate(&e->stream));
  for (int i = 0; i < 4; i++) HIPCHKP(hipEventCreate(&e->ev[i]));
  HIPCHKP(hipFuncSetAttribute((const void *)e->kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)e->lds_bytes));
  if (e->tierB.k) HIPCHKP(hipFuncSetAttribute((const void *)e->tierB.k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)e->tierB.lds));
  { hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) e->num_cu = prop.multiProcessorCount; }
  // kernel parameters that no call decides
  bind_params(e);
  return e;
}

void mjpc_hip_destroy(MjpcHipEngine *e) {
  if (!e) return;
  hipSetDevice(e->device);
  if (e->stream) hipStreamSynchronize(e->stream);
  for (DevBuf &b : e->buf) b.release();
  for (int i = 0; i < 2; i++) if (e->ev_task[i]) hipEventDestroy(e->ev_task[i]);
  for (int i = 0; i < 4; i++) if (e->ev[i]) hipEventDestroy(e->ev[i]);
  for (int i = 0; i < 2; i++) if (e->ev_fb[i]) hipEventDestroy(e->ev_fb[i]);
  if (e->stream) hipStreamDestroy(e->stream);
  delete e;
}

int mjpc_hip_set_task(MjpcHipEngine *e, const MjpcHipTask *task) {
  if (!e || !task) { set_error("mjpc_hip_set_task: invalid argument"); return -1; }
  if (!check_views(nullptr, task, "mjpc_hip_set_task")) return -1;
  HIPCHK(hipSetDevice(e->device));
  if (task->num_residual != e->nr || 3 * task->num_trace != e->ntr) { set_error("mjpc_hip_set_task: residual/trace dimensions changed"); return -1; }
  if (e->pending) { set_error("mjpc_hip_set_task: a plan step is in flight (call mjpc_hip_plan_fetch first)"); return -1; }
  if (!mjpc_host::repack_task(e->pm, task)) { set_error("mjpc_hip_set_task: " + e->pm.error); return -1; }
  e->cost_rows_ok = cost_rows_tile(e);
  // only the task block changes (cost table, residual parameters, frozen ResidualFn state): one small stream-ordered copy per
  // buffer out of the engine's own packed image, ahead of the next plan's kernels; the model and key-frame tables stay put
  const PackedModel &pm = e->pm;
  size_t bi = pm.task_i_cap * sizeof(int), bd = pm.task_d_cap * sizeof(double), bl = pm.late_cap * sizeof(int);
  int slot = e->task_slot ^= 1;                       // two pinned staging slots: the copy of the previous call may still be in flight
  HIPCHK(e->buf[H_TASK0 + slot].reserve(bi + bd + bl + 16));
  if (!e->ev_task[slot]) HIPCHK(hipEventCreateWithFlags(&e->ev_task[slot], hipEventDisableTiming));
  else HIPCHK(hipEventSynchronize(e->ev_task[slot]));
  char *h = e->at<char>(H_TASK0 + slot);
  memcpy(h, pm.db.data() + pm.task_d0, bd);
  memcpy(h + bd, pm.ib.data() + pm.task_i0, bi);
  if (bl) memcpy(h + bd + bi, pm.ib.data() + pm.late_i0, bl);
  HIPCHK(hipMemcpyAsync(e->at(B_DB) + pm.task_d0, h, bd, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(e->at<int>(B_IB) + pm.task_i0, h + bd, bi, hipMemcpyHostToDevice, e->stream));
  if (bl) HIPCHK(hipMemcpyAsync(e->at<int>(B_IB) + pm.late_i0, h + bd + bi, bl, hipMemcpyHostToDevice, e->stream));      // the late table (host.h)
  HIPCHK(hipEventRecord(e->ev_task[slot], e->stream));
  e->K.M = mjpc_host::relocate(e->pm, e->at<int>(B_IB), e->at(B_DB));
  return 0;
}

// first_explicit < 0: mjpc_hip_plan_async; >= 0: mjpc_hip_plan_mixed_async (the candidate table is assembled on the device)
static int plan_async_impl(MjpcHipEngine *e, const MjpcHipPlanInput *in, int first_explicit) {
  if (!e || !in) { set_error("mjpc_hip_plan: invalid argument"); return -1; }
  if (e->pending) { set_error("mjpc_hip_plan_async: the previous plan step has not been fetched (one plan in flight per engine)"); return -1; }
  int P = in->num_spline_points, H = in->horizon, nl = in->num_local, nu = e->nu;
  if (P < 1 || P > e->P_max) { set_error("mjpc_hip_plan: num_spline_points out of range (1..36)"); return -1; }
  if (H < 1 || H > e->max_horizon) { set_error("mjpc_hip_plan: horizon out of range"); return -1; }
  if (nl < 1 || nl > e->max_local || in->candidate_offset < 0 || in->candidate_offset + nl > in->num_trajectory) { set_error("mjpc_hip_plan: candidate range out of bounds"); return -1; }
  if (in->interpolation < 0 || in->interpolation > 2) { set_error("mjpc_hip_plan: unknown interpolation"); return -1; }
  if (!in->state || !in->knot_times || !in->knot_values || (e->nmocap > 0 && !in->mocap)) { set_error("mjpc_hip_plan: null input"); return -1; }
  e->fb_resampled = 0; e->fb_resample_us = 0;      // (mjpc_hip_feedback_resample_time_us speaks of the last call: this one resamples nothing)
  const bool mixed = first_explicit >= 0;
  if (mixed) {
    if (first_explicit > in->num_trajectory) { set_error("mjpc_hip_plan_mixed: first_explicit out of range (0..num_trajectory)"); return -1; }
    if (!in->noise_std) { set_error("mjpc_hip_plan_mixed: noise_std is required"); return -1; }
    if (first_explicit < in->num_trajectory && !in->candidate_knots) { set_error("mjpc_hip_plan_mixed: candidate_knots is required for the rows from first_explicit on"); return -1; }
  }
  if (in->xfrc_std > 0 && !(in->xfrc_rate > 0)) { set_error("mjpc_hip_plan: xfrc_rate must be positive when xfrc_std > 0"); return -1; }
  HIPCHK(hipSetDevice(e->device));
  // the buffers that grow with the plan (a repeated plan allocates nothing); the packed result: pack_kernel
  const size_t need = (size_t)nl * P * nu;
  const bool table = in->candidate_knots || mixed;
  const size_t need_pack = pack_doubles(e, nl, H, P);
  HIPCHK(e->buf[B_EPS].reserve(sizeof(double) * (need + 1)));
  HIPCHK(reserve_knots(e, P));
  if (table) HIPCHK(e->buf[B_CAND].reserve(sizeof(double) * (need + 1)));
  HIPCHK(e->buf[B_PACK].reserve(sizeof(double) * need_pack));
  HIPCHK(e->buf[H_PACK].reserve(sizeof(double) * need_pack));
  double *d_eps = e->at(B_EPS), *d_cand = e->at(B_CAND), *d_std = e->at(B_STD);
  int *d_sel = e->at<int>(B_SEL);
  // small inputs through pinned staging
  const Staging &s = e->hs;
  HIPCHK(stage(e, s.state, in->state, e->ds, B_STATE));
  if (e->nmocap) HIPCHK(stage(e, s.mocap, in->mocap, 7 * e->nmocap, B_MOCAP));
  HIPCHK(stage(e, s.kt, in->knot_times, P, B_KT));
  HIPCHK(stage(e, s.kv, in->knot_values, P * nu, B_KV));
  if (e->nuserdata) HIPCHK(stage(e, s.userdata, in->userdata, e->nuserdata, B_USERDATA));
  if (in->noise_std) HIPCHK(stage(e, s.std, in->noise_std, P * nu, B_STD));
  HIPCHK(hipEventRecord(e->ev[0], e->stream));
  if (in->noise_eps) {
    HIPCHK(hipMemcpyAsync(d_eps, in->noise_eps + (size_t)in->candidate_offset * P * nu, sizeof(double) * need, hipMemcpyHostToDevice, e->stream));
    if (in->noise_sel) HIPCHK(hipMemcpyAsync(d_sel, in->noise_sel + in->candidate_offset, sizeof(int) * nl, hipMemcpyHostToDevice, e->stream));
    else HIPCHK(hipMemsetAsync(d_sel, 0, sizeof(int) * nl, e->stream));
  } else {
    size_t total = need > (size_t)nl ? need : (size_t)nl;
    int blocks = (int)((total + 255) / 256);
    hipLaunchKernelGGL(noise_kernel, dim3(blocks), dim3(256), 0, e->stream, d_eps, d_sel, (unsigned long long)in->seed,
                       (unsigned long long)in->stream, in->candidate_offset, nl, P * nu, in->noise_exploration[1]);
  }
  // what this plan decides of the kernel parameters (the rest: bind_params)
  KParams &K = e->K;
  K.noise_eps = d_eps; K.noise_std = in->noise_std ? d_std : nullptr; K.cand_knots = table ? d_cand : nullptr;
  K.time = in->time; K.sigma0 = in->noise_exploration[0]; K.sigma1 = in->noise_exploration[1];
  K.seed = in->seed; K.stream = in->stream;
  K.P = P; K.interp = in->interpolation; K.H = H; K.N = in->num_trajectory; K.offset = in->candidate_offset; K.nlocal = nl;
  K.use_device_noise = in->noise_eps ? 0 : 1;
  K.nominal_index = in->nominal_index; K.xfrc_std = in->xfrc_std; K.xfrc_rate = in->xfrc_rate;
  if (table && !mixed) HIPCHK(hipMemcpyAsync(d_cand, in->candidate_knots + (size_t)in->candidate_offset * P * nu, sizeof(double) * need, hipMemcpyHostToDevice, e->stream));
  if (mixed) {
    // the caller's rows [first_explicit, offset + nl) verbatim, straight into the table; the kernel builds the rows below them
    const size_t row = (size_t)P * nu;
    const int r0 = first_explicit > in->candidate_offset ? first_explicit - in->candidate_offset : 0;      // first explicit local row
    if (r0 < nl) HIPCHK(hipMemcpyAsync(d_cand + r0 * row, in->candidate_knots + ((size_t)in->candidate_offset + r0) * row, sizeof(double) * (nl - r0) * row,
                                       hipMemcpyHostToDevice, e->stream));
    if (r0 > 0) {
      SgAssembleArgs sa{e->at(B_KV), d_std, d_eps, e->K.M.actuator_ctrlrange, d_cand, e->at(B_HIST), (long long)e->P_max * nu,
                        in->candidate_offset, nl, P * nu, nu, in->nominal_index, first_explicit};
      hipLaunchKernelGGL(sg_assemble_kernel, dim3((unsigned)((need + 255) / 256)), dim3(256), 0, e->stream, sa);
    }
    e->have_mixed = 1;
  }
  HIPCHK(hipEventRecord(e->ev[1], e->stream));
  const DenseTier &B = e->tierB;
  const bool dense = B.k && e->force_tier != 1 && (nl > e->num_cu || e->force_tier == 2) && !(in->xfrc_std > 0);   // (the lean layout has no body-force block)
  if (dense) {
    KParams KB = K;
    KB.M.nefcmax = B.nefc; KB.M.nconmax = B.ncon; KB.L = B.lay; KB.cache_i = B.ci; KB.cache_d = B.cd; KB.tier = 1;
    hipLaunchKernelGGL(B.k, dim3(nl), dim3(mjpc_rollout_threads_cached()), B.lds, e->stream, KB);
    K.retry = 1;                       // full capacity for whoever overflowed the dense tier (usually nobody: the launch drains at once)
  }
  hipLaunchKernelGGL(e->kernel, dim3(nl), dim3(mjpc_rollout_threads_cached()), e->lds_bytes, e->stream, K);
  K.retry = 0;
  e->last_dense = dense;
  HIPCHK(hipEventRecord(e->ev[2], e->stream));
  return plan_tail(e, nl, H, P, in->candidate_offset, need_pack);
}

int mjpc_hip_plan_async(MjpcHipEngine *e, const MjpcHipPlanInput *in) { return plan_async_impl(e, in, -1); }

// row arrays of local candidate `local` of the last plan from the device into the caller's (non-null) arrays
static int fetch_rows(MjpcHipEngine *e, int local, MjpcHipPlanOutput *out) {
  for (int k = 0; k < NROWS; k++) {
    const size_t n = row_doubles(e, k, e->last_H, e->last_P);
    if (out_row(out, k) && n) HIPCHK(hipMemcpyAsync(out_row(out, k), e->at(B_KNOTS + k) + local * n, sizeof(double) * n, hipMemcpyDeviceToHost, e->stream));
  }
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
}

int mjpc_hip_plan_fetch(MjpcHipEngine *e, MjpcHipPlanOutput *out) {
  if (!e || !out || !e->last_nlocal) { set_error("mjpc_hip_plan_fetch: nothing planned"); return -1; }
  HIPCHK(hipSetDevice(e->device));
  hipError_t sync_rc = hipStreamSynchronize(e->stream);       // the packed result of plan_async is in pinned host memory now
  // whatever this fetch returns, the plan step is over: the engine accepts the next plan_async / set_task (a failed fetch used
  // to leave `pending` set for good)
  const int was_pending = e->pending;
  e->pending = 0;
  if (sync_rc != hipSuccess) { set_error(std::string("mjpc_hip_plan_fetch: hipStreamSynchronize: ") + hipGetErrorString(sync_rc)); return -2; }
  if (was_pending && e->fb_resampled) { float tr = 0; hipEventElapsedTime(&tr, e->ev_fb[0], e->ev_fb[1]); e->fb_resample_us = 1e3 * tr; }
  if (was_pending) {
    float t01 = 0, t12 = 0, t03 = 0;
    hipEventElapsedTime(&t01, e->ev[0], e->ev[1]); hipEventElapsedTime(&t12, e->ev[1], e->ev[2]); hipEventElapsedTime(&t03, e->ev[0], e->ev[3]);
    out->noise_compute_time_us = 1e3 * t01; out->rollouts_compute_time_us = 1e3 * t12;
    e->acc_rollout_us += 1e3 * t12; e->acc_total_us += 1e3 * t03; e->acc_n++;
  }
  const double *p = e->at(H_PACK);
  int nl = e->last_nlocal;
  int wl = (int)p[0]; double wv = p[1];
  p += 2;
  if (out->returns) memcpy(out->returns, p, sizeof(double) * nl);
  if (out->failure) for (int i = 0; i < nl; i++) out->failure[i] = (int)p[nl + i];
  p += 2 * (size_t)nl;
  // no candidate with a comparable return (every return NaN, e.g. a NaN cost weight): returns[] / failure[] above are valid,
  // there is no winner
  if (wl < 0 || wl >= nl) { set_error("mjpc_hip_plan_fetch: no finite return among the candidates (argmin out of range)"); return -3; }
  out->winner = e->last_offset + wl; out->winner_return = wv;
  for (int k = 0; k < (e->last_summary ? 1 : NROWS); k++) {        // summary mode: the rows stay on the device (mjpc_hip_get_candidate)
    const size_t n = row_doubles(e, k, e->last_H, e->last_P);
    if (out_row(out, k) && n) memcpy(out_row(out, k), p, sizeof(double) * n);
    p += n;
  }
  return 0;
}

int mjpc_hip_set_fetch_mode(MjpcHipEngine *e, int mode) {
  if (!e || (mode != MJPC_FETCH_WINNER_ROWS && mode != MJPC_FETCH_SUMMARY)) { set_error("mjpc_hip_set_fetch_mode: invalid argument"); return -1; }
  e->summary_only = mode == MJPC_FETCH_SUMMARY;
  return 0;
}

int mjpc_hip_plan(MjpcHipEngine *e, const MjpcHipPlanInput *in, MjpcHipPlanOutput *out) {
  int rc = mjpc_hip_plan_async(e, in);
  if (rc != 0) return rc;
  return mjpc_hip_plan_fetch(e, out);
}

// ------------------------------------------------------------------------------ rollouts under a feedback policy (feedback.h)
int mjpc_hip_plan_feedback_async(MjpcHipEngine *e, const MjpcHipPlanInput *in, const MjpcHipFeedbackPolicy *p) {
  const char *who = "mjpc_hip_plan_feedback";
  auto bad = [&](const std::string &m) { set_error(std::string(who) + ": " + m); return -1; };
  if (!e || !in || !p) return bad("invalid argument");
  if (p->struct_size != (int)sizeof(MjpcHipFeedbackPolicy)) return bad("MjpcHipFeedbackPolicy.struct_size does not match this library");
  if (e->pending) return bad("the previous plan step has not been fetched (one plan in flight per engine)");
  const int H = in->horizon, nl = in->num_trajectory - in->candidate_offset, nu = e->nu, ds = e->ds, nv = e->nv, nd = e->nd, T = p->T;
  if (nu < 1) return bad("the model has no actuators");
  if (H < 1 || H > e->max_horizon) return bad("horizon out of range");
  if (in->candidate_offset < 0 || nl < 1) return bad("candidate range out of bounds");
  if (nl > e->max_local) return bad("the batch exceeds max_samples (" + std::to_string(e->max_local) + ")");
  if (p->mode != MJPC_FEEDBACK_INDEXED && p->mode != MJPC_FEEDBACK_TIME) return bad("unknown mode");
  if (T < 2) return bad("T < 2");
  if (p->mode == MJPC_FEEDBACK_INDEXED && T < H) return bad("indexed mode needs T >= horizon");
  if (p->mode == MJPC_FEEDBACK_TIME && (p->representation < 0 || p->representation > 2)) return bad("unknown representation");
  if (!in->state || (e->nmocap > 0 && !in->mocap) || !p->times || !p->states || !p->actions || !p->feedback_gain || !p->action_step || !p->feedback_scaling) return bad("null input");
  for (int i = 0; i < nl; i++) {
    const double a = p->action_step[in->candidate_offset + i], s = p->feedback_scaling[in->candidate_offset + i];
    if (a != a || s != s) return bad("NaN in action_step / feedback_scaling of candidate " + std::to_string(in->candidate_offset + i));
  }
  if (nd > FB_DX_CAPACITY(nv)) return bad("2 nv + na exceeds the state-difference scratch of the kernel");
  HIPCHK(hipSetDevice(e->device));
  if (!e->fb_kernel) for (int i = 0; i < 2; i++) HIPCHK(hipEventCreate(&e->ev_fb[i]));      // (the resampling's two, with the family's first call)
  if (int rc = FAMILY_KERNEL(e, fb)) return rc;
  // the call's device block (FbLay, carve.h)
  const size_t Tz = (size_t)T;
  const bool timed = p->mode == MJPC_FEEDBACK_TIME;
  const size_t need_pack = pack_doubles(e, nl, H, 0);
  FbLay L;
  PLACE(B_FBP, L, e->dims(), Tz, H, nl, timed);
  HIPCHK(reserve_knots(e, 1));
  HIPCHK(e->buf[B_PACK].reserve(sizeof(double) * need_pack));
  HIPCHK(e->buf[H_PACK].reserve(sizeof(double) * need_pack));
  double *d_impr = p->action_improvement ? L.improvement : nullptr;
  const Staging &s = e->hs;
  HIPCHK(stage(e, s.state, in->state, ds, B_STATE));
  if (e->nmocap) HIPCHK(stage(e, s.mocap, in->mocap, 7 * e->nmocap, B_MOCAP));
  if (e->nuserdata) HIPCHK(stage(e, s.userdata, in->userdata, e->nuserdata, B_USERDATA));
  HIPCHK(hipEventRecord(e->ev[0], e->stream));
  const size_t D = sizeof(double);
  HIPCHK(hipMemcpyAsync(L.times, p->times, D * Tz, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(L.states, p->states, D * Tz * ds, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(L.actions, p->actions, D * Tz * nu, hipMemcpyHostToDevice, e->stream));
  if (d_impr) HIPCHK(hipMemcpyAsync(d_impr, p->action_improvement, D * Tz * nu, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(L.gain, p->feedback_gain, D * Tz * nu * nd, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(L.alpha, p->action_step + in->candidate_offset, D * nl, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(L.scale, p->feedback_scaling + in->candidate_offset, D * nl, hipMemcpyHostToDevice, e->stream));
  const double *xbar = L.states, *ubar = L.actions, *kbar = d_impr, *Kbar = L.gain;
  e->fb_resampled = 0; e->fb_resample_us = 0;
  if (timed) {
    FbResampleArgs ra;
    ra.times = L.times; ra.states = L.states; ra.actions = L.actions; ra.gains = L.gain; ra.improvement = d_impr;
    ra.jnt_type = e->K.M.jnt_type; ra.jnt_qposadr = e->K.M.jnt_qposadr;
    ra.T = T; ra.H = H; ra.ds = ds; ra.nu = nu; ra.nd = nd; ra.njnt = e->K.M.njnt; ra.representation = p->representation;
    ra.time0 = in->time; ra.timestep = e->K.M.timestep;
    ra.xbar = L.xbar; ra.ubar = L.ubar; ra.kbar = L.kbar; ra.Kbar = L.Kbar;
    HIPCHK(hipEventRecord(e->ev_fb[0], e->stream));
    hipLaunchKernelGGL(fb_resample_kernel, dim3(H), dim3(256), 0, e->stream, ra);
    HIPCHK(hipEventRecord(e->ev_fb[1], e->stream));
    e->fb_resampled = 1;
    xbar = ra.xbar; ubar = ra.ubar; kbar = d_impr ? ra.kbar : nullptr; Kbar = ra.Kbar;
  }
  if (!p->use_feedback) xbar = nullptr;
  KParams K = bare_params(e);
  K.time = in->time; K.P = 0; K.H = H; K.N = in->num_trajectory; K.offset = in->candidate_offset; K.nlocal = nl;
  HIPCHK(hipEventRecord(e->ev[1], e->stream));
  e->fb_launch(e->fb_kernel, nl, e->lds_bytes, e->stream, &K, xbar, ubar, kbar, Kbar, L.alpha, L.scale);
  e->last_dense = 0;
  HIPCHK(hipEventRecord(e->ev[2], e->stream));
  return plan_tail(e, nl, H, 0, in->candidate_offset, need_pack);
}

int mjpc_hip_plan_feedback(MjpcHipEngine *e, const MjpcHipPlanInput *in, const MjpcHipFeedbackPolicy *p, MjpcHipPlanOutput *out) {
  int rc = mjpc_hip_plan_feedback_async(e, in, p);
  if (rc != 0) return rc;
  return mjpc_hip_plan_fetch(e, out);
}

double mjpc_hip_feedback_resample_time_us(MjpcHipEngine *e) { return e ? e->fb_resample_us : 0.0; }

int mjpc_hip_plan_mixed_async(MjpcHipEngine *e, const MjpcHipPlanInput *in, int first_explicit) {
  if (first_explicit < 0) { set_error("mjpc_hip_plan_mixed: first_explicit out of range (0..num_trajectory)"); return -1; }
  return plan_async_impl(e, in, first_explicit);
}

int mjpc_hip_plan_mixed(MjpcHipEngine *e, const MjpcHipPlanInput *in, int first_explicit, MjpcHipPlanOutput *out) {
  int rc = mjpc_hip_plan_mixed_async(e, in, first_explicit);
  if (rc != 0) return rc;
  return mjpc_hip_plan_fetch(e, out);
}

int mjpc_hip_noise_history_reset(MjpcHipEngine *e) {
  if (!e) { set_error("mjpc_hip_noise_history_reset: invalid argument"); return -1; }
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipMemsetAsync(e->at(B_HIST), 0, sizeof(double) * (size_t)e->max_local * e->P_max * e->nu, e->stream));     // stream-ordered: behind a plan in flight
  return 0;
}

int mjpc_hip_sample_gradient(MjpcHipEngine *e, int n, const int *slot, const double *scale, double *gradient_out) {
  if (!e || !slot || !scale || !gradient_out) { set_error("mjpc_hip_sample_gradient: invalid argument"); return -1; }
  if (e->pending) { set_error("mjpc_hip_sample_gradient: a plan step is in flight (call mjpc_hip_plan_fetch first)"); return -1; }
  if (!e->have_mixed || e->last_P < 1) { set_error("mjpc_hip_sample_gradient: no mixed plan yet (mjpc_hip_plan_mixed fills the noise history)"); return -1; }
  if (n < 1 || n > e->max_local) { set_error("mjpc_hip_sample_gradient: n out of range (1..max_local)"); return -1; }
  for (int i = 0; i < n; i++)
    if (slot[i] < 0 || slot[i] >= e->max_local) { set_error("mjpc_hip_sample_gradient: slot[" + std::to_string(i) + "] = " + std::to_string(slot[i]) + " out of range (0..max_local-1)"); return -1; }
  HIPCHK(hipSetDevice(e->device));
  const int PN = e->last_P * e->nu;
  HIPCHK(hipMemcpyAsync(e->at(B_SLOT), slot, sizeof(int) * n, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(e->at(B_SCALE), scale, sizeof(double) * n, hipMemcpyHostToDevice, e->stream));
  SgGradArgs ga{e->at(B_HIST), (long long)e->P_max * e->nu, e->at<int>(B_SLOT), e->at(B_SCALE), n, PN, e->at(B_GRAD)};
  hipLaunchKernelGGL(sg_gradient_kernel, dim3((PN + SG_KT - 1) / SG_KT), dim3(256), 0, e->stream, ga);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(gradient_out, e->at(B_GRAD), sizeof(double) * PN, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
}

// ------------------------------------------------------------------------------ batched one-step evaluation, FD derivatives
// common front of mjpc_hip_step_batch / mjpc_hip_transition_fd: argument checks that do not depend on the call, the step kernel
// of the engine's flavour, the shared inputs (mocap, userdata) and the kernel parameters of a one-step launch
static int step_prepare(MjpcHipEngine *e, const char *who, const double *mocap, const double *userdata, KParams *Kout) {
  if (e->pending) { set_error(std::string(who) + ": a plan step is in flight (call mjpc_hip_plan_fetch first)"); return -1; }
  if (e->max_horizon < 2) { set_error(std::string(who) + ": the engine was created with max_horizon < 2 (a step records two state rows)"); return -1; }
  if (e->nmocap > 0 && !mocap) { set_error(std::string(who) + ": null input"); return -1; }
  HIPCHK(hipSetDevice(e->device));
  if (int rc = FAMILY_KERNEL(e, step)) return rc;
  HIPCHK(reserve_knots(e, 1));
  if (e->nmocap) HIPCHK(stage(e, e->hs.mocap, mocap, 7 * e->nmocap, B_MOCAP));
  if (e->nuserdata) HIPCHK(stage(e, e->hs.userdata, userdata, e->nuserdata, B_USERDATA));
  // a step has no plan state either, one knot (its control) and two state rows per workgroup
  KParams K = bare_params(e);
  K.state = nullptr;
  K.frame = nullptr;                       // (the kinematic frame of the last plan stays what it was)
  K.time = 0; K.P = 1; K.H = 2; K.N = e->max_local; K.offset = 0; K.nlocal = 0;
  *Kout = K;
  // the row buffers are about to be overwritten: the last plan's candidates are no longer there to be fetched
  e->last_nlocal = 0;
  return 0;
}

// rows [0, rows) of the tables through the step kernel, at most max_local workgroups per launch (stream-ordered: a launch reuses
// the row buffers, the slab and the CU's LDS of the one before it)
static void step_rows(MjpcHipEngine *e, const KParams &K, size_t rows, const StepTab &t) {
  // the task's late table (host.h): null without late rows, and the step kernel then has no late phase
  const int *late = e->pm.late_blocks ? e->at<int>(B_IB) + e->pm.late_i0 : nullptr;
  for (size_t r0 = 0; r0 < rows; r0 += (size_t)e->max_local) {
    const int nl = (int)(rows - r0 < (size_t)e->max_local ? rows - r0 : (size_t)e->max_local);
    e->step_launch(e->step_kernel, nl, e->lds_bytes, e->stream, &K, t.state + r0 * e->ds, t.ctrl + r0 * e->nu, t.time + r0, t.next + r0 * e->ds,
                   t.residual + r0 * e->nr, t.fail + r0, late);
  }
}

// rows of one pass over the device tables: bounds the memory of a call whose n / T is large (the passes are independent)
#define STEP_PASS_ROWS 32768

int mjpc_hip_step_batch(MjpcHipEngine *e, int n, const double *states, const double *ctrl, const double *time, const double *mocap,
                        const double *userdata, double *next_states, double *residual, int *failure) {
  if (!e) { set_error("mjpc_hip_step_batch: invalid argument"); return -1; }
  if (n < 1) { set_error("mjpc_hip_step_batch: n < 1"); return -1; }
  if (!states || !time || (e->nu > 0 && !ctrl) || !next_states || !residual || !failure) { set_error("mjpc_hip_step_batch: null input"); return -1; }
  KParams K;
  int rc = step_prepare(e, "mjpc_hip_step_batch", mocap, userdata, &K);
  if (rc != 0) return rc;
  const size_t ds = e->ds, nu = e->nu, nr = e->nr;
  for (size_t p0 = 0; p0 < (size_t)n; p0 += STEP_PASS_ROWS) {
    const size_t R = (size_t)n - p0 < STEP_PASS_ROWS ? (size_t)n - p0 : STEP_PASS_ROWS;
    StepTab t;
    PLACE(B_FD, t, e->dims(), R);
    HIPCHK(hipMemcpyAsync(t.state, states + p0 * ds, sizeof(double) * R * ds, hipMemcpyHostToDevice, e->stream));
    if (nu) HIPCHK(hipMemcpyAsync(t.ctrl, ctrl + p0 * nu, sizeof(double) * R * nu, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(t.time, time + p0, sizeof(double) * R, hipMemcpyHostToDevice, e->stream));
    step_rows(e, K, R, t);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(next_states + p0 * ds, t.next, sizeof(double) * R * ds, hipMemcpyDeviceToHost, e->stream));
    if (nr) HIPCHK(hipMemcpyAsync(residual + p0 * nr, t.residual, sizeof(double) * R * nr, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(failure + p0, t.fail, sizeof(int) * R, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
  }
  return 0;
}

// dof -> (qpos address, quaternion axis or -1) from the engine's own packed model
static std::vector<int> fd_dofmap(const MjpcHipEngine *e) {
  const int nv = e->nv;
  std::vector<int> dofmap(2 * nv + 2, -1);
  const DevModel hm = mjpc_host::relocate(e->pm, e->pm.ib.data(), e->pm.db.data());
  for (int j = 0; j < hm.njnt; j++) {
    const int type = hm.jnt_type[j], qa = hm.jnt_qposadr[j], da = hm.jnt_dofadr[j];
    if (type == 0) { for (int k = 0; k < 3; k++) { dofmap[2 * (da + k)] = qa + k; dofmap[2 * (da + k) + 1] = -1; dofmap[2 * (da + 3 + k)] = qa + 3; dofmap[2 * (da + 3 + k) + 1] = k; } }
    else if (type == 1) { for (int k = 0; k < 3; k++) { dofmap[2 * (da + k)] = qa; dofmap[2 * (da + k) + 1] = k; } }
    else { dofmap[2 * da] = qa; dofmap[2 * da + 1] = -1; }
  }
  return dofmap;
}

// one pass of mjpc_hip_transition_fd over the Tg knots from t0 on, everything stream-ordered and nothing downloaded: the nominal rows
// go up, the table is assembled, stepped and differenced; the matrices and failure[] stay in B_FD where `a` points.  L: the pass's
// layout, placed by the caller (alone, or inside the layout of a call that keeps more behind the pass's doubles)
static int fd_pass(MjpcHipEngine *e, const KParams &K, const std::vector<int> &dofmap, const FdLay &L, size_t t0, size_t Tg, int term, const double *x,
                   const double *u, const double *time, double eps, int centered, FdArgs *out) {
  const size_t ds = e->ds, nu = e->nu, nr = e->nr, nv = e->nv, nd = e->nd, R = L.R;
  HIPCHK(hipMemcpyAsync(L.x, x + t0 * ds, sizeof(double) * Tg * ds, hipMemcpyHostToDevice, e->stream));
  if (nu) HIPCHK(hipMemcpyAsync(L.u, u + t0 * nu, sizeof(double) * Tg * nu, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(L.time, time + t0, sizeof(double) * Tg, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(L.dofmap, dofmap.data(), sizeof(int) * (2 * nv + 2), hipMemcpyHostToDevice, e->stream));
  FdArgs a;
  a.x = L.x; a.u = L.u; a.time = L.time; a.dofmap = L.dofmap; a.ctrllimited = e->K.M.actuator_ctrllimited; a.ctrlrange = e->K.M.actuator_ctrlrange;
  a.T = (int)Tg; a.nq = e->nq; a.nv = e->nv; a.na = e->na; a.nu = e->nu; a.nr = e->nr; a.centered = centered; a.last_is_terminal = term;
  a.eps = eps; a.cs = cos(0.5 * eps); a.sn = sin(0.5 * eps);
  a.state_tab = L.t.state; a.ctrl_tab = L.t.ctrl; a.time_tab = L.t.time; a.next_state = L.t.next; a.residual = L.t.residual; a.fail = L.t.fail;
  a.A = L.A; a.B = L.B; a.C = L.C; a.D = L.D; a.failure = L.failure;
  hipLaunchKernelGGL(fd_assemble_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, e->stream, a, (unsigned)R);
  step_rows(e, K, R, L.t);
  hipLaunchKernelGGL(fd_difference_kernel, dim3((unsigned)((nd + nu + FD_TILE - 1) / FD_TILE), (unsigned)((nd + nr + FD_TILE - 1) / FD_TILE), (unsigned)Tg),
                     dim3(FD_TILE * FD_TILE), 0, e->stream, a);
  HIPCHK(hipGetLastError());
  *out = a;
  return 0;
}
// knots of one pass: its table stays below STEP_PASS_ROWS rows
static size_t fd_pass_knots(const MjpcHipEngine *e, int centered) {
  const size_t E = fd_rows_per_knot(e->dims(), centered);
  return STEP_PASS_ROWS / E < 1 ? 1 : STEP_PASS_ROWS / E;
}

int mjpc_hip_transition_fd(MjpcHipEngine *e, int T, const double *x, const double *u, const double *time, const double *mocap,
                           const double *userdata, double eps, int centered, int last_is_terminal, double *A, double *B, double *C,
                           double *D, int *failure) {
  if (!e) { set_error("mjpc_hip_transition_fd: invalid argument"); return -1; }
  if (T < 1) { set_error("mjpc_hip_transition_fd: T < 1"); return -1; }
  if (!(eps > 0)) { set_error("mjpc_hip_transition_fd: eps <= 0"); return -1; }
  if (!x || !time || (e->nu > 0 && !u) || !A || !B || !C || !D || !failure) { set_error("mjpc_hip_transition_fd: null input"); return -1; }
  KParams K;
  int rc = step_prepare(e, "mjpc_hip_transition_fd", mocap, userdata, &K);
  if (rc != 0) return rc;
  centered = centered ? 1 : 0; last_is_terminal = last_is_terminal ? 1 : 0;
  const size_t nu = e->nu, nr = e->nr, nd = e->nd;
  const std::vector<int> dofmap = fd_dofmap(e);
  const size_t Tg_max = fd_pass_knots(e, centered);
  for (size_t t0 = 0; t0 < (size_t)T; t0 += Tg_max) {
    const size_t Tg = (size_t)T - t0 < Tg_max ? (size_t)T - t0 : Tg_max;
    const int term = last_is_terminal && t0 + Tg == (size_t)T;
    FdLay L;
    PLACE(B_FD, L, e->dims(), Tg, centered);
    FdArgs a;
    rc = fd_pass(e, K, dofmap, L, t0, Tg, term, x, u, time, eps, centered, &a);
    if (rc != 0) return rc;
    const size_t Tw = Tg - (term ? 1 : 0);            // a terminal knot's A / B / D blocks stay the caller's
    if (Tw && nd) HIPCHK(hipMemcpyAsync(A + t0 * nd * nd, a.A, sizeof(double) * Tw * nd * nd, hipMemcpyDeviceToHost, e->stream));
    if (Tw && nd * nu) HIPCHK(hipMemcpyAsync(B + t0 * nd * nu, a.B, sizeof(double) * Tw * nd * nu, hipMemcpyDeviceToHost, e->stream));
    if (nr * nd) HIPCHK(hipMemcpyAsync(C + t0 * nr * nd, a.C, sizeof(double) * Tg * nr * nd, hipMemcpyDeviceToHost, e->stream));
    if (Tw && nr * nu) HIPCHK(hipMemcpyAsync(D + t0 * nr * nu, a.D, sizeof(double) * Tw * nr * nu, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(failure + t0, a.failure, sizeof(int) * Tg, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
  }
  return 0;
}

// ------------------------------------------------------------------------------ batched inverse dynamics, FD derivatives
// common front of mjpc_hip_inverse_batch / mjpc_hip_inverse_fd: the refusal of the discrete form for the dense implicit integrators (before
// anything is touched), step_prepare's checks, inputs and parameters, and the inverse kernel of the engine's flavour
static int inverse_prepare(MjpcHipEngine *e, const char *who, const double *mocap, const double *userdata, int discrete, KParams *Kout) {
  if (discrete && e->K.M.int_dense) {
    set_error(std::string(who) + ": discrete != 0 is not built for models with a dense implicit integrator (mjINT_IMPLICIT, implicitfast with fluid forces): "
              "the integrator's matrix needs the velocity derivative of the bias forces; use discrete = 0");
    return -1;
  }
  // (step_prepare also picks the step kernel of the flavour and sets its LDS attribute at the engine's first one-step call: an inverse call
  // never launches it, the coupling only loads that kernel's code object early; its checks, staged inputs and parameters are what is wanted)
  int rc = step_prepare(e, who, mocap, userdata, Kout);
  if (rc != 0) return rc;
  return FAMILY_KERNEL(e, inv);
}

// rows [0, rows) of the tables through the inverse kernel, at most max_local workgroups per launch (stream-ordered, as step_rows)
static void inverse_rows(MjpcHipEngine *e, const KParams &K, size_t rows, const InvTab &t, int discrete) {
  const int *late = e->pm.late_blocks ? e->at<int>(B_IB) + e->pm.late_i0 : nullptr;
  for (size_t r0 = 0; r0 < rows; r0 += (size_t)e->max_local) {
    const int nl = (int)(rows - r0 < (size_t)e->max_local ? rows - r0 : (size_t)e->max_local);
    e->inv_launch(e->inv_kernel, nl, e->lds_bytes, e->stream, &K, t.state + r0 * e->ds, t.ctrl + r0 * e->nu, t.time + r0, t.qacc + r0 * e->nv, discrete,
                  t.qfrc + r0 * e->nv, t.qfrc_constraint + r0 * e->nv, t.residual + r0 * e->nr, t.fail + r0, late);
  }
}

int mjpc_hip_inverse_batch(MjpcHipEngine *e, int n, const double *states, const double *ctrl, const double *qacc, const double *time, const double *mocap,
                           const double *userdata, int discrete, double *qfrc_inverse, double *qfrc_constraint, double *residual, int *failure) {
  if (!e) { set_error("mjpc_hip_inverse_batch: invalid argument"); return -1; }
  if (n < 1) { set_error("mjpc_hip_inverse_batch: n < 1"); return -1; }
  if (!states || !time || !qacc || (e->nu > 0 && !ctrl) || !qfrc_inverse || !failure) { set_error("mjpc_hip_inverse_batch: null input"); return -1; }
  KParams K;
  discrete = discrete ? 1 : 0;
  int rc = inverse_prepare(e, "mjpc_hip_inverse_batch", mocap, userdata, discrete, &K);
  if (rc != 0) return rc;
  const size_t ds = e->ds, nu = e->nu, nr = e->nr, nv = e->nv;
  for (size_t p0 = 0; p0 < (size_t)n; p0 += STEP_PASS_ROWS) {
    const size_t R = (size_t)n - p0 < STEP_PASS_ROWS ? (size_t)n - p0 : STEP_PASS_ROWS;
    InvTab t;
    PLACE(B_FD, t, e->dims(), R);
    HIPCHK(hipMemcpyAsync(t.state, states + p0 * ds, sizeof(double) * R * ds, hipMemcpyHostToDevice, e->stream));
    if (nu) HIPCHK(hipMemcpyAsync(t.ctrl, ctrl + p0 * nu, sizeof(double) * R * nu, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(t.time, time + p0, sizeof(double) * R, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(t.qacc, qacc + p0 * nv, sizeof(double) * R * nv, hipMemcpyHostToDevice, e->stream));
    inverse_rows(e, K, R, t, discrete);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(qfrc_inverse + p0 * nv, t.qfrc, sizeof(double) * R * nv, hipMemcpyDeviceToHost, e->stream));
    if (qfrc_constraint) HIPCHK(hipMemcpyAsync(qfrc_constraint + p0 * nv, t.qfrc_constraint, sizeof(double) * R * nv, hipMemcpyDeviceToHost, e->stream));
    if (nr && residual) HIPCHK(hipMemcpyAsync(residual + p0 * nr, t.residual, sizeof(double) * R * nr, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(failure + p0, t.fail, sizeof(int) * R, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
  }
  return 0;
}

int mjpc_hip_inverse_fd(MjpcHipEngine *e, int T, const double *states, const double *ctrl, const double *qacc, const double *time, const double *mocap,
                        const double *userdata, int discrete, double eps, int centered, double *DfDq, double *DfDv, double *DfDa, double *DsDq,
                        double *DsDv, double *DsDa, int *failure) {
  if (!e) { set_error("mjpc_hip_inverse_fd: invalid argument"); return -1; }
  if (T < 1) { set_error("mjpc_hip_inverse_fd: T < 1"); return -1; }
  if (!(eps > 0)) { set_error("mjpc_hip_inverse_fd: eps <= 0"); return -1; }
  if (!states || !time || !qacc || (e->nu > 0 && !ctrl) || !failure) { set_error("mjpc_hip_inverse_fd: null input"); return -1; }
  KParams K;
  discrete = discrete ? 1 : 0; centered = centered ? 1 : 0;
  int rc = inverse_prepare(e, "mjpc_hip_inverse_fd", mocap, userdata, discrete, &K);
  if (rc != 0) return rc;
  const size_t ds = e->ds, nu = e->nu, nr = e->nr, nv = e->nv;
  const std::vector<int> dofmap = fd_dofmap(e);
  const size_t E = inv_fd_rows_per_config(e->dims(), centered), Tg_max = STEP_PASS_ROWS / E < 1 ? 1 : STEP_PASS_ROWS / E;
  double *const Df[3] = {DfDq, DfDv, DfDa}, *const Ds[3] = {DsDq, DsDv, DsDa};
  for (size_t t0 = 0; t0 < (size_t)T; t0 += Tg_max) {
    const size_t Tg = (size_t)T - t0 < Tg_max ? (size_t)T - t0 : Tg_max;
    InvFdLay L;
    PLACE(B_FD, L, e->dims(), Tg, centered);
    HIPCHK(hipMemcpyAsync(L.x, states + t0 * ds, sizeof(double) * Tg * ds, hipMemcpyHostToDevice, e->stream));
    if (nu) HIPCHK(hipMemcpyAsync(L.u, ctrl + t0 * nu, sizeof(double) * Tg * nu, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(L.a, qacc + t0 * nv, sizeof(double) * Tg * nv, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(L.time, time + t0, sizeof(double) * Tg, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(L.dofmap, dofmap.data(), sizeof(int) * (2 * nv + 2), hipMemcpyHostToDevice, e->stream));
    InvFdArgs a;
    a.x = L.x; a.u = L.u; a.a = L.a; a.time = L.time; a.dofmap = L.dofmap;
    a.T = (int)Tg; a.nq = e->nq; a.nv = e->nv; a.na = e->na; a.nu = e->nu; a.nr = e->nr; a.centered = centered;
    a.eps = eps; a.cs = cos(0.5 * eps); a.sn = sin(0.5 * eps);
    a.state_tab = L.t.state; a.ctrl_tab = L.t.ctrl; a.time_tab = L.t.time; a.qacc_tab = L.t.qacc; a.qfrc = L.t.qfrc; a.residual = L.t.residual; a.fail = L.t.fail;
    // a block the caller does not want is not computed
    a.DfDq = Df[0] ? L.Df[0] : nullptr; a.DfDv = Df[1] ? L.Df[1] : nullptr; a.DfDa = Df[2] ? L.Df[2] : nullptr;
    a.DsDq = Ds[0] && nr ? L.Ds[0] : nullptr; a.DsDv = Ds[1] && nr ? L.Ds[1] : nullptr; a.DsDa = Ds[2] && nr ? L.Ds[2] : nullptr;
    a.failure = L.failure;
    hipLaunchKernelGGL(ifd_assemble_kernel, dim3((unsigned)((L.R + 3) / 4)), dim3(256), 0, e->stream, a, (unsigned)L.R);
    inverse_rows(e, K, L.R, L.t, discrete);
    hipLaunchKernelGGL(ifd_difference_kernel, dim3((unsigned)((3 * nv + FD_TILE - 1) / FD_TILE), (unsigned)((nv + nr + FD_TILE - 1) / FD_TILE), (unsigned)Tg),
                       dim3(FD_TILE * FD_TILE), 0, e->stream, a);
    HIPCHK(hipGetLastError());
    for (int k = 0; k < 3; k++) {
      if (Df[k]) HIPCHK(hipMemcpyAsync(Df[k] + t0 * nv * nv, L.Df[k], sizeof(double) * Tg * nv * nv, hipMemcpyDeviceToHost, e->stream));
      if (Ds[k] && nr) HIPCHK(hipMemcpyAsync(Ds[k] + t0 * nr * nv, L.Ds[k], sizeof(double) * Tg * nr * nv, hipMemcpyDeviceToHost, e->stream));
    }
    HIPCHK(hipMemcpyAsync(failure + t0, L.failure, sizeof(int) * Tg, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
  }
  return 0;
}

// ------------------------------------------------------------------------------ estimators: unscented moments, one-knot linearisation
// position coordinate -> (dof, quaternion component or -1): the inverse of fd_dofmap
static std::vector<int> ukf_qmap(const MjpcHipEngine *e) {
  std::vector<int> qmap(2 * e->nq + 2, -1);
  const DevModel hm = mjpc_host::relocate(e->pm, e->pm.ib.data(), e->pm.db.data());
  for (int j = 0; j < hm.njnt; j++) {
    const int type = hm.jnt_type[j], qa = hm.jnt_qposadr[j], da = hm.jnt_dofadr[j];
    if (type == 0) { for (int k = 0; k < 3; k++) { qmap[2 * (qa + k)] = da + k; qmap[2 * (qa + k) + 1] = -1; }
                     for (int k = 0; k < 4; k++) { qmap[2 * (qa + 3 + k)] = da + 3; qmap[2 * (qa + 3 + k) + 1] = k; } }
    else if (type == 1) { for (int k = 0; k < 4; k++) { qmap[2 * (qa + k)] = da; qmap[2 * (qa + k) + 1] = k; } }
    else { qmap[2 * qa] = da; qmap[2 * qa + 1] = -1; }
  }
  return qmap;
}

int mjpc_hip_unscented_moments(MjpcHipEngine *e, const double *state, const double *factor, double sigma_step, const double *weights,
                               const double *ctrl, double time, const double *mocap, const double *userdata, const double *noise_process,
                               const double *noise_sensor, int sensor_first_row, int ns, double *state_mean, double *sensor_mean,
                               double *cov_ss, double *cov_sy, double *cov_yy, double *sigma_next, int *failure) {
  if (!e) { set_error("mjpc_hip_unscented_moments: invalid argument"); return -1; }
  if (ns < 1) { set_error("mjpc_hip_unscented_moments: ns < 1"); return -1; }
  if (sensor_first_row < 0 || (long long)sensor_first_row + ns > e->nr) {
    set_error("mjpc_hip_unscented_moments: sensor rows [" + std::to_string(sensor_first_row) + ", " + std::to_string((long long)sensor_first_row + ns) +
              ") are outside the task's " + std::to_string(e->nr) + " residual rows");
    return -1;
  }
  if (!state || !factor || !weights || (e->nu > 0 && !ctrl) || !noise_process || !noise_sensor || !state_mean || !sensor_mean || !cov_ss || !cov_sy ||
      !cov_yy || !failure) { set_error("mjpc_hip_unscented_moments: null input"); return -1; }
  KParams K;
  int rc = step_prepare(e, "mjpc_hip_unscented_moments", mocap, userdata, &K);
  if (rc != 0) return rc;
  const size_t ds = e->ds, nu = e->nu, nv = e->nv, nq = e->nq, nd = e->nd, nsz = (size_t)ns, R = 2 * nd + 1, D = sizeof(double);
  // B_FD: the block that goes up, the tables the kernels write and read, the block that comes back (UkfLay, carve.h); H_PACK mirrors
  // the two blocks that travel
  UkfLay L;
  UkfHost h;
  PLACE(B_FD, L, e->dims(), nsz);
  PLACE(H_PACK, h, e->dims(), nsz);
  memcpy(h.in.x, state, D * ds);
  memcpy(h.in.L, factor, D * nd * nd);
  if (nu) memcpy(h.in.u, ctrl, D * nu);
  memcpy(h.in.noise_process, noise_process, D * nd);
  memcpy(h.in.noise_sensor, noise_sensor, D * nsz);
  const std::vector<int> dofmap = fd_dofmap(e), qmap = ukf_qmap(e);
  memcpy(h.in.dofmap, dofmap.data(), sizeof(int) * (2 * nv + 2));
  memcpy(h.in.qmap, qmap.data(), sizeof(int) * (2 * nq + 2));
  // each block travels in one copy: the mirror's second begins where its first ends; the moments are the second without the rows
  const size_t in_bytes = (char *)h.back.next - (char *)h.in.x, mom_bytes = (char *)h.back.end - (char *)h.back.state_mean;
  HIPCHK(hipMemcpyAsync(L.in.x, h.in.x, in_bytes, hipMemcpyHostToDevice, e->stream));
  UkfArgs a;
  a.x = L.in.x; a.L = L.in.L; a.u = L.in.u; a.noise_process = L.in.noise_process; a.noise_sensor = L.in.noise_sensor;
  a.dofmap = L.in.dofmap; a.qmap = L.in.qmap;
  a.nq = e->nq; a.nv = e->nv; a.na = e->na; a.nu = e->nu; a.nr = e->nr; a.ns = ns; a.first = sensor_first_row;
  a.sigma_step = sigma_step; a.time = time; a.w_mean0 = weights[0]; a.w_cov0 = weights[1]; a.w_sigma = weights[2];
  a.state_tab = L.t.state; a.ctrl_tab = L.t.ctrl; a.time_tab = L.t.time; a.next_state = L.t.next; a.residual = L.t.residual; a.fail = L.t.fail; a.diff = L.diff;
  a.state_mean = L.back.state_mean; a.sensor_mean = L.back.sensor_mean; a.cov_ss = L.back.cov_ss; a.cov_sy = L.back.cov_sy; a.cov_yy = L.back.cov_yy;
  a.failure = L.back.failure;
  hipLaunchKernelGGL(ukf_sigma_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, e->stream, a);
  step_rows(e, K, R, L.t);
  hipLaunchKernelGGL(ukf_mean_kernel, dim3(1), dim3(256), 0, e->stream, a);
  const unsigned tiles = (unsigned)((nd + nsz + UKF_TILE - 1) / UKF_TILE);
  hipLaunchKernelGGL(ukf_cov_kernel, dim3(tiles, tiles), dim3(UKF_TILE * UKF_TILE), 0, e->stream, a);
  HIPCHK(hipGetLastError());
  if (sigma_next) HIPCHK(hipMemcpyAsync(h.back.next, L.back.next, D * R * ds + mom_bytes, hipMemcpyDeviceToHost, e->stream));
  else HIPCHK(hipMemcpyAsync(h.back.state_mean, L.back.state_mean, mom_bytes, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  if (sigma_next) memcpy(sigma_next, h.back.next, D * R * ds);
  memcpy(state_mean, h.back.state_mean, D * ds);
  memcpy(sensor_mean, h.back.sensor_mean, D * nsz);
  memcpy(cov_ss, h.back.cov_ss, D * nd * nd);
  memcpy(cov_sy, h.back.cov_sy, D * nd * nsz);
  memcpy(cov_yy, h.back.cov_yy, D * nsz * nsz);
  memcpy(failure, h.back.failure, sizeof(int));
  return 0;
}

int mjpc_hip_linearize_step(MjpcHipEngine *e, const double *state, const double *ctrl, double time, const double *mocap, const double *userdata,
                            double eps, int centered, double *next_state, double *residual, double *A, double *C, int *failure) {
  if (!e) { set_error("mjpc_hip_linearize_step: invalid argument"); return -1; }
  if (!(eps > 0)) { set_error("mjpc_hip_linearize_step: eps <= 0"); return -1; }
  if (!state || (e->nu > 0 && !ctrl)) { set_error("mjpc_hip_linearize_step: null input"); return -1; }
  KParams K;
  int rc = step_prepare(e, "mjpc_hip_linearize_step", mocap, userdata, &K);
  if (rc != 0) return rc;
  const size_t ds = e->ds, nr = e->nr, nd = e->nd;
  const std::vector<int> dofmap = fd_dofmap(e);
  FdLay L;
  PLACE(B_FD, L, e->dims(), 1, centered ? 1 : 0);
  FdArgs a;
  rc = fd_pass(e, K, dofmap, L, 0, 1, 0, state, ctrl, &time, eps, centered ? 1 : 0, &a);
  if (rc != 0) return rc;
  // the base row (slot 0) of the table is the step from `state` itself
  if (next_state) HIPCHK(hipMemcpyAsync(next_state, a.next_state, sizeof(double) * ds, hipMemcpyDeviceToHost, e->stream));
  if (residual && nr) HIPCHK(hipMemcpyAsync(residual, a.residual, sizeof(double) * nr, hipMemcpyDeviceToHost, e->stream));
  if (A && nd) HIPCHK(hipMemcpyAsync(A, a.A, sizeof(double) * nd * nd, hipMemcpyDeviceToHost, e->stream));
  if (C && nr * nd) HIPCHK(hipMemcpyAsync(C, a.C, sizeof(double) * nr * nd, hipMemcpyDeviceToHost, e->stream));
  if (failure) HIPCHK(hipMemcpyAsync(failure, a.failure, sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
}

// ------------------------------------------------------------------------------ cost derivatives, trajectory gradient
// the cost-derivative kernel's arguments over T knots whose inputs and outputs are on the device already
static CdArgs cd_args(const MjpcHipEngine *e, const double *residual, const double *C, const double *D, const CdOut &o, int T, int last_is_terminal, int hessians) {
  CdArgs a;
  memset(&a, 0, sizeof(a));
  a.residual = residual; a.C = C; a.D = D; a.T = T; a.nd = e->nd; a.nu = e->nu; a.nr = e->nr; a.last_is_terminal = last_is_terminal; a.hessians = hessians;
  a.cr = o.cr; a.cx = o.cx; a.cu = o.cu; a.cxx = o.cxx; a.cuu = o.cuu; a.cxu = o.cxu;
  return a;
}
// the kernel itself (the engine's cost table goes into `a` here)
static int cd_launch(MjpcHipEngine *e, CdArgs a, const char *who) {
  const DevTask &tk = e->K.M.task;
  a.dim_norm_residual = tk.dim_norm_residual; a.norm = tk.norm; a.num_norm_parameter = tk.num_norm_parameter;
  a.weight = tk.weight; a.norm_parameter = tk.norm_parameter; a.num_term = tk.num_term; a.risk = tk.risk;
  if (!e->cost_rows_ok) { set_error(std::string(who) + ": the cost terms' residual dimensions do not add up to num_residual"); return -1; }
  const size_t lds = CD_LDS_DOUBLES(a.nr, a.num_term) * sizeof(double);
  if (lds > 64 * 1024) { set_error(std::string(who) + ": num_residual too large for the cost-derivative kernel's LDS (64 KiB)"); return -1; }
  const unsigned tiles = (unsigned)((a.nd + a.nu + CD_TILE - 1) / CD_TILE);
  hipLaunchKernelGGL(cd_kernel, dim3(tiles, a.hessians ? tiles : 1, (unsigned)a.T), dim3(CD_TILE * CD_TILE), lds, e->stream, a);
  return 0;
}

int mjpc_hip_cost_derivatives(MjpcHipEngine *e, int T, const double *residual, const double *C, const double *D, int last_is_terminal, int hessians,
                              double *cr, double *cx, double *cu, double *cxx, double *cuu, double *cxu) {
  if (!e) { set_error("mjpc_hip_cost_derivatives: invalid argument"); return -1; }
  if (T < 1) { set_error("mjpc_hip_cost_derivatives: T < 1"); return -1; }
  if (e->pending) { set_error("mjpc_hip_cost_derivatives: a plan step is in flight (call mjpc_hip_plan_fetch first)"); return -1; }
  last_is_terminal = last_is_terminal ? 1 : 0; hessians = hessians ? 1 : 0;
  const size_t nu = e->nu, nr = e->nr, nd = e->nd, Tz = (size_t)T;
  const size_t Td = Tz - last_is_terminal;          // knots that have a D
  if ((nr && !residual) || (nr * nd && !C) || (nr * nu * Td && !D)) { set_error("mjpc_hip_cost_derivatives: null input"); return -1; }
  HIPCHK(hipSetDevice(e->device));
  CdLay L;
  PLACE(B_FD, L, e->dims(), Tz, hessians);
  CdArgs a = cd_args(e, L.residual, L.C, L.D, L.out, T, last_is_terminal, hessians);
  if (nr) HIPCHK(hipMemcpyAsync(L.residual, residual, sizeof(double) * Tz * nr, hipMemcpyHostToDevice, e->stream));
  if (nr * nd) HIPCHK(hipMemcpyAsync(L.C, C, sizeof(double) * Tz * nr * nd, hipMemcpyHostToDevice, e->stream));
  if (nr * nu * Td) HIPCHK(hipMemcpyAsync(L.D, D, sizeof(double) * Td * nr * nu, hipMemcpyHostToDevice, e->stream));
  int rc = cd_launch(e, a, "mjpc_hip_cost_derivatives");
  if (rc != 0) return rc;
  HIPCHK(hipGetLastError());
  // (without Hessians their fields are null, and nothing comes back for them)
  auto down = [&](double *dst, const double *src, size_t n) { return dst && src && n ? hipMemcpyAsync(dst, src, sizeof(double) * n, hipMemcpyDeviceToHost, e->stream) : hipSuccess; };
  HIPCHK(down(cr, L.out.cr, Tz * nr)); HIPCHK(down(cx, L.out.cx, Tz * nd)); HIPCHK(down(cu, L.out.cu, Tz * nu));
  HIPCHK(down(cxx, L.out.cxx, Tz * nd * nd)); HIPCHK(down(cuu, L.out.cuu, Tz * nu * nu)); HIPCHK(down(cxu, L.out.cxu, Tz * nd * nu));
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
}

// hand-out of one field of a pinned mirror to the caller's array (which may be null)
static void give(double *dst, const double *src, size_t n) { if (dst && n) memcpy(dst, src, sizeof(double) * n); }

int mjpc_hip_trajectory_gradient(MjpcHipEngine *e, int T, const double *x, const double *u, const double *time, const double *residual, const double *mocap,
                                 const double *userdata, double eps, int centered, double *k, double *Vx, double *Qx, double *Qu, double *dV, int *failure) {
  if (!e) { set_error("mjpc_hip_trajectory_gradient: invalid argument"); return -1; }
  if (T < 2) { set_error("mjpc_hip_trajectory_gradient: T < 2"); return -1; }
  if (!(eps > 0)) { set_error("mjpc_hip_trajectory_gradient: eps <= 0"); return -1; }
  if (!x || !time || (e->nu > 0 && !u) || (e->nr > 0 && !residual) || !failure) { set_error("mjpc_hip_trajectory_gradient: null input"); return -1; }
  centered = centered ? 1 : 0;
  if ((size_t)T > fd_pass_knots(e, centered)) { set_error("mjpc_hip_trajectory_gradient: T too large for one pass of the step tables (" + std::to_string(fd_pass_knots(e, centered)) + " knots for this model)"); return -1; }
  KParams K;
  int rc = step_prepare(e, "mjpc_hip_trajectory_gradient", mocap, userdata, &K);
  if (rc != 0) return rc;
  const size_t nu = e->nu, nr = e->nr, nd = e->nd, Tz = (size_t)T;
  // B_FD: behind the pass's doubles the residual rows, cr / cx / cu and the block that goes back in one copy (GradLay, carve.h)
  GradLay L;
  GradOut h;
  PLACE(H_PACK, h, e->dims(), Tz);
  const std::vector<int> dofmap = fd_dofmap(e);          // (outlives the stream's copy of it)
  PLACE(B_FD, L, e->dims(), Tz, centered);
  FdArgs f;
  rc = fd_pass(e, K, dofmap, L.fd, 0, Tz, 1, x, u, time, eps, centered, &f);
  if (rc != 0) return rc;
  if (nr) HIPCHK(hipMemcpyAsync(L.residual, residual, sizeof(double) * Tz * nr, hipMemcpyHostToDevice, e->stream));
  rc = cd_launch(e, cd_args(e, L.residual, f.C, f.D, L.cd, T, 1, 0), "mjpc_hip_trajectory_gradient");
  if (rc != 0) return rc;
  GdArgs g;
  g.A = f.A; g.B = f.B; g.cx = L.cd.cx; g.cu = L.cd.cu; g.T = T; g.nd = (int)nd; g.nu = (int)nu;
  g.k = L.out.k; g.Vx = L.out.Vx; g.Qx = L.out.Qx; g.Qu = L.out.Qu; g.dV = L.out.dV;
  const size_t gd_lds = sizeof(double) * (2 * (nd + nu) + (nd * (nd + nu) <= (size_t)GD_THREADS * GD_R ? nd * (nd + nu) : 0));
  if (gd_lds > 48 * 1024) HIPCHK(hipFuncSetAttribute((const void *)gd_backward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gd_lds));
  hipLaunchKernelGGL(gd_backward_kernel, dim3(1), dim3(GD_THREADS), gd_lds, e->stream, g);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(L.out.failure, f.failure, sizeof(int) * Tz, hipMemcpyDeviceToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(h.k, L.out.k, (char *)h.end - (char *)h.k, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  give(k, h.k, Tz * nu); give(Vx, h.Vx, Tz * nd); give(Qx, h.Qx, (Tz - 1) * nd); give(Qu, h.Qu, (Tz - 1) * nu); give(dV, h.dV, 2);
  memcpy(failure, h.failure, sizeof(int) * Tz);
  return 0;
}

// ------------------------------------------------------------------------------ iLQG backward pass
static int rc_settings(RcArgs &g, const MjpcHipRiccatiSettings *s, const char *who) {
  if (!s || s->struct_size != (int)sizeof(MjpcHipRiccatiSettings)) { set_error(std::string(who) + ": MjpcHipRiccatiSettings.struct_size does not match this library"); return -1; }
  g.reg_type = s->regularization_type; g.action_limits = s->action_limits ? 1 : 0; g.max_iter = s->max_regularization_iterations;
  g.reg_min = s->min_regularization; g.reg_max = s->max_regularization; g.reg_factor = s->regularization_factor;
  return 0;
}
// doubles of rc_backward_kernel's work image where it has to lie in global memory, 0 where it fits the workgroup's LDS
static size_t rc_work_doubles(size_t n, size_t m) { return RC_WORK_DOUBLES(n, m) * sizeof(double) <= RC_LDS_LIMIT ? 0 : RC_WORK_DOUBLES(n, m); }
// zero the outputs, hand in the regularisation, run the kernel, bring the block back and hand it out.  o: the block on the device (the
// nfail failure ints behind it are the caller's and come back with it, into failure[]); scratch: the work image when it is not in LDS
static int rc_run(MjpcHipEngine *e, RcArgs g, const RcOut &o, size_t nfail, double *scratch, double *regularization, double *rate, double *k, double *K,
                  double *Vx, double *Vxx, double *Qx, double *Qu, double *Qxx, double *Qxu, double *Quu, double *dV, int *status, int *failure) {
  const size_t T = g.T, n = g.nd, m = g.nu;
  RcOut h;
  PLACE(H_PACK, h, T, n, m, nfail);
  g.k = o.k; g.K = o.K; g.Vx = o.Vx; g.Vxx = o.Vxx; g.Qx = o.Qx; g.Qu = o.Qu; g.Qxx = o.Qxx; g.Qxu = o.Qxu; g.Quu = o.Quu; g.dV = o.dV; g.reg = o.reg;
  g.status = o.status;
  g.scratch = scratch;
  h.reg[0] = *regularization; h.reg[1] = *rate;          // (staged in the mirror's own field: the block overwrites it on its way back)
  HIPCHK(hipMemsetAsync(o.k, 0, (char *)o.tail - (char *)o.k, e->stream));
  HIPCHK(hipMemcpyAsync(o.reg, h.reg, sizeof(double) * 2, hipMemcpyHostToDevice, e->stream));
  const size_t lds = rc_work_doubles(n, m) ? 0 : RC_WORK_DOUBLES(n, m) * sizeof(double);
  if (lds > 48 * 1024) HIPCHK(hipFuncSetAttribute((const void *)rc_backward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(rc_backward_kernel, dim3(1), dim3(RC_THREADS), lds, e->stream, g);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(h.k, o.k, (char *)o.end - (char *)o.k, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  give(k, h.k, T * m); give(K, h.K, T * m * n); give(Vx, h.Vx, T * n); give(Vxx, h.Vxx, T * n * n);
  give(Qx, h.Qx, (T - 1) * n); give(Qu, h.Qu, (T - 1) * m); give(Qxx, h.Qxx, (T - 1) * n * n); give(Qxu, h.Qxu, (T - 1) * n * m);
  give(Quu, h.Quu, (T - 1) * m * m); give(dV, h.dV, 2);
  *regularization = h.reg[0]; *rate = h.reg[1];
  if (status) memcpy(status, h.status, sizeof(int) * 3);
  if (nfail) memcpy(failure, h.failure, sizeof(int) * nfail);
  return 0;
}

int mjpc_hip_ilqg_backward_pass(MjpcHipEngine *e, int T, int nd, int nu, const double *A, const double *B, const double *cx, const double *cu,
                                const double *cxx, const double *cxu, const double *cuu, const double *actions, const double *action_limits,
                                const MjpcHipRiccatiSettings *s, double *regularization, double *regularization_rate, double *k, double *K,
                                double *Vx, double *Vxx, double *Qx, double *Qu, double *Qxx, double *Qxu, double *Quu, double *dV, int *status) {
  const char *who = "mjpc_hip_ilqg_backward_pass";
  if (!e) { set_error(std::string(who) + ": invalid argument"); return -1; }
  if (T < 2) { set_error(std::string(who) + ": T < 2"); return -1; }
  if (nd < 1 || nu < 1) { set_error(std::string(who) + ": nd < 1 or nu < 1"); return -1; }
  if (e->pending) { set_error(std::string(who) + ": a plan step is in flight (call mjpc_hip_plan_fetch first)"); return -1; }
  RcArgs g;
  memset(&g, 0, sizeof(g));
  if (rc_settings(g, s, who) != 0) return -1;
  if (!A || !B || !cx || !cu || !cxx || !cxu || !cuu || !regularization || !regularization_rate || (g.action_limits && (!actions || !action_limits))) {
    set_error(std::string(who) + ": null input"); return -1; }
  HIPCHK(hipSetDevice(e->device));
  const size_t Tz = T, n = nd, m = nu;
  RcLay L;
  PLACE(B_FD, L, Tz, n, m, g.action_limits, rc_work_doubles(n, m));
  auto up = [&](double *dst, const double *src, size_t cnt) { return cnt ? hipMemcpyAsync(dst, src, sizeof(double) * cnt, hipMemcpyHostToDevice, e->stream) : hipSuccess; };
  HIPCHK(up(L.A, A, (Tz - 1) * n * n)); HIPCHK(up(L.B, B, (Tz - 1) * n * m)); HIPCHK(up(L.cx, cx, Tz * n)); HIPCHK(up(L.cu, cu, (Tz - 1) * m));
  HIPCHK(up(L.cxx, cxx, Tz * n * n)); HIPCHK(up(L.cxu, cxu, (Tz - 1) * n * m)); HIPCHK(up(L.cuu, cuu, (Tz - 1) * m * m));
  if (g.action_limits) { HIPCHK(up(L.actions, actions, (Tz - 1) * m)); HIPCHK(up(L.limits, action_limits, 2 * m)); }
  g.A = L.A; g.B = L.B; g.cx = L.cx; g.cu = L.cu; g.cxx = L.cxx; g.cxu = L.cxu; g.cuu = L.cuu; g.actions = L.actions; g.limits = L.limits;
  g.T = T; g.nd = nd; g.nu = nu;
  return rc_run(e, g, L.out, 0, L.scratch, regularization, regularization_rate, k, K, Vx, Vxx, Qx, Qu, Qxx, Qxu, Quu, dV, status, nullptr);
}

int mjpc_hip_riccati_layout_bytes(int nd, int nu, int *in_lds) {
  if (nd < 1 || nu < 1) { set_error("mjpc_hip_riccati_layout_bytes: nd < 1 or nu < 1"); return -1; }
  const size_t bytes = RC_WORK_DOUBLES(nd, nu) * sizeof(double);
  if (in_lds) *in_lds = bytes <= RC_LDS_LIMIT ? 1 : 0;
  return bytes > 0x7fffffff ? 0x7fffffff : (int)bytes;
}

int mjpc_hip_trajectory_ilqg(MjpcHipEngine *e, int T, const double *x, const double *u, const double *time, const double *residual, const double *mocap,
                             const double *userdata, double eps, int centered, const MjpcHipRiccatiSettings *s, double *regularization,
                             double *regularization_rate, double *k, double *K, double *Vx, double *Vxx, double *Qx, double *Qu, double *Qxx, double *Qxu,
                             double *Quu, double *dV, int *status, int *failure) {
  const char *who = "mjpc_hip_trajectory_ilqg";
  if (!e) { set_error(std::string(who) + ": invalid argument"); return -1; }
  if (T < 2) { set_error(std::string(who) + ": T < 2"); return -1; }
  if (!(eps > 0)) { set_error(std::string(who) + ": eps <= 0"); return -1; }
  if (e->nu < 1) { set_error(std::string(who) + ": the model has no actuator"); return -1; }
  if (!x || !time || !u || (e->nr > 0 && !residual) || !failure || !regularization || !regularization_rate) { set_error(std::string(who) + ": null input"); return -1; }
  RcArgs g;
  memset(&g, 0, sizeof(g));
  if (rc_settings(g, s, who) != 0) return -1;
  centered = centered ? 1 : 0;
  if ((size_t)T > fd_pass_knots(e, centered)) { set_error(std::string(who) + ": T too large for one pass of the step tables (" + std::to_string(fd_pass_knots(e, centered)) + " knots for this model)"); return -1; }
  KParams K_;
  int rc = step_prepare(e, who, mocap, userdata, &K_);
  if (rc != 0) return rc;
  const size_t nu = e->nu, nr = e->nr, Tz = (size_t)T;
  // B_FD: behind the pass's doubles the residual rows, the cost derivatives, the limits, the block that goes back, the scratch (IlqgLay)
  IlqgLay L;
  const std::vector<int> dofmap = fd_dofmap(e);
  PLACE(B_FD, L, e->dims(), Tz, centered, rc_work_doubles(e->nd, nu));
  FdArgs f;
  rc = fd_pass(e, K_, dofmap, L.fd, 0, Tz, 1, x, u, time, eps, centered, &f);
  if (rc != 0) return rc;
  if (nr) HIPCHK(hipMemcpyAsync(L.residual, residual, sizeof(double) * Tz * nr, hipMemcpyHostToDevice, e->stream));
  // the model's ctrlrange; an unlimited actuator gets -inf, +inf (kept alive until the stream has been synchronised in rc_run)
  std::vector<double> lim(2 * nu);
  {
    const DevModel hm = mjpc_host::relocate(e->pm, e->pm.ib.data(), e->pm.db.data());
    for (size_t i = 0; i < nu; i++) {
      const bool limited = hm.actuator_ctrllimited[i] != 0;
      lim[2 * i] = limited ? hm.actuator_ctrlrange[2 * i] : -HUGE_VAL;
      lim[2 * i + 1] = limited ? hm.actuator_ctrlrange[2 * i + 1] : HUGE_VAL;
    }
  }
  HIPCHK(hipMemcpyAsync(L.limits, lim.data(), sizeof(double) * 2 * nu, hipMemcpyHostToDevice, e->stream));
  rc = cd_launch(e, cd_args(e, L.residual, f.C, f.D, L.cd, T, 1, 1), who);
  if (rc != 0) return rc;
  g.A = f.A; g.B = f.B; g.cx = L.cd.cx; g.cu = L.cd.cu; g.cxx = L.cd.cxx; g.cxu = L.cd.cxu; g.cuu = L.cd.cuu; g.actions = f.u; g.limits = L.limits;
  g.T = T; g.nd = e->nd; g.nu = e->nu;
  // failure[] travels behind the block; rc_run zeroes the block alone, so this copy may be queued first
  HIPCHK(hipMemcpyAsync(L.out.failure, f.failure, sizeof(int) * Tz, hipMemcpyDeviceToDevice, e->stream));
  return rc_run(e, g, L.out, Tz, L.scratch, regularization, regularization_rate, k, K, Vx, Vxx, Qx, Qu, Qxx, Qxu, Quu, dV, status, failure);
}

// ------------------------------------------------------------------------------ the direct optimiser's window cost
// the settings' checks (every refusal of the header, before anything is touched) and the sensors' row tables
static int dc_check(const char *w, int T, int nv, int nr, const MjpcHipDirectSettings *s, std::vector<int> &first, std::vector<int> &row_sensor) {
  const std::string who = w;
  if (!s || s->struct_size != (int)sizeof(MjpcHipDirectSettings)) { set_error(who + ": MjpcHipDirectSettings.struct_size does not match this library"); return -1; }
  if (T < 3) { set_error(who + ": T < 3"); return -1; }
  if (nv < 1) { set_error(who + ": nv < 1"); return -1; }
  if (s->num_sensor < 0 || s->num_sensor_rows < 0) { set_error(who + ": num_sensor < 0"); return -1; }
  if (!(s->timestep > 0)) { set_error(who + ": timestep <= 0"); return -1; }
  if (!s->noise_process || (s->num_sensor && (!s->sensor_dim || !s->sensor_stage || !s->sensor_norm || !s->sensor_norm_parameter || !s->noise_sensor))) {
    set_error(who + ": null input"); return -1; }
  if (s->sensor_first_row < 0 || (long long)s->sensor_first_row + s->num_sensor_rows > nr) { set_error(who + ": the sensor rows lie outside the residual"); return -1; }
  first.assign(s->num_sensor, 0); row_sensor.assign(s->num_sensor_rows, 0);
  long long rows = 0;
  for (int i = 0; i < s->num_sensor; i++) {
    if (s->sensor_dim[i] < 1) { set_error(who + ": a sensor dimension < 1"); return -1; }
    if (s->sensor_stage[i] < 0 || s->sensor_stage[i] > 2) { set_error(who + ": a sensor stage outside 0 .. 2"); return -1; }
    if (!(s->noise_sensor[i] > 0)) { set_error(who + ": a sensor noise value <= 0"); return -1; }
    first[i] = (int)rows;
    for (int r = 0; r < s->sensor_dim[i] && rows + r < s->num_sensor_rows; r++) row_sensor[rows + r] = i;
    rows += s->sensor_dim[i];
  }
  if (rows != s->num_sensor_rows) { set_error(who + ": the sensor dimensions do not sum to num_sensor_rows"); return -1; }
  for (int i = 0; i < nv; i++) if (!(s->noise_process[i] > 0)) { set_error(who + ": a process noise value <= 0"); return -1; }
  return 0;
}

// the sensors go up; the kernels' arguments over the layout
static int dc_upload_spec(MjpcHipEngine *e, const DcSpec &d, const DcWork &w, int T, int nv, int nr, const MjpcHipDirectSettings *s, const std::vector<int> &first,
                          const std::vector<int> &row_sensor, DcArgs *out) {
  const size_t m = s->num_sensor, ns = s->num_sensor_rows;
  auto upd = [&](double *dst, const double *src, size_t n) { return n ? hipMemcpyAsync(dst, src, sizeof(double) * n, hipMemcpyHostToDevice, e->stream) : hipSuccess; };
  auto upi = [&](int *dst, const int *src, size_t n) { return n ? hipMemcpyAsync(dst, src, sizeof(int) * n, hipMemcpyHostToDevice, e->stream) : hipSuccess; };
  HIPCHK(upd(d.prm, s->sensor_norm_parameter, 2 * m)); HIPCHK(upd(d.noise_sensor, s->noise_sensor, m)); HIPCHK(upd(d.noise_process, s->noise_process, nv));
  HIPCHK(upi(d.dim, s->sensor_dim, m)); HIPCHK(upi(d.first, first.data(), m)); HIPCHK(upi(d.stage, s->sensor_stage, m)); HIPCHK(upi(d.norm, s->sensor_norm, m));
  HIPCHK(upi(d.row_sensor, row_sensor.data(), ns));
  if (s->sensor_mask) HIPCHK(upi(d.mask, s->sensor_mask, (size_t)T * m));
  DcArgs a;
  memset(&a, 0, sizeof(a));
  a.T = T; a.nv = nv; a.nr = nr; a.ns = (int)ns; a.row0 = s->sensor_first_row; a.num_sensor = (int)m;
  a.dim = d.dim; a.first = d.first; a.stage = d.stage; a.norm = d.norm; a.row_sensor = d.row_sensor;
  a.prm = d.prm; a.noise_sensor = d.noise_sensor; a.noise_process = d.noise_process; a.mask = s->sensor_mask ? d.mask : nullptr;
  a.sensor_flag = s->sensor_flag ? 1 : 0; a.force_flag = s->force_flag ? 1 : 0; a.time_scaling_sensor = s->time_scaling_sensor ? 1 : 0;
  a.time_scaling_force = s->time_scaling_force ? 1 : 0; a.first_pos = s->first_step_position_sensors ? 1 : 0;
  a.last_pos = s->last_step_position_sensors ? 1 : 0; a.last_vel = s->last_step_velocity_sensors ? 1 : 0; a.h = s->timestep;
  a.res_s = w.res_s; a.ng_s = w.ng_s; a.hd_s = w.hd_s; a.hs_s = w.hs_s; a.w_s = w.w_s; a.wy_s = w.wy_s; a.res_f = w.res_f; a.ng_f = w.ng_f; a.y_f = w.y_f;
  a.Js = w.Js; a.Jf = w.Jf; a.NJs = w.NJs; a.NJf = w.NJf; a.gradient = w.gradient; a.band = w.band; a.cost = w.cost;
  *out = a;
  return 0;
}

// norms, totals, chain rule, N J, gradient and band: five launches in stream order, nothing in between
static void dc_launch(MjpcHipEngine *e, const DcArgs &a) {
  const size_t T = a.T, no = (size_t)a.ns + a.nv, nb = 3 * (size_t)a.nv;
  const size_t n_nj = T * no * nb, n_entry = T * a.nv * (nb + 1);
  hipLaunchKernelGGL(dc_norm_kernel, dim3((unsigned)T, 1), dim3(64), 0, e->stream, a);
  hipLaunchKernelGGL(dc_cost_kernel, dim3(1), dim3(64), 0, e->stream, a);
  hipLaunchKernelGGL(dc_block_kernel, dim3((unsigned)T, (unsigned)((no + DC_TILE - 1) / DC_TILE), (unsigned)((nb + DC_TILE - 1) / DC_TILE)), dim3(DC_TILE * DC_TILE), 0,
                     e->stream, a);
  hipLaunchKernelGGL(dc_nj_kernel, dim3((unsigned)((n_nj + DC_THREADS - 1) / DC_THREADS)), dim3(DC_THREADS), 0, e->stream, a, n_nj);
  hipLaunchKernelGGL(dc_entry_kernel, dim3((unsigned)((n_entry + DC_THREADS - 1) / DC_THREADS)), dim3(DC_THREADS), 0, e->stream, a, n_entry);
}

int mjpc_hip_direct_assemble(MjpcHipEngine *e, int T, int nv, int nr, const MjpcHipDirectSettings *s, const double *residual_sensor, const double *residual_force,
                             const double *DfDq, const double *DfDv, const double *DfDa, const double *DsDq, const double *DsDv, const double *DsDa,
                             const double *dvdq0, const double *dvdq1, double *cost, double *gradient, double *hessian_band, double *block_sensor,
                             double *block_force, double *norm_gradient_sensor, double *norm_gradient_force, double *residual_sensor_out, double *residual_force_out) {
  const char *who = "mjpc_hip_direct_assemble";
  if (!e) { set_error(std::string(who) + ": invalid argument"); return -1; }
  if (e->pending) { set_error(std::string(who) + ": a plan step is in flight (call mjpc_hip_plan_fetch first)"); return -1; }
  std::vector<int> first, row_sensor;
  if (dc_check(who, T, nv, nr, s, first, row_sensor) != 0) return -1;
  const size_t Tz = T, n = nv, ns = s->num_sensor_rows, nb = 3 * n;
  if (nr < 0 || (ns && (!residual_sensor || !DsDq || !DsDv || !DsDa)) || !residual_force || !DfDq || !DfDv || !DfDa || !dvdq0 || !dvdq1 || !cost || !gradient ||
      !hessian_band) { set_error(std::string(who) + ": null input"); return -1; }
  // the grids: one block per DC_THREADS entries, the chain rule's tiles in y and z
  if ((Tz * (ns + n) * nb + DC_THREADS - 1) / DC_THREADS > 0x7fffffffull || (Tz * n * (nb + 1) + DC_THREADS - 1) / DC_THREADS > 0x7fffffffull ||
      (ns + n + DC_TILE - 1) / DC_TILE > 65535 || (nb + DC_TILE - 1) / DC_TILE > 65535) {
    set_error(std::string(who) + ": the window is too large for one launch"); return -1; }
  HIPCHK(hipSetDevice(e->device));
  DcLay L;
  PLACE(B_FD, L, Tz, n, (size_t)nr, ns, (size_t)s->num_sensor);
  auto up = [&](double *dst, const double *src, size_t cnt) { return cnt ? hipMemcpyAsync(dst, src, sizeof(double) * cnt, hipMemcpyHostToDevice, e->stream) : hipSuccess; };
  HIPCHK(up(L.rs, residual_sensor, Tz * ns)); HIPCHK(up(L.rf, residual_force, Tz * n));
  const double *Df[3] = {DfDq, DfDv, DfDa}, *Ds[3] = {DsDq, DsDv, DsDa};
  for (int k = 0; k < 3; k++) { HIPCHK(up(L.Df[k], Df[k], Tz * n * n)); if (ns) HIPCHK(up(L.Ds[k], Ds[k], Tz * (size_t)nr * n)); }
  HIPCHK(up(L.V0, dvdq0, Tz * n * n)); HIPCHK(up(L.V1, dvdq1, Tz * n * n));
  DcArgs a;
  int rc = dc_upload_spec(e, L.spec, L.work, T, nv, nr, s, first, row_sensor, &a);
  if (rc != 0) return rc;
  a.rs = L.rs; a.rf = L.rf; a.V0 = L.V0; a.V1 = L.V1;
  for (int k = 0; k < 3; k++) { a.Df[k] = L.Df[k]; a.Ds[k] = L.Ds[k]; }
  dc_launch(e, a);
  HIPCHK(hipGetLastError());
  auto down = [&](double *dst, const double *src, size_t cnt) { return dst && cnt ? hipMemcpyAsync(dst, src, sizeof(double) * cnt, hipMemcpyDeviceToHost, e->stream) : hipSuccess; };
  const DcWork &w = L.work;
  HIPCHK(down(cost, w.cost, 3)); HIPCHK(down(gradient, w.gradient, Tz * n)); HIPCHK(down(hessian_band, w.band, Tz * n * nb));
  HIPCHK(down(block_sensor, w.Js, Tz * ns * nb)); HIPCHK(down(block_force, w.Jf, Tz * n * nb));
  HIPCHK(down(norm_gradient_sensor, w.ng_s, Tz * ns)); HIPCHK(down(norm_gradient_force, w.ng_f, Tz * n));
  HIPCHK(down(residual_sensor_out, w.res_s, Tz * ns)); HIPCHK(down(residual_force_out, w.res_f, Tz * n));
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
}

// common front of the two window calls: the refusals, in the header's order, before anything is touched
static int dc_window_check(MjpcHipEngine *e, const char *w, int nwin, int T, const MjpcHipDirectSettings *s, const double *q, const double *act, const double *ctrl,
                           const double *time, const double *y_s, const double *y_f, std::vector<int> &first, std::vector<int> &row_sensor) {
  const std::string who = w;
  if (nwin < 1) { set_error(who + ": nwin < 1"); return -1; }
  if (dc_check(w, T, e->nv, e->nr, s, first, row_sensor) != 0) return -1;
  if (!q || !time || (e->na > 0 && !act) || (e->nu > 0 && !ctrl) || (s->num_sensor_rows && !y_s) || !y_f) { set_error(who + ": null input"); return -1; }
  if ((size_t)nwin * T > STEP_PASS_ROWS) { set_error(who + ": nwin * T too large for one pass of the inverse tables"); return -1; }
  return 0;
}

static DcWinArgs dc_win_args(const MjpcHipEngine *e, int nwin, int T, double h, const double *q, const double *act, const double *ctrl, const double *time,
                             const int *dofmap, double *x, double *u, double *a, double *tm, double *V0, double *V1) {
  DcWinArgs w;
  w.q = q; w.act = act; w.ctrl = ctrl; w.time = time; w.dofmap = dofmap; w.nwin = nwin; w.T = T; w.nq = e->nq; w.nv = e->nv; w.na = e->na; w.nu = e->nu; w.h = h;
  w.x = x; w.u = u; w.a = a; w.tm = tm; w.V0 = V0; w.V1 = V1;
  return w;
}

int mjpc_hip_direct_cost(MjpcHipEngine *e, int nwin, int T, const MjpcHipDirectSettings *s, int discrete, const double *q, const double *act, const double *ctrl,
                         const double *time, const double *sensor_measurement, const double *force_measurement, const double *mocap, const double *userdata,
                         double *cost, double *velocity, double *acceleration, double *sensor_prediction, double *force_prediction, int *failure) {
  const char *who = "mjpc_hip_direct_cost";
  if (!e) { set_error(std::string(who) + ": invalid argument"); return -1; }
  std::vector<int> first, row_sensor;
  if (dc_window_check(e, who, nwin, T, s, q, act, ctrl, time, sensor_measurement, force_measurement, first, row_sensor) != 0) return -1;
  if (!cost) { set_error(std::string(who) + ": null input"); return -1; }
  KParams K;
  discrete = discrete ? 1 : 0;
  int rc = inverse_prepare(e, who, mocap, userdata, discrete, &K);
  if (rc != 0) return rc;
  const size_t Tz = T, W = nwin, R = W * Tz, nq = e->nq, nv = e->nv, na = e->na, nu = e->nu, nr = e->nr, ds = e->ds, ns = s->num_sensor_rows, m = s->num_sensor;
  const std::vector<int> dofmap = fd_dofmap(e);
  DcCostLay L;
  PLACE(B_FD, L, e->dims(), W, Tz, ns, m);
  auto up = [&](double *dst, const double *src, size_t cnt) { return cnt ? hipMemcpyAsync(dst, src, sizeof(double) * cnt, hipMemcpyHostToDevice, e->stream) : hipSuccess; };
  HIPCHK(up(L.q, q, R * nq)); HIPCHK(up(L.act, act, R * na)); HIPCHK(up(L.ctrl, ctrl, R * nu)); HIPCHK(up(L.time, time, Tz));
  HIPCHK(up(L.y_s, sensor_measurement, Tz * ns)); HIPCHK(up(L.y_f, force_measurement, Tz * nv));
  HIPCHK(hipMemcpyAsync(L.dofmap, dofmap.data(), sizeof(int) * (2 * nv + 2), hipMemcpyHostToDevice, e->stream));
  DcArgs a;
  rc = dc_upload_spec(e, L.spec, L.work, T, (int)nv, (int)nr, s, first, row_sensor, &a);
  if (rc != 0) return rc;
  a.rs = L.rs; a.rf = L.rf;
  const DcWinArgs w = dc_win_args(e, nwin, T, s->timestep, L.q, L.act, L.ctrl, L.time, L.dofmap, L.t.state, L.t.ctrl, L.t.qacc, L.t.time, nullptr, nullptr);
  hipLaunchKernelGGL(dc_window_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, e->stream, w, (unsigned)R);
  inverse_rows(e, K, R, L.t, discrete);
  DcResArgs r;
  r.residual = L.t.residual; r.qfrc = L.t.qfrc; r.y_s = L.y_s; r.y_f = L.y_f; r.T = T; r.nv = (int)nv; r.nr = (int)nr; r.ns = (int)ns; r.row0 = s->sensor_first_row; r.E = 1;
  r.rs = L.rs; r.rf = L.rf;
  const size_t n_res = R * (ns + nv);
  hipLaunchKernelGGL(dc_residual_kernel, dim3((unsigned)((n_res + DC_THREADS - 1) / DC_THREADS)), dim3(DC_THREADS), 0, e->stream, r, n_res);
  hipLaunchKernelGGL(dc_norm_kernel, dim3((unsigned)Tz, (unsigned)W), dim3(64), 0, e->stream, a);
  hipLaunchKernelGGL(dc_cost_kernel, dim3((unsigned)W), dim3(64), 0, e->stream, a);
  HIPCHK(hipGetLastError());
  auto down = [&](double *dst, const double *src, size_t cnt) { return dst && cnt ? hipMemcpyAsync(dst, src, sizeof(double) * cnt, hipMemcpyDeviceToHost, e->stream) : hipSuccess; };
  HIPCHK(down(cost, L.work.cost, 3 * W));
  if (velocity) HIPCHK(hipMemcpy2DAsync(velocity, sizeof(double) * nv, L.t.state + nq, sizeof(double) * ds, sizeof(double) * nv, R, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(down(acceleration, L.t.qacc, R * nv)); HIPCHK(down(force_prediction, L.t.qfrc, R * nv));
  if (sensor_prediction && ns) HIPCHK(hipMemcpy2DAsync(sensor_prediction, sizeof(double) * ns, L.t.residual + s->sensor_first_row, sizeof(double) * nr, sizeof(double) * ns, R,
                                                       hipMemcpyDeviceToHost, e->stream));
  if (failure) HIPCHK(hipMemcpyAsync(failure, L.t.fail, sizeof(int) * R, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
}

int mjpc_hip_direct_cost_derivatives(MjpcHipEngine *e, int T, const MjpcHipDirectSettings *s, double fd_eps, int centered, int discrete, const double *q,
                                     const double *act, const double *ctrl, const double *time, const double *sensor_measurement, const double *force_measurement,
                                     const double *mocap, const double *userdata, double *cost, double *gradient, double *hessian_band, double *block_sensor,
                                     double *block_force, double *norm_gradient_sensor, double *norm_gradient_force, double *residual_sensor, double *residual_force,
                                     double *DfDq, double *DfDv, double *DfDa, double *DsDq, double *DsDv, double *DsDa, double *dvdq0, double *dvdq1, int *failure) {
  const char *who = "mjpc_hip_direct_cost_derivatives";
  if (!e) { set_error(std::string(who) + ": invalid argument"); return -1; }
  if (!(fd_eps > 0)) { set_error(std::string(who) + ": fd_eps <= 0"); return -1; }
  std::vector<int> first, row_sensor;
  if (dc_window_check(e, who, 1, T, s, q, act, ctrl, time, sensor_measurement, force_measurement, first, row_sensor) != 0) return -1;
  if (!cost || !gradient || !hessian_band) { set_error(std::string(who) + ": null input"); return -1; }
  centered = centered ? 1 : 0; discrete = discrete ? 1 : 0;
  const size_t E = inv_fd_rows_per_config(e->dims(), centered);
  if ((size_t)T * E > STEP_PASS_ROWS) { set_error(std::string(who) + ": T too large for one pass of the inverse tables (" + std::to_string(STEP_PASS_ROWS / E) + " configurations for this model)"); return -1; }
  KParams K;
  int rc = inverse_prepare(e, who, mocap, userdata, discrete, &K);
  if (rc != 0) return rc;
  const size_t Tz = T, nq = e->nq, nv = e->nv, na = e->na, nu = e->nu, nr = e->nr, ns = s->num_sensor_rows, m = s->num_sensor, nb = 3 * nv;
  const std::vector<int> dofmap = fd_dofmap(e);
  DcDerivLay L;
  PLACE(B_FD, L, e->dims(), Tz, centered, ns, m);
  auto up = [&](double *dst, const double *src, size_t cnt) { return cnt ? hipMemcpyAsync(dst, src, sizeof(double) * cnt, hipMemcpyHostToDevice, e->stream) : hipSuccess; };
  HIPCHK(up(L.q, q, Tz * nq)); HIPCHK(up(L.act, act, Tz * na)); HIPCHK(up(L.ctrl, ctrl, Tz * nu)); HIPCHK(up(L.time, time, Tz));
  HIPCHK(up(L.y_s, sensor_measurement, Tz * ns)); HIPCHK(up(L.y_f, force_measurement, Tz * nv));
  HIPCHK(hipMemcpyAsync(L.fd.dofmap, dofmap.data(), sizeof(int) * (2 * nv + 2), hipMemcpyHostToDevice, e->stream));
  DcArgs a;
  rc = dc_upload_spec(e, L.spec, L.work, T, (int)nv, (int)nr, s, first, row_sensor, &a);
  if (rc != 0) return rc;
  // the window's nominal rows where ifd_assemble reads them, and the velocity blocks
  const DcWinArgs w = dc_win_args(e, 1, T, s->timestep, L.q, L.act, L.ctrl, L.time, L.fd.dofmap, L.fd.x, L.fd.u, L.fd.a, L.fd.time, L.V0, L.V1);
  hipLaunchKernelGGL(dc_window_kernel, dim3((unsigned)((Tz + 3) / 4)), dim3(256), 0, e->stream, w, (unsigned)Tz);
  const size_t n_vb = Tz * nv * nv;
  hipLaunchKernelGGL(dc_vblock_kernel, dim3((unsigned)((n_vb + DC_THREADS - 1) / DC_THREADS)), dim3(DC_THREADS), 0, e->stream, w, n_vb);
  // mjpc_hip_inverse_fd's table, evaluations and differences, all six blocks
  InvFdArgs f;
  f.x = L.fd.x; f.u = L.fd.u; f.a = L.fd.a; f.time = L.fd.time; f.dofmap = L.fd.dofmap;
  f.T = T; f.nq = e->nq; f.nv = e->nv; f.na = e->na; f.nu = e->nu; f.nr = e->nr; f.centered = centered;
  f.eps = fd_eps; f.cs = cos(0.5 * fd_eps); f.sn = sin(0.5 * fd_eps);
  f.state_tab = L.fd.t.state; f.ctrl_tab = L.fd.t.ctrl; f.time_tab = L.fd.t.time; f.qacc_tab = L.fd.t.qacc; f.qfrc = L.fd.t.qfrc; f.residual = L.fd.t.residual; f.fail = L.fd.t.fail;
  f.DfDq = L.fd.Df[0]; f.DfDv = L.fd.Df[1]; f.DfDa = L.fd.Df[2]; f.DsDq = nr ? L.fd.Ds[0] : nullptr; f.DsDv = nr ? L.fd.Ds[1] : nullptr; f.DsDa = nr ? L.fd.Ds[2] : nullptr;
  f.failure = L.fd.failure;
  hipLaunchKernelGGL(ifd_assemble_kernel, dim3((unsigned)((L.fd.R + 3) / 4)), dim3(256), 0, e->stream, f, (unsigned)L.fd.R);
  inverse_rows(e, K, L.fd.R, L.fd.t, discrete);
  hipLaunchKernelGGL(ifd_difference_kernel, dim3((unsigned)((3 * nv + FD_TILE - 1) / FD_TILE), (unsigned)((nv + nr + FD_TILE - 1) / FD_TILE), (unsigned)Tz),
                     dim3(FD_TILE * FD_TILE), 0, e->stream, f);
  // residuals of the base evaluations, then the algebra on the blocks where they lie
  DcResArgs r;
  r.residual = L.fd.t.residual; r.qfrc = L.fd.t.qfrc; r.y_s = L.y_s; r.y_f = L.y_f; r.T = T; r.nv = (int)nv; r.nr = (int)nr; r.ns = (int)ns; r.row0 = s->sensor_first_row;
  r.E = (int)E; r.rs = L.rs; r.rf = L.rf;
  const size_t n_res = Tz * (ns + nv);
  hipLaunchKernelGGL(dc_residual_kernel, dim3((unsigned)((n_res + DC_THREADS - 1) / DC_THREADS)), dim3(DC_THREADS), 0, e->stream, r, n_res);
  a.rs = L.rs; a.rf = L.rf; a.V0 = L.V0; a.V1 = L.V1;
  for (int k = 0; k < 3; k++) { a.Df[k] = L.fd.Df[k]; a.Ds[k] = L.fd.Ds[k]; }
  dc_launch(e, a);
  HIPCHK(hipGetLastError());
  auto down = [&](double *dst, const double *src, size_t cnt) { return dst && cnt ? hipMemcpyAsync(dst, src, sizeof(double) * cnt, hipMemcpyDeviceToHost, e->stream) : hipSuccess; };
  const DcWork &k = L.work;
  HIPCHK(down(cost, k.cost, 3)); HIPCHK(down(gradient, k.gradient, Tz * nv)); HIPCHK(down(hessian_band, k.band, Tz * nv * nb));
  HIPCHK(down(block_sensor, k.Js, Tz * ns * nb)); HIPCHK(down(block_force, k.Jf, Tz * nv * nb));
  HIPCHK(down(norm_gradient_sensor, k.ng_s, Tz * ns)); HIPCHK(down(norm_gradient_force, k.ng_f, Tz * nv));
  HIPCHK(down(residual_sensor, k.res_s, Tz * ns)); HIPCHK(down(residual_force, k.res_f, Tz * nv));
  double *const Dfo[3] = {DfDq, DfDv, DfDa}, *const Dso[3] = {DsDq, DsDv, DsDa};
  for (int i = 0; i < 3; i++) { HIPCHK(down(Dfo[i], L.fd.Df[i], Tz * nv * nv)); HIPCHK(down(Dso[i], L.fd.Ds[i], Tz * nr * nv)); }
  HIPCHK(down(dvdq0, L.V0, Tz * nv * nv)); HIPCHK(down(dvdq1, L.V1, Tz * nv * nv));
  if (failure) HIPCHK(hipMemcpyAsync(failure, L.fd.failure, sizeof(int) * Tz, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
}

int mjpc_hip_get_frame(MjpcHipEngine *e, double *xpos, double *xmat, double *site_xpos, double *subtree_com, double *subtree_linvel) {
  if (!e || e->last_nlocal < 1) { set_error("mjpc_hip_get_frame: no finished plan"); return -1; }
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipStreamSynchronize(e->stream));
  size_t nb = (size_t)e->nbody, ns = (size_t)e->nsite;
  const double *d_frame = e->at(B_FRAME);
  if (xpos) HIPCHK(hipMemcpy(xpos, d_frame, sizeof(double) * 3 * nb, hipMemcpyDeviceToHost));
  if (xmat) HIPCHK(hipMemcpy(xmat, d_frame + 3 * nb, sizeof(double) * 9 * nb, hipMemcpyDeviceToHost));
  if (site_xpos && ns) HIPCHK(hipMemcpy(site_xpos, d_frame + 12 * nb, sizeof(double) * 3 * ns, hipMemcpyDeviceToHost));
  if (subtree_com) HIPCHK(hipMemcpy(subtree_com, d_frame + 12 * nb + 3 * ns, sizeof(double) * 3 * nb, hipMemcpyDeviceToHost));
  if (subtree_linvel) HIPCHK(hipMemcpy(subtree_linvel, d_frame + 15 * nb + 3 * ns, sizeof(double) * 3 * nb, hipMemcpyDeviceToHost));
  return 0;
}

int mjpc_hip_get_knots(MjpcHipEngine *e, double *knots) {
  if (!e || !knots || e->last_nlocal < 1) { set_error("mjpc_hip_get_knots: no finished plan"); return -1; }
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipMemcpy(knots, e->at(B_KNOTS), sizeof(double) * e->last_nlocal * row_doubles(e, 0, e->last_H, e->last_P), hipMemcpyDeviceToHost));
  return 0;
}

int mjpc_hip_get_candidate(MjpcHipEngine *e, int local_index, MjpcHipPlanOutput *out) {
  if (!e || !out || local_index < 0 || local_index >= e->last_nlocal) { set_error("mjpc_hip_get_candidate: index out of range"); return -1; }
  HIPCHK(hipSetDevice(e->device));
  if (out->returns) HIPCHK(hipMemcpyAsync(out->returns, e->at(B_RETURNS) + local_index, sizeof(double), hipMemcpyDeviceToHost, e->stream));
  if (out->failure) HIPCHK(hipMemcpyAsync(out->failure, e->at<int>(B_FAILURE) + local_index, sizeof(int), hipMemcpyDeviceToHost, e->stream));
  out->winner = e->last_offset + local_index;
  return fetch_rows(e, local_index, out);
}

int mjpc_hip_kernel_time(MjpcHipEngine *e, double *avg_rollout_us, double *avg_total_us) {
  if (!e) return 0;
  int n = e->acc_n;
  if (avg_rollout_us) *avg_rollout_us = n ? e->acc_rollout_us / n : 0;
  if (avg_total_us) *avg_total_us = n ? e->acc_total_us / n : 0;
  e->acc_rollout_us = 0; e->acc_total_us = 0; e->acc_n = 0;
  return n;
}

int mjpc_hip_device_ptrs(MjpcHipEngine *e, void **returns, void **states, void **residual) {
  if (!e) return -1;
  if (returns) *returns = e->at(B_RETURNS);
  if (states) *states = e->at(B_STATES);
  if (residual) *residual = e->at(B_RESIDUAL);
  return 0;
}

// every local candidate's trace rows [num_local][H][3*num_trace] of the last plan in one copy (GUI: SamplingPlanner::Traces)
int mjpc_hip_get_traces(MjpcHipEngine *e, double *traces) {
  if (!e || !traces || !e->last_nlocal) { set_error("mjpc_hip_get_traces: no finished plan"); return -1; }
  if (!e->ntr) return 0;
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipMemcpy(traces, e->at(B_TRACE), sizeof(double) * e->last_nlocal * row_doubles(e, 6, e->last_H, e->last_P), hipMemcpyDeviceToHost));
  return 0;
}

// every local candidate's Trajectory arrays of the last plan (any pointer may be NULL); diag = per candidate
// [Newton iterations summed over the steps, max contacts, max constraint rows, warning bits]
int mjpc_hip_get_all_candidates(MjpcHipEngine *e, double *states, double *actions, double *times, double *residual,
                             double *costs, double *trace, double *knots, int *diag) {
  if (!e || !e->last_nlocal) { set_error("mjpc_hip_get_all_candidates: no finished plan"); return -1; }
  HIPCHK(hipSetDevice(e->device));
  const size_t n = (size_t)e->last_nlocal;
  HIPCHK(hipStreamSynchronize(e->stream));
  double *dst[NROWS] = {knots, states, actions, times, residual, costs, trace};
  for (int k = 0; k < NROWS; k++) {
    const size_t cnt = n * row_doubles(e, k, e->last_H, e->last_P);
    if (dst[k] && cnt) HIPCHK(hipMemcpy(dst[k], e->at(B_KNOTS + k), sizeof(double) * cnt, hipMemcpyDeviceToHost));
  }
  if (diag) HIPCHK(hipMemcpy(diag, e->at(B_DIAG), sizeof(int) * n * 4, hipMemcpyDeviceToHost));
  return 0;
}

int mjpc_hip_lds_bytes(MjpcHipEngine *e) { return e ? (int)e->lds_bytes : 0; }
// 1 when the engine runs the spill flavour; *slab_bytes = its HBM slab per candidate (0 without one)
int mjpc_hip_debug_spill(MjpcHipEngine *e, int *slab_bytes) {
  if (slab_bytes) *slab_bytes = e ? e->slab_bytes : 0;
  return (e && e->spill) ? 1 : 0;
}
// host-only (no HIP call): the (LDS bytes, slab bytes per candidate) of the full-capacity flavour mjpc_hip_create would choose for
// this model under the current knobs; returns 1 when that is the spill flavour, 0 otherwise, < 0: refused (mjpc_hip_last_error)
int mjpc_hip_debug_spill_layout(const MjpcHipModel *model, const MjpcHipTask *task, int *lds_bytes, int *slab_bytes) {
  if (!model || !task) { set_error("mjpc_hip_debug_spill_layout: invalid argument"); return -1; }
  if (!check_views(model, task, "mjpc_hip_debug_spill_layout")) return -1;
  PackedModel pm;
  RolloutFn k = nullptr; bool cached = true, spill = false;
  if (!pick_flavour(model, task, 36, pm, &k, &cached, &spill, "mjpc_hip_debug_spill_layout")) return -1;
  if (lds_bytes) *lds_bytes = (int)((size_t)pm.L.total_doubles * sizeof(double));
  if (slab_bytes) *slab_bytes = spill ? (int)(((size_t)pm.slab_doubles * sizeof(double) + 255) / 256 * 256) : 0;
  return spill ? 1 : 0;
}
void mjpc_hip_debug_dense_capacity(MjpcHipEngine *e, int *nefc, int *ncon, int *hot) {
  if (nefc) *nefc = (e && e->tierB.k) ? e->tierB.nefc : 0;
  if (ncon) *ncon = (e && e->tierB.k) ? e->tierB.ncon : 0;
  if (hot) *hot = (e && e->tierB.k && e->tierB.cd > 0) ? 1 : 0;
}
// LDS bytes of the dense (two workgroups per CU) tier, 0 when the model has none; *used_last = 1 when the last plan ran on it
int mjpc_hip_dense_tier(MjpcHipEngine *e, int *used_last) {
  if (!e) return 0;
  if (used_last) *used_last = e->last_dense;
  return e->tierB.k ? (int)e->tierB.lds : 0;
}

// host-only (no HIP call): bytes of LDS one candidate would occupy; use_cache bit 0: with / without the LDS copy of the model
// tables, bit 1: the dense tier's lean layout (knots and entry tables stay in global memory).
// < 0: the model is refused (mjpc_hip_last_error tells why)
int mjpc_hip_layout_bytes(const MjpcHipModel *model, const MjpcHipTask *task, int use_cache) {
  if (!model || !task) { set_error("mjpc_hip_layout_bytes: invalid argument"); return -1; }
  if (!check_views(model, task, "mjpc_hip_layout_bytes")) return -1;
  PackedModel pm;
  int exact = 0;
  if (use_cache & 2) mjpc_pick_rollout_dense2(model->nv, &exact); else if (use_cache & 1) mjpc_pick_rollout_cached(model->nv, &exact); else mjpc_pick_rollout_direct(model->nv, &exact);
  if (!mjpc_host::build(pm, model, task, 36, (use_cache & 1) != 0, (use_cache & 2) != 0, (use_cache & 3) == 0, exact != 0)) { set_error("mjpc_hip_layout_bytes: " + pm.error); return -1; }
  return (int)((size_t)pm.L.total_doubles * sizeof(double));
}

#ifdef MJPC_PROFILE
// MJPC_PROFILE builds only (tools/profile_phases.py): per-candidate phase cycle counters of the last plan ([nlocal][24] int64)
int mjpc_hip_debug_fetch_prof(MjpcHipEngine *e, long long *prof) {
  if (!e || !e->last_nlocal) return -1;
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipMemcpy(prof, e->at(B_PROF), sizeof(long long) * (size_t)e->last_nlocal * 24, hipMemcpyDeviceToHost));
  return 0;
}
#endif

}  // extern "C"
