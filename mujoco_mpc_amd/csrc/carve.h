// carve.h — how the engine's host side (engine.hip) divides the grown-on-demand blocks of its one-step calls (B_FD, B_FBP and the
// pinned mirror H_PACK).  Host only and free of HIP: the host tests compile it with plain g++ (tests/host/carve_main.cpp).
//
// A layout is a plain struct of pointers and one lay() function that names each field once, in the order it lies in memory.  The
// entry point runs lay() on a null base for the byte count it reserves, on the buffer for the pointers and, where a block comes back
// in one copy, on the pinned mirror for the hand-out: size, pointers and hand-out are one statement and cannot disagree.
#pragma once
#include <stddef.h>

// bump carver over a base pointer: take<T>(n) is the next n elements of T (null while the base is null), bytes() what has been taken
struct Carve {
  char *base;
  size_t off = 0;
  explicit Carve(void *b = nullptr) : base((char *)b) {}
  // the running offset up to a whole T: after ints that are kept in whole doubles ("two to a double")
  template <class T> void align_to() { off = (off + alignof(T) - 1) / alignof(T) * alignof(T); }
  template <class T> T *take(size_t n) {
    align_to<T>();
    T *p = base ? (T *)(base + off) : nullptr;
    off += n * sizeof(T);
    return p;
  }
  size_t bytes() const { return off; }
};

// Spare doubles that every block on the device has carried since it was hand-carved, behind its last double field (the fd pass: in
// front of its callers' fields and the int tail).  No kernel is known to read them; none has been shown not to, so they stay.
#define CARVE_SPARE_DOUBLES 8

// the model's and task's sizes a layout depends on: nd = 2 nv + na (tangent state), ds = nq + nv + na
struct Dims { size_t nq, nv, na, nu, nr, ds, nd; };

// ------------------------------------------------------------------------------ the step kernel's tables, R rows
struct StepTab { double *state, *ctrl, *time, *next, *residual; int *fail; };
static inline void lay_step_rows(Carve &c, StepTab &t, const Dims &d, size_t R) {
  t.state = c.take<double>(R * d.ds); t.ctrl = c.take<double>(R * d.nu); t.time = c.take<double>(R);
  t.next = c.take<double>(R * d.ds); t.residual = c.take<double>(R * d.nr);
}
// mjpc_hip_step_batch
static inline void lay(Carve &c, StepTab &t, const Dims &d, size_t R) {
  lay_step_rows(c, t, d, R);
  c.take<double>(CARVE_SPARE_DOUBLES);
  t.fail = c.take<int>(R);
}

// ------------------------------------------------------------------------------ one finite-difference pass over Tg knots
struct FdLay { size_t R; StepTab t; double *x, *u, *time, *A, *B, *C, *D; int *failure, *dofmap; };
static inline size_t fd_rows_per_knot(const Dims &d, int centered) { return centered ? 1 + 2 * (d.nd + d.nu) : 1 + d.nd + d.nu; }
// the pass's block has a seam: its doubles, then whatever the call keeps behind them (lay() of GradLay, IlqgLay), then its ints
static inline void lay_fd_doubles(Carve &c, FdLay &f, const Dims &d, size_t Tg, int centered) {
  f.R = Tg * fd_rows_per_knot(d, centered);
  lay_step_rows(c, f.t, d, f.R);
  f.x = c.take<double>(Tg * d.ds); f.u = c.take<double>(Tg * d.nu); f.time = c.take<double>(Tg);
  f.A = c.take<double>(Tg * d.nd * d.nd); f.B = c.take<double>(Tg * d.nd * d.nu); f.C = c.take<double>(Tg * d.nr * d.nd); f.D = c.take<double>(Tg * d.nr * d.nu);
  c.take<double>(CARVE_SPARE_DOUBLES);
}
static inline void lay_fd_ints(Carve &c, FdLay &f, const Dims &d, size_t Tg) {
  c.align_to<double>();
  f.t.fail = c.take<int>(f.R); f.failure = c.take<int>(Tg); f.dofmap = c.take<int>(2 * d.nv + 2);
}
// mjpc_hip_transition_fd, mjpc_hip_linearize_step
static inline void lay(Carve &c, FdLay &f, const Dims &d, size_t Tg, int centered) {
  lay_fd_doubles(c, f, d, Tg, centered);
  lay_fd_ints(c, f, d, Tg);
}

// ------------------------------------------------------------------------------ the inverse kernel's tables, R rows
struct InvTab { double *state, *ctrl, *time, *qacc, *qfrc, *qfrc_constraint, *residual; int *fail; };
static inline void lay_inv_rows(Carve &c, InvTab &t, const Dims &d, size_t R) {
  t.state = c.take<double>(R * d.ds); t.ctrl = c.take<double>(R * d.nu); t.time = c.take<double>(R); t.qacc = c.take<double>(R * d.nv);
  t.qfrc = c.take<double>(R * d.nv); t.qfrc_constraint = c.take<double>(R * d.nv); t.residual = c.take<double>(R * d.nr);
}
// mjpc_hip_inverse_batch
static inline void lay(Carve &c, InvTab &t, const Dims &d, size_t R) {
  lay_inv_rows(c, t, d, R);
  c.take<double>(CARVE_SPARE_DOUBLES);
  t.fail = c.take<int>(R);
}
// mjpc_hip_inverse_fd: one pass over Tg configurations; the six blocks stand in the order DfDq, DfDv, DfDa, DsDq, DsDv, DsDa
struct InvFdLay { size_t R; InvTab t; double *x, *u, *a, *time, *Df[3], *Ds[3]; int *failure, *dofmap; };
static inline size_t inv_fd_rows_per_config(const Dims &d, int centered) { return 1 + (centered ? 6 : 3) * d.nv; }
static inline void lay(Carve &c, InvFdLay &f, const Dims &d, size_t Tg, int centered) {
  f.R = Tg * inv_fd_rows_per_config(d, centered);
  lay_inv_rows(c, f.t, d, f.R);
  f.x = c.take<double>(Tg * d.ds); f.u = c.take<double>(Tg * d.nu); f.a = c.take<double>(Tg * d.nv); f.time = c.take<double>(Tg);
  for (int k = 0; k < 3; k++) f.Df[k] = c.take<double>(Tg * d.nv * d.nv);
  for (int k = 0; k < 3; k++) f.Ds[k] = c.take<double>(Tg * d.nr * d.nv);
  c.take<double>(CARVE_SPARE_DOUBLES);
  f.t.fail = c.take<int>(f.R); f.failure = c.take<int>(Tg); f.dofmap = c.take<int>(2 * d.nv + 2);
}

// ------------------------------------------------------------------------------ cost derivatives
// what cd_kernel writes; the Hessians only on request (null otherwise)
struct CdOut { double *cr, *cx, *cu, *cxx, *cuu, *cxu; };
static inline void lay(Carve &c, CdOut &o, const Dims &d, size_t T, int hessians) {
  o.cr = c.take<double>(T * d.nr); o.cx = c.take<double>(T * d.nd); o.cu = c.take<double>(T * d.nu);
  o.cxx = hessians ? c.take<double>(T * d.nd * d.nd) : nullptr;
  o.cuu = hessians ? c.take<double>(T * d.nu * d.nu) : nullptr;
  o.cxu = hessians ? c.take<double>(T * d.nd * d.nu) : nullptr;
}
// mjpc_hip_cost_derivatives
struct CdLay { double *residual, *C, *D; CdOut out; };
static inline void lay(Carve &c, CdLay &l, const Dims &d, size_t T, int hessians) {
  l.residual = c.take<double>(T * d.nr); l.C = c.take<double>(T * d.nr * d.nd); l.D = c.take<double>(T * d.nr * d.nu);
  lay(c, l.out, d, T, hessians);
  c.take<double>(CARVE_SPARE_DOUBLES);
}

// ------------------------------------------------------------------------------ trajectory gradient
// the block that comes back in one copy; failure: ints, two to a double; end: one past the block
struct GradOut { double *k, *Vx, *Qx, *Qu, *dV; int *failure; double *end; };
static inline void lay(Carve &c, GradOut &o, const Dims &d, size_t T) {
  o.k = c.take<double>(T * d.nu); o.Vx = c.take<double>(T * d.nd); o.Qx = c.take<double>((T - 1) * d.nd); o.Qu = c.take<double>((T - 1) * d.nu);
  o.dV = c.take<double>(2);
  o.failure = c.take<int>(T);
  o.end = c.take<double>(0);
}
// mjpc_hip_trajectory_gradient: the pass, the residual rows, cr / cx / cu, the block that goes back
struct GradLay { FdLay fd; double *residual; CdOut cd; GradOut out; };
static inline void lay(Carve &c, GradLay &g, const Dims &d, size_t T, int centered) {
  lay_fd_doubles(c, g.fd, d, T, centered);
  g.residual = c.take<double>(T * d.nr);
  lay(c, g.cd, d, T, 0);
  lay(c, g.out, d, T);
  lay_fd_ints(c, g.fd, d, T);
}

// ------------------------------------------------------------------------------ iLQG backward pass
// the block that comes back in one copy: the gains and value / Q expansions, the regularisation and its rate, status (three ints in
// two doubles); behind it (tail) the nfail failure ints, two to a double, of a call that has them; end: one past the block
struct RcOut { double *k, *K, *Vx, *Vxx, *Qx, *Qu, *Qxx, *Qxu, *Quu, *dV, *reg; int *status; double *tail; int *failure; double *end; };
static inline void lay(Carve &c, RcOut &o, size_t T, size_t n, size_t m, size_t nfail) {
  o.k = c.take<double>(T * m); o.K = c.take<double>(T * m * n); o.Vx = c.take<double>(T * n); o.Vxx = c.take<double>(T * n * n);
  o.Qx = c.take<double>((T - 1) * n); o.Qu = c.take<double>((T - 1) * m); o.Qxx = c.take<double>((T - 1) * n * n);
  o.Qxu = c.take<double>((T - 1) * n * m); o.Quu = c.take<double>((T - 1) * m * m);
  o.dV = c.take<double>(2); o.reg = c.take<double>(2);
  o.status = c.take<int>(3);
  o.tail = c.take<double>(0);
  o.failure = c.take<int>(nfail);
  o.end = c.take<double>(0);
}
// mjpc_hip_ilqg_backward_pass; work: doubles of the kernel's scratch when it does not fit into LDS, else 0
struct RcLay { double *A, *B, *cx, *cu, *cxx, *cxu, *cuu, *actions, *limits; RcOut out; double *scratch; };
static inline void lay(Carve &c, RcLay &l, size_t T, size_t n, size_t m, int action_limits, size_t work) {
  l.A = c.take<double>((T - 1) * n * n); l.B = c.take<double>((T - 1) * n * m); l.cx = c.take<double>(T * n); l.cu = c.take<double>((T - 1) * m);
  l.cxx = c.take<double>(T * n * n); l.cxu = c.take<double>((T - 1) * n * m); l.cuu = c.take<double>((T - 1) * m * m);
  l.actions = c.take<double>(action_limits ? (T - 1) * m : 0); l.limits = c.take<double>(action_limits ? 2 * m : 0);
  lay(c, l.out, T, n, m, 0);
  l.scratch = c.take<double>(work);
  c.take<double>(CARVE_SPARE_DOUBLES);
}
// mjpc_hip_trajectory_ilqg: the pass, the residual rows, the cost derivatives, the limits, the block that goes back, the scratch
struct IlqgLay { FdLay fd; double *residual; CdOut cd; double *limits; RcOut out; double *scratch; };
static inline void lay(Carve &c, IlqgLay &l, const Dims &d, size_t T, int centered, size_t work) {
  lay_fd_doubles(c, l.fd, d, T, centered);
  l.residual = c.take<double>(T * d.nr);
  lay(c, l.cd, d, T, 1);
  l.limits = c.take<double>(2 * d.nu);
  lay(c, l.out, T, d.nd, d.nu, T);
  l.scratch = c.take<double>(work);
  lay_fd_ints(c, l.fd, d, T);
}

// ------------------------------------------------------------------------------ the direct optimiser's window cost (direct_cost.h)
// the sensors' description and the mask, uploaded as they are; the ints behind the doubles, two to a double
struct DcSpec { double *prm, *noise_sensor, *noise_process; int *dim, *first, *stage, *norm, *row_sensor, *mask; };
static inline void lay(Carve &c, DcSpec &s, size_t T, size_t nv, size_t ns, size_t num_sensor) {
  s.prm = c.take<double>(2 * num_sensor); s.noise_sensor = c.take<double>(num_sensor); s.noise_process = c.take<double>(nv);
  s.dim = c.take<int>(num_sensor); s.first = c.take<int>(num_sensor); s.stage = c.take<int>(num_sensor); s.norm = c.take<int>(num_sensor);
  s.row_sensor = c.take<int>(ns); s.mask = c.take<int>(T * num_sensor);
  c.align_to<double>();
}
// what the dc_* kernels write: per configuration the residuals, norm gradients and Hessian parts, weights and values; the blocks J and
// N J [T][ns + nv][3 nv]; the band, the gradient and the three costs
struct DcWork { double *res_s, *ng_s, *hd_s, *hs_s, *w_s, *wy_s, *res_f, *ng_f, *y_f, *Js, *Jf, *NJs, *NJf, *band, *gradient, *cost; };
static inline void lay(Carve &c, DcWork &w, size_t T, size_t nv, size_t ns, size_t num_sensor) {
  w.res_s = c.take<double>(T * ns); w.ng_s = c.take<double>(T * ns); w.hd_s = c.take<double>(T * ns);
  w.hs_s = c.take<double>(2 * T * num_sensor); w.w_s = c.take<double>(T * num_sensor); w.wy_s = c.take<double>(T * num_sensor);
  w.res_f = c.take<double>(T * nv); w.ng_f = c.take<double>(T * nv); w.y_f = c.take<double>(T);
  w.Js = c.take<double>(T * ns * 3 * nv); w.Jf = c.take<double>(T * nv * 3 * nv); w.NJs = c.take<double>(T * ns * 3 * nv); w.NJf = c.take<double>(T * nv * 3 * nv);
  w.band = c.take<double>(T * nv * 3 * nv); w.gradient = c.take<double>(T * nv); w.cost = c.take<double>(3);
}
// mjpc_hip_direct_assemble: the caller's arrays (residuals, the six inverse blocks in the order DfDq, DfDv, DfDa, DsDq, DsDv, DsDa, the two
// velocity blocks), the sensors, the kernels' own
struct DcLay { double *rs, *rf, *Df[3], *Ds[3], *V0, *V1; DcSpec spec; DcWork work; };
static inline void lay(Carve &c, DcLay &l, size_t T, size_t nv, size_t nr, size_t ns, size_t num_sensor) {
  l.rs = c.take<double>(T * ns); l.rf = c.take<double>(T * nv);
  for (int k = 0; k < 3; k++) l.Df[k] = c.take<double>(T * nv * nv);
  for (int k = 0; k < 3; k++) l.Ds[k] = c.take<double>(T * nr * nv);
  l.V0 = c.take<double>(T * nv * nv); l.V1 = c.take<double>(T * nv * nv);
  lay(c, l.spec, T, nv, ns, num_sensor);
  lay(c, l.work, T, nv, ns, num_sensor);
  c.take<double>(CARVE_SPARE_DOUBLES);
}

// mjpc_hip_direct_cost: nwin windows of T configurations through the inverse kernel's table (R = nwin T rows), value only: the work
// arrays of every window but no blocks
struct DcCostLay { InvTab t; double *q, *act, *ctrl, *time, *y_s, *y_f, *rs, *rf; int *dofmap; DcSpec spec; DcWork work; };
static inline void lay(Carve &c, DcCostLay &l, const Dims &d, size_t W, size_t T, size_t ns, size_t num_sensor) {
  const size_t R = W * T;
  lay_inv_rows(c, l.t, d, R);
  l.q = c.take<double>(R * d.nq); l.act = c.take<double>(R * d.na); l.ctrl = c.take<double>(R * d.nu); l.time = c.take<double>(T);
  l.y_s = c.take<double>(T * ns); l.y_f = c.take<double>(T * d.nv); l.rs = c.take<double>(R * ns); l.rf = c.take<double>(R * d.nv);
  lay(c, l.spec, T, d.nv, ns, num_sensor);
  DcWork &w = l.work;
  w = DcWork();
  w.res_s = c.take<double>(R * ns); w.ng_s = c.take<double>(R * ns); w.hd_s = c.take<double>(R * ns);
  w.hs_s = c.take<double>(2 * R * num_sensor); w.w_s = c.take<double>(R * num_sensor); w.wy_s = c.take<double>(R * num_sensor);
  w.res_f = c.take<double>(R * d.nv); w.ng_f = c.take<double>(R * d.nv); w.y_f = c.take<double>(R); w.cost = c.take<double>(3 * W);
  c.take<double>(CARVE_SPARE_DOUBLES);
  l.t.fail = c.take<int>(R); l.dofmap = c.take<int>(2 * d.nv + 2);
}
// mjpc_hip_direct_cost_derivatives: one pass of mjpc_hip_inverse_fd over the window (its nominal rows are written on the device), the
// window's inputs and measurements, the residuals, the velocity blocks, the sensors, the algebra's work arrays
struct DcDerivLay { InvFdLay fd; double *q, *act, *ctrl, *time, *y_s, *y_f, *rs, *rf, *V0, *V1; DcSpec spec; DcWork work; };
static inline void lay(Carve &c, DcDerivLay &l, const Dims &d, size_t T, int centered, size_t ns, size_t num_sensor) {
  lay(c, l.fd, d, T, centered);
  c.align_to<double>();
  l.q = c.take<double>(T * d.nq); l.act = c.take<double>(T * d.na); l.ctrl = c.take<double>(T * d.nu); l.time = c.take<double>(T);
  l.y_s = c.take<double>(T * ns); l.y_f = c.take<double>(T * d.nv); l.rs = c.take<double>(T * ns); l.rf = c.take<double>(T * d.nv);
  l.V0 = c.take<double>(T * d.nv * d.nv); l.V1 = c.take<double>(T * d.nv * d.nv);
  lay(c, l.spec, T, d.nv, ns, num_sensor);
  lay(c, l.work, T, d.nv, ns, num_sensor);
  c.take<double>(CARVE_SPARE_DOUBLES);
}

// ------------------------------------------------------------------------------ unscented moments, ns sensor rows, R = 2 nd + 1 points
// the block that goes up in one copy; dofmap, qmap: ints, two to a double
struct UkfIn { double *x, *L, *u, *noise_process, *noise_sensor; int *dofmap, *qmap; };
static inline void lay(Carve &c, UkfIn &i, const Dims &d, size_t ns) {
  i.x = c.take<double>(d.ds); i.L = c.take<double>(d.nd * d.nd); i.u = c.take<double>(d.nu);
  i.noise_process = c.take<double>(d.nd); i.noise_sensor = c.take<double>(ns);
  i.dofmap = c.take<int>(2 * d.nv + 2); i.qmap = c.take<int>(2 * d.nq + 2);
  c.align_to<double>();
}
// the block that comes back in one copy (without the next-state rows when the caller does not ask for them); failure: an int in a double
// end: one past the block
struct UkfBack { double *next, *state_mean, *sensor_mean, *cov_ss, *cov_sy, *cov_yy; int *failure; double *end; };
static inline void lay(Carve &c, UkfBack &b, const Dims &d, size_t ns) {
  b.next = c.take<double>((2 * d.nd + 1) * d.ds);
  b.state_mean = c.take<double>(d.ds); b.sensor_mean = c.take<double>(ns);
  b.cov_ss = c.take<double>(d.nd * d.nd); b.cov_sy = c.take<double>(d.nd * ns); b.cov_yy = c.take<double>(ns * ns);
  b.failure = c.take<int>(1);
  b.end = c.take<double>(0);
}
// on the device: between the two, the tables the kernels write and read (t.next is back.next)
struct UkfLay { UkfIn in; StepTab t; double *diff; UkfBack back; };
static inline void lay(Carve &c, UkfLay &l, const Dims &d, size_t ns) {
  const size_t R = 2 * d.nd + 1;
  lay(c, l.in, d, ns);
  l.t.state = c.take<double>(R * d.ds); l.t.ctrl = c.take<double>(R * d.nu); l.t.time = c.take<double>(R);
  l.t.residual = c.take<double>(R * d.nr);
  l.diff = c.take<double>(R * (d.nd + ns));
  l.t.fail = c.take<int>(R);
  lay(c, l.back, d, ns);
  l.t.next = l.back.next;
  c.take<double>(CARVE_SPARE_DOUBLES);
}
// the pinned mirror: the two blocks that travel, back to back
struct UkfHost { UkfIn in; UkfBack back; };
static inline void lay(Carve &c, UkfHost &h, const Dims &d, size_t ns) {
  lay(c, h.in, d, ns);
  lay(c, h.back, d, ns);
}

// ------------------------------------------------------------------------------ feedback rollouts (B_FBP)
// the policy [T], the steps of the nl candidates and, in time mode, the resampled tables [H] (null in indexed mode)
struct FbLay { double *times, *states, *actions, *improvement, *gain, *alpha, *scale, *xbar, *ubar, *kbar, *Kbar; };
static inline void lay(Carve &c, FbLay &l, const Dims &d, size_t T, size_t H, size_t nl, bool timed) {
  l.times = c.take<double>(T); l.states = c.take<double>(T * d.ds); l.actions = c.take<double>(T * d.nu); l.improvement = c.take<double>(T * d.nu);
  l.gain = c.take<double>(T * d.nu * d.nd);
  l.alpha = c.take<double>(nl); l.scale = c.take<double>(nl);
  l.xbar = timed ? c.take<double>(H * d.ds) : nullptr; l.ubar = timed ? c.take<double>(H * d.nu) : nullptr;
  l.kbar = timed ? c.take<double>(H * d.nu) : nullptr; l.Kbar = timed ? c.take<double>(H * d.nu * d.nd) : nullptr;
  c.take<double>(CARVE_SPARE_DOUBLES);
}
