// tests/hip/reduce_hooks.hip — TEST / MEASUREMENT HOOKS, not part of the product library.
// Built into tests/hip/libmjpc_hip_reducehooks.so by tests/test_wave_sum_bits.py (the flags of
// __graft_entry__.build_test_hooks()).  Holds the multi-value wave reductions of mujoco_mpc_amd/csrc/spmd.h as they were before
// they were transposed (the reference: one butterfly chain per sum), kernels that run reference and product side by side on the
// same inputs, and a lone-wave timing loop for the variants (tools/wavesum_time.py).
#include <hip/hip_runtime.h>
#include <string>
#include "../../mujoco_mpc_amd/csrc/spmd.h"

static thread_local std::string g_error;
static void set_error(const std::string &s) { g_error = s; }
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { set_error(std::string(#x) + ": " + hipGetErrorString(e_)); return -2; } } while (0)

// ---- reference: the reductions before the change, with the helpers they used (copied, prefixed ref_) -----------------------
DEV double ref_dpp_xchg(double v, const int ctrl_sel) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  switch (ctrl_sel) {
    case 0: lo = __builtin_amdgcn_update_dpp(0, lo, 0xB1, 0xF, 0xF, true); hi = __builtin_amdgcn_update_dpp(0, hi, 0xB1, 0xF, 0xF, true); break;   // quad_perm [1,0,3,2]
    case 1: lo = __builtin_amdgcn_update_dpp(0, lo, 0x4E, 0xF, 0xF, true); hi = __builtin_amdgcn_update_dpp(0, hi, 0x4E, 0xF, 0xF, true); break;   // quad_perm [2,3,0,1]
    case 2: lo = __builtin_amdgcn_update_dpp(0, lo, 0x141, 0xF, 0xF, true); hi = __builtin_amdgcn_update_dpp(0, hi, 0x141, 0xF, 0xF, true); break; // row_half_mirror
    default: lo = __builtin_amdgcn_update_dpp(0, lo, 0x140, 0xF, 0xF, true); hi = __builtin_amdgcn_update_dpp(0, hi, 0x140, 0xF, 0xF, true); break; // row_mirror
  }
  return __hiloint2double(hi, lo);
}
DEV double ref_row_total(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  double t = __hiloint2double(__builtin_amdgcn_update_dpp(0, hi, 0x142, 0xA, 0xF, false), __builtin_amdgcn_update_dpp(0, lo, 0x142, 0xA, 0xF, false));
  v += t;
  lo = __double2loint(v); hi = __double2hiint(v);
  t = __hiloint2double(__builtin_amdgcn_update_dpp(0, hi, 0x143, 0xC, 0xF, false), __builtin_amdgcn_update_dpp(0, lo, 0x143, 0xC, 0xF, false));
  v += t;
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
}
DEV void ref_wave_sum3(double &a, double &b, double &c) {
#pragma unroll
  for (int s = 0; s < 4; s++) {
    double ta = ref_dpp_xchg(a, s), tb = ref_dpp_xchg(b, s), tc = ref_dpp_xchg(c, s);
    a += ta; b += tb; c += tc;
  }
  a = ref_row_total(a); b = ref_row_total(b); c = ref_row_total(c);
}
DEV void ref_wave_sum4(double &a, double &b, double &c, double &d) {
#pragma unroll
  for (int s = 0; s < 4; s++) {
    double ta = ref_dpp_xchg(a, s), tb = ref_dpp_xchg(b, s), tc = ref_dpp_xchg(c, s), td = ref_dpp_xchg(d, s);
    a += ta; b += tb; c += tc; d += td;
  }
  a = ref_row_total(a); b = ref_row_total(b); c = ref_row_total(c); d = ref_row_total(d);
}

// ---- the alternative that was weighed against the transposed form (timing only): one butterfly chain per sum inside the rows,
// then the three row sums share a register (quad 0 of a row a, quad 1 b, quads 2 and 3 c) for the two swap levels
DEV void hybrid_wave_sum3(double &a, double &b, double &c) {
#pragma unroll
  for (int s = 0; s < 4; s++) {
    double ta = ref_dpp_xchg(a, s), tb = ref_dpp_xchg(b, s), tc = ref_dpp_xchg(c, s);
    a += ta; b += tb; c += tc;
  }
  const int q = (LANE >> 2) & 3;
  double v = q == 0 ? a : q == 1 ? b : c;
  v = swap_add32(swap_add16(v));
  a = lane_value(v, 0); b = lane_value(v, 4); c = lane_value(v, 8);
}

// set s: x[(s * 4 + k) * 64 + lane], k = 0 .. 3.  out[(s * 4 + v) * 4 + k]: v = 0 reference wave_sum3 (k < 3), 1 product wave_sum3,
// 2 reference wave_sum4, 3 product wave_sum4.  Every lane gets the sums; lane `s % 64` stores them (so a result that is right in
// lane 0 only does not pass).
__global__ void __launch_bounds__(64) reduce_bits_kernel(const double *x, unsigned long long *out, int nsets) {
  for (int s = blockIdx.x; s < nsets; s += gridDim.x) {
    const double *xs = x + (size_t)s * 4 * 64;
    const double a = xs[LANE], b = xs[64 + LANE], c = xs[128 + LANE], d = xs[192 + LANE];
    double r[4][4];
    r[0][0] = a; r[0][1] = b; r[0][2] = c; r[0][3] = 0.0; ref_wave_sum3(r[0][0], r[0][1], r[0][2]);
    r[1][0] = a; r[1][1] = b; r[1][2] = c; r[1][3] = 0.0; wave_sum3(r[1][0], r[1][1], r[1][2]);
    r[2][0] = a; r[2][1] = b; r[2][2] = c; r[2][3] = d; ref_wave_sum4(r[2][0], r[2][1], r[2][2], r[2][3]);
    r[3][0] = a; r[3][1] = b; r[3][2] = c; r[3][3] = d; wave_sum4(r[3][0], r[3][1], r[3][2], r[3][3]);
    if (LANE == (s & 63)) {
#pragma unroll
      for (int v = 0; v < 4; v++)
#pragma unroll
        for (int k = 0; k < 4; k++) out[((size_t)s * 4 + v) * 4 + k] = (unsigned long long)__double_as_longlong(r[v][k]);
    }
  }
}

// lone-wave timing: one wave per workgroup (the owner wave's situation: nothing else issues on its SIMD), `reps` reductions in a
// dependent chain - every lane's next inputs hang on the previous sums, as a line-search evaluation's do on the step length.
// out[0] = s_memtime ticks per repetition, out[1] keeps the chain alive
template <int MODE>
__global__ void __launch_bounds__(64) reduce_time_kernel(double *out, int reps, double seed) {
  double a = seed + LANE * 1e-3, b = a + 1.0, c = a + 2.0, d = a + 3.0;
  const double la = a, lb = b, lc = c, ld = d;
  const long long t0 = (long long)__builtin_amdgcn_s_memtime();
  for (int r = 0; r < reps; r++) {
    if (MODE == 0) ref_wave_sum3(a, b, c);
    if (MODE == 1) wave_sum3(a, b, c);
    if (MODE == 2) hybrid_wave_sum3(a, b, c);
    if (MODE == 3) ref_wave_sum4(a, b, c, d);
    if (MODE == 4) wave_sum4(a, b, c, d);
    if (MODE == 5) { /* the loop's own arithmetic */ }
    const double al = (a + b + c + d) * 1e-6;
    a = la + al; b = lb * al; c = lc - al; d = ld + al * lb;
  }
  const long long t1 = (long long)__builtin_amdgcn_s_memtime();
  if (LANE == 0 && blockIdx.x == 0) { out[0] = (double)(t1 - t0) / reps; out[1] = a + b + c + d; }
}

extern "C" {
const char *mjpc_hip_reducehooks_last_error(void) { return g_error.c_str(); }

// x: nsets x 4 x 64 doubles; out: nsets x 4 x 4 words (layout at reduce_bits_kernel).  One launch of 64 workgroups of one wave.
int mjpc_hip_debug_wave_sums(int nsets, const double *x, unsigned long long *out, int device) {
  if (nsets <= 0) { set_error("mjpc_hip_debug_wave_sums: nsets must be positive"); return -1; }
  HIPCHK(hipSetDevice(device));
  double *dx = nullptr; unsigned long long *dout = nullptr;
  const size_t nx = (size_t)nsets * 4 * 64, no = (size_t)nsets * 16;
  HIPCHK(hipMalloc(&dx, sizeof(double) * nx)); HIPCHK(hipMalloc(&dout, sizeof(unsigned long long) * no));
  HIPCHK(hipMemcpy(dx, x, sizeof(double) * nx, hipMemcpyHostToDevice));
  HIPCHK(hipMemset(dout, 0xFF, sizeof(unsigned long long) * no));
  hipLaunchKernelGGL(reduce_bits_kernel, dim3(64), dim3(64), 0, 0, dx, dout, nsets);
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(out, dout, sizeof(unsigned long long) * no, hipMemcpyDeviceToHost));
  hipFree(dx); hipFree(dout);
  return 0;
}

// mode: 0 reference wave_sum3 | 1 product wave_sum3 | 2 hybrid wave_sum3 | 3 reference wave_sum4 | 4 product wave_sum4 | 5 empty loop
int mjpc_hip_debug_wave_sum_time(int mode, int reps, double *out, int device) {
  if (mode < 0 || mode > 5 || reps <= 0) { set_error("mjpc_hip_debug_wave_sum_time: bad mode / reps"); return -1; }
  HIPCHK(hipSetDevice(device));
  double *dout = nullptr;
  HIPCHK(hipMalloc(&dout, sizeof(double) * 2));
  for (int w = 0; w < 2; w++) {
    switch (mode) {
      case 0: hipLaunchKernelGGL(reduce_time_kernel<0>, dim3(256), dim3(64), 0, 0, dout, reps, 0.5); break;
      case 1: hipLaunchKernelGGL(reduce_time_kernel<1>, dim3(256), dim3(64), 0, 0, dout, reps, 0.5); break;
      case 2: hipLaunchKernelGGL(reduce_time_kernel<2>, dim3(256), dim3(64), 0, 0, dout, reps, 0.5); break;
      case 3: hipLaunchKernelGGL(reduce_time_kernel<3>, dim3(256), dim3(64), 0, 0, dout, reps, 0.5); break;
      case 4: hipLaunchKernelGGL(reduce_time_kernel<4>, dim3(256), dim3(64), 0, 0, dout, reps, 0.5); break;
      default: hipLaunchKernelGGL(reduce_time_kernel<5>, dim3(256), dim3(64), 0, 0, dout, reps, 0.5); break;
    }
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(out, dout, sizeof(double) * 2, hipMemcpyDeviceToHost));
  hipFree(dout);
  return 0;
}
}  // extern "C"
